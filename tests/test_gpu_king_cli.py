"""-m gpu: --king-cutoff on the command line, on the fileset of tests/king_util.py's cli_case(): 24 individuals at 900 variants, founders of
two populations with a duplicate, two trios with sibs and a pair of parents with a child planted among them (tests/test_king_cpu.py
shows that at 0.125 the related pairs are exactly the planted ones, and that the case tells every mutant from the real thing).

The stdout line and the three files are king_util's rule on king_util's kinships (which tests/test_gpu_king.py holds the device to);
a run with the option is, byte for byte, the run on the fileset of the individuals kept, which the test writes itself -- plain, after
--prune, with --fill and with --query (a query file of I' tokens); what is refused; and without the option nothing of it appears.  (No
committed golden is a run on a fileset: the goldens of tests/golden/cli_* are the reference's, on STRUCTURE files, and
tests/test_gpu_cli.py holds the program to them as before.)"""
import os
import re

import numpy as np
import pytest

import bedfiles as bf
from cli_util import BIN, id_lines, option_is_there, run_cli, write_fileset_inputs
import king_util as ku
import ld_util as lu
from multiclust_amd import hip, host
from procutil import run_program

pytestmark = pytest.mark.gpu
KING_LINE = re.compile(r"^Relatedness: kept (\d+) of (\d+) individuals \(KING-robust kinship > (\S+): (\d+) pairs\)$")
PRUNE_LINE = re.compile(r"^LD pruning: kept \d+ of \d+ variants ")
T = ku.CLI["t"]
FIT = ["-a", "-k", "3", "-s", "3", "-n", "2", "-r", "7"]
KING = ["--king-cutoff", "%g" % T]
PRUNE = ["--prune", "0.5", "--prune-window", "20"]
LISTS = {"stem.king.cutoff.in", "stem.king.cutoff.out", "stem.king.kin0"}


@pytest.fixture(autouse=True, scope="module")
def the_option_is_there():
    """every test of this file is about --king-cutoff, the one on its absence included: the usage text names the option"""
    option_is_there("--king-cutoff <t>")


@pytest.fixture(scope="module")
def case():
    """codes, ids, the reference kinships and the individuals the rule keeps, on all variants and on the variants --prune keeps:
    computed once, never changed"""
    codes, planted, fids, iids = ku.cli_case()
    I, L = codes.shape
    phi, _ = ku.kinship(codes)
    keep = ku.greedy(ku.related(phi, T))
    vkeep = lu.greedy(lu.band(bf.pack(codes), I, 20), 20, 0.5)
    assert 0.5 * L < vkeep.sum() < L
    phi_p, _ = ku.kinship(codes[:, vkeep])
    return dict(codes=codes, planted=planted, fids=fids, iids=iids, I=I, L=L, keep=keep, vkeep=vkeep,
                keep_pruned=ku.greedy(ku.related(phi_p, T)), n_pairs_pruned=int(ku.related(phi_p, T).sum()) // 2)


def write_inputs(d, case, keep=None, vkeep=None):
    """the fileset `data` in directory d: everything, or the individuals of keep (what `plink --keep` would write) at the variants of
    vkeep (`plink --extract`)"""
    return write_fileset_inputs(d, case, None if keep is None else np.flatnonzero(keep), None if vkeep is None else np.flatnonzero(vkeep))


def run(d, args, expect=0):
    """the program in directory d on its fileset `data`; its stdout lines (clock normalised) and every file it wrote"""
    return run_cli(["--bed", "data"] + args + ["-o", "stem"], d, expect)


def test_line_and_lists_are_the_rule_on_the_devices_kinships(case, tmp_path):
    I, keep = case["I"], case["keep"]
    ctx = hip.Context(0)
    try:
        phi, cnt = ctx.bed_king(I, bf.pack(case["codes"], padding=1))
    finally:
        ctx.close()
    want_phi, want_cnt = ku.kinship(case["codes"])
    assert ku.same_bits(phi, want_phi) and np.array_equal(cnt, want_cnt)
    d = write_inputs(tmp_path / "in", case)
    lines, files, _ = run(d, FIT + KING)
    said = [KING_LINE.match(ln).groups() for ln in lines if KING_LINE.match(ln)]
    assert said == [("%d" % keep.sum(), "%d" % I, "%g" % T, "%d" % len(case["planted"]))]
    assert lines[0] == "Relatedness: kept %d of %d individuals (KING-robust kinship > %g: %d pairs)" % (keep.sum(), I, T, len(case["planted"]))
    assert files["stem.king.cutoff.in"].decode() == id_lines(case, keep)
    assert files["stem.king.cutoff.out"].decode() == id_lines(case, ~keep)
    assert files["stem.king.kin0"].decode() == ku.kin0_text(case["codes"], case["fids"], case["iids"], T)
    # the library's reader says the same
    rc, dat = host.read_bed(os.path.join(str(d), "data"), decode=False, king_cutoff=T)
    kept = list(np.flatnonzero(keep))
    assert rc == 0 and dat["I"] == keep.sum() and dat["I_file"] == I and dat["individual_of"] == kept and dat["L"] == case["L"]
    assert np.array_equal(dat["bed"], bf.pack(case["codes"][keep], padding=0))
    assert dat["names"] == [case["iids"][i] for i in kept] and dat["fam_iid"] == case["iids"] and dat["fam_fid"] == case["fids"]
    assert [dat["pops"][x] for x in dat["locale"]] == [case["fids"][i] for i in kept] and sum(dat["i_p"]) == len(kept)
    assert {(p[0], p[1]) for p in dat["king_pairs"]} == case["planted"]
    rc0, same = host.read_bed(os.path.join(str(write_inputs(tmp_path / "kept", case, keep)), "data"), decode=False)
    for field in ("I", "L", "T", "M", "missing_data", "names", "pops", "numpops", "i_p"):
        assert dat[field] == same[field], field
    assert rc0 == 0 and np.array_equal(dat["locale"], same["locale"]) and np.array_equal(dat["ua"], same["ua"])
    assert np.array_equal(dat["bed"], same["bed"])
    rc, dat = host.read_bed(os.path.join(str(d), "data"), decode=False)
    assert rc == 0 and dat["I"] == I and dat["individual_of"] is None


@pytest.mark.parametrize("extra", ["plain", "prune", "fill", "query", "streams"])
def test_a_run_with_the_option_is_the_run_on_the_kept_fileset(case, extra, tmp_path):
    pruned = extra == "prune"
    keep = case["keep_pruned"] if pruned else case["keep"]
    full = write_inputs(tmp_path / "full", case)
    kept = write_inputs(tmp_path / "kept", case, keep, case["vkeep"] if pruned else None)
    args = {"plain": [], "prune": [], "fill": ["--fill"], "query": ["--query", "q.txt"], "streams": ["--streams", "2"]}[extra]
    if extra == "query":      # I' tokens: the file describes the kept individuals, as it would for the --keep fileset
        tokens = " ".join("1" if x % 5 == 2 else "0" for x in range(int(keep.sum()))) + "\n"
        for d in (full, kept):
            (d / "q.txt").write_text(tokens)
    lines1, files1, _ = run(full, FIT + args + (PRUNE if pruned else []) + KING)
    lines0, files0, _ = run(kept, FIT + args)
    told = [ln for ln in lines1 if KING_LINE.match(ln) or PRUNE_LINE.match(ln)]
    assert len(told) == (2 if pruned else 1) and lines1[:len(told)] == told and KING_LINE.match(told[-1])      # directly after the LD line
    assert lines1[len(told):] == lines0
    if pruned:
        assert KING_LINE.match(told[-1]).groups() == ("%d" % keep.sum(), "%d" % case["I"], "%g" % T, "%d" % case["n_pairs_pruned"])
    lists = LISTS | ({"stem.prune.in", "stem.prune.out"} if pruned else set())
    assert set(files1) == set(files0) | lists and len(files0) >= 5
    for f in files0:
        assert files1[f] == files0[f], f
    assert files1["stem.king.cutoff.in"].decode() == id_lines(case, keep)
    if extra == "fill":
        assert files1["stem.admix.K=3.filled.fam"] == open(os.path.join(str(kept), "data.fam"), "rb").read()
        assert len(files1["stem.admix.K=3.filled.bed"]) == 3 + case["L"] * ((int(keep.sum()) + 3) // 4)
    if extra == "query":
        assert len(files1["stem.admix.K=3.query.txt"].decode().split("\n")) == 2 + sum(x % 5 == 2 for x in range(int(keep.sum())))


def test_refusals_and_their_exit_statuses(case, tmp_path):
    d = write_inputs(tmp_path / "in", case)
    stru = os.path.join(str(d), "data.stru")
    bf.write_equivalent_stru(stru, case["codes"][:, :20])
    res = run_program([BIN, "-f", stru, "-a", "-k", "2", "--king-cutoff", "0.125"], cwd=str(d), timeout=60)
    assert res.returncode == 10 and "--king-cutoff needs a PLINK fileset (--bed)" in res.stderr and res.stdout == ""      # MC_EXIT_INVALID_CMD_ARGUMENT
    for t in ("0", "-0.125", "0.5", "1"):
        _, files, res = run(d, ["-a", "-k", "2", "--king-cutoff", t], expect=10)
        assert "the kinship threshold of --king-cutoff must lie in (0, 0.5)" in res.stderr and files == {} and res.stdout == ""
    _, files, res = run(d, ["-a", "-k", "2", "--king-cutoff"], expect=10)       # no threshold
    assert files == {} and res.stdout == ""
    # K is checked against the individuals kept, as on their fileset
    _, files, res = run(d, ["-a", "-k", "%d" % (case["keep"].sum() + 1)] + KING, expect=11)
    assert "cannot exceed the number of individuals (%d)" % case["keep"].sum() in res.stderr


def test_without_the_option_nothing_of_it_appears(case, tmp_path):
    d = write_inputs(tmp_path / "in", case)
    lines, files, _ = run(d, FIT)
    assert not any(ln.startswith("Relatedness") for ln in lines) and not (set(files) & LISTS) and len(files) >= 5
    assert any("data.bed" in ln for ln in lines)
