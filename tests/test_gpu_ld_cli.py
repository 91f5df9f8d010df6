"""-m gpu: --prune on the command line, on the fileset of tests/ld_util.py's cli_case(): 200 individuals at 600 variants in LD blocks
on two chromosomes, special variants planted, a run of duplicates across the chromosome boundary and a copy at either end of the
window (tests/test_ld_cpu.py shows that this case tells every mutant of the rule from the rule).

The lists are ld_util's greedy rule on the device's band; a pruned run is, byte for byte, the run on the fileset of the variants kept,
which the test writes itself; what is refused; and a threshold of 1, which removes nothing."""
import os
import re

import numpy as np
import pytest

import bedfiles as bf
from cli_util import BIN, run_cli, write_fileset_inputs
import ld_util as lu
from multiclust_amd import hip, host
from procutil import run_program

pytestmark = pytest.mark.gpu
PRUNE_LINE = re.compile(r"^LD pruning: kept (\d+) of (\d+) variants \(r2 > (\S+) within (\d+)\)$")
I, L, T, W = lu.CLI["I"], lu.CLI["L"], lu.CLI["t"], lu.CLI["window"]
FIT = ["-s", "3", "-n", "2", "-r", "7"]
PRUNE = ["--prune", "%g" % T, "--prune-window", "%d" % W]


@pytest.fixture(scope="module")
def case():
    """codes, chromosomes, packed records, the reference band and the variants the rule keeps: computed once, never changed"""
    codes, chrom = lu.cli_case()
    bed = bf.pack(codes, padding=1)
    r2 = lu.band(bed, I, W)
    keep = lu.greedy(r2, W, T, chrom)
    assert 0.2 * L < keep.sum() < 0.9 * L
    return dict(codes=codes, chrom=chrom, bed=bed, r2=r2, keep=keep, ids=["rs%d" % (7 * l) for l in range(L)])


def write_inputs(d, case, keep=None):
    """the fileset `data` in directory d: all variants, or the ones of keep (what `plink --extract` would write)"""
    return write_fileset_inputs(d, case, cols=None if keep is None else np.flatnonzero(keep), chrom=case["chrom"], ids=case["ids"])


def run(d, args, expect=0):
    """the program in directory d on its fileset `data`; its stdout lines (clock normalised) and every file it wrote"""
    return run_cli(["--bed", "data"] + args + ["-o", "stem"], d, expect)


def without_prune_line(lines):
    return [ln for ln in lines if not PRUNE_LINE.match(ln)]


def test_lists_are_the_greedy_rule_on_the_devices_band(case, tmp_path):
    ctx = hip.Context(0)
    try:
        r2 = ctx.bed_ld_band(I, case["bed"], window=W)
    finally:
        ctx.close()
    assert lu.same_bits(r2, case["r2"])
    keep = lu.greedy(r2, W, T, case["chrom"])
    d = write_inputs(tmp_path / "in", case)
    lines, files, _ = run(d, ["-a", "-k", "3"] + FIT + PRUNE)
    said = [PRUNE_LINE.match(ln).groups() for ln in lines if PRUNE_LINE.match(ln)]
    assert said == [("%d" % keep.sum(), "%d" % L, "%g" % T, "%d" % W)]
    assert lines.index("LD pruning: kept %d of %d variants (r2 > %g within %d)" % (keep.sum(), L, T, W)) == 0
    assert files["stem.prune.in"].decode() == "".join(case["ids"][l] + "\n" for l in range(L) if keep[l])
    assert files["stem.prune.out"].decode() == "".join(case["ids"][l] + "\n" for l in range(L) if not keep[l])
    # the library's reader says the same
    rc, dat = host.read_bed(os.path.join(str(d), "data"), decode=False, prune=T, prune_window=W)
    assert rc == 0 and dat["L"] == keep.sum() and dat["L_file"] == L and dat["variant_of"] == list(np.flatnonzero(keep))
    assert np.array_equal(dat["bed"], case["bed"][keep]) and dat["chrom"] == case["chrom"] and dat["variant_id"] == case["ids"]
    rc, dat = host.read_bed(os.path.join(str(d), "data"), decode=False)
    assert rc == 0 and dat["L"] == L and dat["variant_of"] is None and np.array_equal(dat["bed"], case["bed"])


@pytest.mark.parametrize("args", [["-a", "-k", "3"], ["-a", "-k", "3", "--fill"], ["-a", "-k", "3", "--streams", "2"]],
                         ids=["admixture", "fill", "streams"])
def test_a_pruned_run_is_the_run_on_the_extracted_fileset(case, args, tmp_path):
    full = write_inputs(tmp_path / "full", case)
    extracted = write_inputs(tmp_path / "extracted", case, case["keep"])
    lines1, files1, _ = run(full, args + FIT + PRUNE)
    lines0, files0, _ = run(extracted, args + FIT)
    assert len(lines1) == len(lines0) + 1 and without_prune_line(lines1) == lines0
    lists = {"stem.prune.in", "stem.prune.out"}
    assert set(files1) == set(files0) | lists and len(files0) >= 5
    for f in files0:
        assert files1[f] == files0[f], f
    if "--fill" in args:
        bim = files1["stem.admix.K=3.filled.bim"].decode().split("\n")
        assert len(bim) == case["keep"].sum() + 1 and [ln.split("\t")[1] for ln in bim[:-1]] == [case["ids"][l] for l in np.flatnonzero(case["keep"])]
        assert files1["stem.admix.K=3.filled.bim"] == open(os.path.join(str(extracted), "data.bim"), "rb").read()
        assert len(files1["stem.admix.K=3.filled.bed"]) == 3 + case["keep"].sum() * ((I + 3) // 4)


def test_refused_without_a_fileset_and_with_a_threshold_of_zero(case, tmp_path):
    d = write_inputs(tmp_path / "in", case)
    stru = os.path.join(str(d), "data.stru")
    bf.write_equivalent_stru(stru, case["codes"][:, :20])
    res = run_program([BIN, "-f", stru, "-a", "-k", "2", "--prune", "0.5"], cwd=str(d), timeout=60)
    assert res.returncode == 11 and "--prune and --prune-window need a PLINK fileset (--bed)" in res.stderr      # MC_EXIT_INVALID_USER_SETUP
    for t in ("0", "-0.5", "1.0001"):
        _, files, res = run(d, ["-a", "-k", "2", "--prune", t], expect=11)
        assert "the r2 threshold of --prune must lie in (0, 1]" in res.stderr and files == {} and res.stdout == ""


def test_a_threshold_of_one_keeps_every_variant(case, tmp_path):
    a = write_inputs(tmp_path / "a", case)
    b = write_inputs(tmp_path / "b", case)
    lines1, files1, _ = run(a, ["-a", "-k", "3"] + FIT + ["--prune", "1"])
    lines0, files0, _ = run(b, ["-a", "-k", "3"] + FIT)
    assert lines1[0] == "LD pruning: kept %d of %d variants (r2 > 1 within 50)" % (L, L) and lines1[1:] == lines0
    assert files1["stem.prune.in"].decode() == "".join(i + "\n" for i in case["ids"]) and files1["stem.prune.out"] == b""
    assert set(files1) == set(files0) | {"stem.prune.in", "stem.prune.out"}
    for f in files0:
        assert files1[f] == files0[f], f
