"""-m gpu: --mind, --geno, --maf and --hwe on the command line, on the fileset of tests/qc_util.py's cli_case(): 60 individuals of two
populations at 400 variants on two chromosomes, with three bad samples, rare, monomorphic, all-missing and badly typed variants,
variants far out of Hardy-Weinberg proportions, two duplicated individuals and a run of identical variants across the chromosomes'
boundary (tests/test_qc_cpu.py shows what each rule takes of it, and that the case tells every mutant from the real thing).

The stdout line, the four lists and the two tables are qc_util's rules on qc_util's counts (which tests/test_gpu_qc.py holds the
device to); a run with each option, and with all four, is byte for byte the run on the fileset of the individuals and variants kept,
which the test writes itself -- plain, followed by --prune, by --king-cutoff and by both, with --fill and with --query; the lists of
the chained filters name the final fileset; an emptied data set ends the run; and without the options nothing of them appears."""
import os

import numpy as np
import pytest

import bedfiles as bf
from cli_util import id_lines, option_is_there, run_cli, write_fileset_inputs
import king_util as ku
import qc_util as qu

pytestmark = pytest.mark.gpu
FIT = ["-a", "-k", "3", "-s", "3", "-n", "2", "-r", "7"]
C = qu.CLI
ALL = dict(mind=C["mind"], geno=C["geno"], maf=C["maf"], hwe=C["hwe"])
PRUNE = ["--prune", "%g" % C["prune_t"], "--prune-window", "%d" % C["prune_window"]]
KING = ["--king-cutoff", "%g" % C["king_t"]]
QC_FILES = {"stem.mind.in", "stem.mind.out", "stem.qc.in", "stem.qc.out", "stem.qc.var.txt", "stem.qc.ind.txt"}


@pytest.fixture(autouse=True, scope="module")
def the_options_are_there():
    """every test of this file is about the four options, the one on their absence included: the usage text names them"""
    for o in ALL:
        option_is_there("--%s <t>" % o)


@pytest.fixture(scope="module")
def case():
    codes, fids, iids, chrom = qu.cli_case()
    I, L = codes.shape
    return dict(codes=codes, fids=fids, iids=iids, chrom=chrom, I=I, L=L, ids=["rs%d" % (7 * l) for l in range(L)], pipelines={})


def pipeline(case, options, prune=False, king=False):
    """the restated pre-fit stage under these options: computed once per combination, never changed"""
    key = (tuple(sorted(options.items())), prune, king)
    if key not in case["pipelines"]:
        case["pipelines"][key] = qu.pipeline(case["codes"], case["chrom"], prune=prune, king=king, **options)
    return case["pipelines"][key]


def write_inputs(d, case, rows=None, cols=None):
    return write_fileset_inputs(d, case, rows, cols, chrom=case["chrom"], ids=case["ids"])


def flags(options):
    return [x for k, t in options.items() for x in ("--" + k, repr(float(t)))]


def run(d, args, expect=0):
    """the program in directory d on its fileset `data`; its stdout lines (clock normalised) and every file it wrote"""
    return run_cli(["--bed", "data"] + args + ["-o", "stem"], d, expect)


def variant_lines(case, cols):
    cols = set(int(l) for l in cols)
    return ("".join(case["ids"][l] + "\n" for l in range(case["L"]) if l in cols),
            "".join(case["ids"][l] + "\n" for l in range(case["L"]) if l not in cols))


RUNS = [("mind", dict(mind=C["mind"]), ""), ("geno", dict(geno=C["geno"]), ""), ("maf", dict(maf=C["maf"]), ""), ("hwe", dict(hwe=C["hwe"]), ""),
        ("all", ALL, ""), ("all", ALL, "prune"), ("all", ALL, "king"), ("all", ALL, "prune+king"), ("all", ALL, "fill"), ("all", ALL, "query")]


@pytest.mark.parametrize("name,options,extra", RUNS, ids=["%s-%s" % (n, e or "plain") for n, _, e in RUNS])
def test_a_run_with_the_options_is_the_run_on_the_kept_fileset(case, name, options, extra, tmp_path):
    prune, king = "prune" in extra, "king" in extra
    want = pipeline(case, options, prune, king)
    qc, rows, cols = want["qc"], want["rows"], want["cols"]
    assert 3 <= len(rows) <= case["I"] and 100 < len(cols) <= case["L"] and (len(rows) < case["I"] or len(cols) < case["L"])
    full = write_inputs(tmp_path / "full", case)
    kept = write_inputs(tmp_path / "kept", case, rows, cols)
    more = ["--fill"] if extra == "fill" else ["--query", "q.txt"] if extra == "query" else []
    if extra == "query":      # I' tokens: the file describes the kept individuals, as it would for the --keep fileset
        for d in (full, kept):
            (d / "q.txt").write_text(" ".join("1" if x % 5 == 2 else "0" for x in range(len(rows))) + "\n")
    lines1, files1, _ = run(full, FIT + more + flags(options) + (PRUNE if prune else []) + (KING if king else []))
    lines0, files0, _ = run(kept, FIT + more)
    told = [qu.line_text(qc, **options)[:-1]]
    lists = {"stem.qc.var.txt", "stem.qc.ind.txt"} | ({"stem.mind.in", "stem.mind.out"} if "mind" in options else set())
    lists |= {"stem.qc.in", "stem.qc.out"} if set(options) & {"geno", "maf", "hwe"} else set()
    n_l = int((qc["reason"] == qu.KEPT).sum())
    if prune:       # "of <n>": what the filter itself saw
        told.append("LD pruning: kept %d of %d variants (r2 > %g within %d)" % (len(cols), n_l, C["prune_t"], C["prune_window"]))
        lists |= {"stem.prune.in", "stem.prune.out"}
        assert want["seen"]["prune"] == n_l < case["L"] and len(cols) < n_l
    if king:
        n_pairs = int(ku.related(want["phi"], C["king_t"]).sum()) // 2
        told.append("Relatedness: kept %d of %d individuals (KING-robust kinship > %g: %d pairs)" % (len(rows), want["seen"]["king"], C["king_t"], n_pairs))
        lists |= {"stem.king.cutoff.in", "stem.king.cutoff.out", "stem.king.kin0"}
        assert want["seen"]["king"] == int(qc["ind_keep"].sum()) < case["I"] and len(rows) < want["seen"]["king"]
    assert lines1[:len(told)] == told
    assert lines1[len(told):] == lines0
    assert set(files1) == set(files0) | lists and len(files0) >= 5
    for f in files0:
        assert files1[f] == files0[f], f
    # the lists and the tables
    text = {f: files1[f].decode() for f in lists}
    assert text["stem.qc.var.txt"] == qu.var_table_text(qc, case["ids"])
    assert text["stem.qc.ind.txt"] == qu.ind_table_text(qc, case["fids"], case["iids"], case["L"])
    if "mind" in options:
        assert (text["stem.mind.in"], text["stem.mind.out"]) == (id_lines(case, qc["ind_keep"]), id_lines(case, ~qc["ind_keep"]))
    if "stem.qc.in" in lists:
        assert (text["stem.qc.in"], text["stem.qc.out"]) == variant_lines(case, np.flatnonzero(qc["reason"] == qu.KEPT))
    if prune:       # `plink --extract` on it writes the fileset the run was made on
        assert (text["stem.prune.in"], text["stem.prune.out"]) == variant_lines(case, cols)
    if king:
        kept_rows = np.isin(np.arange(case["I"]), rows)
        assert (text["stem.king.cutoff.in"], text["stem.king.cutoff.out"]) == (id_lines(case, kept_rows), id_lines(case, ~kept_rows))
        seen = want["rows_seen"]
        assert text["stem.king.kin0"] == ku.kin0_text(case["codes"][np.ix_(seen, cols)], [case["fids"][i] for i in seen],
                                                      [case["iids"][i] for i in seen], C["king_t"])
    if extra == "fill":      # the filtered fileset, filled
        for ext in ("fam", "bim"):
            assert files1["stem.admix.K=3.filled." + ext] == open(os.path.join(str(kept), "data." + ext), "rb").read()
        assert len(files1["stem.admix.K=3.filled.bed"]) == 3 + len(cols) * ((len(rows) + 3) // 4)
    if extra == "query":
        assert len(files1["stem.admix.K=3.query.txt"].decode().split("\n")) == 2 + sum(x % 5 == 2 for x in range(len(rows)))


def test_an_emptied_data_set_ends_the_run(case, tmp_path):
    d = write_inputs(tmp_path / "in", case)
    _, files, res = run(d, FIT + ["--mind", "0"], expect=11)        # every individual has a missing call
    assert "--mind 0 removes every one of the 60 individuals" in res.stderr and files == {} and res.stdout == ""
    small = dict(case, codes=np.full((40, 6), bf.HET, dtype=np.uint8), I=40, L=6, fids=case["fids"][:40], iids=case["iids"][:40])
    d = write_inputs(tmp_path / "het", small)
    _, files, res = run(d, FIT + ["--maf", "0.5", "--hwe", "0.001"], expect=11)
    assert "--hwe 0.001 removes the last of the 6 variants" in res.stderr and files == {} and res.stdout == ""
    # K is checked against the individuals kept, as on their fileset
    d = write_inputs(tmp_path / "k", case)
    _, files, res = run(d, ["-a", "-k", "58", "--mind", "%g" % C["mind"]], expect=11)
    assert "cannot exceed the number of individuals (57)" in res.stderr


def test_without_the_options_nothing_of_them_appears(case, tmp_path):
    d = write_inputs(tmp_path / "in", case)
    lines, files, _ = run(d, FIT)
    assert not any(ln.startswith("Quality control") for ln in lines) and not (set(files) & QC_FILES) and len(files) >= 5
    assert any("data.bed" in ln for ln in lines)
