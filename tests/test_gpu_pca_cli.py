"""-m gpu: --pca on the command line, on a fileset of 120 individuals at 2000 variants: three planted populations (tests/pca_util.py),
two duplicates for --king-cutoff to remove, a run of copied variants for --prune, rare variants for --maf.

--pca is no filter: a run with it is, byte for byte, the run without it, apart from the `PCA:` line and the three new files -- plain
and after every filter; the components are those of the fileset the filters left, which the test writes out from the .in lists and
runs on its own; the files agree with the entry point, whose numbers tests/test_gpu_pca.py holds to the definition."""
import re

import numpy as np
import pytest

import bedfiles as bf
from cli_util import option_is_there, run_cli, write_fileset_inputs
import pca_util as pu
from multiclust_amd import hip

pytestmark = pytest.mark.gpu
PCA_LINE = re.compile(r"^PCA: (\d+) components of (\d+) individuals x (\d+) of (\d+) variants \((\d+) iterations, largest residual (\S+)\): variance explained((?: \S+)+)$")
FIT = ["-a", "-k", "3", "-s", "3", "-n", "1", "-r", "7"]
PCA = ["--pca", "3"]
FILES = {"stem.eigenvec", "stem.eigenval", "stem.pca.txt"}
FILTERS = {"maf": ["--maf", "0.05"], "prune": ["--prune", "0.5", "--prune-window", "20"], "king": ["--king-cutoff", "0.2"]}
FILTERS["all"] = FILTERS["maf"] + FILTERS["prune"] + FILTERS["king"]


@pytest.fixture(scope="module")
def case():
    codes, pop = pu.planted(118, 2000, 3, seed=77, missing=0.03)
    codes = np.concatenate([codes, codes[[0, 1]]])                      # two duplicates, later in the file: --king-cutoff removes them
    pop = np.concatenate([pop, pop[[0, 1]]])
    for l in range(100, 130, 2):
        codes[:, l + 1] = codes[:, l]                                   # copied variants: --prune removes the copies
    rng = np.random.default_rng(5)
    for l in range(300, 340):                                           # rare variants: --maf removes them
        codes[:, l] = bf.HOM1
        codes[rng.integers(0, 118, size=2), l] = bf.HET
    I, L = codes.shape
    return dict(codes=codes, pop=pop, I=I, L=L, fids=["pop%d" % p for p in pop], iids=["ind%d" % i for i in range(I)],
                vids=["rs%d" % (7 * l) for l in range(L)])


def write_inputs(d, case, rows=None, cols=None):
    """the fileset `data` in directory d: everything, or the individuals `rows` at the variants `cols`; the padding bits are set
    whenever every individual is in it"""
    return write_fileset_inputs(d, case, rows, cols, ids=case["vids"], padding=1 if rows is None or len(rows) == case["I"] else 0)


def run(d, args, expect=0):
    """the program in directory d on its fileset `data`; its stdout lines (clock normalised) and every file it wrote"""
    return run_cli(["--bed", "data"] + args + ["-o", "stem"], d, expect)


@pytest.fixture(autouse=True, scope="module")
def the_option_is_there():
    option_is_there("--pca <n>")


@pytest.fixture(scope="module")
def plain(case, tmp_path_factory):
    """the run with --pca 3 and the run without, on the whole fileset"""
    with_pca = run(write_inputs(tmp_path_factory.mktemp("pca") / "with", case), FIT + PCA)
    without = run(write_inputs(tmp_path_factory.mktemp("pca") / "without", case), FIT)
    return with_pca, without


def test_a_run_with_the_option_is_the_run_without_it(plain):
    (lines1, files1, res1), (lines0, files0, _) = plain
    told = [ln for ln in lines1 if ln.startswith("PCA:")]
    assert len(told) == 1 and PCA_LINE.match(told[0]) and lines1[0] == told[0]
    assert [ln for ln in lines1 if ln != told[0]] == lines0
    assert set(files1) == set(files0) | FILES and len(files0) >= 5 and not (set(files0) & FILES)
    for f in files0:
        assert files1[f] == files0[f], f
    assert "WARNING" not in res1.stderr


def test_files_agree_with_the_entry_point_and_the_populations_separate(case, plain):
    (lines, files, _), _ = plain
    I = case["I"]
    ctx = hip.Context(0)
    try:
        r = ctx.bed_pca(I, bf.pack(case["codes"], padding=1), 3, n_extra=10, max_iter=200, tol=1e-6)
    finally:
        ctx.close()
    share = r["eigenvalues"] / r["trace"]
    assert lines[0] == "PCA: 3 components of %d individuals x %d of %d variants (%d iterations, largest residual %.6g): variance explained %s" % (
        I, r["n_used"], case["L"], r["n_iter"], r["residuals"].max(), " ".join("%.6g" % s for s in share))
    assert files["stem.eigenval"].decode() == "".join("%.6g\n" % v for v in r["eigenvalues"])
    assert files["stem.pca.txt"].decode() == "PC\tEIGENVALUE\tSHARE\tRESIDUAL\tCONVERGED\n" + "".join(
        "%d\t%.6g\t%.6g\t%.6g\t%d\n" % (c + 1, r["eigenvalues"][c], share[c], r["residuals"][c], r["residuals"][c] <= 1e-6) for c in range(3))
    assert files["stem.eigenvec"].decode() == "".join(
        "%s %s %s\n" % (case["fids"][i], case["iids"][i], " ".join("%.6g" % v for v in r["eigenvectors"][i])) for i in range(I))
    assert (r["residuals"] <= 1e-6).all()
    # every individual is nearer its own population's centroid on PC1 and PC2
    pc = np.array([[float(v) for v in ln.split()[2:4]] for ln in files["stem.eigenvec"].decode().splitlines()])
    centroids = np.stack([pc[case["pop"] == p].mean(axis=0) for p in range(3)])
    nearest = np.argmin(((pc[:, None, :] - centroids[None, :, :]) ** 2).sum(axis=2), axis=1)
    assert np.array_equal(nearest, case["pop"])


@pytest.mark.parametrize("which", ["maf", "prune", "king", "all"])
def test_after_the_filters_the_components_are_the_kept_filesets(case, which, tmp_path):
    args = FILTERS[which]
    lines1, files1, _ = run(write_inputs(tmp_path / "with", case), FIT + args + PCA)
    lines0, files0, _ = run(write_inputs(tmp_path / "without", case), FIT + args)
    told = [ln for ln in lines1 if ln.startswith("PCA:")]
    assert len(told) == 1 and [ln for ln in lines1 if ln != told[0]] == lines0
    at = lines1.index(told[0])
    assert at >= 1 and all(re.match(r"^(Quality control|LD pruning|Relatedness):", ln) for ln in lines1[:at])      # the last stage before the fit
    assert set(files1) == set(files0) | FILES
    for f in files0:
        assert files1[f] == files0[f], f
    # the fileset the filters left, from their lists: the last variant list and the individual list
    vlist = files1.get("stem.prune.in", files1.get("stem.qc.in"))
    cols = np.arange(case["L"]) if vlist is None else np.array([case["vids"].index(v) for v in vlist.decode().split()])
    ilist = files1.get("stem.king.cutoff.in")
    rows = np.arange(case["I"]) if ilist is None else np.array([case["iids"].index(ln.split("\t")[1]) for ln in ilist.decode().splitlines()])
    assert (which in ("maf", "prune", "all")) == (len(cols) < case["L"]) and (which in ("king", "all")) == (len(rows) == case["I"] - 2)
    lines2, files2, _ = run(write_inputs(tmp_path / "kept", case, rows, cols), FIT + PCA)
    assert lines2[0] == told[0]
    for f in FILES:
        assert files2[f] == files1[f], f
    ids = [tuple(ln.split()[:2]) for ln in files1["stem.eigenvec"].decode().splitlines()]
    assert ids == [(case["fids"][i], case["iids"][i]) for i in rows]                 # the kept .fam lines, in their order
    m = PCA_LINE.match(told[0])
    assert int(m.group(2)) == len(rows) and int(m.group(4)) == len(cols) and int(m.group(3)) <= len(cols)


def test_one_iteration_warns_and_the_exit_status_is_unchanged(case, tmp_path):
    lines, files, res = run(write_inputs(tmp_path / "in", case), FIT + PCA + ["--pca-iter", "1"])
    warned = [ln for ln in res.stderr.splitlines() if ln.startswith("WARNING [mc_pca.c]")]
    assert len(warned) == 1 and "PC1" in warned[0] and "--pca-iter" in warned[0]
    assert PCA_LINE.match(lines[0]).group(5) == "1" and FILES <= set(files)
    assert [ln.split("\t")[4] for ln in files["stem.pca.txt"].decode().splitlines()[1:]] == ["0", "0", "0"]


def test_more_components_than_the_individuals_allow_ends_the_run(case, tmp_path):
    d = write_inputs(tmp_path / "in", case, rows=np.arange(4))
    _, files, res = run(d, ["-a", "-k", "2", "--pca", "4"], expect=11)
    assert "--pca 4 asks for more components than the 4 individuals" in res.stderr and not (set(files) & FILES)
