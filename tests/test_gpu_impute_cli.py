"""-m gpu: --fill on the command line.  Nothing but its own line and files depends on it, the line and the files are Fit.impute()'s
and the writers' on the same fit (STRUCTURE and PLINK input), there is one line and one file set per K, and --cv and --se, which
install other data sets on the way, say what they say without it."""
import os
import re

import numpy as np
import pytest

import bedfiles as bf
from cli_util import run_fresh
import cv_util as cu
import impute_util as iu
from multiclust_amd import host

pytestmark = pytest.mark.gpu
FILL_LINE = re.compile(r"^Imputation \(K=(\d+)\): (\d+) copies filled in (\d+) genotypes, (\d+) left missing, mean confidence (\S+)$")
STANDARD = ["stem.admix.K=%d.out.txt", "stem.admix.K=%d.etaik.txt", "stem.admix.K=%d.pklm.txt", "stem_admix_indivq_%d.indivq",
            "stem_admix_popq_%d.popq"]

I, L, CLUSTERS = 72, 400, 3
ARGS = ["-a", "-s", "3", "-n", "2", "-r", "7"]


def codes():
    """clustered diploid biallelic data as .bed codes, 5 % of the calls missing, one locus without a call"""
    _, geno = cu.clustered_dataset(I, L, CLUSTERS, 11)
    n = geno.astype(np.int64).sum(axis=2)
    c = np.array([bf.HOM1, bf.HET, bf.HOM2], dtype=np.uint8)[n]
    c[np.random.default_rng(6).random((I, L)) < 0.05] = bf.MISS
    c[:, 17] = bf.MISS
    return c


def write_inputs(d, bed=False):
    d.mkdir()
    stru = os.path.join(str(d), "data.stru")
    bf.write_equivalent_stru(stru, codes())
    if bed:
        bf.write_fileset(os.path.join(str(d), "data"), codes(), padding=1)
        return ["--bed", os.path.join(str(d), "data")], stru
    return ["-f", stru], stru


def run(data, args, d):
    others, own, files = run_fresh(data + args, d / "out", own=FILL_LINE)
    return others, [m.groups() for m in own], files, str(d / "out")


def test_nothing_else_changes(tmp_path):
    data, _ = write_inputs(tmp_path / "in")
    args = ARGS + ["-k", "3"]
    lines0, fill0, files0, _ = run(data, args, tmp_path / "a")
    lines1, fill1, files1, _ = run(data, args + ["--fill"], tmp_path / "b")
    assert fill0 == [] and len(fill1) == 1 and lines0 == lines1
    standard = [f % 3 for f in STANDARD]
    assert sorted(files0) == sorted(standard) and sorted(files1) == sorted(standard + ["stem.admix.K=3.filled.stru"])
    for f in standard:
        assert files0[f] == files1[f], f


@pytest.mark.parametrize("form", ["structure", "bed"])
def test_command_line_equals_library(form, tmp_path):
    data, stru = write_inputs(tmp_path / "in", bed=form == "bed")
    _, fill, files, outdir = run(data, ARGS + ["-k", "3", "--fill"], tmp_path / "in")
    rc, d = host.read_structure(stru)
    assert rc == 0
    fit = host.Fit(d["ua"], d["geno"], 3, admixture=1, accel_scheme=3, seed=7)
    try:
        ll = [fit.fit_unit(7, u).logL for u in (0, 1)]
        fit.fit_unit(7, 0 if ll[0] >= ll[1] else 1)
        q = fit.get_q(fit.mod.pindex)
        filled, r = fit.impute()
        assert np.array_equal(fit.get_q(fit.mod.pindex), q)
    finally:
        fit.close()
    assert fill == [("3", "%d" % r["n_filled"], "%d" % r["n_genotypes"], "%d" % r["n_left"], "%.6f" % r["mean_conf"])]
    miss = d["geno"] == iu.MISSING
    assert r["n_filled"] + r["n_left"] == miss.sum() and r["n_left"] == 2 * I and (filled[:, 17] == iu.MISSING).all()
    assert np.array_equal(filled[~miss], d["geno"][~miss]) and r["n_filled"] == (filled[miss] != iu.MISSING).sum()
    if form == "structure":
        want = str(tmp_path / "want.stru")
        assert host.write_filled_structure(stru, want, filled) == 0
        assert files["stem.admix.K=3.filled.stru"] == open(want, "rb").read()
        rc2, d2 = host.read_structure(os.path.join(outdir, "stem.admix.K=3.filled.stru"))
        assert rc2 == 0 and np.array_equal(d2["geno"], filled)
    else:
        want = str(tmp_path / "want")
        assert host.write_filled_bed(data[1], want, filled) == 0
        for ext in (".bed", ".bim", ".fam"):
            assert files["stem.admix.K=3.filled" + ext] == open(want + ext, "rb").read(), ext
        rc2, d2 = host.read_bed(os.path.join(outdir, "stem.admix.K=3.filled"))
        assert rc2 == 0 and np.array_equal(d2["geno"], np.sort(filled, axis=2))
        assert "stem.admix.K=3.filled.stru" not in files


def test_one_line_and_one_file_set_per_k(tmp_path):
    data, _ = write_inputs(tmp_path / "in")
    _, fill, files, _ = run(data, ARGS + ["-1", "2", "-2", "3", "--fill"], tmp_path / "in")
    assert [ln[0] for ln in fill] == ["2", "3"]
    assert sorted(f for f in files if ".filled." in f) == ["stem.admix.K=2.filled.stru", "stem.admix.K=3.filled.stru"]
    assert fill[0][1:4] == fill[1][1:4]                          # the same copies are missing for every K


def test_with_cv_and_se_their_lines_stand(tmp_path):
    data, _ = write_inputs(tmp_path / "in")
    args = ARGS + ["-k", "3", "--cv", "2", "--se", "2"]
    lines0, _, files0, _ = run(data, args, tmp_path / "a")
    lines1, fill1, files1, _ = run(data, args + ["--fill"], tmp_path / "b")
    assert lines0 == lines1 and len(fill1) == 1
    assert any(ln.startswith("CV error (K=3") for ln in lines0) and any(ln.startswith("Bootstrap SE (K=3") for ln in lines0)
    assert files0["stem.admix.K=3.se.txt"] == files1["stem.admix.K=3.se.txt"]
    # ... and --fill says what it says without them: --cv and --se have installed the data set again
    _, fill2, files2, _ = run(data, ARGS + ["-k", "3", "--fill"], tmp_path / "c")
    assert fill2 == fill1 and files2["stem.admix.K=3.filled.stru"] == files1["stem.admix.K=3.filled.stru"]
