"""-m gpu: --cv on the command line.  It adds one stdout line per K and changes nothing else: every other line and the five
result files are those of the same command without it; the value printed is mc_cross_validate's on the same fit."""
import os
import re

import numpy as np
import pytest

from cli_util import DATA, run_fresh
from multiclust_amd import host

pytestmark = pytest.mark.gpu
CV_LINE = re.compile(r"^CV error \(K=(\d+), (\d+) folds\): (\S+)  \[(\d+) held-out copies, (\d+) floored\]$")

FIXTURES = {
    "structure": ["-f", os.path.join(DATA, "multi.stru")],
    "bed": ["--bed", os.path.join(DATA, "cv_panel")],          # tests/bedfiles.py: draw_codes(60, 200, missing=0.03, seed=21)
}


def run(data, args, d):
    others, own, files = run_fresh(data + args, d, own=CV_LINE)
    return others, [m.groups() for m in own], files


def read_fixture(name):
    if name == "bed":
        rc, d = host.read_bed(FIXTURES[name][1])
    else:
        rc, d = host.read_structure(FIXTURES[name][1])
    assert rc == 0
    return d["ua"], d["geno"]


@pytest.mark.parametrize("fixture", sorted(FIXTURES))
def test_cv_adds_one_line_and_changes_nothing_else(fixture, tmp_path):
    args = ["-a", "-k", "2", "-s", "3", "-n", "2", "-r", "7"]
    plain, none, files_plain = run(FIXTURES[fixture], args, tmp_path / "plain")
    with_cv, cv_lines, files_cv = run(FIXTURES[fixture], args + ["--cv", "5"], tmp_path / "cv")
    assert none == [] and len(cv_lines) == 1
    assert with_cv == plain
    assert len(files_plain) == 5 and sorted(files_cv) == sorted(files_plain)
    for f in files_plain:
        assert files_cv[f] == files_plain[f], f
    K, F, value, copies, floored = cv_lines[0]
    assert (K, F) == ("2", "5")
    # the same fit through the host library: the better of the run's two initialisations, then mc_cross_validate
    ua, geno = read_fixture(fixture)
    fit = host.Fit(ua, geno, 2, admixture=1, accel_scheme=3, seed=7)
    try:
        ll = [fit.fit_unit(7, u).logL for u in (0, 1)]
        fit.fit_unit(7, 0 if ll[0] >= ll[1] else 1)
        cv, _, n_copies, n_floored, _ = fit.cross_validate(5)
    finally:
        fit.close()
    assert value == "%.10f" % cv and (int(copies), int(floored)) == (n_copies, n_floored)
    assert n_copies == int((geno != 0xFF).sum())


def test_one_line_per_k_on_the_same_folds(tmp_path):
    args = ["-a", "-1", "1", "-2", "3", "-s", "3", "-n", "2", "-r", "7"]
    plain, none, files_plain = run(FIXTURES["structure"], args, tmp_path / "plain")
    with_cv, cv_lines, files_cv = run(FIXTURES["structure"], args + ["--cv", "5"], tmp_path / "cv")
    assert none == [] and with_cv == plain and files_cv == files_plain
    assert [ln[0] for ln in cv_lines] == ["1", "2", "3"] and all(ln[1] == "5" for ln in cv_lines)
    # every K is scored on the same partition of the same copies: all of them, once
    ua, geno = read_fixture("structure")
    assert {ln[3] for ln in cv_lines} == {str(int((geno != 0xFF).sum()))}
    values = [float(ln[2]) for ln in cv_lines]
    assert all(np.isfinite(values)) and len(set(values)) == 3
    # K = 1 has one fit whatever the folds of the other K: its line is that of a run with -k 1 alone
    _, alone, _ = run(FIXTURES["structure"], ["-a", "-k", "1", "-s", "3", "-n", "2", "-r", "7", "--cv", "5"], tmp_path / "k1")
    assert alone == cv_lines[:1]
