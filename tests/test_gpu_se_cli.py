"""-m gpu: --se on the command line.  It adds one stdout line per K and one file and changes nothing else: every other line and the
five result files are those of the same command without it; the figures printed and written are mc_locus_bootstrap's on the same
fit."""
import os
import re

import numpy as np
import pytest

from cli_util import DATA, run_fresh, split_own
from multiclust_amd import host

pytestmark = pytest.mark.gpu
SE_LINE = re.compile(r"^Bootstrap SE \(K=(\d+), (\d+) replicates, block (\d+)\): mean (\S+)  max (\S+)  \[(\d+) failed\]$")
CV_LINE = re.compile(r"^CV error \(K=(\d+), (\d+) folds\): (\S+)  \[(\d+) held-out copies, (\d+) floored\]$")

FIXTURES = {
    "structure": ["-f", os.path.join(DATA, "multi.stru")],
    "bed": ["--bed", os.path.join(DATA, "cv_panel")],          # tests/bedfiles.py: draw_codes(60, 200, missing=0.03, seed=21)
}


def run(data, args, d):
    return run_fresh(data + args, d)[:2]


def split(lines):
    others, own = split_own(lines, SE_LINE)
    return others, [m.groups() for m in own]


def read_fixture(name):
    if name == "bed":
        rc, d = host.read_bed(FIXTURES[name][1])
    else:
        rc, d = host.read_structure(FIXTURES[name][1])
    assert rc == 0
    return d["ua"], d["geno"]


def number(v):
    """a double as the program's %.10f prints it"""
    return ("-nan" if np.signbit(v) else "nan") if np.isnan(v) else "%.10f" % v


@pytest.mark.parametrize("fixture,extra", [("structure", []), ("bed", []), ("structure", ["--streams", "2"])])
def test_se_adds_one_line_and_one_file_and_changes_nothing_else(fixture, extra, tmp_path):
    args = ["-a", "-k", "2", "-s", "3", "-n", "2", "-r", "7"] + extra
    plain, files_plain = run(FIXTURES[fixture], args, tmp_path / "plain")
    with_se, files_se = run(FIXTURES[fixture], args + ["--se", "5"], tmp_path / "se")
    assert split(plain)[1] == []
    rest, se_lines = split(with_se)
    assert rest == plain and len(se_lines) == 1
    name = "stem.admix.K=2.se.txt"
    assert len(files_plain) == 5 and sorted(files_se) == sorted(list(files_plain) + [name])
    for f in files_plain:
        assert files_se[f] == files_plain[f], f
    # the same fit through the host library: the better of the run's two initialisations, then mc_locus_bootstrap
    ua, geno = read_fixture(fixture)
    fit = host.Fit(ua, geno, 2, admixture=1, accel_scheme=3, seed=7)
    try:
        ll = [fit.fit_unit(7, u).logL for u in (0, 1)]
        fit.fit_unit(7, 0 if ll[0] >= ll[1] else 1)
        q = fit.get_q(fit.mod.pindex)
        mean, se, count, res = fit.locus_bootstrap(5, 1)
    finally:
        fit.close()
    assert se_lines[0] == ("2", "5", "1", "%.10f" % res.mean_se, "%.10f" % res.max_se, str(res.n_failed))
    assert res.mean_se > 0 and res.n_failed == 0
    want = ["i\tk\teta\tse\tmean\tn"]
    for i in range(q.shape[0]):
        for k in range(2):
            want.append("%d\t%d\t%s\t%s\t%s\t%d" % (i, k, number(q[i, k]), number(se[i, k]), number(mean[i, k]), count[i, k]))
    assert files_se[name].decode().split("\n") == want + [""]


@pytest.mark.parametrize("model", ["shared", "mixture"])
def test_shared_proportions_have_no_individual_column(model, tmp_path):
    args = (["-a", "-c"] if model == "shared" else []) + ["-k", "2", "-s", "3", "-n", "2", "-r", "7"]
    plain, files_plain = run(FIXTURES["structure"], args, tmp_path / "plain")
    with_se, files_se = run(FIXTURES["structure"], args + ["--se", "4", "--se-block", "3"], tmp_path / "se")
    rest, se_lines = split(with_se)
    assert rest == plain and len(se_lines) == 1 and se_lines[0][:3] == ("2", "4", "3")
    name = "stem.%s.K=2.se.txt" % ("admix" if model == "shared" else "mix")
    assert sorted(files_se) == sorted(list(files_plain) + [name])
    assert all(files_se[f] == files_plain[f] for f in files_plain)
    rows = files_se[name].decode().split("\n")
    assert rows[0] == "k\teta\tse\tmean\tn" and len(rows) == 4 and rows[3] == ""
    for k, row in enumerate(rows[1:3]):
        cells = row.split("\t")
        assert cells[0] == str(k) and cells[4] == "4" and float(cells[2]) >= 0 and abs(float(cells[3]) - float(cells[1])) < 0.5


def test_cv_and_se_together(tmp_path):
    args = ["-a", "-1", "1", "-2", "2", "-s", "3", "-n", "2", "-r", "7"]
    plain, files_plain = run(FIXTURES["structure"], args, tmp_path / "plain")
    only_cv, _ = run(FIXTURES["structure"], args + ["--cv", "3"], tmp_path / "cv")
    only_se, _ = run(FIXTURES["structure"], args + ["--se", "5"], tmp_path / "se")
    both, files_both = run(FIXTURES["structure"], args + ["--cv", "3", "--se", "5"], tmp_path / "both")
    marks = [("cv" if CV_LINE.match(ln) else "se") for ln in both if CV_LINE.match(ln) or SE_LINE.match(ln)]
    assert marks == ["cv", "se", "cv", "se"]                    # one pair per K, the CV line first
    for K in (1, 2):
        at = [n for n, ln in enumerate(both) if CV_LINE.match(ln) and CV_LINE.match(ln).group(1) == str(K)][0]
        assert SE_LINE.match(both[at + 1]).group(1) == str(K)
    # each option's line is the line of a run with that option alone, and the rest is the plain run
    assert [ln for ln in both if CV_LINE.match(ln)] == [ln for ln in only_cv if CV_LINE.match(ln)]
    assert [ln for ln in both if SE_LINE.match(ln)] == [ln for ln in only_se if SE_LINE.match(ln)]
    assert [ln for ln in both if not CV_LINE.match(ln) and not SE_LINE.match(ln)] == plain
    assert all(files_both[f] == files_plain[f] for f in files_plain)
    assert sorted(set(files_both) - set(files_plain)) == ["stem.admix.K=1.se.txt", "stem.admix.K=2.se.txt"]
