"""-m gpu: --resid on the command line.  Nothing but its own line and its two files depends on it -- STRUCTURE and PLINK input,
individual and shared mixing proportions, --streams 2, together with --fst, --cv, --se and --fill --; the line and the files say what
tests/resid_util.py computes from the Q and P files written beside them, to the digits those carry; with --query the query
individuals' rows and columns are NaN; and every refusal has its exit status and message.

Each run of the program is made once per module and shared by the tests that read it.

To the printed digits: etaik / etak and pklm carry six decimals, so every q and p read back is within eps = 5.1e-7 of the number the
program used.  That moves t = sum_k q_k p_k by (K + 1) eps at most and a residual by dr = ploidy (K + 1) eps; G_ij by at most
dr (|r_i|_1 + |r_j|_1) and D_ij by 2 dr |r_i|_1, where |r_i|_1 <= sqrt(T D_i); so cor_ij = G_ij / sqrt(D_ij D_ji) moves by at most
dr sqrt(T) (1 / sqrt(D_ij) + 1 / sqrt(D_ji)) (1 + |cor_ij|), second-order terms covered by a factor 1.5.  The program's own figures
carry six decimals."""
import re
import subprocess

import numpy as np
import pytest

from cli_util import BIN, clustered_codes, fit_inputs, Runs, written_fit
import resid_util as ru
from multiclust_amd import host

pytestmark = pytest.mark.gpu
NUM = r"(-?\d+\.\d+)"
LINE = re.compile(r"^Residual correlation \(K=(\d+)\): mean " + NUM + r" mean \|r\| " + NUM + " max " + NUM +
                  r" \((\d+), (\d+)\) over (\d+) pairs$")
I, L, CLUSTERS, K = 72, 400, 3, 3
ARGS = ["-s", "3", "-n", "2", "-r", "7", "-k", "3"]
EPS, P6 = 5.1e-7, 5.1e-7
OWN = ["stem.admix.K=3.resid.txt", "stem.admix.K=3.resid.ind.txt"]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    inputs = fit_inputs(tmp_path_factory, "resid_in", clustered_codes(I, L, CLUSTERS))
    return dict(inputs, runs=Runs(lambda: tmp_path_factory.mktemp("resid_out"), own="Residual"))


def run(inputs, args, bed=False):
    """one run of the program per distinct command line: (other stdout lines, the matches of the Residual lines, files)"""
    others, own, files = inputs["runs"]((["--bed", inputs["bed"]] if bed else ["-f", inputs["stru"]]) + list(args))
    return others, [LINE.match(ln) for ln in own], files


FORMS = {"admix": ["-a"], "shared": ["-a", "-c"]}


@pytest.mark.parametrize("name,extra,bed", [
    ("admix", [], False), ("admix", [], True), ("shared", [], False), ("admix", ["--streams", "2"], False),
    ("admix", ["--fst", "--cv", "2"], False), ("admix", ["--se", "2", "--fill"], False)])
def test_nothing_else_changes(name, extra, bed, inputs):
    args = FORMS[name] + ARGS + extra
    lines0, own0, files0 = run(inputs, args, bed)
    lines1, own1, files1 = run(inputs, args + ["--resid"], bed)
    assert own0 == [] and len(own1) == 1 and own1[0] is not None and lines0 == lines1
    assert sorted(files1) == sorted(list(files0) + OWN) and len(files0) >= 5
    for f in files0:
        assert files0[f] == files1[f], f
    if extra or bed:                                             # ... and --resid says what it says without the other analyses, from either input
        _, own2, files2 = run(inputs, FORMS[name] + ARGS + ["--resid"])
        assert own2[0].groups() == own1[0].groups() and all(files2[f] == files1[f] for f in OWN)


def own_files(files):
    """(cor [I][I], per individual: mean, max, partner) as --resid wrote them"""
    text = files[OWN[0]].decode().split("\n")
    assert text[-1] == "" and len(text) == I + 1
    cor = np.array([[float(x) for x in ln.split("\t")] for ln in text[:-1]])
    assert cor.shape == (I, I) and b"nan" not in files[OWN[0]]
    ind = files[OWN[1]].decode().split("\n")
    assert ind[0] == "i\tmean\tmax\tpartner" and ind[-1] == ""
    rows = [ln.split("\t") for ln in ind[1:-1]]
    assert [int(r[0]) for r in rows] == list(range(I))
    return cor, np.array([float(r[1]) for r in rows]), np.array([float(r[2]) for r in rows]), np.array([int(r[3]) for r in rows])


def agree_with_the_written_fit(inputs, args, query_rows=()):
    ua, geno = inputs["ua"], inputs["geno"].copy()
    _, own, files = run(inputs, args)
    T = int(ua.sum())
    q, P = written_fit(files, ua, I, K)
    if q.ndim == 2:
        assert np.flatnonzero(np.isnan(q).any(axis=1)).tolist() == list(query_rows)
        q[list(query_rows)] = 1.0 / K                             # hidden from the fit: no observed copy on the device, any finite row serves
    geno[list(query_rows)] = ru.MISSING
    ref = ru.reference(ua, geno, q, P)
    cor, mean, big, partner = own_files(files)
    want = ref["cor"].astype(np.float64)
    nan = np.isnan(want)
    expect = np.eye(I, dtype=bool)
    expect[list(query_rows), :] = True
    expect[:, list(query_rows)] = True
    assert np.array_equal(nan, expect) and np.array_equal(np.isnan(cor), nan) and np.array_equal(cor, cor.T, equal_nan=True)
    dr = geno.shape[2] * (K + 1) * EPS
    D = ref["D"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        tol = 1.5 * dr * np.sqrt(T) * (1 / np.sqrt(D) + 1 / np.sqrt(D.T)) * (1 + np.abs(want)) + P6
    err = np.abs(cor - want)[~nan]
    print("largest |cor - reference| %.3g, its tolerance %.3g" % (err.max(), tol[~nan][err.argmax()]))
    assert (err <= tol[~nan]).all()
    # the per-individual file and the line are summaries of the matrix in the file
    fin = ~nan
    for i in range(I):
        if not fin[i].any():
            assert np.isnan(mean[i]) and np.isnan(big[i]) and partner[i] == -1
            continue
        row = cor[i][fin[i]]
        assert abs(mean[i] - row.mean()) <= 2 * P6 and abs(big[i] - row.max()) <= P6 and abs(cor[i, partner[i]] - row.max()) <= P6
    g = own[0].groups()
    iu = np.triu_indices(I, 1)
    pairs = cor[iu][fin[iu]]
    assert int(g[0]) == K and int(g[6]) == pairs.size == (I - len(query_rows)) * (I - len(query_rows) - 1) // 2
    assert abs(float(g[1]) - pairs.mean()) <= 2 * P6 and abs(float(g[2]) - np.abs(pairs).mean()) <= 2 * P6
    assert abs(float(g[3]) - pairs.max()) <= P6 and int(g[4]) < int(g[5]) and abs(cor[int(g[4]), int(g[5])] - pairs.max()) <= P6
    return cor, ref


@pytest.mark.parametrize("name", ["admix", "shared"])
def test_line_and_files_agree_with_the_written_fit(name, inputs):
    cor, ref = agree_with_the_written_fit(inputs, FORMS[name] + ARGS + ["--resid"])
    if name == "admix":                                          # the right K on clustered data: the negative baseline, no block
        z = np.arange(I) % CLUSTERS
        same = cor[(z[:, None] == z[None, :]) & ~np.eye(I, dtype=bool)]
        assert -2.0 * CLUSTERS / I <= same.mean() <= 0.0


def test_with_query_individuals_their_rows_are_nan(inputs):
    rows = [i for i in range(I) if i % 9 == 4]
    args = ["-a"] + ARGS + ["--query", inputs["query"], "--resid"]
    agree_with_the_written_fit(inputs, args, query_rows=rows)
    assert "stem.admix.K=3.query.txt" in run(inputs, args)[2]
    lines0, _, files0 = run(inputs, ["-a"] + ARGS + ["--query", inputs["query"]])
    lines1, _, files1 = run(inputs, args)
    assert lines0 == lines1 and all(files0[f] == files1[f] for f in files0) and sorted(files1) == sorted(list(files0) + OWN)


def test_the_line_equals_the_library_on_the_same_fit(inputs):
    _, own, _ = run(inputs, ["-a"] + ARGS + ["--resid"])
    fit = host.Fit(inputs["ua"], inputs["geno"], K, admixture=1, accel_scheme=3, seed=7)
    try:
        ll = [fit.fit_unit(7, u).logL for u in (0, 1)]
        fit.fit_unit(7, 0 if ll[0] >= ll[1] else 1)
        r = fit.residual_correlation()
    finally:
        fit.close()
    assert own[0].groups() == ("3", "%.6f" % r["mean"], "%.6f" % r["mean_abs"], "%.6f" % r["max"], "%d" % r["max_pair"][0],
                               "%d" % r["max_pair"][1], "%d" % r["n_pairs"])


@pytest.mark.parametrize("args,why", [
    (["-k", "2", "--resid"], "--resid needs the admixture model (-a)"),
    (["-a", "-k", "2", "--resid", "-b", "2"], "--resid cannot be combined with the bootstrap (-b)"),
    (["-a", "-k", "2", "--resid", "-w", "n", "2"], "--resid cannot be combined with -w or -M"),
    (["-a", "-k", "2", "--resid", "-M"], "--resid cannot be combined with -w or -M"),
    (["-a", "-k", "2", "--resid", "--gpus", "2"], "--resid cannot be combined with --gpus above 1"),
])
def test_refusals(args, why, inputs, tmp_path):
    res = subprocess.run([BIN, "-f", inputs["stru"]] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60,
                         cwd=str(tmp_path))
    assert res.returncode == 10, (args, res.returncode, res.stderr[-500:])
    assert "ERROR [mc_main.c::parse_options]: " + why + " (argument '--resid')" in res.stderr


def test_a_seed_is_still_a_seed(inputs):
    """-r takes its number as before; only the whole word --resid is the new option"""
    lines0, _, _ = run(inputs, ["-a"] + ARGS)
    lines1, _, _ = run(inputs, ["-a", "-s", "3", "-n", "2", "-k", "3", "-r", "7"])
    assert lines0 == lines1
