"""Query individuals (--query), the part that needs no GPU: the numpy restatement of mchip_fit_q_rows against itself in a wider
float type on the GPU tests' own inputs, the query-file reader, and the command line's usage errors."""
import os
import subprocess

import numpy as np
import pytest

from cli_util import BIN, ROOT
import query_util as qu
from multiclust_amd import host

MULTI = os.path.join(ROOT, "tests", "golden", "data", "multi.stru")      # 40 diploid individuals
I_MULTI = 40


# ---- the restatement: its float64 trajectory is the reference the GPU is held to, so its own rounding must be far below the
# GPU tolerance.  1 / 16 of it, along the whole trajectory.
@pytest.mark.parametrize("name", qu.CASE_NAMES)
def test_float64_restatement_against_longdouble(name):
    assert np.finfo(np.longdouble).eps < 2.0 ** -60, "this platform's long double is no wider than double"
    ua, geno, _, p = qu.case(name)
    K = p.shape[0]
    tol = qu.q_tolerance(qu.copies_per_row(geno), K) / 16
    worst = 0.0
    for updates in (1, 5, 20, 100):
        q64, _, n64, _, _ = qu.fit_rows(ua, geno, p, range(qu.I_ROWS), updates, lb=qu.LOWER_BOUND)
        q80, _, n80, _, _ = qu.fit_rows(ua, geno, p, range(qu.I_ROWS), updates, lb=qu.LOWER_BOUND, dtype=np.longdouble)
        assert (n64 == n80).all() and (n64 == np.where(qu.copies_per_row(geno) > 0, updates, 0)).all()
        diff = np.abs(q64 - q80).max(axis=1)
        worst = max(worst, float((diff / tol).max()))
        print("%s: %d updates: largest difference %.3g, smallest bound %.3g" % (name, updates, diff.max(), tol.min()))
        assert (diff <= tol).all(), (name, updates, diff, tol)
    print("%s: largest difference / bound = %.3g" % (name, worst))


def test_restatement_special_rows_and_stopping():
    ua, geno, q, p = qu.case("k3")
    K = 3
    empty = qu.fit_row(ua, geno[0], p, q[0], 7)
    assert empty["copies"] == 0 and (empty["q"] == 1.0 / K).all() and (empty["logL"], empty["n"], empty["converged"]) == (0.0, 0, 0)
    single = qu.fit_row(ua, geno[1], p, None, 3)
    assert single["copies"] == 1 and single["n"] == 3 and abs(single["q"].sum() - 1) < 1e-12
    # a copy whose allele has frequency 0 everywhere: log 0 at the first evaluation
    pz = p.copy()
    pz[:, qu.row_columns(ua, geno[2])[0]] = 0.0
    bad = qu.fit_row(ua, geno[2], pz, None, 5, do_projection=False)
    assert np.isnan(bad["q"]).all() and bad["logL"] == -np.inf and (bad["n"], bad["converged"]) == (0, 0)
    # no test made: the loop runs to its cap and is not converged; a test made stops it earlier, converged
    cap = qu.fit_row(ua, geno[2], p, None, 30)
    assert (cap["n"], cap["converged"]) == (30, 0)
    for kw in (dict(abs_error=1e-6), dict(rel_error=1e-9), dict(abs_error=1e-3, rel_error=1e-9)):
        r = qu.fit_row(ua, geno[2], p, None, 100000, **kw)
        assert r["converged"] == 1 and 1 <= r["n"] < 100000
        d, prev = r["deltas"][-1], r["prevs"][-1]
        assert all(x > kw.get("abs_error", np.inf) or x / abs(y) > kw.get("rel_error", np.inf) for x, y in zip(r["deltas"][:-1], r["prevs"][:-1]))
        assert d <= kw.get("abs_error", np.inf) and d / abs(prev) <= kw.get("rel_error", np.inf)


def test_michelot_restatement_against_the_oracle():
    import oracle_bind as ob
    rng = np.random.default_rng(3)
    for K in (1, 2, 5, 64):
        for _ in range(20):
            x = rng.dirichlet(np.ones(K)) + rng.normal(0, 0.05, K)
            np.testing.assert_array_equal(qu.michelot(x, 1e-3), ob.michelot(x.copy(), 1e-3))


# ---- the query file
def write(path, text):
    path.write_text(text)
    return str(path)


def test_query_file_reader(tmp_path):
    rc, mask = host.query_read(write(tmp_path / "good.txt", "0 1\n0\t0 1\n\n1 0\n"), 7)
    assert rc == 0 and mask.tolist() == [0, 1, 0, 0, 1, 1, 0]
    assert host.query_read(write(tmp_path / "short.txt", "0 1 0 1"), 5) == (7, None)
    assert host.query_read(write(tmp_path / "long.txt", "0 1 0 1 0 1"), 5) == (7, None)
    assert host.query_read(write(tmp_path / "two.txt", "0 1 2 1 0"), 5) == (7, None)
    assert host.query_read(write(tmp_path / "word.txt", "0 1 01 1 0"), 5) == (7, None)
    assert host.query_read(write(tmp_path / "minus.txt", "0 1 -1 1 0"), 5) == (7, None)
    assert host.query_read(write(tmp_path / "panel.txt", "0 0 0 0 0"), 5) == (7, None)
    assert host.query_read(write(tmp_path / "query.txt", "1 1 1 1 1"), 5) == (7, None)
    assert host.query_read(str(tmp_path / "missing.txt"), 5) == (5, None)


# ---- the command line: what --query cannot be combined with is a usage error (status 10), found before any GPU is needed
def run(args, cwd):
    return subprocess.run([BIN] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, cwd=str(cwd))


@pytest.fixture
def qfile(tmp_path):
    return write(tmp_path / "query.txt", " ".join("1" if i % 5 == 0 else "0" for i in range(I_MULTI)))


EXCLUDED = [
    ([], "-a"),                                  # the mixture model
    (["-a", "-c"], "-c"), (["-a", "-b", "2"], "-b"), (["-a", "-w", "n", "2"], "-w"), (["-a", "-M"], "-M"),
    (["-a", "-A", "partition.txt"], "-A"), (["-a", "--cv", "5"], "--cv"), (["-a", "--se", "10"], "--se"),
    (["-a", "--randem"], "--randem"), (["-a", "--gpus", "2"], "--gpus"), (["-a", "--streams", "2"], "--streams"),
]


@pytest.mark.parametrize("extra,word", EXCLUDED, ids=[w for _, w in EXCLUDED])
def test_query_usage_errors(extra, word, qfile, tmp_path):
    for args in (["-f", MULTI, "-k", "2", "--query", qfile] + extra, ["-f", MULTI, "-k", "2"] + extra + ["--query", qfile]):
        res = run(args, tmp_path)
        assert res.returncode == 10, (args, res.returncode, res.stderr[-500:])
        assert "--query" in res.stderr and word in res.stderr and res.stdout == ""


def test_query_argument_and_file_errors(qfile, tmp_path):
    assert run(["-f", MULTI, "-a", "-k", "2", "--query"], tmp_path).returncode == 10          # no file name
    assert run(["-f", MULTI, "-a", "-k", "2", "-q", qfile], tmp_path).returncode == 9         # only the word --query is an option
    assert run(["-f", MULTI, "-a", "-k", "2", "--query", str(tmp_path / "none.txt")], tmp_path).returncode == 5
    assert run(["-f", MULTI, "-a", "-k", "2", "--query", write(tmp_path / "short.txt", "0 1 0")], tmp_path).returncode == 7
    assert run(["-f", MULTI, "-a", "-k", "2", "--query", write(tmp_path / "all.txt", "1 " * I_MULTI)], tmp_path).returncode == 7
    # a good query file passes the parser and the reader: the next check (more clusters than individuals) answers
    assert run(["-f", MULTI, "-a", "-k", "200", "--query", qfile], tmp_path).returncode == 11


@pytest.mark.parametrize("word", ["--projection", "--proj", "--pr"])
def test_projection_still_parses_as_before(word, qfile, tmp_path):
    """every --pr... word switches the simplex projection off and takes no argument: the word behind it is parsed as an option"""
    assert run(["-f", MULTI, "-a", word, "-k", "200"], tmp_path).returncode == 11
    assert run(["-f", MULTI, "-a", word, "-Z"], tmp_path).returncode == 9
    assert run(["-f", MULTI, "-a", word, "--query", qfile, "-k", "200"], tmp_path).returncode == 11
