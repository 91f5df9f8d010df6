"""Divergence of the fitted clusters, without a GPU: the long-double reference (tests/divergence_util.py) against exact rational
arithmetic, the identities that tie its non-negative forms to the textbook ones, float64 restatements of the sums in three
summation orders inside a stated fraction of every bound (the bounds are neither violated by honest arithmetic nor far above it),
mutants the checker has to catch, the host's weights and tables (multiclust_amd/host/mc_diverge.c), and the command line's
refusals."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from cli_util import BIN, ROOT
import divergence_util as du
from multiclust_amd import host

MULTI = os.path.join(ROOT, "tests", "golden", "data", "multi.stru")
F = Fraction


def exact(ua, P, w):
    """every quantity in rationals; pbar is the exact weighted mean"""
    K, T = len(P), len(P[0])
    off = [0]
    for M in ua:
        off.append(off[-1] + M)
    L1 = sum(1 for M in ua if M > 0)
    h = [sum(P[a][c] * (1 - P[a][c]) for c in range(T)) for a in range(K)]
    s = [[sum((P[a][c] - P[b][c]) ** 2 for c in range(T)) for b in range(K)] for a in range(K)]
    pbar = [sum(w[k] * P[k][c] for k in range(K)) for c in range(T)]
    HT = [sum(pbar[c] * (1 - pbar[c]) for c in range(off[l], off[l + 1])) for l in range(len(ua))]
    V = [sum(w[k] * (P[k][c] - pbar[c]) ** 2 for c in range(off[l], off[l + 1]) for k in range(K)) for l in range(len(ua))]
    H = [x / L1 for x in h]
    D = [[x / (2 * L1) for x in row] for row in s]
    return dict(L1=L1, off=off, h=h, s=s, pbar=pbar, HT=HT, V=V, H=H, D=D)


def dyadic_case(seed, K, ua):
    """allele frequencies and weights that are multiples of 2^-10 and sum to 1 exactly: every fma of the chain is exact"""
    rng = np.random.default_rng(seed)

    def simplex(n):
        cuts = np.sort(rng.integers(0, 1025, size=n - 1))
        return np.diff(np.concatenate(([0], cuts, [1024])))
    P = [[] for _ in range(K)]
    for M in ua:
        for k in range(K):
            P[k] += [F(int(x), 1024) for x in simplex(M)] if M else []
    w = [F(int(x), 1024) for x in simplex(K)]
    return P, w


@pytest.mark.parametrize("seed,K,ua", [(1, 1, [2]), (2, 2, [3, 0, 1]), (3, 3, [2, 4, 0, 3, 1]), (4, 5, [1, 1, 6, 0])])
def test_reference_against_rationals_and_the_identities(seed, K, ua):
    P, w = dyadic_case(seed, K, ua)
    ex = exact(ua, P, w)
    Pf, wf = np.array([[float(x) for x in row] for row in P]).reshape(K, -1), np.array([float(x) for x in w])
    for exact_pbar in (False, True):                             # (the chain is exact on these inputs: both forms are the same)
        ref = du.reference(ua, Pf, wf, exact_pbar=exact_pbar)
        tol = 2.0 ** -60

        def close(got, want):
            hi = float(got)                                      # (a long double is two doubles: hi + lo, exactly)
            return abs(F(hi) + F(float(np.longdouble(got) - hi)) - want) <= tol * abs(want)
        assert ref["n_loci"] == ex["L1"]
        for a in range(K):
            assert close(ref["het"][a], ex["h"][a]) and close(ref["H"][a], ex["H"][a])
            for b in range(K):
                assert close(ref["sqdiff"][a, b], ex["s"][a][b]) and close(ref["D"][a, b], ex["D"][a][b])
                den = ex["D"][a][b] + (ex["H"][a] + ex["H"][b]) / 2
                assert np.isnan(ref["F"][a, b]) if den == 0 else close(ref["F"][a, b], ex["D"][a][b] / den)
        for l, M in enumerate(ua):
            assert close(ref["locus_ht"][l], ex["HT"][l]) and close(ref["locus_v"][l], ex["V"][l])
            assert np.isnan(ref["locus_f"][l]) if (M == 0 or ex["HT"][l] == 0) else close(ref["locus_f"][l], ex["V"][l] / ex["HT"][l])
        assert close(ref["sum_v"], sum(ex["V"])) and close(ref["sum_ht"], sum(ex["HT"]))
    # the identities, exactly: V_l = H_T - H_S, and D_ab + (H_a + H_b) / 2 = 1 - sum_c p_a p_b / L1
    off, T = ex["off"], len(P[0])
    for l, M in enumerate(ua):
        cols = range(off[l], off[l + 1])
        if M:
            h_t = 1 - sum(ex["pbar"][c] ** 2 for c in cols)
            h_s = sum(w[k] * (1 - sum(P[k][c] ** 2 for c in cols)) for k in range(K))
            assert ex["V"][l] == h_t - h_s and ex["HT"][l] == h_t
    for a in range(K):
        for b in range(K):
            assert ex["D"][a][b] + (ex["H"][a] + ex["H"][b]) / 2 == 1 - sum(P[a][c] * P[b][c] for c in range(T)) / ex["L1"]


def test_fma_chain_rounds_once_per_step():
    """the chain against its definition on inputs where a product needs more than 53 bits"""
    w = np.array([1 / 3, 1 / 7, 11 / 21])
    P = np.array([[0.1, 1 - 1e-12], [0.7, 1e-12], [1 / 3, 0.5]])
    got = du.fma_chain(w, P)
    for c in range(2):
        acc = F(0)
        for k in range(3):
            acc = F(float(F(float(w[k])) * F(float(P[k, c])) + acc))
        assert got[c] == float(acc)
    # ... and it is not the two-rounding form everywhere: some column of a larger table differs from multiply-then-add
    rng = np.random.default_rng(0)
    w, P = rng.dirichlet(np.ones(8)), rng.random((8, 400))
    two = np.zeros(400)
    for k in range(8):
        two = w[k] * P[k] + two
    assert (du.fma_chain(w, P) != two).any()


CASE_UA = du.shaped_ua(40)


@pytest.mark.parametrize("maker", du.MAKERS, ids=lambda m: m.__name__)
@pytest.mark.parametrize("K", [2, 8])
def test_float64_restatements_sit_inside_the_bounds(maker, K):
    """forward, backward and pairwise float64 sums: every error is at most HALF its bound.  And the bounds are not vacuous: on
    ordinary parameters the sums over all columns come within a factor 2000 of theirs -- n roundings of either sign add up to about
    sqrt(n) / 2 of them, 1 / (2 sqrt(n)) of a bound of n, and n is below 4000 here.  (The special parameter sets have sums that
    float64 gets exactly: V = 0 under weights (0, 1), a twin pair's differences are exact.)"""
    P, w = maker(CASE_UA, K, seed=K)
    worst = {}
    for order in ("forward", "backward", "pairwise"):
        r = du.check(du.restate(CASE_UA, P, w, order=order), CASE_UA, P, w)
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    assert all(v <= 0.5 for v in worst.values()), worst
    if maker is du.ordinary:
        assert K * int(CASE_UA.sum()) < 4000 and all(worst[k] >= 1 / 2000 for k in ("het", "sqdiff", "sum_v", "sum_ht")), worst


def test_mutants_are_caught():
    ua, K = CASE_UA, 4
    # a Gram-difference form of s_ab on the twin clusters: fails the relative bound by orders of magnitude
    P, w = du.twin_clusters(ua, K, seed=1)
    r = du.ratios(du.restate(ua, P, w, mutant="gram"), ua, P, w)
    assert r["sqdiff"] > 1e6 and all(v <= 1 for k, v in r.items() if k != "sqdiff"), r
    du.check(du.restate(ua, P, w), ua, P, w)
    P, w = du.ordinary(ua, K, seed=2)
    # the phantom column dropped
    r = du.ratios(du.restate(ua, P, w, mutant="no_phantom"), ua, P, w)
    assert min(r["het"], r["sqdiff"], r["locus_v"], r["locus_ht"], r["sum_v"], r["sum_ht"]) > 1e6, r
    # L instead of L1 (the case has two loci without a column)
    assert (ua == 0).sum() == 2
    r = du.ratios(du.restate(ua, P, w, mutant="all_loci"), ua, P, w)
    assert r["shape"] == np.inf and all(v <= 1 for k, v in r.items() if k != "shape"), r
    # unweighted pbar
    r = du.ratios(du.restate(ua, P, w, mutant="unweighted"), ua, P, w)
    assert min(r["locus_v"], r["locus_v_exact"], r["locus_ht"], r["sum_v"], r["sum_ht"]) > 1e6 and max(r["het"], r["sqdiff"]) <= 1, r
    with pytest.raises(AssertionError):
        du.check(du.restate(ua, P, w, mutant="unweighted"), ua, P, w)


def test_nan_where_the_definition_says():
    """F_l: a locus without a column, and a locus where every cluster is fixed on one allele; F_ab: two clusters fixed everywhere"""
    ua = np.array([2, 0, 2], dtype=np.int32)
    P = np.array([[1.0, 0.0, 0.5, 0.5], [1.0, 0.0, 0.25, 0.75]])
    ref = du.reference(ua, P, np.array([0.5, 0.5]))
    assert np.isnan(ref["locus_f"][:2]).all() and ref["locus_f"][2] > 0 and ref["n_loci"] == 2
    fixed = np.array([[1.0, 0.0], [1.0, 0.0]])
    ref = du.reference(np.array([2]), fixed, np.array([0.5, 0.5]))
    assert np.isnan(ref["F"]).all() and np.isnan(ref["f_all"])
    H, D, Fm, (n, mean, lo, hi) = host.divergence_tables(np.zeros(2), np.zeros((2, 2)), 1)
    assert np.isnan(Fm).all() and n == 0 and np.isnan([mean, lo, hi]).all() and not H.any() and not D.any()


def test_host_weights_and_tables():
    rng = np.random.default_rng(5)
    K, I = 4, 9
    q = rng.dirichlet(np.ones(K), size=I)
    q[2] = np.nan
    q[7, 1] = np.nan
    w = host.divergence_weights(q, K)
    assert np.array_equal(w, du.weights_from_q(q, K)) and abs(w.sum() - 1) < 1e-15
    assert np.allclose(w, np.delete(q, [2, 7], axis=0).mean(axis=0), rtol=1e-15)
    assert np.array_equal(host.divergence_weights(np.full((I, K), np.nan), K), np.full(K, 0.25))
    eta = rng.dirichlet(np.ones(K))
    assert np.array_equal(host.divergence_weights(eta, K), eta)                  # shared proportions and the mixture model: eta itself
    ua = du.shaped_ua(12)
    P, _ = du.ordinary(ua, K, seed=6)
    ref = du.reference(ua, P, w)
    sums = du.restate(ua, P, w)
    H, D, Fm, (n, mean, lo, hi) = host.divergence_tables(sums["het"], sums["sqdiff"], sums["n_loci"])
    tol = du.derived_bound(ref["T"])
    assert (np.abs(H - ref["H"]) <= tol * ref["H"]).all() and (np.abs(D - ref["D"]) <= tol * ref["D"]).all()
    assert (np.abs(Fm - ref["F"]) <= tol * ref["F"]).all() and not np.diag(Fm).any()
    pairs = Fm[np.triu_indices(K, 1)]
    assert n == K * (K - 1) // 2 and lo == pairs.min() and hi == pairs.max() and abs(mean - pairs.mean()) <= 4 * du.U * mean


# ---- the command line ----
@pytest.mark.parametrize("args", [
    ["-a", "-k", "2", "--fst", "-b", "2"],
    ["-k", "2", "--fst", "-b", "2"],                          # either model
    ["-a", "-k", "2", "--fst", "-w", "n", "2"],
    ["-a", "-k", "2", "--fst", "-M"],
    ["-a", "-c", "-k", "2", "--fst", "--gpus", "2"],
    ["-a", "-k", "2", "--fs"],                                # in full: a shorter word is -f without its file name
])
def test_refused_combinations(args, tmp_path):
    res = subprocess.run([BIN, "-f", MULTI] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, cwd=str(tmp_path))
    assert res.returncode == 10, (args, res.returncode, res.stderr[-500:])
    assert "ERROR [mc_main.c::parse_options]" in res.stderr
    if "--fst" in args:
        assert "--fst cannot be combined" in res.stderr


def test_longer_words_are_still_the_data_file(tmp_path):
    """--fstx is not --fst: like every other word that starts with f (but --fill, --fst and --fo...) it names the data file"""
    res = subprocess.run([BIN, "-a", "-k", "2", "--fstx", "/nonexistent/data.stru"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         timeout=60, cwd=str(tmp_path))
    assert res.returncode == 5 and "/nonexistent/data.stru" in res.stderr
    usage = subprocess.run([BIN, "-h"], stdout=subprocess.PIPE, text=True, timeout=60).stdout
    assert "--fst " in usage and "Divergence (K=..)" in usage
