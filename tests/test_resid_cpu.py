"""The residual correlation on the CPU (no GPU): the long-double reference of tests/resid_util.py against exact rationals, float64
restatements of the sums in three summation orders inside half of every bound, the mutants the checker has to catch, the host's
ratios and summary (multiclust_amd/host/mc_resid.c; also as a program of its own under the sanitizers), and -- with the oracle's
fit -- that the definition has teeth: a duplicated individual stands out, and a K that is too small shows as positive correlation
where the right K shows the negative baseline.

The teeth, sized here (I, L and the seeds below; the figures are printed):
  duplicate    120 individuals of 3 clusters at 1200 biallelic loci and a copy of individual 0 as individual 120, fitted with K = 3.
               The copy has its original's genotype and, to the fit's tolerance, its mixing proportions: their residuals coincide
               and the correlation is 1 but for that tolerance.  The other members of the cluster: the pair weighs twice in the
               cluster's frequencies, so the baseline is about -2 / 41, and the scatter of a correlation over 2400 columns, most
               of them nearly fixed, a few hundredths (measured: between -0.13 and 0.03; at 60 individuals and 400 loci the
               scatter alone reached 0.29).
  K too small  90 individuals of 3 clusters at 400 loci.  K = 2 puts two of the clusters into one fitted cluster: the members of one
               true cluster then miss the merged frequencies the same way, a positive correlation of the order of the F_ST between
               the two; with K = 3 the same pairs have the baseline, about -1 / 30."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from cli_util import BIN, ROOT
import cv_util as cu
import host_driver
import resid_util as ru
from multiclust_amd import host

MULTI = os.path.join(ROOT, "tests", "golden", "data", "multi.stru")


def frac(x):
    """a long double as the rational it is (its upper 53 bits and the rest)"""
    hi = float(x)
    return Fraction(hi) + Fraction(float(x - np.longdouble(hi)))


def small_case(seed, I=5, ploidy=2, K=3, missing=0.2, shared=False):
    ua = np.array([2, 3, 0, 1, 4, 2], dtype=np.int32)
    geno = ru.genotypes(ua, I, ploidy, seed, missing)
    geno[1, 1] = ru.MISSING                                     # a genotype without a copy, and one with a copy missing
    geno[2, 0, 0], geno[2, 0, 1:] = ru.MISSING, 1
    Q, P = ru.parameters(ua, I, K, seed)
    return ua, geno, (Q[0] if shared else Q), P


@pytest.mark.parametrize("seed,ploidy,K,shared", [(1, 2, 3, False), (2, 1, 1, False), (3, 4, 2, True), (4, 2, 5, False)])
def test_reference_against_exact_rationals(seed, ploidy, K, shared):
    ua, geno, Q, P = small_case(seed, ploidy=ploidy, K=K, shared=shared)
    ref = ru.reference(ua, geno, Q, P)
    r, G, D = ru.exact(ua, geno, Q, P)
    I, T = ref["I"], ref["T"]
    tol = 2.0 ** -60                                            # long double: 64 bits; a few operations each
    for i in range(I):
        for c in range(T):
            assert abs(frac(ref["r"][i, c]) - r[i][c]) <= tol * (1 + abs(r[i][c]))
        for j in range(I):
            assert abs(frac(ref["G"][i, j]) - G[i][j]) <= 2.0 ** -56 * sum(abs(r[i][c] * r[j][c]) for c in range(T)) + tol
            assert abs(frac(ref["D"][i, j]) - D[i][j]) <= 2.0 ** -56 * D[i][j] + tol
    # the residual the device forms, bit for bit by its definition, lies within e of the exact one; 0 where the genotype has no copy
    dev = ru.device_residuals(ua, geno, Q, P)
    cl = ru.col_locus(ua)
    for i in range(I):
        for c in range(T):
            assert abs(Fraction(float(dev[i, c])) - r[i][c]) <= frac(ref["e"][i, c])
            if ref["a"][i, cl[c]] == 0:
                assert dev[i, c] == 0.0 and r[i][c] == 0
    assert (ref["a"] == 0).any() and ((ref["a"] > 0) & (ref["a"] < ploidy)).any() or ploidy == 1
    # D_ij is G_ii over the loci where j has data: equal where j has a copy everywhere, smaller where i has residuals j lacks
    full = [j for j in range(I) if all(ref["a"][j, l] > 0 for l in range(len(ua)) if ua[l] > 0)]
    for j in full:
        assert all(D[i][j] == G[i][i] for i in range(I))
    assert any(D[i][j] < G[i][i] for i in range(I) for j in range(I))


@pytest.mark.parametrize("order", ["forward", "backward", "mfma"])
@pytest.mark.parametrize("missing", [0.0, 0.2])
def test_float64_restatements_stay_within_half_of_every_bound(order, missing):
    ua = np.array([2] * 30 + [3, 0 if missing else 2, 5, 1] + [2] * 31, dtype=np.int32)   # (a locus without a column is all missing)
    I, K = 9, 3
    geno = ru.genotypes(ua, I, 2, seed=11, missing=missing)
    if missing:
        geno[4] = ru.MISSING                                    # an individual without a copy
    Q, P = ru.parameters(ua, I, K, seed=11)
    ref = ru.reference(ua, geno, Q, P)
    G, D = ru.restate(ua, geno, Q, P, order)
    r = ru.check(G, D, ref, limit=0.5)
    print(order, missing, r)
    assert ref["no_missing"] == (missing == 0.0)


@pytest.fixture(scope="module")
def mutant_case():
    ua, geno = ru.biallelic(7, 120, seed=3, missing=0.03)         # a few genotypes lack one copy, 20 % lack both
    geno[np.random.default_rng(4).random(geno.shape[:2]) < 0.2] = ru.MISSING
    Q, P = ru.parameters(ua, 7, 3, seed=3)
    return ua, geno, Q, P, ru.reference(ua, geno, Q, P), ru.device_residuals(ua, geno, Q, P)


def test_the_checker_passes_the_unmutated_restatement(mutant_case):
    ua, geno, Q, P, ref, r = mutant_case
    ru.check(*ru.restate(ua, geno, Q, P, r=r), ref)
    ru.check(ru.restate(ua, geno, Q, P, r=r)[0], None, ref)


@pytest.mark.parametrize("mutant,group", [("diag_norms", "norms"), ("ploidy", "gram"), ("drop_chunk", "gram"), ("transposed", "norms")])
def test_mutants_are_caught(mutant, group, mutant_case):
    ua, geno, Q, P, ref, r = mutant_case
    G, D = ru.restate(ua, geno, Q, P, mutant=mutant, r=r, chunk=16)
    got = ru.ratios(G, D, ref)
    print(mutant, got)
    assert got[group] > 1e6
    with pytest.raises(AssertionError):
        ru.check(G, D, ref)
    if mutant == "diag_norms":                                   # ... and what it does to the correlations: they shrink by about the missing rate
        good = ru.correlation(*ru.restate(ua, geno, Q, P, r=r))
        shrunk = ru.correlation(G, D)
        ok = np.isfinite(good) & (np.abs(good) > 0.05)
        ratio = shrunk[ok] / good[ok]
        assert ok.sum() >= 10 and 0.7 <= ratio.mean() <= 0.9 and (ratio < 1).all()


def test_an_asymmetric_gram_fails_the_shape_check(mutant_case):
    ua, geno, Q, P, ref, r = mutant_case
    G, D = ru.restate(ua, geno, Q, P, r=r)
    G[1, 2] = np.nextafter(G[1, 2], 1)
    assert ru.ratios(G, D, ref)["shape"] == np.inf and ru.ratios(G, D, ref)["gram"] <= 1


# ---- the host's ratios and summary ----
def test_host_ratios_and_summary(mutant_case):
    ua, geno, Q, P, ref, r = mutant_case
    G, D = ru.restate(ua, geno, Q, P, r=r)
    D[3, :] = 0.0                                                # individual 3 as one without an observed copy: its row of D is 0
    G[3, :] = G[:, 3] = 0.0
    cor = host.residual_ratios(G, D)
    want = ru.correlation(G, D)
    assert np.array_equal(cor, want, equal_nan=True) and np.array_equal(cor, cor.T, equal_nan=True)
    assert np.isnan(cor[3]).all() and np.isnan(cor[:, 3]).all() and np.isnan(np.diag(cor)).all()
    fin = np.isfinite(cor)
    assert fin.sum() == 6 * 5
    s = host.residual_summary(cor)
    iu = np.triu_indices(7, 1)
    pairs = cor[iu][fin[iu]]
    assert s["n_pairs"] == 15 and abs(s["mean"] - pairs.mean()) <= 1e-15 and abs(s["mean_abs"] - np.abs(pairs).mean()) <= 1e-15
    assert s["max"] == pairs.max() and cor[s["max_pair"]] == pairs.max() and s["max_pair"][0] < s["max_pair"][1]
    assert np.isnan(s["ind_mean"][3]) and np.isnan(s["ind_max"][3]) and s["ind_partner"][3] == -1
    for i in (0, 6):
        row = cor[i][fin[i]]
        assert abs(s["ind_mean"][i] - row.mean()) <= 1e-15 and s["ind_max"][i] == row.max() and cor[i, s["ind_partner"][i]] == row.max()
    none = host.residual_summary(np.full((3, 3), np.nan))
    assert none["n_pairs"] == 0 and np.isnan(none["mean"]) and np.isnan(none["max"]) and none["max_pair"] == (-1, -1)


# ---- the definition has teeth: with the oracle's fit ----
def oracle_fit(ua, geno, K, seed=7):
    import oracle_bind as ob
    I, L, pl = geno.shape
    mod = ob.Model(ob.Data(I, L, pl, ua, geno), ob.make_options(accel_scheme=3), K)
    mod.init_random(seed)
    mod.em()
    assert mod.fatal == 0
    return mod.q(mod.pindex).copy(), mod.p(mod.pindex).copy()


def test_a_duplicated_individual_stands_out():
    I, L, clusters = 120, 1200, 3
    ua, geno = cu.clustered_dataset(I, L, clusters, 21)
    geno = np.concatenate((geno, geno[:1]))                      # individual 60 = individual 0
    q, p = oracle_fit(ua, geno, clusters)
    cor = ru.reference(ua, geno, q, p)["cor"].astype(np.float64)
    mates = [i for i in range(1, I) if i % clusters == 0]
    print("duplicate %.4f; its cluster: min %.4f max %.4f mean %.4f" % (cor[0, I], cor[0, mates].min(), cor[0, mates].max(),
                                                                          cor[0, mates].mean()))
    assert cor[0, I] > 0.9 and cor[I, 0] == cor[0, I]
    assert (np.abs(cor[0, mates]) <= 0.2).all() and (np.abs(cor[I, mates]) <= 0.2).all()


def test_a_k_that_is_too_small_shows_and_the_right_k_does_not():
    I, L, clusters = 90, 400, 3
    ua, geno = cu.clustered_dataset(I, L, clusters, 22)
    z = np.arange(I) % clusters
    q2, p2 = oracle_fit(ua, geno, 2)
    q3, p3 = oracle_fit(ua, geno, 3)
    home = [int(q2[z == g].mean(axis=0).argmax()) for g in range(clusters)]
    merged = [g for g in range(clusters) if home.count(home[g]) >= 2]
    assert len(merged) >= 2, home
    same = [(i, j) for i in range(I) for j in range(i + 1, I) if z[i] == z[j] and z[i] in merged]
    ii, jj = np.array(same).T
    c2 = ru.reference(ua, geno, q2, p2)["cor"].astype(np.float64)[ii, jj]
    c3 = ru.reference(ua, geno, q3, p3)["cor"].astype(np.float64)[ii, jj]
    n_c = I // clusters
    print("merged clusters %s: K = 2 mean %.4f, K = 3 mean %.4f (baseline -1 / %d = %.4f)" % (merged, c2.mean(), c3.mean(), n_c, -1.0 / n_c))
    assert c2.mean() > 0.05
    assert -2.0 / n_c <= c3.mean() <= 0.0


# ---- the command line ----
@pytest.mark.parametrize("args,why", [
    (["-k", "2", "--resid"], "--resid needs the admixture model (-a)"),
    (["-a", "-k", "2", "--resid", "-b", "2"], "--resid cannot be combined with the bootstrap (-b)"),
    (["-a", "-k", "2", "--resid", "-w", "n", "2"], "--resid cannot be combined with -w or -M"),
    (["-a", "-k", "2", "--resid", "-M"], "--resid cannot be combined with -w or -M"),
    (["-a", "-k", "2", "--resid", "--gpus", "2"], "--resid cannot be combined with --gpus above 1"),
])
def test_refused_combinations(args, why, tmp_path):
    res = subprocess.run([BIN, "-f", MULTI] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, cwd=str(tmp_path))
    assert res.returncode == 10, (args, res.returncode, res.stderr[-500:])
    assert "ERROR [mc_main.c::parse_options]: " + why + " (argument '--resid')" in res.stderr


# ---- mc_resid.c under AddressSanitizer + UBSan, as a program of its own (the device entry point stubbed) ----
@pytest.mark.parametrize("n", [1, 2, 7])
def test_host_code_is_sanitizer_clean(n, tmp_path):
    exe = host_driver.build(tmp_path, "resid_host", ["tests/resid_host_driver.c", "multiclust_amd/host/mc_resid.c"], werror=True)
    res = host_driver.run(exe, [n, tmp_path / "stem"], cwd=tmp_path)
    assert "wrote 0" in res.stdout
    line = res.stdout.split("\n")[0]
    rows = open(str(tmp_path / "stem.admix.K=2.resid.txt")).read().split("\n")
    ind = open(str(tmp_path / "stem.admix.K=2.resid.ind.txt")).read().split("\n")
    assert len(rows) == n + 1 and all(len(r.split("\t")) == n for r in rows[:-1]) and len(ind) == n + 2
    if n == 7:                                                   # individual 1 has no data: 6 others, 15 pairs
        cor = np.array([[float(x) for x in r.split("\t")] for r in rows[:-1]])
        assert np.isnan(cor[1]).all() and np.isnan(cor[:, 1]).all() and np.isfinite(cor).sum() == 30
        assert line.startswith("Residual correlation (K=2): mean ") and line.endswith(" over 15 pairs")
        assert ind[2] == "1\tNaN\tNaN\t-1"
    else:
        assert line == "Residual correlation (K=2): no pairs" and "NaN" in rows[0]
