"""Kinship under the fitted admixture model on the CPU (no GPU): the long-double reference of tests/kin_util.py against exact rationals,
float64 restatements of the two sums in three summation orders inside half of every bound, the mutants the checker has to catch, what
the estimator buys on a pedigree with admixed founders, the host's rules (multiclust_amd/host/mc_kinship.c as a program of its own
under the sanitizers) and the command line's refusals.

The pedigree, sized here (the figures are printed): 40 founders of Beta(1/2, 1/2) admixture between two populations of F_ST 0.15, a
duplicate, two families with sibs and a trio, 3 000 SNPs, 5 % missing, seed 1.  With the true parameters the duplicate comes out at
0.487, the parent-child and sib pairs from 0.236 up, every other pair at 0.031 at most: visible room to the cuts 0.354, 0.177 and
0.0884.  With the pooled sample frequencies (the homogeneous estimator) an unrelated pair reaches 0.137, past the second-degree cut."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from cli_util import BIN, ROOT
import host_driver
import kin_util as ku
import resid_util as ru

MULTI = os.path.join(ROOT, "tests", "golden", "data", "multi.stru")
PED = dict(seed=1, L=3000, founders=40)


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


# ---- the reference ----
@pytest.mark.parametrize("seed,ploidy,K,shared", [(1, 2, 3, False), (2, 1, 1, False), (3, 4, 2, True), (4, 2, 5, False)])
def test_reference_against_exact_rationals(seed, ploidy, K, shared):
    """w from exact t, the square root compared through w^2 = a^2 v; V as the sum of the products of those w.  The reference's own
    t is a long double: where t is within 2^-50 of 1 its 1 - t, and so v, carries an absolute 2^-64 a term of the sum -- nothing
    beside the K u t^2 of the device's bound, and allowed for here"""
    ua, geno, Q, P = small_case(seed, ploidy=ploidy, K=K, shared=shared)
    ref = ku.reference(ua, geno, Q, P)
    I, T = ref["I"], ref["T"]
    a, _ = ru.counts(ua, geno)
    cl = ru.col_locus(ua)
    q = ru.rows_of(Q, I)
    tol = 2.0 ** -60
    for i in range(I):
        for c in range(T):
            t = sum(Fraction(float(q[i, k])) * Fraction(float(P[k][c])) for k in range(K))
            ai = int(a[i, cl[c]])
            w2 = ai ** 2 * t * max(1 - t, 0)
            got = frac(ref["w"][i, c])
            assert abs(got * got - w2) <= 4 * tol * w2 + ai ** 2 * (K + 2) * 2.0 ** -63
            assert ai > 0 or ref["w"][i, c] == 0
    for i in range(I):
        for j in range(I):
            want = sum(frac(ref["w"][i, c]) * frac(ref["w"][j, c]) for c in range(T))
            assert abs(frac(ref["V"][i, j]) - want) <= 2.0 ** -56 * want + tol
            assert ref["V"][i, j] == ref["V"][j, i]
    # the operand the device forms lies within e of the exact one
    _, w = ku.device_operands(ua, geno, Q, P)
    err = np.abs(w.astype(ku.LD) - ref["w"])
    assert (err <= ref["e_w"]).all()
    assert (ref["a"] == 0).any() and ((ref["a"] > 0) & (ref["a"] < ploidy)).any() or ploidy == 1


@pytest.mark.parametrize("order", ["forward", "backward", "mfma"])
@pytest.mark.parametrize("missing", [0.0, 0.2])
def test_float64_restatements_stay_within_half_of_every_bound(order, missing):
    ua = np.array([2] * 30 + [3, 0 if missing else 2, 5, 1] + [2] * 31, dtype=np.int32)
    I, K = 9, 3
    geno = ru.genotypes(ua, I, 2, seed=11, missing=missing)
    if missing:
        geno[4] = ru.MISSING
    Q, P = ru.parameters(ua, I, K, seed=11)
    ref = ku.reference(ua, geno, Q, P)
    G, V = ku.restate(ua, geno, Q, P, order)
    r = ku.check(G, V, ref, limit=0.5)
    print(order, missing, r)
    if missing:
        assert not V[4].any() and not V[:, 4].any() and np.isnan(ku.kinship(G, V)[4]).all()


# ---- mutants ----
def test_without_the_fmax_a_frequency_one_ulp_above_one_gives_nan():
    """t one ulp above 1: p = 1 in both clusters and a one-hot q row with 2^-52 left in the other cluster -- q = (1, 2^-52) is what a
    projection's last rounding can leave of a vertex, and the device does not ask for an exact simplex point -- so the chain ends at
    1 + 2^-52.  With the fmax w is 0 there; without it the root of a negative number poisons the individual's whole row of V"""
    ua = np.array([2, 2], dtype=np.int32)
    geno = np.zeros((3, 2, 2), dtype=np.uint8)
    Q = np.array([[1.0, 2.0 ** -52], [1.0, 0.0], [0.5, 0.5]])
    P = np.array([[1.0, 0.0, 1.0, 0.0], [1.0, 0.0, 1.0, 0.0]])
    _, w = ku.device_operands(ua, geno, Q, P)
    t = np.stack([ku.fma_chain(q, P) for q in Q])
    assert t[0, 0] == 1.0 + 2.0 ** -52 and np.isfinite(w).all() and w[0, 0] == 0.0
    ref = ku.reference(ua, geno, Q, P)
    ku.check(*ku.restate(ua, geno, Q, P), ref)
    G, V = ku.restate(ua, geno, Q, P, mutant="no_fmax")
    assert np.isnan(V[0]).all() and ku.ratios(G, V, ref)["scale"] == np.inf
    with pytest.raises(AssertionError):
        ku.check(G, V, ref)


@pytest.fixture(scope="module")
def polyploid_case():
    ua = np.array([2, 3, 2, 4, 2, 2, 3, 2] * 4, dtype=np.int32)
    geno = ru.genotypes(ua, 7, 4, seed=5, missing=0.25)           # tetraploid: most genotypes lack some of their copies
    Q, P = ru.parameters(ua, 7, 3, seed=5)
    ref = ku.reference(ua, geno, Q, P)
    assert ((ref["a"] > 0) & (ref["a"] < 4)).mean() > 0.3
    return ua, geno, Q, P, ref


@pytest.mark.parametrize("mutant", ["no_copies", "gram_diag", "pooled"])
def test_mutants_are_caught(mutant, polyploid_case):
    ua, geno, Q, P, ref = polyploid_case
    ku.check(*ku.restate(ua, geno, Q, P), ref)
    G, V = ku.restate(ua, geno, Q, P, mutant=mutant)
    got = ku.ratios(G, V, ref)
    print(mutant, got)
    assert got["scale"] > 1e6
    with pytest.raises(AssertionError):
        ku.check(G, V, ref)


def test_an_asymmetric_scale_fails_the_shape_check(polyploid_case):
    ua, geno, Q, P, ref = polyploid_case
    G, V = ku.restate(ua, geno, Q, P)
    V[1, 2] = np.nextafter(V[1, 2], 1)
    assert ku.ratios(G, V, ref)["shape"] == np.inf and ku.ratios(G, V, ref)["scale"] <= 1


# ---- what the estimator buys ----
@pytest.fixture(scope="module")
def planted():
    ped = ku.pedigree(**PED)
    ua, geno = ku.genotypes_of(ped["codes"])
    return ped, ua, geno


def test_planted_pedigree_with_the_true_parameters(planted):
    ped, ua, geno = planted
    phi = ku.reference(ua, geno, ped["Q"], ped["P"])["phi"].astype(np.float64)
    dup, first, other = ku.margins(phi, ped)
    print("true parameters: duplicate %.4f (cut 0.354), smallest first degree %.4f (cut 0.177), largest other pair %.4f (cut 0.0884)"
          % (dup, first, other))
    assert all(phi[p] > 0.354 for p in ped["dup"]) and all(phi[p] > 0.177 for p in ped["first"])
    assert other < 0.0884
    assert np.array_equal(phi, phi.T) and (np.abs(2 * np.diag(phi) - 1) < 0.25).all()   # self-kinship: no inbreeding was planted
    pooled = ku.reference(ua, geno, np.ones((geno.shape[0], 1)), ku.pooled_frequencies(ua, geno))["phi"].astype(np.float64)
    _, _, other_pooled = ku.margins(pooled, ped)
    print("pooled sample frequencies: largest other pair %.4f" % other_pooled)
    assert other_pooled > 0.0884


def test_planted_pedigree_with_the_oracles_fit():
    """the same pedigree at 1 500 SNPs, the oracle's fit with K = 2: the planted pairs are the largest entries; the margins are printed
    (measured: duplicate 0.461, first degree from 0.138 -- fitted with the relatives in the data, the estimates fall short of 1/4 --
    other pairs up to 0.053.  With 24 founders the family of five was fitted as a cluster and its pairs fell to 0.014: the limit the
    documentation names)"""
    import oracle_bind as ob
    ped = ku.pedigree(seed=1, L=1500, founders=40)
    ua, geno = ku.genotypes_of(ped["codes"])
    I, L, pl = geno.shape
    mod = ob.Model(ob.Data(I, L, pl, ua, geno), ob.make_options(accel_scheme=3), 2)
    mod.init_random(7)
    mod.em()
    assert mod.fatal == 0
    phi = ku.reference(ua, geno, mod.q(mod.pindex).copy(), mod.p(mod.pindex).copy())["phi"].astype(np.float64)
    dup, first, other = ku.margins(phi, ped)
    print("oracle's fit: duplicate %.4f, smallest first degree %.4f, largest other pair %.4f" % (dup, first, other))
    assert min(dup, first) > other


# ---- mc_kinship.c under AddressSanitizer + UBSan, as a program of its own (the device entry point stubbed) ----
def driver_sums(n):
    """the sums tests/kinship_host_driver.c makes up"""
    G, V = np.zeros((n, n)), np.zeros((n, n))
    ladder = [0.354, 0.177, 0.0884, 0.0442]
    for i in range(n):
        for j in range(n):
            lo, hi = min(i, j), max(i, j)
            if i == 1 or j == 1:                                  # individual 1 has no data
                continue
            V[i, j] = 8.0 + lo + 2 * hi
            if i == j:
                G[i, j] = V[i, j] * (0.5 + 0.03125 * (i % 3))
            elif lo == 0 and 2 <= hi < 6:
                V[i, j] = 16.0
                G[i, j] = 16.0 * ladder[hi - 2]                   # exactly on a cut: not above it
            elif lo == 2 and 3 <= hi < 7:
                G[i, j] = V[i, j] * (ladder[hi - 3] + 0.001)      # just above
            else:
                G[i, j] = V[i, j] * 0.01 * float((lo * 3 + hi * 7) % 11 - 5) / 8.0
    return G, V


@pytest.mark.parametrize("n,ploidy", [(1, 2), (2, 2), (9, 2), (9, 4)])
def test_host_code_is_sanitizer_clean_and_follows_the_rules(n, ploidy, tmp_path):
    exe = host_driver.build(tmp_path, "kinship_host", ["tests/kinship_host_driver.c", "multiclust_amd/host/mc_kinship.c"], werror=True)
    t = 0.04
    res = host_driver.run(exe, [n, ploidy, repr(t), tmp_path / "stem"], cwd=tmp_path)
    assert "wrote 0" in res.stdout
    G, V = driver_sums(n)
    want = ku.report(G, V, ploidy, t, K=2)
    assert res.stdout.split("\n")[0] == want["line"]
    assert open(str(tmp_path / "stem.admix.K=2.kin0")).read() == want["kin0"]
    assert open(str(tmp_path / "stem.admix.K=2.kin.ind.txt")).read() == want["ind"]
    if n == 9:
        # individual 1 has no data: NaN everywhere, in no pair; a phi on a cut has the degree below it, one just above the degree itself
        ind = want["ind"].split("\n")
        assert ind[2] == "1\tNaN\tNaN\t0\tNaN\t-1" and all(1 not in p[:2] for p in want["pairs"])
        deg = {p[:2]: p[5] for p in want["pairs"]}
        assert [deg[(0, j)] for j in (2, 3, 4, 5)] == [1, 2, 3, 4]  # (0.0442 is above t = 0.04: reported, as more distant than third degree)
        assert [deg[(2, j)] for j in (3, 4, 5, 6)] == [0, 1, 2, 3]
        assert want["n_finite"] == 28 and want["line"].startswith("Kinship (K=2): 8 pairs above 0.04 (1 duplicates, 2 first, 2 second, 2 third degree); largest ")
        assert ("NaN" in ind[1].split("\t")[2]) == (ploidy != 2)
    else:
        assert want["line"] == "Kinship (K=2): no pairs" and want["kin0"].count("\n") == 1


# ---- the command line ----
@pytest.mark.parametrize("args,why", [
    (["-a", "-k", "2", "--kinship", "0"], "the kinship threshold of --kinship must lie in (0, 0.5)"),
    (["-a", "-k", "2", "--kinship", "0.5"], "the kinship threshold of --kinship must lie in (0, 0.5)"),
    (["-a", "-k", "2", "--kinship", "nan"], "the kinship threshold of --kinship must lie in (0, 0.5)"),
    (["-k", "2", "--kinship", "0.1"], "--kinship needs the admixture model (-a)"),
    (["-a", "-k", "2", "--kinship", "0.1", "-b", "2"], "--kinship cannot be combined with the bootstrap (-b)"),
    (["-a", "-k", "2", "--kinship", "0.1", "-w", "n", "2"], "--kinship cannot be combined with -w or -M"),
    (["-a", "-k", "2", "--kinship", "0.1", "-M"], "--kinship cannot be combined with -w or -M"),
    (["-a", "-k", "2", "--kinship", "0.1", "--gpus", "2"], "--kinship cannot be combined with --gpus above 1"),
])
def test_refused_combinations(args, why, tmp_path):
    res = subprocess.run([BIN, "-f", MULTI] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, cwd=str(tmp_path))
    assert res.returncode == 10, (args, res.returncode, res.stderr[-500:])
    assert "ERROR [mc_main.c::parse_options]: " + why + " (argument '--kinship')" in res.stderr


def test_a_missing_argument_is_a_bad_argument(tmp_path):
    res = subprocess.run([BIN, "-f", MULTI, "-a", "--kinship"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60,
                         cwd=str(tmp_path))
    assert res.returncode == 10 and "ERROR [mc_main.c::parse_options]: --kinship (argument '')" in res.stderr


@pytest.mark.parametrize("args,why,status", [
    # the neighbours in the `k` case parse as before: --king-cutoff reaches its own refusal, -k 3 its number (the mixture model then
    # refuses --kinship: the option after -k 3 was read as an option, not swallowed)
    (["--king-cutoff", "0.1"], "--king-cutoff needs a PLINK fileset (--bed) (argument '--king-cutoff')", 10),
    (["--king-cutoff", "0.7", "--kinship", "0.1", "-a"], "--king-cutoff needs a PLINK fileset (--bed) (argument '--king-cutoff')", 10),
    (["-k", "3", "--kinship", "0.1"], "--kinship needs the admixture model (-a) (argument '--kinship')", 10),
    (["-k", "0"], "-k (argument '0')", 10),
])
def test_the_neighbouring_options_parse_as_before(args, why, status, tmp_path):
    res = subprocess.run([BIN, "-f", MULTI] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, cwd=str(tmp_path))
    assert res.returncode == status, (args, res.returncode, res.stderr[-500:])
    assert "ERROR [mc_main.c::parse_options]: " + why in res.stderr


def test_the_usage_text_names_the_option(tmp_path):
    res = subprocess.run([BIN, "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, cwd=str(tmp_path))
    assert "  --kinship <t> " in res.stdout and "--king-cutoff <t>" in res.stdout
