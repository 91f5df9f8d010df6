"""-m gpu: the mixture model's initialisation on the device (mchip_init_from_individual_centers: random_individual_center +
initialize_parameters_mixture, rnd_init.c:192-339) against the host body kept behind MC_HOST_INIT, bit for bit.

Distances and allele counts are integers, 1 + (K - k) * c and the row sums are exact integers, and the divisions are IEEE divisions
of the same operands: every comparison below is np.array_equal.  The assignment is compared with a restatement of the rule in
numpy (a center k joins k, even when an earlier center is identical to it; everyone else joins the FIRST center of minimal L1
distance between allele-count vectors over observed copies), which the host's eta = (1 + n_k) / (I + K) pins as well."""
import ctypes as C

import numpy as np
import pytest

from device_util import ctx
import oracle_bind as ob
from golden_util import Golden
from multiclust_amd import hip, host
from synth import make_dataset
from test_bootstrap_cpu import counts_of, golden_bootstrap

pytestmark = pytest.mark.gpu


def drawn_centers(I, K, seed):
    """the centers mc_initialize_mixture draws for srand(seed): random_individual_center's rejection walk"""
    lib = host.load()
    rng = host.McRng()
    lib.mc_srand(C.byref(rng), seed)
    center = (C.c_int * max(K, 1))()
    lib.mc_test_center_walk(I, K, C.byref(rng), center)
    return [int(c) for c in center[:K]]


def assignment_rule(geno, ua, centers):
    """rnd_init.c:221-258 restated on the allele counts"""
    cnt = counts_of(geno, ua).astype(np.int64)
    K = len(centers)
    if K == 1:
        return np.zeros(len(geno), dtype=np.int32)
    dist = np.stack([np.abs(cnt - cnt[c][None, :]).sum(axis=1) for c in centers], axis=1)      # [I][K]
    out = np.argmin(dist, axis=1).astype(np.int32)                                                # first minimum
    for k, c in enumerate(centers):
        out[c] = k
    return out


def host_body(ua, geno, K, seed, monkeypatch):
    monkeypatch.setenv("MC_HOST_INIT", "1")
    fit = host.Fit(ua, geno, K, admixture=0, verbosity=1)
    fit.initialize(seed)
    q, p = fit.get_q(0), fit.get_p(0)
    fit.close()
    monkeypatch.delenv("MC_HOST_INIT")
    return q, p


def check_against_host(ctx, ua, geno, K, seed, monkeypatch):
    I = geno.shape[0]
    q_host, p_host = host_body(ua, geno, K, seed, monkeypatch)
    centers = drawn_centers(I, K, seed)
    ctx.set_genotypes(ua, geno)
    ctx.set_model(K, admixture=0, lower_bound=1e-8)
    assign = ctx.init_from_individual_centers(centers, 1)
    want = assignment_rule(geno, ua, centers)
    assert np.array_equal(assign, want), np.nonzero(assign != want)[0][:10]
    assert np.array_equal(ctx.get_q(1), q_host)
    assert np.array_equal(ctx.get_p(1), p_host)
    assert np.array_equal(q_host, (1.0 + np.bincount(want, minlength=K)) / (I + K))
    # the whole host route (center draws on the host, the rest on the device) gives the same bits
    fit = host.Fit(ua, geno, K, admixture=0, verbosity=1)
    fit.initialize(seed)
    assert np.array_equal(fit.get_q(0), q_host) and np.array_equal(fit.get_p(0), p_host)
    fit.close()
    return centers, assign


# (I, L, ploidy, K, max alleles, missing rate): K = 1, 2, 3, 8, 27, 64; ploidy 1..8 and 9; 2..254 alleles; I = 255 / 257 / 513
INIT_CASES = [
    (255, 37, 1, 1, 4, 0.05), (257, 41, 2, 2, 2, 0.05), (513, 29, 3, 3, 5, 0.05), (257, 33, 4, 8, 4, 0.1),
    (255, 21, 5, 27, 7, 0.05), (257, 19, 6, 64, 4, 0.05), (255, 23, 7, 3, 3, 0.2), (257, 27, 8, 8, 254, 0.05),
    (255, 17, 9, 27, 30, 0.05), (257, 15, 9, 64, 254, 0.05), (513, 203, 2, 64, 2, 0.0), (257, 1100, 4, 3, 4, 0.02),
    (255, 13, 12, 2, 3, 0.3),
]


@pytest.mark.parametrize("I,L,ploidy,K,maxal,missing", INIT_CASES,
                         ids=["I%d-L%d-pl%d-K%d-M%d" % c[:5] for c in INIT_CASES])
def test_device_initialisation_equals_the_host_body(ctx, monkeypatch, I, L, ploidy, K, maxal, missing):
    ua, geno = make_dataset(I, L, max(K, 2), ploidy=ploidy, max_alleles=maxal, seed=I + L + K, missing=missing)
    geno[I // 3] = 0xFF                 # an individual with no observed copy
    geno[5, L // 2:] = 0xFF             # and one observed on half of the loci only
    if maxal == 254:
        ua[0] = 254
        geno[::2, 0, 0] = 253
    for seed in (7, 20250118):
        check_against_host(ctx, ua, geno, K, seed, monkeypatch)


@pytest.mark.parametrize("K,ploidy", [(2, 2), (3, 4), (5, 9)])
def test_duplicated_individuals_first_minimum_and_centers_keep_their_own_cluster(ctx, monkeypatch, K, ploidy):
    """(a) a non-center equidistant from two centers joins the first; (b) a center k > 0 identical to center 0 still joins k"""
    I, L, seed = 257, 43, 31
    ua, geno = make_dataset(I, L, K, ploidy=ploidy, max_alleles=4, seed=K, missing=0.05)
    centers = drawn_centers(I, K, seed)
    bystander, other = [i for i in range(I) if i not in centers][:2]
    geno[centers[0], 0] = 0
    geno[centers[1]] = geno[centers[0]]
    geno[bystander] = geno[centers[0]]          # distance 0 to centers 0 and 1
    geno[other] = geno[centers[0]]
    geno[other, 0] = 1                          # distance 2 * ploidy to centers 0 and 1
    got_centers, assign = check_against_host(ctx, ua, geno, K, seed, monkeypatch)
    assert got_centers == centers
    assert assign[centers[1]] == 1 and assign[centers[0]] == 0 and assign[bystander] == 0 and assign[other] == 0


def test_bad_centers_and_the_wrong_model_are_refused(ctx):
    ua, geno = make_dataset(40, 11, 3, ploidy=2, max_alleles=3, seed=2)
    ctx.set_genotypes(ua, geno)
    ctx.set_model(3, admixture=0, lower_bound=1e-8)
    for bad in ([0, 1, 40], [-1, 2, 3], [4, 9, 4]):
        with pytest.raises(hip.HipError, match="INVALID"):
            ctx.init_from_individual_centers(bad, 0)
    ctx.init_from_individual_centers([4, 9, 5], 0)
    ctx.set_model(3, admixture=1, lower_bound=1e-8)
    with pytest.raises(hip.HipError, match="STATE"):
        ctx.init_from_individual_centers([4, 9, 5], 0)


@pytest.mark.parametrize("name", ["multi_mix_k3", "missing_mix_k2", "allmiss_mix_k2", "hexaploid_mix_k2"])
def test_host_fit_initialises_with_the_same_bits_either_way(name, monkeypatch):
    g = Golden(name)
    out = []
    for host_init in (False, True):
        if host_init:
            monkeypatch.setenv("MC_HOST_INIT", "1")
        else:
            monkeypatch.delenv("MC_HOST_INIT", raising=False)
        fit = host.Fit(g.ua, g.geno, g.K, admixture=0, verbosity=1)
        rng = fit.initialize(g.m["seed"])
        out.append((fit.get_q(0), fit.get_p(0), host.load().mc_rand(C.byref(rng))))
        fit.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]


def test_device_form_on_a_device_generated_replicate_initialises_like_the_reference(ctx):
    """q_bsinit / p_bsinit of the reference (dumped with the bootstrap data set in place) from a replicate that never was on
    the host: generated on the device, initialised on the device"""
    g = Golden("multi_mix_k3")
    window, _ = ob.glibc_window(g.m["bootstrap_seed"])
    ctx.simulate_genotypes_mixture(g.I, g.L, g.ploidy, g.ua, window, g.K, g.q("bs"), g.p("bs"))
    assert np.array_equal(counts_of(ctx.get_genotypes(), g.ua), golden_bootstrap(g))
    ctx.set_model(g.K, admixture=0, lower_bound=g.lower_bound)
    ctx.init_from_individual_centers(drawn_centers(g.I, g.K, g.m["seed"]), 0)
    np.testing.assert_allclose(ctx.get_q(0).ravel(), g.q("bsinit").ravel(), rtol=1e-15, atol=1e-18)
    np.testing.assert_allclose(ctx.get_p(0), g.p("bsinit"), rtol=1e-15, atol=1e-18)
