"""-m gpu: standard errors of the mixing proportions by a bootstrap over loci (mc_locus_bootstrap, multiclust_amd/host/mc_se.c): the
driver against the same sequence call by call, the locus lists against the stream convention, a known answer, and the standard
error falling with the number of loci as it does on the CPU."""
import numpy as np
import pytest

from bits import bits
import cv_util as cu
import oracle_bind as ob
import rand_window as rw
import se_util as su
from multiclust_amd import host

pytestmark = pytest.mark.gpu


def host_state(fit):
    m = fit.mod
    return (m.logL, m.n_iter, m.pindex, m.findex, m.tindex, m.converged, m.delta_index)


def set_model(fit, ctx):
    """mchip_set_model with the arguments mc_model_create uses"""
    o = fit.opt
    rc = ctx.lib.mchip_set_model(ctx.h, fit.K, o.admixture, o.eta_constrained, o.do_projection, o.eta_lower_bound, o.p_lower_bound,
                                 o.q if o.accel_scheme else 0)
    assert rc == 0
    ctx.K = fit.K


def fit_replicate(fit, ctx, src, q, p):
    """one replicate of mc_locus_bootstrap, call by call; returns Q of the fit, or None when it stopped on a fatal condition"""
    ua2 = np.ascontiguousarray(fit.ua[src])
    ctx.resample_loci(src)
    set_model(fit, ctx)
    fit.reset()
    ctx.set_q(0, q)
    ctx.set_p(0, p[:, su.gather_columns(fit.ua, src)])
    keep = (fit.dat.L, fit.dat.uniquealleles, fit.dat.geno)
    fit.dat.L, fit.dat.uniquealleles, fit.dat.geno = len(src), ua2.ctypes.data, None     # the replicate's shape, no genotype
    try:
        fit.em()
    finally:
        fit.dat.L, fit.dat.uniquealleles, fit.dat.geno = keep
    return None if fit.mod.fatal else fit.get_q(fit.mod.pindex)


def se_dataset(seed, lists):
    """I = 120, L = 150, diploid: individual 5 wholly missing; individual 9 observed at two neighbouring loci only, chosen so that
    some of the lists hold neither of them and some hold one"""
    I, L = 120, 150
    ua, geno = cu.cv_dataset(I, L, 2, seed=seed)
    before = geno.copy()
    geno[5] = cu.MISSING
    for a in range(2, L - 1):
        absent = [not np.isin([a, a + 1], src).any() for src in lists]
        if 0 < sum(absent) < len(lists):
            break
    else:
        raise AssertionError("no pair of neighbouring loci is absent from some lists and present in others")
    keep = geno[9, a:a + 2].copy()
    keep[keep == cu.MISSING] = 0
    geno[9] = cu.MISSING
    geno[9, a:a + 2] = keep
    return su.with_phantoms(ua, before, geno), geno, absent


# ---------------------------------------------------------------- 1. the driver

@pytest.mark.parametrize("block", [1, 7])
@pytest.mark.parametrize("model,accel", [("individual", 0), ("individual", 3), ("shared", 3), ("mixture", 3)])
def test_driver_equals_the_call_sequence(model, accel, block):
    K, B, seed = 3, 6, 11
    admixture, constrained = {"individual": (1, 0), "shared": (1, 1), "mixture": (0, 0)}[model]
    lists = su.locus_lists(rw.draws(ob.glibc_window(seed)[0], -(-150 // block) * B), 150, block, B)
    ua, geno, absent = se_dataset(31, lists)
    I = geno.shape[0]
    fit = host.Fit(ua, geno, K, admixture=admixture, eta_constrained=constrained, accel_scheme=accel, seed=seed, max_iter=60)
    try:
        if admixture:
            fit.fit_unit(seed, 0)
        else:                                             # the mixture model: a few EM steps from random parameters
            from synth import random_params
            q0, p0 = random_params(I, ua, K, seed=3)
            fit.set_params(q0.mean(axis=0), p0)
            fit.em()
        assert fit.mod.fatal == 0
        slot, state = fit.mod.pindex, host_state(fit)
        q, p = fit.get_q(slot), fit.get_p(slot)
        assert model != "individual" or np.isnan(q[5]).all()
        assert [bits(x) for x in fit.locus_lists(B, block)] == [bits(x) for x in lists]
        mean, se, count, res = fit.locus_bootstrap(B, block)
        # the model is as it was found
        assert host_state(fit) == state
        assert bits(fit.get_q(slot)) == bits(q) and bits(fit.get_p(slot)) == bits(p)
        ctx = su.device_of(fit)
        assert bits(ctx.get_genotypes()) == bits(geno)
        # the same, call by call
        acc, failed, n_iter, empty9 = su.Welford(q.shape), 0, 0, []
        for src in lists:
            x = fit_replicate(fit, ctx, src, q, p)
            empty9.append(bool((ctx.get_genotypes()[9] == cu.MISSING).all()))
            n_iter += fit.mod.n_iter
            if x is None:
                failed += 1
            else:
                acc.add(x)
        ctx.resample_loci(None)
        assert bits(ctx.get_genotypes()) == bits(geno)
        assert empty9 == absent and 0 < sum(empty9) < B       # individual 9 is empty in some replicates and not in others
        want_mean, want_se, want_count = acc.result()
        assert (res.n_replicates, res.block, res.n_failed, res.n_iter) == (B, block, failed, n_iter) and failed == 0
        assert bits(count) == bits(want_count) and bits(mean) == bits(want_mean) and bits(se) == bits(want_se)
        if model == "individual":
            assert (count[5] == 0).all() and np.isnan(mean[5]).all() and np.isnan(se[5]).all()
            assert (count[9] == B - sum(empty9)).all() and (np.delete(count, [5, 9], axis=0) == B).all()
        else:
            assert (count == B).all()
        m, mx = su.summary(se)
        assert bits(np.float64(res.mean_se)) == bits(np.float64(m)) and bits(np.float64(res.max_se)) == bits(np.float64(mx))
        assert mx > 0
    finally:
        fit.close()


def test_limits():
    ua, geno = cu.cv_dataset(67, 61, 2, seed=1)
    fit = host.Fit(ua, geno, 2, admixture=1, seed=3, max_iter=5)
    try:
        fit.fit_unit(3, 0)
        state, q = host_state(fit), fit.get_q(fit.mod.pindex)
        for B, block in ((1, 1), (10001, 1), (5, 0), (5, 62)):
            with pytest.raises(Exception, match="mc_locus_bootstrap failed"):
                fit.locus_bootstrap(B, block)
        assert host_state(fit) == state and bits(fit.get_q(fit.mod.pindex)) == bits(q)
    finally:
        fit.close()


# ---------------------------------------------------------------- 2. the lists

def test_locus_lists_follow_the_stream_convention():
    L, B, seed = 150, 5, 20261017
    ua, geno = cu.cv_dataset(20, L, 1, seed=2)
    fits = [host.Fit(ua, geno, K, admixture=1, seed=seed) for K in (2, 3)]
    try:
        for block in (1, 4, 7, 75, 149, 150):             # 4, 7 and 149 do not divide 150: the last block is shorter
            nb = -(-L // block)
            want = su.locus_lists(rw.draws(ob.glibc_window(seed)[0], nb * B), L, block, B)
            for fit in fits:                              # the lists do not depend on K
                got = fit.locus_lists(B, block)
                assert len(got) == B and all(g.dtype == np.int32 for g in got)
                assert [bits(g) for g in got] == [bits(w) for w in want], block
            assert all(0 <= w.min() and w.max() < L for w in want)
        assert [bits(g) for g in fits[0].locus_lists(2, 150)] == [bits(np.arange(L, dtype=np.int32))] * 2
    finally:
        for fit in fits:
            fit.close()


# ---------------------------------------------------------------- 3. a known answer

@pytest.mark.parametrize("model", ["individual", "shared"])
def test_one_block_gives_zero_standard_errors(model):
    """block = L: one block, every replicate is the base, every fit the same fit: se = 0 exactly, mean = that fit's Q"""
    I, L, K, seed = 67, 61, 3, 5
    ua, geno = cu.cv_dataset(I, L, 2, seed=7)
    geno[4] = cu.MISSING
    fit = host.Fit(ua, geno, K, admixture=1, eta_constrained=int(model == "shared"), accel_scheme=3, seed=seed, max_iter=40)
    try:
        fit.fit_unit(seed, 0)
        slot = fit.mod.pindex
        q, p = fit.get_q(slot), fit.get_p(slot)
        mean, se, count, res = fit.locus_bootstrap(4, L)
        ctx = su.device_of(fit)
        x = fit_replicate(fit, ctx, np.arange(L, dtype=np.int32), q, p)
        ctx.resample_loci(None)
        seen = ~np.isnan(x)
        assert res.n_failed == 0 and (count[seen] == 4).all() and (count[~seen] == 0).all()
        assert (se[seen] == 0.0).all() and not np.signbit(se[seen]).any() and np.isnan(se[~seen]).all()
        assert bits(mean) == bits(np.where(seen, x, np.nan))
        assert (res.mean_se, res.max_se) == (0.0, 0.0)
        if model == "individual":
            assert not seen[4].any() and seen.sum() == (I - 1) * K
    finally:
        fit.close()


# ---------------------------------------------------------------- 4. it measures something

# CPU values for these very data sets, seed and lists (tests/se_util.cpu_locus_bootstrap: the oracle's EM with SQUAREM S3 from the
# random allele partition of srand(seed), each of the 20 replicates fitted by the oracle from that estimate, block 1, Welford in
# replicate order; mean over the 900 entries):
#   L = 200: 0.0096462100    L = 800: 0.0024146664    gap: 0.0072315436; the GPU's gap must be at least half of it
SE_CPU = {200: 0.0096462100, 800: 0.0024146664}
SE_GAP = SE_CPU[200] - SE_CPU[800]


def test_standard_errors_fall_with_more_loci():
    seed, se = 20261017, {}
    for L in (200, 800):
        ua, geno = cu.clustered_dataset(300, L, 3, seed)
        fit = host.Fit(ua, geno, 3, admixture=1, accel_scheme=3, seed=seed)
        try:
            fit.fit_unit(seed, 0)
            assert fit.mod.fatal == 0
            _, _, count, res = fit.locus_bootstrap(20, 1)
            assert res.n_failed == 0 and (count == 20).all()
            se[L] = res.mean_se
        finally:
            fit.close()
    print("mean SE by L:", se, "CPU:", SE_CPU, "CPU gap:", SE_GAP)
    assert se[200] - se[800] >= 0.5 * SE_GAP, (se, SE_CPU)
