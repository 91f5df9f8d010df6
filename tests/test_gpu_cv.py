"""-m gpu: K-fold cross-validation on the device (mchip_cv_*, multiclust_amd/csrc/mchip_cv.hip) and its host driver
(mc_cross_validate): the fold draw against the serial rand() stream, the hold-out against the numpy mask, a fit to a held-out data
set against the fit of the masked data uploaded afresh, the held-out score against numpy, the driver against the same sequence
call by call, and the choice of K on clustered data."""
import ctypes as C

import numpy as np
import pytest

from bits import bits
import cv_util as cu
from device_util import contexts, status_of
import impute_util as iu
import oracle_bind as ob
import rand_window as rw
from feature_geometry import EDGES
from multiclust_amd import hip, host
from synth import make_dataset, random_params

pytestmark = pytest.mark.gpu

SHAPES = [(I, L, pl) for I in (67, 300) for L in (61, 130) for pl in (1, 2, 4)]
STATUS = {v: k for k, v in hip.STATUS.items()}


def windows():
    """windows of the rand() stream: chosen draws placed at draw 0 (rand_window.window_placing: the extreme values of rand()
    first), the start of a seeded stream, and the same stream more than 2^32 draws on (window_placing walks the stream back word
    by word, so that position is reached with the host's O(log n) jump-ahead, mc_rng_jump, instead)"""
    placed = rw.window_placing([rw.RAND_MAX, 0, 12345, rw.RAND_MAX - 1], 0, fill_seed=3)
    first = ob.glibc_window(20261017)[0]
    lib = host.load()
    rng = host.McRng()
    lib.mc_srand(C.byref(rng), 20261017)
    lib.mc_rng_jump(C.byref(rng), (1 << 32) + 12345)
    far = np.array([rng.r[(rng.f + t) % 31] for t in range(31)], dtype=np.int64).astype(np.uint32)
    assert not np.array_equal(far, first)
    return {"first": first, "placed": placed, "far": far}


# ---------------------------------------------------------------- 1. folds

@pytest.mark.parametrize("where", sorted(windows()))
def test_folds_are_the_serial_stream(where, contexts):
    ctx = contexts[0]
    window = windows()[where]
    I, L = 67, 61
    ua, geno = make_dataset(I, L, 2, ploidy=2, seed=1)
    ctx.set_genotypes(ua, geno)
    serial = rw.draws(window, I * L)
    for F in (2, 5, 7, 64):
        ctx.cv_draw_folds(window, F)
        assert np.array_equal(ctx.cv_get_folds().ravel(), serial % F), F


def test_folds_cross_generator_chunks_and_blocks(contexts):
    """1009 x 1009 draws: 257 chunks of 3 968 draws, so a second block of 256 threads, the last chunk partial"""
    ctx = contexts[0]
    I = L = 1009
    ua, geno = make_dataset(I, L, 2, ploidy=1, seed=2)
    ctx.set_genotypes(ua, geno)
    assert I * L > 256 * 3968
    for window in (windows()["first"], windows()["far"]):
        serial = rw.draws(window, I * L)
        ctx.cv_draw_folds(window, 5)
        assert np.array_equal(ctx.cv_get_folds().ravel(), serial % 5)


def test_set_folds_round_trip_and_refusals(contexts):
    ctx = contexts[0]
    I, L = 67, 61
    ua, geno = make_dataset(I, L, 2, ploidy=2, seed=1)
    ctx.set_genotypes(ua, geno)
    lib = ctx.lib
    out = np.empty((I, L), np.uint8)
    assert status_of(lib.mchip_cv_get_folds(ctx.h, out.ctypes.data)) == "STATE"      # a new data set has no folds
    assert status_of(lib.mchip_cv_hold_out(ctx.h, 0)) == "STATE"
    folds = np.random.default_rng(4).integers(0, 7, size=(I, L)).astype(np.uint8)
    ctx.cv_set_folds(folds, 7)
    assert np.array_equal(ctx.cv_get_folds(), folds)
    bad = folds.copy()
    bad[66, 60] = 7
    assert status_of(lib.mchip_cv_set_folds(ctx.h, bad.ctypes.data, 7)) == "INVALID"
    assert np.array_equal(ctx.cv_get_folds(), folds)
    w = windows()["first"]
    for F in (0, 1, 65):
        assert status_of(lib.mchip_cv_draw_folds(ctx.h, w.ctypes.data, F)) == "INVALID"
        assert status_of(lib.mchip_cv_set_folds(ctx.h, folds.ctypes.data, F)) == "INVALID"
    for f in (-2, 7):
        assert status_of(lib.mchip_cv_hold_out(ctx.h, f)) == "INVALID"
    ctx.set_genotypes(ua, geno)                                                       # ... and drops them
    assert status_of(lib.mchip_cv_get_folds(ctx.h, out.ctypes.data)) == "STATE"
    fresh = hip.Context(0)
    assert status_of(lib.mchip_cv_draw_folds(fresh.h, w.ctypes.data, 5)) == "STATE"   # no data set
    fresh.close()


# ---------------------------------------------------------------- 2. hold-out

def forced_folds(window, geno, F):
    """serial folds, with every genotype of individual 3 in fold 0"""
    I, L, _ = geno.shape
    folds = cu.serial_folds(window, I, L, F)
    folds[3, :] = 0
    return folds


@pytest.mark.parametrize("I,L,pl", SHAPES)
def test_hold_out_installs_the_masked_set(I, L, pl, contexts):
    ctx = contexts[0]
    ua, geno = cu.cv_dataset(I, L, pl, seed=100 * I + 10 * L + pl)
    assert ua[0] >= 35 and not (geno[:, 1] == cu.MISSING).any() and (geno == cu.MISSING).any()
    ctx.set_genotypes(ua, geno)
    ctx.set_model(3)
    plen = C.c_int()
    ctx.lib.mchip_p_length(ctx.h, C.byref(plen))
    counts = ctx.data_counts()
    for F in (2, 5):
        folds = forced_folds(windows()["first"], geno, F)
        ctx.cv_set_folds(folds, F)
        for f in range(F):
            ctx.cv_hold_out(f)
            want = cu.masked(geno, folds, f)
            assert np.array_equal(ctx.get_genotypes(), want), (F, f)
            assert ctx.empty_individuals() == cu.empty_individuals(want), (F, f)
            cells, copies = ctx.data_counts()
            assert copies == int((want != cu.MISSING).sum()) and cells <= counts[0]
            n = C.c_int()
            ctx.lib.mchip_p_length(ctx.h, C.byref(n))
            assert n.value == plen.value
        assert cu.empty_individuals(cu.masked(geno, folds, 0))[0] >= 1           # individual 3
        ctx.cv_hold_out(-1)
        assert bits(ctx.get_genotypes()) == bits(geno)
        assert ctx.data_counts() == counts and ctx.empty_individuals() == cu.empty_individuals(geno)


# ---------------------------------------------------------------- 3. a masked fit is the fit of the masked data

def fit_data(kind):
    if kind == "biallelic":                    # no missing copy before the mask: the hold-out changes the kernels' variant
        return make_dataset(300, 130, 3, ploidy=2, max_alleles=2, seed=7)
    return cu.cv_dataset(300, 130, 2, seed=8)


@pytest.mark.parametrize("kind", ["biallelic", "general"])
@pytest.mark.parametrize("model", ["individual", "shared", "mixture"])
def test_masked_fit_is_the_fit_of_the_masked_data(model, kind, contexts):
    held, fresh = contexts
    ua, geno = fit_data(kind)
    I, L, _ = geno.shape
    F, f = 5, 2
    folds = cu.serial_folds(windows()["first"], I, L, F)
    want = cu.masked(geno, folds, f)
    admixture, constrained = (0, 0) if model == "mixture" else (1, int(model == "shared"))
    for K in (1, 8, 27, 28, 64):
        q0, p0 = random_params(I, ua, K, seed=K)
        if model != "individual":
            q0 = q0.mean(axis=0)
        held.set_genotypes(ua, geno)
        held.set_model(K, admixture=admixture, eta_constrained=constrained)
        held.set_q(0, q0)
        held.set_p(0, p0)
        held.set_q(1, q0[::-1].copy())
        before = [bits(held.get_q(s)) + bits(held.get_p(s)) for s in range(3)]
        held.cv_set_folds(folds, F)
        held.cv_hold_out(f)
        assert [bits(held.get_q(s)) + bits(held.get_p(s)) for s in range(3)] == before      # the model survives
        fresh.set_genotypes(ua, want)
        fresh.set_model(K, admixture=admixture, eta_constrained=constrained)
        fresh.set_q(0, q0)
        fresh.set_p(0, p0)
        for step in range(5):
            a, b = held.em_step(0, 0), fresh.em_step(0, 0)
            assert np.isfinite(b) and bits(np.float64(a)) == bits(np.float64(b)), (K, step, a, b)
        assert bits(held.get_q(0)) == bits(fresh.get_q(0)) and bits(held.get_p(0)) == bits(fresh.get_p(0)), K
        assert bits(held.expected_counts()) == bits(fresh.expected_counts()), K


# ---------------------------------------------------------------- 4. the score

def check_score(ctx, ua, geno, folds, f, q_dev, p, K, floor, label):
    """one mchip_cv_heldout_loglik against numpy; q_dev is Q as the device stores it"""
    got = ctx.cv_heldout_loglik(0, floor)
    exact, n, n_floored, sum_abs = cu.heldout_score(ua, geno, folds, f, q_dev, p, floor)
    # one rounding per addition of the running sum (n of them), the K-term dot product and the log of each term
    bound = (n + K + 8) * 2.0 ** -52 * sum_abs
    print("%s: device %.17g exact %.17g |diff| %.3g bound %.3g n %d floored %d" % (label, got[0], exact, abs(got[0] - exact), bound, n, n_floored))
    assert got[1] == n and got[2] == n_floored, (label, got, n, n_floored)
    assert abs(got[0] - exact) <= bound, (label, got[0], exact, bound)
    assert bits(np.float64(ctx.cv_heldout_loglik(0, floor)[0])) == bits(np.float64(got[0])), label     # the same bits again
    return got


@pytest.mark.parametrize("I,L,pl", SHAPES)
def test_heldout_score(I, L, pl, contexts):
    ctx = contexts[0]
    ua, geno = cu.cv_dataset(I, L, pl, seed=100 * I + 10 * L + pl)
    T = int(ua.sum())
    ctx.set_genotypes(ua, geno)
    floor = 1.0 / (I * pl + 1)
    rng = np.random.default_rng(I + L + pl)
    for F in (2, 5):
        folds = forced_folds(windows()["first"], geno, F)
        ctx.cv_set_folds(folds, F)
        for f in range(F):
            ctx.cv_hold_out(f)
            n_empty, first = ctx.empty_individuals()
            if f == 0:
                assert n_empty >= 1 and (geno[3] != cu.MISSING).any()         # individual 3: every observed genotype held out
            for K in (1, 2, 8, 27, 28, 64):
                q0, p0 = random_params(I, ua, K, seed=K + f)
                p0[:, rng.integers(0, T, size=max(2, T // 10))] = 0.0       # alleles no cluster carries: t = 0, floored
                for constrained in ((0, 1) if K in (2, 28) else (0,)):
                    ctx.set_model(K, admixture=1, eta_constrained=constrained)
                    q_in = q0.mean(axis=0) if constrained else q0.copy()
                    q_dev = q_in.copy()
                    if f == 0 and not constrained:
                        q_in[3] = np.nan                                      # accepted for an individual without an observed copy ...
                        q_dev[3] = 1.0 / K                                    # ... and kept as the finite 1 / K
                    ctx.set_q(0, q_in)
                    ctx.set_p(0, p0)
                    label = "I%d L%d pl%d F%d f%d K%d c%d" % (I, L, pl, F, f, K, constrained)
                    got = check_score(ctx, ua, geno, folds, f, q_dev, p0, K, floor, label)
                    assert got[2] > 0, label
                    if f == 0:       # floor = 1: q rows sum to one and every p is below one, so every term is floored: log 1
                        assert ctx.cv_heldout_loglik(0, 1.0) == (0.0, got[1], got[1]), label
        ctx.cv_hold_out(-1)


@pytest.mark.parametrize("K,alleles", sorted(EDGES))
def test_heldout_score_on_either_side_of_every_edge(K, alleles, contexts):
    """k_cv_score takes its lanes and its staging from the geometry k_impute has (lane_pass_geometry_of; tests/feature_geometry.py):
    the (K, alleles) pairs on either side of every edge of it, with a second, partial tile of individuals at every workgroup size
    (I = 257) and a partial block of 8 loci (L = 9)"""
    ctx = contexts[0]
    I, L, pl, F = 257, 9, 2, 5
    ua, _, geno = iu.impute_dataset(I, L, pl, alleles, 0.05, seed=K + alleles, specials=False)
    assert int(ua.max()) == alleles + 1
    ctx.set_genotypes(ua, geno)
    folds = forced_folds(windows()["first"], geno, F)
    ctx.cv_set_folds(folds, F)
    q0, p0 = random_params(I, ua, K, seed=K)
    for f in range(F):
        ctx.cv_hold_out(f)
        ctx.set_model(K, admixture=1)
        ctx.set_q(0, q0)
        ctx.set_p(0, p0)
        got = check_score(ctx, ua, geno, folds, f, q0, p0, K, 1.0 / (I * pl + 1), "edge K%d alleles%d f%d" % (K, alleles, f))
        assert got[1] > 0
    ctx.cv_hold_out(-1)


def test_floor_one_scores_exactly_zero(contexts):
    """parameters that are probabilities (rows sum to one, nothing clipped up): t < 1 for every copy, so floor = 1 floors them all"""
    ctx = contexts[0]
    ua, geno = cu.cv_dataset(67, 61, 2, seed=5)
    ctx.set_genotypes(ua, geno)
    folds = cu.serial_folds(windows()["first"], 67, 61, 2)
    ctx.cv_set_folds(folds, 2)
    ctx.cv_hold_out(1)
    for K in (2, 27):
        ctx.set_model(K)
        q0, p0 = random_params(67, ua, K, seed=1, lower_bound=0.0)
        ctx.set_q(0, q0 * 0.999)
        ctx.set_p(0, p0)
        s, n, nf = ctx.cv_heldout_loglik(0, 1.0)
        assert n == int(((folds == 1)[:, :, None] & (geno != cu.MISSING)).sum()) and nf == n and s == 0.0 and not np.signbit(s)


def test_score_refusals(contexts):
    ctx = contexts[0]
    ua, geno = cu.cv_dataset(67, 61, 2, seed=5)
    lib = ctx.lib
    s = C.c_double()

    def score(slot=0, floor=0.01):
        return status_of(lib.mchip_cv_heldout_loglik(ctx.h, slot, floor, C.byref(s), None, None))

    ctx.set_genotypes(ua, geno)
    ctx.set_model(2)
    assert score() == "STATE"                                       # no folds
    ctx.cv_draw_folds(windows()["first"], 5)
    assert score() == "STATE"                                       # no fold held out
    ctx.cv_hold_out(1)
    assert score() == "OK"
    for floor in (0.0, -1.0, 1.0000001, float("nan")):
        assert score(floor=floor) == "INVALID", floor
    assert score(slot=3) == "INVALID"
    ctx.cv_hold_out(-1)
    assert score() == "STATE"
    ctx.cv_hold_out(0)
    ctx.set_model(2, admixture=0)
    assert score() == "UNSUPPORTED"                                 # the mixture model
    ctx.set_genotypes(ua, geno)
    assert score() == "STATE"                                       # no folds, no model


# ---------------------------------------------------------------- 5. the host driver

def device_of(fit):
    """the model's own context, seen through the C-ABI wrappers"""
    ctx = hip.Context.__new__(hip.Context)
    ctx.lib = hip.load()
    ctx.h = C.c_void_p(fit.mod.dev)
    ctx.I, ctx.L, ctx.ploidy = fit.geno.shape
    ctx.T, ctx.K, ctx.indiv_q = fit.T, fit.K, fit.indiv_q
    ctx.close = lambda: None                                        # the Fit owns it
    return ctx


@pytest.mark.parametrize("accel,constrained", [(0, 0), (3, 0), (3, 1)])
def test_driver_equals_the_call_sequence(accel, constrained):
    I, L, K, F, seed = 120, 150, 3, 4, 11
    ua, geno = cu.cv_dataset(I, L, 2, seed=31)
    geno[5] = cu.MISSING                                            # an individual without a copy: its row is reported as NaN
    fit = host.Fit(ua, geno, K, admixture=1, eta_constrained=constrained, accel_scheme=accel, seed=seed, max_iter=60)
    try:
        fit.fit_unit(seed, 0)
        slot = fit.mod.pindex
        state = (fit.mod.logL, fit.mod.n_iter, fit.mod.pindex, fit.mod.findex, fit.mod.tindex, fit.mod.converged, fit.mod.delta_index)
        q, p = fit.get_q(slot), fit.get_p(slot)
        assert constrained or np.isnan(q[5]).all()
        cv, sum_log, n_copies, n_floored, per_fold = fit.cross_validate(F)
        assert state == (fit.mod.logL, fit.mod.n_iter, fit.mod.pindex, fit.mod.findex, fit.mod.tindex, fit.mod.converged, fit.mod.delta_index)
        assert bits(fit.get_q(slot)) == bits(q) and bits(fit.get_p(slot)) == bits(p)
        # the same, call by call
        ctx = device_of(fit)
        assert bits(ctx.get_genotypes()) == bits(geno)
        floor = 1.0 / (I * 2 + 1)
        window = ob.glibc_window(seed)[0]
        ctx.cv_draw_folds(window, F)
        assert np.array_equal(ctx.cv_get_folds(), cu.serial_folds(window, I, L, F))
        total, copies, floored = 0.0, 0, 0
        for f in range(F):
            ctx.cv_hold_out(f)
            fit.reset()
            ctx.set_q(0, q)
            ctx.set_p(0, p)
            fit.em()
            assert fit.mod.fatal == 0
            s, n, nf = ctx.cv_heldout_loglik(fit.mod.pindex, floor)
            assert (bits(np.float64(s)), n, nf, fit.mod.n_iter) == (bits(np.float64(per_fold[f][0])),) + tuple(per_fold[f][1:]), f
            total += s
            copies += n
            floored += nf
        ctx.cv_hold_out(-1)
        assert (copies, floored) == (n_copies, n_floored) and copies == int((geno != cu.MISSING).sum())
        assert bits(np.float64(total)) == bits(np.float64(sum_log)) and bits(np.float64(-total / copies)) == bits(np.float64(cv))
        assert np.isfinite(cv)
    finally:
        fit.close()


# ---------------------------------------------------------------- 6. it chooses K

# CPU values for this very data set, seed and folds (oracle EM with SQUAREM S3 from one random initialisation, each fold's fit
# warm-started from the full-data estimate, tests/cv_util.heldout_score on the folds of the serial stream, floor 1 / 601):
#   K = 1: 0.5776337908    K = 2: 0.4431199137    K = 3: 0.2964503547
# smallest gap to K = 3: 0.1466695590; the margin asserted below is half of it
CV_CPU = {1: 0.5776337908, 2: 0.4431199137, 3: 0.2964503547}
CV_MARGIN = 0.5 * min(CV_CPU[1] - CV_CPU[3], CV_CPU[2] - CV_CPU[3])


def test_cross_validation_chooses_k():
    seed = 20261017
    ua, geno = cu.clustered_dataset(300, 400, 3, seed)
    cv = {}
    for K in (1, 2, 3):
        fit = host.Fit(ua, geno, K, admixture=1, accel_scheme=3, seed=seed)
        try:
            fit.fit_unit(seed, 0)
            assert fit.mod.fatal == 0
            cv[K], _, n_copies, _, _ = fit.cross_validate(5)
            assert n_copies == geno.size
        finally:
            fit.close()
    print("CV error by K:", cv, "CPU:", CV_CPU, "margin:", CV_MARGIN)
    assert cv[3] + CV_MARGIN < cv[2] and cv[3] + CV_MARGIN < cv[1], cv
