"""-m gpu: a data set made of a selection of loci with repeats (mchip_resample_loci, multiclust_amd/csrc/mchip_resample.hip):
the selection installed against the numpy gather and against a fresh upload of the gathered data, fits included, bit for bit; the
base restored; a base that came from a .bed upload; refusals and what they leave behind."""
import ctypes as C

import numpy as np
import pytest

import bedfiles as bf
from bits import bits
import cv_util as cu
from device_util import status_of
import oracle_bind as ob
import se_util as su
from multiclust_amd import hip
from synth import random_params

pytestmark = pytest.mark.gpu

SHAPES = [(I, L, pl) for I in (67, 300) for L in (61, 130) for pl in (1, 2, 4)]
MODELS = {"individual": (1, 0), "shared": (1, 1), "mixture": (0, 0)}


@pytest.fixture(scope="module")
def contexts():
    ctxs = [hip.Context(0) for _ in range(3)]
    yield ctxs
    for c in ctxs:
        c.close()


def src_lists(ua, geno, seed):
    I, L, _ = geno.shape
    rng = np.random.default_rng(seed)
    miss = geno == su.MISSING
    no_missing = np.flatnonzero(~miss.any(axis=(0, 2)))
    blind3 = np.flatnonzero(miss[3].all(axis=1))          # loci at which individual 3 has no observed copy
    assert 1 in no_missing and len(blind3) >= L // 3 - 1
    lists = {
        "identity": np.arange(L),
        "reverse": np.arange(L)[::-1],
        "single": np.array([L // 2]),
        "repeats": rng.integers(0, L, size=L + 17),
        "locus0": np.zeros(L, dtype=np.int64),
        "no_missing": rng.choice(no_missing, size=max(5, len(no_missing) + 2)),
        "blind3": rng.choice(blind3, size=len(blind3) + 5),
    }
    assert len(np.unique(lists["repeats"])) < L + 17 and int(ua[lists["locus0"]].sum()) >= 35 * L
    return {k: v.astype(np.int32) for k, v in lists.items()}


def check_data(ctx, want_ua, want):
    assert (ctx.L, ctx.T) == (want.shape[1], int(want_ua.sum()))
    assert bits(ctx.get_genotypes()) == bits(want)
    assert ctx.data_counts() == su.data_counts(want)
    assert ctx.empty_individuals() == cu.empty_individuals(want)


def compare_fits(held, fresh, ua, K, model, install, steps=5):
    """five EM steps of `held` (its data set installed by install()) and of `fresh` (which holds the same data uploaded): logL, Q, P
    and the expected counts as bits"""
    admixture, constrained = MODELS[model]
    q0, p0 = random_params(held.I, ua, K, seed=K)
    if model != "individual":
        q0 = q0.mean(axis=0)
    for ctx in (held, fresh):
        if ctx is held:
            install()                                     # every model starts from a newly installed selection
        ctx.set_model(K, admixture=admixture, eta_constrained=constrained)
        ctx.set_q(0, q0)
        ctx.set_p(0, p0)
    for step in range(steps):
        a, b = held.em_step(0, 0), fresh.em_step(0, 0)
        assert np.isfinite(b) and bits(np.float64(a)) == bits(np.float64(b)), (model, K, step, a, b)
    assert bits(held.get_q(0)) == bits(fresh.get_q(0)) and bits(held.get_p(0)) == bits(fresh.get_p(0)), (model, K)
    assert bits(held.expected_counts()) == bits(fresh.expected_counts()), (model, K)


# ---------------------------------------------------------------- 1. the selection installed

@pytest.mark.parametrize("I,L,pl", SHAPES)
def test_resample_installs_the_gathered_set(I, L, pl, contexts):
    held, fresh, copy = contexts
    ua, geno = su.resample_dataset(I, L, pl, seed=100 * I + 10 * L + pl)
    assert ua[0] >= 35 and not (geno[:, 1] == su.MISSING).any() and (geno == su.MISSING).any()
    held.set_genotypes(ua, geno)
    base_empty = cu.empty_individuals(geno)
    for name, src in src_lists(ua, geno, seed=I + L + pl).items():
        want_ua, want = ua[src], np.ascontiguousarray(geno[:, src, :])
        held.resample_loci(src)
        check_data(held, want_ua, want)
        if name == "blind3":                              # individual 3 is observed in the base and empty in the selection
            assert cu.empty_individuals(want)[0] == base_empty[0] + 1 and (want[3] == su.MISSING).all()
        if name == "no_missing":                          # the kernels' other variant: no missing copy anywhere
            assert not (want == su.MISSING).any()
        copy.copy_genotypes(held)
        check_data(copy, want_ua, want)
        fresh.set_genotypes(want_ua, want)
        assert held.data_counts() == fresh.data_counts()
        for model in MODELS:
            for K in ((2, 8, 28) if (I, L) == (67, 61) else (8,)):
                compare_fits(held, fresh, want_ua, K, model, lambda: held.resample_loci(src))


# ---------------------------------------------------------------- 2. the base restored

def test_base_is_restored_and_every_selection_gathers_from_it(contexts):
    held, fresh, _ = contexts
    I, L, pl = 67, 130, 2
    ua, geno = su.resample_dataset(I, L, pl, seed=9)
    held.set_genotypes(ua, geno)
    fresh.set_genotypes(ua, geno)
    counts, empty = held.data_counts(), held.empty_individuals()
    lists = src_lists(ua, geno, seed=3)
    for name in ("repeats", "locus0", "blind3"):
        held.resample_loci(lists[name])
    held.resample_loci(None)
    check_data(held, ua, geno)
    assert held.data_counts() == counts and held.empty_individuals() == empty
    for model in MODELS:
        compare_fits(held, fresh, ua, 8, model, lambda: held.resample_loci(None))
    # a second chain: a list applied twice gives the same data set both times, the gather of the BASE (indices of `repeats` applied
    # to the previous selection would address other loci, and its indices above the length of `single` would be out of range)
    src = lists["repeats"]
    want_ua, want = ua[src], np.ascontiguousarray(geno[:, src, :])
    held.resample_loci(lists["single"])
    for _ in range(2):
        held.resample_loci(src)
        check_data(held, want_ua, want)
    assert not np.array_equal(want[:, src % want.shape[1], :], want)
    held.resample_loci(None)
    check_data(held, ua, geno)


# ---------------------------------------------------------------- 3. a base installed from packed records

def test_bed_base(contexts):
    held, fresh, plain = contexts
    I, L = 67, 130
    codes = bf.draw_codes(I, L, missing=0.03, seed=5)
    ua = held.set_genotypes_bed(I, bf.pack(codes))
    geno = held.get_genotypes()
    plain.set_genotypes(ua, geno)                         # the same data set, uploaded unpacked
    assert (geno == su.MISSING).any() and cu.empty_individuals(geno)[0] == 1 and (ua == 0).any()
    rng = np.random.default_rng(2)
    for src in (rng.integers(0, L, size=L + 17).astype(np.int32), np.flatnonzero(ua > 0)[::-1].astype(np.int32)):
        want_ua, want = ua[src], np.ascontiguousarray(geno[:, src, :])
        held.resample_loci(src)
        check_data(held, want_ua, want)
        fresh.set_genotypes(want_ua, want)
        for model in MODELS:
            compare_fits(held, fresh, want_ua, 8, model, lambda: held.resample_loci(src))
    held.resample_loci(None)
    check_data(held, ua, geno)
    for model in MODELS:
        compare_fits(held, plain, ua, 8, model, lambda: held.resample_loci(None))


# ---------------------------------------------------------------- 4. refusals and state

def test_refusals_and_state(contexts):
    ctx, fresh, _ = contexts
    lib = ctx.lib
    I, L, pl = 67, 61, 2
    ua, geno = su.resample_dataset(I, L, pl, seed=4)

    def resample(c, src):
        if src is None:
            return status_of(lib.mchip_resample_loci(c.h, None, 0))
        s = np.ascontiguousarray(src, dtype=np.int32)
        return status_of(lib.mchip_resample_loci(c.h, s.ctypes.data, s.size))

    empty = hip.Context(0)
    assert resample(empty, [0, 1]) == "STATE"                             # no data set
    assert resample(empty, None) == "STATE"
    empty.close()

    ctx.set_genotypes(ua, geno)
    assert resample(ctx, None) == "STATE"                                 # no saved base
    s = np.zeros(4, np.int32)
    assert status_of(lib.mchip_resample_loci(ctx.h, s.ctypes.data, 0)) == "INVALID"     # L2 < 1
    assert status_of(lib.mchip_resample_loci(ctx.h, s.ctypes.data, -3)) == "INVALID"
    assert resample(ctx, None) == "STATE"                                 # ... and a refused call saves no base

    # a hold-out in force
    window = ob.glibc_window(11)[0]
    ctx.cv_draw_folds(window, 5)
    ctx.cv_hold_out(2)
    assert resample(ctx, [0, 1]) == "STATE"
    ctx.cv_hold_out(-1)
    assert bits(ctx.get_genotypes()) == bits(geno)

    # an index out of range: the data set, the folds and the model stay, usable and unchanged
    K = 3
    q0, p0 = random_params(I, ua, K, seed=1)
    ctx.set_model(K)
    ctx.set_q(0, q0)
    ctx.set_p(0, p0)
    fresh.set_genotypes(ua, geno)
    fresh.set_model(K)
    fresh.set_q(0, q0)
    fresh.set_p(0, p0)
    for bad in ([0, L], [-1], [3, 2 ** 31 - 1, 0]):
        assert resample(ctx, bad) == "INVALID", bad
    assert bits(ctx.get_genotypes()) == bits(geno) and bits(ctx.get_q(0)) == bits(q0) and bits(ctx.get_p(0)) == bits(p0)
    assert np.array_equal(ctx.cv_get_folds(), cu.serial_folds(window, I, L, 5))
    assert bits(np.float64(ctx.em_step(0, 0))) == bits(np.float64(fresh.em_step(0, 0)))
    assert bits(ctx.get_q(0)) == bits(fresh.get_q(0)) and bits(ctx.get_p(0)) == bits(fresh.get_p(0))

    # a selection drops the model and the folds drawn before it; the base stays through refused calls
    src = np.array([5, 5, 0, 60, 17], np.int32)
    ctx.resample_loci(src)
    n = C.c_int()
    assert status_of(lib.mchip_q_length(ctx.h, C.byref(n))) == "STATE"    # no model
    out = np.empty((I, len(src)), np.uint8)
    assert status_of(lib.mchip_cv_get_folds(ctx.h, out.ctypes.data)) == "STATE"
    assert status_of(lib.mchip_cv_hold_out(ctx.h, 0)) == "STATE"
    assert resample(ctx, [0, L]) == "INVALID"                             # indices are the base's: L - 1 is in range, 5 is not the limit
    assert bits(ctx.get_genotypes()) == bits(geno[:, src, :])
    ctx.resample_loci(np.array([L - 1, 7], np.int32))
    assert bits(ctx.get_genotypes()) == bits(geno[:, [L - 1, 7], :])
    # a hold-out on a selection is in force like any other, and released it leaves the base where it was
    ctx.cv_draw_folds(window, 2)
    ctx.cv_hold_out(1)
    assert resample(ctx, None) == "STATE" and resample(ctx, [1]) == "STATE"
    ctx.cv_hold_out(-1)
    ctx.resample_loci(None)
    assert bits(ctx.get_genotypes()) == bits(geno) and ctx.empty_individuals() == cu.empty_individuals(geno)

    # any other call that installs a data set drops the base
    ctx.resample_loci(src)
    ctx.set_genotypes(ua[src], np.ascontiguousarray(geno[:, src, :]))
    assert resample(ctx, None) == "STATE"
    ctx.resample_loci(np.array([4, 4], np.int32))                         # the base is now the five-locus set
    assert resample(ctx, [5]) == "INVALID"
    assert bits(ctx.get_genotypes()) == bits(geno[:, src[[4, 4]], :])
    fresh.copy_genotypes(ctx)
    assert resample(fresh, None) == "STATE"                               # a copy is a data set of its own, without a base


# ---------------------------------------------------------------- 5. every installer drops both saved sets

INSTALLERS = ["same_shape", "other_shape", "bed", "simulate", "simulate_mixture", "copy"]


@pytest.mark.parametrize("installer", INSTALLERS)
def test_every_installer_drops_the_folds_the_hold_out_and_the_base(installer, contexts):
    """a selection with a fold held out of it (the base of the selections and the full selection both saved), then a call that
    installs a data set: no folds, no hold-out and no base afterwards, and the data set is the one a fresh context gets from the
    same call, one EM step included, bit for bit"""
    ctx, source, _ = contexts
    lib = ctx.lib
    I, L, pl, K = 67, 61, 2, 3
    ua, geno = su.resample_dataset(I, L, pl, seed=4)
    src = np.array([5, 5, 0, 60, 17], np.int32)
    window = ob.glibc_window(11)[0]
    ctx.set_genotypes(ua, geno)
    ctx.resample_loci(src)
    ctx.cv_draw_folds(window, 2)
    ctx.cv_hold_out(1)

    sel_ua, sel = ua[src], np.ascontiguousarray(geno[:, src, :])
    sim_q, sim_p = random_params(I, ua, K, seed=2)
    packed = bf.pack(bf.draw_codes(I, L, missing=0.03, seed=5))
    source.set_genotypes(ua, geno)
    install = {
        "same_shape": lambda c: c.set_genotypes(sel_ua, sel),          # the shape held: set_shape keeps every buffer
        "other_shape": lambda c: c.set_genotypes(ua, geno),
        "bed": lambda c: c.set_genotypes_bed(I, packed),
        "simulate": lambda c: c.simulate_genotypes(I, L, pl, ua, window, K, sim_q, sim_p),
        "simulate_mixture": lambda c: c.simulate_genotypes_mixture(I, L, pl, ua, window, K, sim_q.mean(axis=0), sim_p),
        "copy": lambda c: c.copy_genotypes(source),
    }[installer]
    fresh = hip.Context(0)
    try:
        install(ctx)
        install(fresh)
        out = np.empty((ctx.I, ctx.L), np.uint8)
        assert status_of(lib.mchip_cv_get_folds(ctx.h, out.ctypes.data)) == "STATE"
        assert status_of(lib.mchip_cv_hold_out(ctx.h, 0)) == "STATE"
        assert status_of(lib.mchip_resample_loci(ctx.h, None, 0)) == "STATE"
        assert (ctx.I, ctx.L, ctx.ploidy, ctx.T) == (fresh.I, fresh.L, fresh.ploidy, fresh.T)
        assert bits(ctx.get_genotypes()) == bits(fresh.get_genotypes())
        assert ctx.data_counts() == fresh.data_counts()
        assert ctx.empty_individuals() == fresh.empty_individuals()
        if installer == "same_shape":
            assert bits(ctx.get_genotypes()) == bits(sel)
        q0, p0 = random_params(I, ctx._ua, K, seed=1)
        for c in (ctx, fresh):
            c.set_model(K)
            c.set_q(0, q0)
            c.set_p(0, p0)
        a, b = ctx.em_step(0, 0), fresh.em_step(0, 0)
        assert np.isfinite(b) and bits(np.float64(a)) == bits(np.float64(b)), (installer, a, b)
        assert bits(ctx.get_q(0)) == bits(fresh.get_q(0)) and bits(ctx.get_p(0)) == bits(fresh.get_p(0)), installer
    finally:
        fresh.close()
