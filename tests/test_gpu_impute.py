"""-m gpu: mchip_impute_missing (multiclust_amd/csrc/mchip_impute.hip) against the numpy form of its rule (tests/impute_util.py).

The edges of the kernel as built (lane_pass_geometry_of): a workgroup has 256, 128 or 64 lanes -- the most whose q rows (K | 1
doubles each) fit into 64 KiB - 512 of LDS beside 2 KiB of reduction space and the staged P rows of a block of 8 loci (8 max_M
(K | 1) doubles) -- and when not even 64 lanes leave room for the P rows, they are read from memory.  With max_M = 3 (two alleles
and the phantom slot) K = 27 | 28 is the edge between 256 and 128 lanes and K = 51 | 52 the one between 128 and 64; with max_M = 5
they are K = 25 | 26 and 45 | 46; at K = 64 the rows are staged up to max_M = 7 and read from memory from max_M = 8 on (35 alleles
included).  EDGES has a case on either side of each, and geometry() (tests/feature_geometry.py, held against the C++ by
test_feature_geometry_cpu.py) restates the arithmetic so that a case that no longer sits where it is meant to fails.
A workgroup walks several blocks of 8 loci (and reuses its staged rows) only when there are more
blocks than 16 x compute units / individual tiles: the LONG case.  A block of 8 loci is partial at L = 1, 7, 9 and 130."""
import ctypes as C
import math

import numpy as np
import pytest

from bits import bits
import cv_util as cu
from device_util import contexts, status_of
import impute_util as iu
from feature_geometry import EDGES, geometry
from multiclust_amd import hip
from synth import random_params

pytestmark = pytest.mark.gpu
MISSING = iu.MISSING
KS = [1, 2, 8, 27, 28, 64]


def install(ctx, ua, geno, K, q, p, shared=False, projection=1):
    ctx.set_genotypes(ua, geno)
    ctx.set_model(K, admixture=1, eta_constrained=int(shared), do_projection=projection)
    ctx.set_q(0, q[0] if shared else q)
    ctx.set_p(0, p)


def check(ctx, ua, n_real, geno, q, p, K, slot=0):
    """every assertion of the rule on one call; q: what the device holds in `slot`, [I][K] or [K]"""
    out, conf, nf, nl, ng, sc = ctx.impute_missing(slot, n_real)
    ii, ll, r = iu.missing_genotypes(geno)
    t, valid = iu.predictive(ua, n_real, ii, ll, q, p)
    ok = iu.fillable(t, valid)
    miss = geno[ii, ll] == MISSING
    vals = out[ii, ll].astype(np.int64)
    # observed bytes, and the copies that cannot be filled
    assert np.array_equal(out[geno != MISSING], geno[geno != MISSING])
    still = ((vals == MISSING) & miss).sum(axis=1)
    assert np.array_equal(still[~ok], r[~ok]) and not still[ok].any()
    # counts
    assert (nf, nl, ng) == (int(r[ok].sum()), int(r[~ok].sum()), int(ok.sum()))
    if not ok.any():
        assert sc == 0.0 and not conf.any()
        return out, conf, sc
    # the multiset: real alleles only, as probable as the reference's mode up to the rounding of both sides
    c_dev = iu.filled_counts(geno, out, ii, ll, t.shape[1])[ok]
    assert (c_dev >= 0).all() and np.array_equal(c_dev.sum(axis=1), r[ok]) and not (c_dev[~valid[ok]] > 0).any()
    c_ref = iu.greedy_counts(t, valid, r)[ok]
    pr_dev, pr_ref = iu.multiset_prob(t[ok], valid[ok], c_dev), iu.multiset_prob(t[ok], valid[ok], c_ref)
    M = np.asarray(n_real)[ll][ok]
    bound = r[ok] * (K + M + 8) * 2.0 ** -51
    assert (pr_dev >= pr_ref * (1 - bound)).all()
    # the confidence: the probability of what was written; 0 elsewhere
    got = conf[ii[ok], ll[ok]]
    assert (np.abs(got - pr_dev) <= bound * pr_dev).all()
    rest = conf.copy()
    rest[ii[ok], ll[ok]] = 0
    assert not rest.any()
    total = math.fsum(got)
    assert abs(sc - total) <= (ng + K + int(M.max()) + 8) * 2.0 ** -52 * total
    # ascending by allele index over the missing positions, in copy order
    prev = np.full(len(ii), -1)
    for a in range(geno.shape[2]):
        sel = miss[:, a] & ok
        assert (vals[sel, a] >= prev[sel]).all()
        prev[sel] = vals[sel, a]
    return out, conf, sc


SWEEP = []
for n, (I, L) in enumerate((I, L) for I in (1, 63, 65, 257) for L in (1, 7, 9, 130)):
    SWEEP.append((I, L, 1 + (n + n // 4) % 4, KS[n % 6], (2, 4)[(n // 2) % 2], (0.05, 0.5)[n % 2], n % 3 == 1))


@pytest.mark.parametrize("I,L,pl,K,alleles,missing,shared", SWEEP)
def test_rule_over_shapes(I, L, pl, K, alleles, missing, shared, contexts):
    ctx = contexts[0]
    ua, n_real, geno = iu.impute_dataset(I, L, pl, alleles, missing, seed=7 * I + L)
    q, p = random_params(I, ua, K, seed=I + L + K)
    install(ctx, ua, geno, K, q, p, shared)
    check(ctx, ua, n_real, geno, q[0] if shared else q, p, K)


@pytest.mark.parametrize("K,alleles", sorted(EDGES))
def test_rule_on_either_side_of_every_edge(K, alleles, contexts):
    ctx = contexts[0]
    I, L, pl = 257, 9, 2
    ua, n_real, geno = iu.impute_dataset(I, L, pl, alleles, 0.5, seed=K + alleles)
    assert int(ua.max()) == alleles + 1 and geometry(K, alleles + 1) == EDGES[(K, alleles)]
    q, p = random_params(I, ua, K, seed=K)
    install(ctx, ua, geno, K, q, p)
    check(ctx, ua, n_real, geno, q, p, K)


def test_a_workgroup_walks_many_blocks(contexts):
    """LONG: more blocks of 8 loci than workgroups wanted, so every workgroup stages rows again and again"""
    ctx = contexts[0]
    I, L, pl, K = 5, 33001, 1, 3
    _, cu_count, _ = ctx.device_info()
    assert (L + 7) // 8 > 16 * cu_count
    ua, n_real, geno = iu.impute_dataset(I, L, pl, 3, 0.3, seed=1)
    q, p = random_params(I, ua, K, seed=2)
    install(ctx, ua, geno, K, q, p)
    check(ctx, ua, n_real, geno, q, p, K)


def test_exact_tie_and_phantom_slot(contexts):
    """two identical P columns: the lower index first, then one of each; the phantom slot holds the largest frequency and is never
    chosen.  Every number is a power of two: the reference is exact."""
    ctx = contexts[0]
    I, L, K = 65, 9, 2
    for pl in (1, 2, 3, 4):
        geno = np.random.default_rng(pl).integers(0, 2, size=(I, L, pl)).astype(np.uint8)
        geno[np.random.default_rng(pl + 10).random(geno.shape) < 0.5] = MISSING
        ua, n_real = np.full(L, 3, np.int32), np.full(L, 2, np.int32)
        q = np.full((I, K), 0.5)
        p = np.tile(np.array([0.25, 0.25, 0.5]), (K, L))
        install(ctx, ua, geno, K, q, p)
        out, conf, sc = check(ctx, ua, n_real, geno, q, p, K)
        ii, ll, r = iu.missing_genotypes(geno)
        c = iu.filled_counts(geno, out, ii, ll, 2)
        assert np.array_equal(c[:, 0], (r + 1) // 2) and np.array_equal(c[:, 1], r // 2)
        want = np.array([0, 0.5, 0.5, 0.375, 0.375])[r]             # r! / (c0! c1!) 2^-r
        assert np.array_equal(conf[ii, ll], want) and not (out == 2).any()


def test_unfillable_copies_stay_missing(contexts):
    """no candidate (n_real = 0, also where the locus has allele columns) and candidates that are all zero (projection off)"""
    ctx = contexts[0]
    I, L, pl, K = 63, 9, 2, 3
    ua, n_real, geno = iu.impute_dataset(I, L, pl, 3, 0.3, seed=5)
    q, p = random_params(I, ua, K, seed=6)
    toff = np.concatenate(([0], np.cumsum(ua)))
    p[:, toff[1]:toff[1] + n_real[1]] = 0.0                      # locus 1: every real allele at frequency 0, the phantom slot has the rest
    n_real = n_real.copy()
    n_real[3] = 0                                                # locus 3: the caller names no candidate
    install(ctx, ua, geno, K, q, p, projection=0)
    assert np.array_equal(ctx.get_p(0), p)
    out, conf, _ = check(ctx, ua, n_real, geno, q, p, K)
    for l in (1, 3, 4):
        assert np.array_equal(out[:, l], geno[:, l]) and not conf[:, l].any()
    assert (geno[:, 1] == MISSING).any() and (geno[:, 3] == MISSING).any()


def test_without_missing_data_nothing_changes(contexts):
    ctx = contexts[0]
    ua, n_real, geno = iu.impute_dataset(65, 9, 2, 4, 0.0, seed=3, specials=False)
    assert not (geno == MISSING).any() and np.array_equal(ua, n_real)
    q, p = random_params(65, ua, 8, seed=4)
    install(ctx, ua, geno, 8, q, p)
    out, conf, nf, nl, ng, sc = ctx.impute_missing(0, n_real)
    assert np.array_equal(out, geno) and np.array_equal(out, ctx.get_genotypes())
    assert (nf, nl, ng, sc) == (0, 0, 0, 0.0) and not conf.any()


def test_q_as_the_device_stores_it(contexts):
    """after an M step the row of an individual without an observed copy stands for NaN (mchip_get_q) and holds 1 / K"""
    ctx = contexts[0]
    I, L, pl, K = 63, 9, 2, 3
    ua, n_real, geno = iu.impute_dataset(I, L, pl, 2, 0.2, seed=8)
    assert (geno[1] == MISSING).all()
    q, p = random_params(I, ua, K, seed=9)
    install(ctx, ua, geno, K, q, p)
    ctx.em_step(0, 1)
    q1, p1 = ctx.get_q(1), ctx.get_p(1)
    assert np.isnan(q1[1]).all() and not np.isnan(np.delete(q1, 1, axis=0)).any()
    q1[1] = 1.0 / K
    check(ctx, ua, n_real, geno, q1, p1, K, slot=1)


def test_same_state_same_bits(contexts):
    ctx = contexts[0]
    ua, n_real, geno = iu.impute_dataset(257, 130, 2, 4, 0.5, seed=11)
    q, p = random_params(257, ua, 8, seed=12)
    install(ctx, ua, geno, 8, q, p)
    a, b = ctx.impute_missing(0, n_real), ctx.impute_missing(0, n_real)
    assert bits(a[0]) == bits(b[0]) and bits(a[1]) == bits(b[1]) and a[2:5] == b[2:5]
    assert np.float64(a[5]).tobytes() == np.float64(b[5]).tobytes() and a[4] > 0
    # without the confidences: the same genotypes and figures
    c = ctx.impute_missing(0, n_real, conf=False)
    assert c[1] is None and bits(c[0]) == bits(a[0]) and c[2:] == a[2:]


def test_state_is_untouched(contexts):
    """a context that filled its data set goes on exactly as one that did not: the held S-side sums, the next EM step, Q and P"""
    ua, n_real, geno = iu.impute_dataset(65, 130, 2, 4, 0.2, seed=13)
    q, p = random_params(65, ua, 8, seed=14)
    seen = []
    for n, ctx in enumerate(contexts):
        install(ctx, ua, geno, 8, q, p)
        ll0 = ctx.loglik_prefetch(0)                             # the S-side sums of slot 0 are held
        if n == 0:
            ctx.impute_missing(0, n_real)
        ll1 = ctx.em_step(0, 1)                                  # uses them
        if n == 0:
            ctx.impute_missing(1, n_real)
        ll2 = ctx.em_step(1, 2)
        seen.append((ll0, ll1, ll2, bits(ctx.get_q(0)), bits(ctx.get_p(0)), bits(ctx.get_q(2)), bits(ctx.get_p(2)),
                     bits(ctx.expected_counts()), bits(ctx.get_genotypes()), ctx.data_counts(), ctx.empty_individuals()))
    assert seen[0] == seen[1]
    assert np.array_equal(contexts[0].get_genotypes(), geno)


def test_under_a_hold_out_the_hidden_genotypes_are_filled(contexts):
    """clustered data, a fifth of the genotypes hidden by a hold-out, fitted on the device: the filled genotypes are the rule's on
    the device's own Q and P, and they match the hidden truth far more often than the locus's most frequent genotype does"""
    ctx = contexts[0]
    I, L, clusters = 72, 400, 3
    ua, truth = cu.clustered_dataset(I, L, clusters, 11)
    folds = np.random.default_rng(111).integers(0, 5, size=(I, L)).astype(np.uint8)
    hidden = folds == 0
    ctx.set_genotypes(ua, truth)
    ctx.cv_set_folds(folds, 5)
    ctx.set_model(clusters)
    ctx.cv_hold_out(0)
    q0, p0 = random_params(I, ua, clusters, seed=7)
    ctx.set_q(0, q0)
    ctx.set_p(0, p0)
    for _ in range(300):
        ctx.em_step(0, 0, sync=False)
    ctx.synchronize()
    q, p = ctx.get_q(0), ctx.get_p(0)
    geno = cu.masked(truth, folds, 0)
    assert np.array_equal(ctx.get_genotypes(), geno) and not np.isnan(q).any()
    out, conf, _ = check(ctx, ua, ua, geno, q, p, clusters)                  # (no phantom slot: the mask adds none)
    assert not (out == MISSING).any() and np.array_equal(out[~hidden], truth[~hidden])
    # equal to the numpy rule, but where two multisets are within rounding of each other
    ref = iu.impute_reference(ua, ua, geno, q, p)
    differ = (np.sort(out, axis=2) != np.sort(ref["filled"], axis=2)).any(axis=2)
    print("filled genotypes that differ from the numpy rule's (near ties): %d of %d" % (differ.sum(), hidden.sum()))
    # (check() above has held each of them to the near-tie rule: as probable as the reference's mode up to rounding)
    assert differ.sum() <= 0.01 * hidden.sum()
    conc, base = iu.concordance(truth, out, hidden), iu.modal_baseline(truth, hidden)
    print("concordance %.4f, modal genotype %.4f, mean confidence %.4f" % (conc, base, conf[hidden].mean()))
    assert conc >= base + 0.10
    ctx.cv_hold_out(-1)
    assert np.array_equal(ctx.get_genotypes(), truth)


def test_errors_leave_the_arrays_alone(contexts):
    ctx = contexts[0]
    lib = ctx.lib
    I, L, pl, K = 9, 7, 2, 2
    ua, n_real, geno = iu.impute_dataset(I, L, pl, 2, 0.3, seed=15)
    q, p = random_params(I, ua, K, seed=16)
    out = np.full((I, L, pl), 0xAB, dtype=np.uint8)
    conf = np.full((I, L), -3.0)
    cnt = [C.c_uint64(77) for _ in range(3)]
    sc = C.c_double(-5.0)

    def call(c, slot, nr, g=out):
        return status_of(lib.mchip_impute_missing(c.h, slot, None if nr is None else nr.ctypes.data, None if g is None else g.ctypes.data,
                                                  conf.ctypes.data, C.byref(cnt[0]), C.byref(cnt[1]), C.byref(cnt[2]),
                                                  C.byref(sc)))

    fresh = hip.Context(0)
    assert call(fresh, 0, n_real) == "STATE"                     # no data set
    fresh.set_genotypes(ua, geno)
    assert call(fresh, 0, n_real) == "STATE"                     # no model
    fresh.set_model(K, admixture=0)
    assert call(fresh, 0, n_real) == "UNSUPPORTED"               # the mixture model
    fresh.close()
    install(ctx, ua, geno, K, q, p)
    for slot in (-1, 3):
        assert call(ctx, slot, n_real) == "INVALID"
    assert call(ctx, 0, None) == "INVALID" and call(ctx, 0, n_real, None) == "INVALID"
    for l, v in ((0, -1), (L - 1, int(ua[L - 1]) + 1), (4, 1)):  # (locus 4 has no allele column)
        bad = n_real.copy()
        bad[l] = v
        assert call(ctx, 0, bad) == "INVALID"
    assert (out == 0xAB).all() and (conf == -3.0).all() and [c.value for c in cnt] == [77, 77, 77] and sc.value == -5.0
    # the null count pointers are allowed, and the call still works afterwards
    assert lib.mchip_impute_missing(ctx.h, 0, n_real.ctypes.data, out.ctypes.data, None, None, None, None, None) == 0
    assert np.array_equal(out, ctx.impute_missing(0, n_real)[0])
