"""-m gpu: mchip_divergence (multiclust_amd/csrc/mchip_divergence.hip) against the long-double reference of its definitions
(tests/divergence_util.py).

The bounds, from the kernels' summation order (u = 2^-53; divergence_util.ratios holds every group of sums to them):
  h_a, s_ab     a thread adds the T terms of an entry in column order inside its chunk of 1024 columns, each term by one fma on a
                factor rounded once (1 - p, or p_a - p_b): n = T terms with at most two roundings, the chunk partials in
                k_reduce_sum's strided order and tree.  Any order of n non-negative terms stays within (n - 1 + 2) u (1 + n u), so
                the relative bound is (T + 8) u.  The twin clusters are the case with teeth: s_ab is 1e-18 of h_a there, and a
                Gram-matrix difference misses this bound by ten orders of magnitude (tests/test_divergence_cpu.py).
  HT_l, V_l     pbar is the fma chain the definition names, reproduced bit for bit by the reference, so HT_l is a sum of M_l and
                V_l of K M_l non-negative terms (three roundings each at most): relative (M_l + 8) u and (K M_l + 8) u; the sums
                over the loci -- tree over a workgroup's 256 loci, then k_reduce_sum -- (T + 8) u and (K T + 8) u.
  V_l against the exact weighted mean pbar*: the chain's |pbar - pbar*| <= e pbar*, e = K u / (1 - K u), moves V_l by at most
                2 e sum_m sum_k w_k |p_klm - pbar*_lm| + e^2 W sum_m pbar*_lm^2 (derived in divergence_util): that absolute
                part is added to the relative (K M_l + 8) u.
NaN: the device returns sums; F_l = V_l / HT_l is formed by mc_divergence, NaN where HT_l = 0 or the locus has no column (the
device gives V_l = HT_l = 0 there), and F_ab NaN where its denominator is 0: checked through host.Fit.divergence below.

The pair kernel's chunk is 1024 columns whatever the device (CHUNK below restates it; the cases on either side of it fail when
it moves), staged 64 columns at a time; the locus kernel has 256 lanes per workgroup, one locus each."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bedfiles as bf
from cli_util import ROOT
from device_util import ctx, snapshot, status_of
import divergence_util as du
from multiclust_amd import hip, host

pytestmark = pytest.mark.gpu
CHUNK, STAGE, LANES = 1024, 64, 256
KS = [1, 2, 3, 8, 27, 28, 64]
LS = [1, 63, 64, 65, 257]
FORMS = [dict(admixture=1, eta_constrained=0), dict(admixture=1, eta_constrained=1), dict(admixture=0, eta_constrained=0)]
I = 8


def install(ctx, ua, K, P, form=FORMS[0], seed=0, geno=None):
    """data set, model and slot 0; returns P as the device holds it"""
    ctx.set_genotypes(ua, du.random_genotypes(ua, I, seed=seed) if geno is None else geno)
    ctx.set_model(K, **form)
    q = np.random.default_rng(seed).dirichlet(np.ones(K), size=I)
    ctx.set_q(0, q if ctx.indiv_q else q[0])
    ctx.set_p(0, P)
    held = ctx.get_p(0)
    assert np.array_equal(held, P)
    return held


def run_case(ctx, ua, K, maker, form=FORMS[0], seed=1):
    P, w = maker(ua, K, seed)
    P = install(ctx, ua, K, P, form, seed)
    res = ctx.divergence(0, w)
    r = du.check(res, ua, P, w)
    print("K=%d L=%d T=%d %s: error / bound %s" % (K, len(ua), int(ua.sum()), maker.__name__,
                                                    " ".join("%s %.3f" % kv for kv in sorted(r.items()))))
    return res, P, w


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("K", KS)
def test_sums_over_k_and_l(K, L, ctx):
    """every K of the list at every L of the lane tail, the parameter sets and the three model forms in rotation"""
    n = KS.index(K) * len(LS) + LS.index(L)
    ua = du.shaped_ua(L)
    if L >= 8:
        assert {0, 1, 3, 35, 254} <= set(ua.tolist()) and ua[L // 2] == 0 and ua[-1] == 0
    run_case(ctx, ua, K, du.MAKERS[n % 4], FORMS[n % 3], seed=n)


@pytest.mark.parametrize("K", [2, 27, 64])
@pytest.mark.parametrize("T", [STAGE - 1, STAGE, STAGE + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_either_side_of_a_chunk(T, K, ctx):
    """T on either side of the columns staged at a time, of one chunk, and in three chunks: the twin clusters, whose s_ab has teeth"""
    ua = du.shaped_ua(65, T=T) if T >= 500 else du.shaped_ua(5, T=T)
    n_chunks = (T + CHUNK - 1) // CHUNK
    assert int(ua.sum()) == T and n_chunks == {63: 1, 64: 1, 65: 1, 1023: 1, 1024: 1, 1025: 2, 2049: 3}[T]
    res, P, w = run_case(ctx, ua, K, du.twin_clusters, seed=T + K)
    assert 0 < res["sqdiff"][0, 1] < 1e-15 * res["het"][0]


@pytest.mark.parametrize("K", [2, 64])
@pytest.mark.parametrize("M", [1, 3, 35, 254])
def test_one_locus_of_every_allele_shape(M, K, ctx):
    for maker in (du.ordinary, du.near_fixed):
        res, P, w = run_case(ctx, np.array([M], dtype=np.int32), K, maker, seed=M)
        assert res["n_loci"] == 1 and res["sum_v"] == res["locus_v"][0] and res["sum_ht"] == res["locus_ht"][0]


def test_a_bed_installed_data_set(ctx):
    codes = bf.draw_codes(I, 70, missing=0.2, seed=4, plant=True)
    codes[:, 0] = bf.HOM2                                       # (a planted one-allele locus may have lost calls: this one has not)
    assert np.array_equal(host.bed_decode(I, bf.pack(codes))[0] > 0, (codes != bf.MISS).any(axis=0))
    ua = ctx.set_genotypes_bed(I, bf.pack(codes))
    assert set(ua.tolist()) == {0, 1, 2, 3}                     # no call at all, one allele, two, two and the phantom slot
    K = 3
    ctx.set_model(K)
    P, w = du.ordinary(ua, K, seed=8)
    ctx.set_q(0, np.full((I, K), 1.0 / K))
    ctx.set_p(0, P)
    du.check(ctx.divergence(0, w), ua, ctx.get_p(0), w)


def test_after_em_steps_every_slot_is_read_as_it_stands(ctx):
    """the tables of slots the M step wrote (phantom columns hold what it left there), one slot at a time"""
    ua = du.shaped_ua(65)
    K = 3
    P, w = du.ordinary(ua, K, seed=2)
    install(ctx, ua, K, P, seed=2)
    ctx.em_step(0, 1)
    ctx.em_step(1, 2)
    for slot in (0, 1, 2):
        du.check(ctx.divergence(slot, w), ua, ctx.get_p(slot), w)


def test_same_state_same_bits_without_the_locus_arrays_too(ctx):
    a = du.fixed_case(ctx)
    b = ctx.divergence(0, du.ordinary(du.shaped_ua(700, T=2600), 8, seed=17)[1])
    assert du.hexbits(a) == du.hexbits(b)
    c = ctx.divergence(0, du.ordinary(du.shaped_ua(700, T=2600), 8, seed=17)[1], loci=False)
    assert c["locus_v"] is None and c["locus_ht"] is None
    assert (np.array_equal(c["het"], a["het"]) and np.array_equal(c["sqdiff"], a["sqdiff"])
            and (c["sum_v"], c["sum_ht"], c["n_loci"]) == (a["sum_v"], a["sum_ht"], a["n_loci"]))


def test_bits_do_not_depend_on_the_launch_geometry(ctx):
    """the same case in fresh processes under MCHIP_BLOCKS_PER_CU = 1, 7 and unset: the chunk is a constant, not a share of the device"""
    here = du.hexbits(du.fixed_case(ctx))
    seen = []
    for knob in (None, "1", "7"):
        env = {k: v for k, v in os.environ.items() if k != "MCHIP_BLOCKS_PER_CU"}
        if knob:
            env["MCHIP_BLOCKS_PER_CU"] = knob
        env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "divergence_util.py")], stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, text=True, timeout=120, env=env, cwd=ROOT)
        assert res.returncode == 0, res.stderr[-2000:]
        seen.append(res.stdout.strip())
    assert seen == [here] * 3


@pytest.mark.parametrize("held_out", [False, True])
def test_state_is_untouched(held_out):
    """slots, secants, expected counts and the data set before and after, bit for bit, also under a hold-out; and a context that
    asked for the divergence goes on exactly as one that did not (the held S-side sums included)"""
    ua = du.shaped_ua(65)
    K = 3
    geno = du.random_genotypes(ua, I, seed=3)
    P, w = du.ordinary(ua, K, seed=3)
    q = np.random.default_rng(3).dirichlet(np.ones(K), size=I)
    seen = []
    ctxs = [hip.Context(0) for _ in range(2)]
    try:
        for n, c in enumerate(ctxs):
            c.set_genotypes(ua, geno)
            if held_out:
                c.cv_set_folds(np.random.default_rng(4).integers(0, 3, size=(I, len(ua))).astype(np.uint8), 3)
            c.set_model(K, n_secants=2)
            if held_out:
                c.cv_hold_out(1)
            c.set_q(0, q)
            c.set_p(0, P)
            c.em_step(0, 1)
            c.em_step(1, 2)
            for j in range(2):
                c.secant(0, j, 1, 0)
                c.secant(1, j, 2, 1)
            ll0 = c.loglik_prefetch(2)                           # the S-side sums of slot 2 are held
            before = snapshot(c, 2)
            if n == 0:
                for slot in (0, 1, 2):
                    du.check(c.divergence(slot, w), ua, c.get_p(slot), w)
                assert snapshot(c, 2) == before
            ll1 = c.em_step(2, 0)                                # uses the held sums
            seen.append((ll0, ll1, snapshot(c, 2)))
            if held_out:
                c.cv_hold_out(-1)
                assert np.array_equal(c.get_genotypes(), geno)
        assert seen[0] == seen[1]
    finally:
        for c in ctxs:
            c.close()


def test_refusals_leave_the_outputs_alone(ctx):
    lib = ctx.lib
    ua = du.shaped_ua(9)
    K, L = 3, 9
    P, w = du.ordinary(ua, K, seed=1)
    het, sq = np.full(K, -3.0), np.full((K, K), -3.0)
    lv, lht = np.full(L, -3.0), np.full(L, -3.0)
    sv, sht, n1 = C.c_double(-5.0), C.c_double(-5.0), C.c_int(77)

    def call(c, slot, wts, skip=None):
        a = dict(w=wts.ctypes.data, het=het.ctypes.data, sq=sq.ctypes.data, sv=C.byref(sv), sht=C.byref(sht), n1=C.byref(n1))
        if skip:
            a[skip] = None
        return status_of(lib.mchip_divergence(c.h, slot, a["w"], a["het"], a["sq"], lv.ctypes.data, lht.ctypes.data, a["sv"],
                                              a["sht"], a["n1"]))

    fresh = hip.Context(0)
    assert call(fresh, 0, w) == "STATE"                          # no data set
    fresh.set_genotypes(ua, du.random_genotypes(ua, I))
    assert call(fresh, 0, w) == "STATE"                          # no model
    fresh.close()
    install(ctx, ua, K, P)
    for slot in (-1, 3):
        assert call(ctx, slot, w) == "INVALID"
    for bad in (np.array([0.5, np.nan, 0.5]), np.array([0.7, -0.1, 0.4]), np.zeros(3), np.array([0.5, np.inf, 0.5]), np.array([-0.0, 0.0, 0.0])):
        assert call(ctx, 0, bad) == "INVALID"
    for skip in ("w", "het", "sq", "sv", "sht", "n1"):
        assert call(ctx, 0, w, skip) == "INVALID"
    assert (het == -3.0).all() and (sq == -3.0).all() and (lv == -3.0).all() and (lht == -3.0).all()
    assert (sv.value, sht.value, n1.value) == (-5.0, -5.0, 77)
    # the locus arrays may be left out, weights need not sum to 1, and the call still works afterwards
    assert lib.mchip_divergence(ctx.h, 0, w.ctypes.data, het.ctypes.data, sq.ctypes.data, None, None, C.byref(sv), C.byref(sht), C.byref(n1)) == 0
    full = ctx.divergence(0, w)
    assert np.array_equal(het, full["het"]) and np.array_equal(sq, full["sqdiff"]) and sv.value == full["sum_v"] and n1.value == 7
    du.check(ctx.divergence(0, 0.5 * w), ua, P, 0.5 * w)


@pytest.mark.parametrize("form", range(3))
def test_host_tables_and_nan(form):
    """host.Fit.divergence (mc_divergence): the weights the fit gives its clusters -- rows of individuals without an observed copy
    drop out, eta itself when the proportions are shared and for the mixture model --, H, D and F_ab from the device's sums, F_l NaN
    exactly where the locus has no column or HT_l = 0, and a model left as it was"""
    ua = du.shaped_ua(65)
    K, L = 3, 65
    geno = du.random_genotypes(ua, I, seed=6)
    geno[2] = 0xFF                                               # an individual without an observed copy
    fit = host.Fit(ua, geno, K, admixture=FORMS[form]["admixture"], eta_constrained=FORMS[form]["eta_constrained"])
    try:
        P, _ = du.near_fixed(ua, K, seed=6)
        P[:, :3] = 0.0                                           # locus 0: pbar = 0 in every column, so HT_0 = 0 exactly
        q = np.random.default_rng(6).dirichlet(np.ones(K), size=I)
        if form == 0:
            q[2] = np.nan
        fit.set_params(q if form == 0 else q[0], P)
        held_q, held_p = fit.get_q(0), fit.get_p(0)
        assert np.array_equal(held_p, P)
        out = fit.divergence()
        assert np.array_equal(fit.get_q(0), held_q, equal_nan=True) and np.array_equal(fit.get_p(0), P)
        w = du.weights_from_q(held_q, K)
        if form == 0:
            assert np.isnan(held_q[2]).all() and np.allclose(w, np.delete(q, 2, axis=0).mean(axis=0), rtol=1e-14)
        else:
            assert np.array_equal(w, q[0])
        assert np.array_equal(out["w"], w) and np.array_equal(out["w"], host.divergence_weights(held_q, K))
        ref = du.reference(ua, P, w)
        tol = du.derived_bound(ref["T"])
        assert out["n_loci"] == ref["n_loci"] == L - 2 and out["n_pairs"] == 3
        for k in ("H", "D", "F"):
            assert (np.abs(out[k] - ref[k]) <= tol * np.abs(ref[k])).all(), k
        nan = np.isnan(ref["locus_f"])
        assert np.array_equal(np.isnan(out["locus_f"]), nan) and np.array_equal(nan, (ua == 0) | (ref["locus_ht"] == 0))
        # (the monomorphic locus is NaN only when the chain of the weights comes to 1 exactly; every locus with a second column has HT > 0)
        assert nan[0] and nan[ua == 0].all() and not nan[ua >= 2][1:].any()
        lf_tol = du.rel_bound(K * ua[~nan]) + du.rel_bound(ua[~nan]) + 2 * du.U
        assert (np.abs(out["locus_f"][~nan] - ref["locus_f"][~nan]) <= lf_tol * ref["locus_f"][~nan]).all()
        assert abs(out["f_all"] - ref["f_all"]) <= (du.rel_bound(K * ref["T"]) + du.rel_bound(ref["T"]) + 2 * du.U) * ref["f_all"]
        pairs = out["F"][np.triu_indices(K, 1)]
        assert (out["f_min"], out["f_max"]) == (pairs.min(), pairs.max()) and abs(out["f_mean"] - pairs.mean()) <= 8 * du.U
    finally:
        fit.close()
