"""-m gpu: mchip_bed_pca_apply and mchip_bed_pca (multiclust_amd/csrc/mchip_pca.hip) against the definition restated in
tests/pca_util.py (which tests/test_pca_cpu.py holds to exact rationals).

The apply: every element of y within gamma (1 / L') sum_l |z_il| sum_j |z_jl| |x_jc|, gamma = (I + L + 20) 2^-53, and of w within
(I + 10) 2^-53 sum_i |z_il| |x_ic| -- bounds that count roundings and hold for any order of addition (pca_util's docstring) --; mu
bit for bit (one correctly rounded division of two integers: the counts behind it are exact), inv within 4 ulp, L' exact, the trace
within the L + 20 roundings of its sum.

What the shapes are sized by: the MFMA instruction takes 4 individuals (project) or 4 variants (expand) and 16 columns at a time; a
wave owns 16 variants / individuals, a workgroup 64; the record tile is 256 individuals; a slab is LSLAB variants.  So I on either
side of 4, 16, 64 and 256, L on either side of 64 and of LSLAB and two slabs and one, n_vec on either side of every multiple of 16
the library pads to; records longer than they need be; garbage in every bit that carries no individual."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bedfiles
from cli_util import ROOT
from device_util import ctx
import pca_util as pu
from multiclust_amd import hip
from synth import random_params

pytestmark = pytest.mark.gpu
LD = pu.LD
assert (pu.LSLAB, pu.VARIANTS, pu.ITILE) == (4096, 64, 64)      # the cases below are written for these
IS = [5, 15, 16, 17, 63, 65, 255, 257]
LS = [1, 63, 65, pu.LSLAB - 1, pu.LSLAB, pu.LSLAB + 1, 2 * pu.LSLAB + 1]
NS = [1, 15, 16, 17, 33, 64]


def check_apply(ctx, I, L, n_vec, seed, missing=0.1, extra=0, wide=False, plant=True):
    codes, where = pu.draw_codes(I, L, seed, missing, plant)
    x = pu.draw_x(I, n_vec, seed, wide)
    bed = pu.repack(codes, seed, extra)
    assert bed.shape == (L, (I + 3) // 4 + extra)
    ref = pu.reference(codes, x)
    if not ref["n_used"]:
        with pytest.raises(hip.HipError, match="no polymorphic variant"):
            ctx.bed_pca_apply(I, bed, x)
        return None
    y, w, scale, n_used, trace = ctx.bed_pca_apply(I, bed, x)
    assert y.shape == (I, n_vec) and w.shape == (L, n_vec) and scale.shape == (L, 2)
    assert n_used == ref["n_used"]
    assert np.array_equal(scale[:, 0], ref["mu"]), "mu = (double)s / (double)n: the counts are exact"
    assert np.array_equal(scale[:, 1] == 0, ~ref["used"])
    worst = pu.ulps(scale[ref["used"], 1], ref["inv"][ref["used"]]).max()
    excess = pu.apply_excess(y, ref, I, L, w=w)
    print("I=%d L=%d n_vec=%d: y, w at %.3f of their bounds, inv within %.1f ulp" % (I, L, n_vec, excess, worst))
    assert worst <= 4
    assert excess <= 1, (I, L, n_vec)
    assert abs(LD(trace) - ref["trace"]) <= (L + 20) * pu.U * ref["trace"]
    if "missing_individual" in where:
        assert not y[where["missing_individual"]].any()                  # exactly 0
    for name in ("all_missing", "monomorphic"):
        if name in where:
            assert not scale[where[name]].any() and not w[where[name]].any()
    if "all_het" in where:
        assert scale[where["all_het"], 0] == 1.0 and not w[where["all_het"]].any()      # mu = 1: used, and every z is exactly 0
    return y, w, scale, n_used, trace


@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("I", IS)
def test_apply_at_every_individual_edge(ctx, I, extra):
    check_apply(ctx, I, 70, 17, 100 + I, extra=extra, wide=bool(extra))


@pytest.mark.parametrize("L", LS)
def test_apply_on_either_side_of_the_variant_tiles_and_slabs(ctx, L):
    check_apply(ctx, 67, L, 16, 200 + L, extra=L % 2, plant=L >= 63)


@pytest.mark.parametrize("n_vec", NS)
def test_apply_at_every_column_padding(ctx, n_vec):
    check_apply(ctx, 130, 321, n_vec, 300 + n_vec, extra=1, wide=True)


def test_apply_without_a_missing_call_and_outputs_that_may_be_null(ctx):
    I, L = 65, 129
    got = check_apply(ctx, I, L, 5, 400, missing=0.0, plant=False)
    codes, _ = pu.draw_codes(I, L, 400, 0.0, False)
    y, w, scale, n_used, trace = ctx.bed_pca_apply(I, pu.repack(codes, 400, 0), pu.draw_x(I, 5, 400), w=False, scale=False)
    assert w is None and scale is None and y.tobytes() == got[0].tobytes() and (n_used, trace) == got[3:]
    lib = ctx.lib
    bed, x, yy, n = pu.repack(codes, 400, 0), pu.draw_x(I, 5, 400), np.empty((I, 5)), np.zeros(1, dtype=np.int32)
    assert lib.mchip_bed_pca_apply(ctx.h, I, L, bed.ctypes.data, bed.shape[1], 5, x.ctypes.data, yy.ctypes.data, None, None, n.ctypes.data, None) == 0
    assert yy.tobytes() == y.tobytes() and n[0] == n_used                                  # trace may be NULL as well


def test_second_call_gives_the_same_bits(ctx):
    bed, x = pu.fresh_case()
    a = ctx.bed_pca_apply(pu.FRESH["I"], bed, x)
    b = ctx.bed_pca_apply(pu.FRESH["I"], bed, x)
    assert pu.digest(*a[:3]) == pu.digest(*b[:3]) and a[3:] == b[3:]


@pytest.fixture(scope="module")
def fresh(ctx):
    """the digests of this process, under the knob it was started with"""
    return pu.fresh_digests(ctx)


@pytest.mark.parametrize("knob", ["1", "4", "64", "again"])
def test_bits_do_not_depend_on_the_launch_knobs_or_the_process(ctx, fresh, knob):
    """fresh processes under MCHIP_BLOCKS_PER_CU = 1, 4 and 64, and one more without the knob: the cut of the variants into slabs is
    a constant of the shape and the projection walks all individuals, so every bit of both entry points' outputs is the same"""
    env = dict(os.environ)
    env.pop("MCHIP_BLOCKS_PER_CU_IND", None)
    env.pop("MCHIP_BLOCKS_PER_CU", None)
    if knob != "again":
        env["MCHIP_BLOCKS_PER_CU"] = knob
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pca_util.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         timeout=120, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    assert tuple(res.stdout.split()) == fresh, knob


def test_an_installed_fit_is_untouched_by_both_entry_points():
    I, L, K = 40, 90, 3
    codes, _ = pu.draw_codes(I, L, 500)
    c = hip.Context(0)
    try:
        ua = c.set_genotypes_bed(I, bedfiles.pack(codes))
        c.set_model(K)
        q0, p0 = random_params(I, ua, K, seed=5, lower_bound=1e-8)
        c.set_q(0, q0)
        c.set_p(0, p0)
        for _ in range(3):
            c.em_step(0, 0)
        before = (c.get_p(0).tobytes(), c.get_q(0).tobytes(), np.float64(c.loglik(0)).tobytes(), c.get_genotypes().tobytes())
        check_apply(c, 70, 130, 7, 501, extra=3)
        other, _ = pu.draw_codes(70, 130, 501)
        r = c.bed_pca(70, pu.repack(other, 501, 3), 2, max_iter=5)
        assert r["n_iter"] >= 1 and (c.I, c.L) == (I, L)
        after = (c.get_p(0).tobytes(), c.get_q(0).tobytes(), np.float64(c.loglik(0)).tobytes(), c.get_genotypes().tobytes())
        assert before == after
        assert np.isfinite(c.em_step(0, 0))
    finally:
        c.close()


def test_every_error_path_leaves_the_outputs_untouched(ctx):
    import ctypes as C
    I, L, n_vec = 10, 12, 3
    codes, _ = pu.draw_codes(I, L, 700)
    bed = pu.repack(codes, 700, 0)
    rb = bed.shape[1]
    x = pu.draw_x(I, n_vec, 700)
    lib = ctx.lib
    SENT = 12345.0

    def outputs():
        return dict(y=np.full((I, 64), SENT), w=np.full((L, 64), SENT), scale=np.full((L, 2), SENT), n=np.full(1, 777, dtype=np.int32), t=np.full(1, SENT),
                    val=np.full(64, SENT), vec=np.full((I, 64), SENT), res=np.full(64, SENT), it=np.full(1, 777, dtype=np.int32))

    def untouched(o):
        return all((v == (777 if v.dtype == np.int32 else SENT)).all() for v in o.values())

    def apply(o, **a):
        a = dict(dict(I=I, L=L, bed=bed.ctypes.data, rb=rb, n_vec=n_vec, x=x.ctypes.data, y=o["y"].ctypes.data, n=o["n"].ctypes.data), **a)
        return lib.mchip_bed_pca_apply(ctx.h, a["I"], a["L"], a["bed"], a["rb"], a["n_vec"], a["x"], a["y"], o["w"].ctypes.data, o["scale"].ctypes.data, a["n"],
                                       o["t"].ctypes.data)

    def pca(o, **a):
        a = dict(dict(I=I, L=L, bed=bed.ctypes.data, rb=rb, n_pc=2, n_extra=10, max_iter=20, tol=1e-6, val=o["val"].ctypes.data, vec=o["vec"].ctypes.data,
                      res=o["res"].ctypes.data, t=o["t"].ctypes.data, n=o["n"].ctypes.data, it=o["it"].ctypes.data), **a)
        return lib.mchip_bed_pca(ctx.h, a["I"], a["L"], a["bed"], a["rb"], a["n_pc"], a["n_extra"], a["max_iter"], C.c_double(a["tol"]), a["val"], a["vec"],
                                 a["res"], a["t"], a["n"], a["it"])

    shape = [dict(I=0), dict(I=-1), dict(L=0), dict(L=-4), dict(rb=rb - 1), dict(rb=0), dict(bed=None)]
    for change in shape + [dict(n_vec=0), dict(n_vec=-1), dict(n_vec=65), dict(x=None), dict(y=None), dict(n=None)]:
        o = outputs()
        rc = apply(o, **change)
        assert hip.STATUS.get(rc, rc) == "INVALID" and untouched(o), ("apply", change, rc)
        assert b"bed_pca_apply" in lib.mchip_last_error(ctx.h)
    for change in shape + [dict(n_pc=0), dict(n_pc=-1), dict(n_pc=I + 1), dict(n_pc=2, n_extra=63), dict(n_pc=2, n_extra=-1), dict(max_iter=0), dict(max_iter=-3),
                           dict(tol=0.0), dict(tol=1.0), dict(tol=-1e-6), dict(tol=float("nan")), dict(val=None), dict(vec=None), dict(res=None), dict(t=None),
                           dict(n=None), dict(it=None)]:
        o = outputs()
        rc = pca(o, **change)
        assert hip.STATUS.get(rc, rc) == "INVALID" and untouched(o), ("pca", change, rc)
        assert b"bed_pca" in lib.mchip_last_error(ctx.h)
    assert lib.mchip_bed_pca_apply(None, I, L, bed.ctypes.data, rb, n_vec, x.ctypes.data, np.empty((I, n_vec)).ctypes.data, None, None,
                                   np.zeros(1, dtype=np.int32).ctypes.data, None) == 1
    # L' = 0: no polymorphic variant -- monomorphic, all heterozygous... no: everyone heterozygous is used (0 < s = n < 2 n)
    flat = np.full((I, L), bedfiles.HOM2, dtype=np.uint8)
    flat[:, ::2] = bedfiles.HOM1
    flat[:, 3] = bedfiles.MISS
    flat[2, :] = bedfiles.MISS
    fb = pu.repack(flat, 1, 0)
    for call in (apply, pca):
        o = outputs()
        rc = call(o, bed=fb.ctypes.data)
        assert hip.STATUS.get(rc, rc) == "INVALID" and untouched(o) and b"no polymorphic variant" in lib.mchip_last_error(ctx.h)
    check_apply(ctx, I, L, n_vec, 700)      # and the context still works


# ---- the whole iteration ----
@pytest.fixture(scope="module")
def planted():
    """the fixtures, their packed records and their long-double matrix: computed once, never changed"""
    out = []
    for k in range(len(pu.PLANTED)):
        case = pu.planted_case(k)
        case["bed"] = bedfiles.pack(case["codes"], padding=3)
        case["G"], case["n_used"], case["trace"] = pu.gram(case["codes"])
        out.append(case)
    return out


@pytest.mark.parametrize("k", range(len(pu.PLANTED)))
def test_eigenpairs_of_the_planted_fixtures(ctx, planted, k):
    case = planted[k]
    I, L, n_pc = case["I"], case["L"], case["n_pc"]
    r = ctx.bed_pca(I, case["bed"], n_pc, n_extra=10, max_iter=case["cap"], tol=1e-9)
    own = pu.check_pairs(r, case["G"], I, L, 1e-9)
    print("I=%d L=%d: %d iterations (cap %d), eigenvalues %s, reported residuals %s, own %s" % (I, L, r["n_iter"], case["cap"], r["eigenvalues"], r["residuals"],
                                                                                               own))
    assert r["n_iter"] <= case["cap"] and r["residuals"].max() <= 1e-9
    assert r["n_used"] == case["n_used"] and abs(LD(r["trace"]) - case["trace"]) <= (L + 20) * pu.U * case["trace"]
    assert (np.diff(r["eigenvalues"]) <= 0).all() and r["eigenvalues"][-1] > 4.5      # the planted structure, above a bulk below 1.7


def test_b_at_least_I_is_exact_after_two_iterations(ctx):
    codes, _ = pu.draw_codes(17, 65, 5)
    r = ctx.bed_pca(17, pu.repack(codes, 5, 2), 3, max_iter=50, tol=1e-9)
    assert r["n_iter"] == 2
    pu.check_pairs(r, pu.gram(codes)[0], 17, 65, 1e-9, planted_fixture=False)


@pytest.mark.parametrize("I,L,n_pc", [(5, 40, 3), (17, 3, 2)])
def test_rank_deficient_cases_give_no_nan(ctx, I, L, n_pc):
    codes, _ = pu.draw_codes(I, L, 70 + I, plant=False)
    r = ctx.bed_pca(I, pu.repack(codes, I, 1), n_pc, max_iter=50, tol=1e-9)
    assert (r["eigenvalues"] >= -1e-14).all()
    pu.check_pairs(r, pu.gram(codes)[0], I, L, 1e-9, planted_fixture=False)


def test_one_iteration_is_no_error(ctx, planted):
    case = planted[1]
    r = ctx.bed_pca(case["I"], case["bed"], case["n_pc"], max_iter=1, tol=1e-9)
    assert r["n_iter"] == 1 and (r["residuals"] > 1e-9).all() and not np.isnan(r["eigenvectors"]).any()
