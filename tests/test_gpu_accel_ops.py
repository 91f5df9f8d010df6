"""-m gpu: the acceleration vector ops of every accelerated cycle -- secants (k_diff), step-size dot products (k_dots,
k_reduce_dots), extrapolation (k_accel_update, k_add, k_axpy2), Michelot projection (k_project_p with michelot_small and
michelot_strided, k_project_q / michelot_k at every K) and the transposes behind the secant buffers -- against tests/accel_ops.py,
staged through the C-ABI with arbitrary base values and secants (no EM step).  tests/test_accel_ops_cpu.py holds the references
and checkers used here to exact arithmetic and to mutants.

1. Element-wise, bit for bit against numpy float64 in the same order: mchip_secant, mchip_accel_update (both forms, four step sizes,
   to != base and to == base), mchip_multisecant_update (0, 1, 4, 9 terms), with random distinct operands -- a transposed or
   shifted secant layout shows here, where the set/get roundtrip cannot show it -- at lengths 1, 255, 257, 4097 and the four
   large shapes of 3, for individual, shared (-c) and mixture proportions.
2. Projection of off-simplex input, bit for bit against numpy's unprojected value put through ob.michelot per Q row and per
   (locus, k) block of P: K = 1 .. 64 with about 70 rows in the families (a)-(g) of tests/accel_ops.py, the shared row at
   K = 1, 8, 33, 64, the P side with loci of 1, 2, 8, 9, 32, 33, 64 (and 65, 100: byte flags) alleles and one locus without an
   allele column, and one case at the bound 1e-75.
3. Dot products against long double: |got - exact| <= (D + 3) eps sum |a_i||b_i| per part, eps = 2^-53, D = accel_ops.kernel_depth
   (derived from the launch geometry there), at n = 1, 255, 4096, 4097, just above 256 * 4096 and just above 2 097 152 on the P side
   and on the Q side, three value families, all three step_dots and all nine secant_dots pairs of three independent secant pairs,
   each call made twice for the same bits.  One WORST line per case (error / bound per sum).
   Largest error / bound seen on an MI355X over all 24 cases: 0.064 (n = 255, "wide"; 0.053 at the 512-block cap).
4. Whole batched fits against cycle-by-cycle fits (MC_NO_BATCH=1), bit for bit, where the dot-product grids have more than one
   block: K = 64 with K T just above 2 * 4096 and just above 2 097 152, and I K above 2 * 4096; schemes 1 to 4.
"""
import numpy as np
import pytest

import accel_ops as ao
from device_util import ctx
import oracle_bind as ob

pytestmark = pytest.mark.gpu

STEPS = (-1.0, -2.5, -37.25, -1e-3)


def bound_of(shape, lb=1e-8):
    return ob.lib.mco_lower_bound(lb, shape["I"], shape["ploidy"])


# ------------------------------------------------------------------------------------------------------------------ 1
SMALL = [ao.make_shape(1, 1, [1]), ao.make_shape(15, 17, [8, 9]), ao.make_shape(1, 257, ao.ua_for(257)),
         ao.make_shape(17, 241, ao.ua_for(241)), ao.make_shape(15, 17, [8, 9], "admix_c"), ao.make_shape(17, 9, ao.ua_for(241), "mix"),
         ao.make_shape(5, 6, ao.ua_for(51, 17), "mix")]
LARGE = ao.dots_shapes()[4:]


@pytest.mark.parametrize("shape", SMALL + LARGE, ids=ao.shape_id)
def test_elementwise_ops_bit_for_bit(ctx, shape):
    full = shape["nq"] + shape["K"] * shape["T"] < 100000
    ao.install(ctx, shape, 0, 1e-8)
    st = ao.random_state(shape, 17 + shape["K"])
    ao.stage(ctx, st)
    x, u, v = st["x"], st["u"], st["v"]
    for which, j, to, frm in ((0, 0, 1, 0), (1, 2, 2, 1), (0, 1, 0, 2))[:3 if full else 1]:
        ctx.secant(which, j, to, frm)
        p, q = ctx.get_secant(which, j)
        ao.check_bits(q, x[to][0] - x[frm][0], "secant(%d, %d) = x%d - x%d, Q part" % (which, j, to, frm))
        ao.check_bits(p, x[to][1] - x[frm][1], "secant(%d, %d) = x%d - x%d, P part" % (which, j, to, frm))
        p, q = ctx.get_secant(1 - which, j)                                   # the pair's other buffer is untouched
        other = (v if which == 0 else u)[j]
        ao.check_bits(q, other[0], "secant buffer beside the one written, Q part")
        ao.check_bits(p, other[1], "secant buffer beside the one written, P part")
    ao.stage(ctx, st)
    updates = [(qn, s, to, base) for qn in (0, 1) for s in STEPS for to, base in ((2, 0), (0, 0))] if full else [(0, -2.5, 2, 0), (1, -1e-3, 0, 0)]
    for qn, s, to, base in updates:
        ctx.accel_update(to, base, 1, s, qn)
        what = "accel_update(to %d, base %d, s %r, qn_form %d)" % (to, base, s, qn)
        ao.check_bits(ctx.get_q(to), ao.ref_accel(x[base][0], u[1][0], v[1][0], s, qn), what + " Q")
        ao.check_bits(ctx.get_p(to), ao.ref_accel(x[base][1], u[1][1], v[1][1], s, qn), what + " P")
        if to == base:
            ctx.set_q(base, x[base][0])
            ctx.set_p(base, x[base][1])
    rng = np.random.default_rng(5)
    for u_index, v_index in (ao.MULTI_PATTERNS if full else ao.MULTI_PATTERNS[3:]):
        ca, cb = rng.standard_normal(len(v_index)) * 3, rng.standard_normal(len(v_index)) * 0.3
        ctx.multisecant_update(2, 1, u_index, v_index, ca, cb)
        what = "multisecant_update(u %d, v %r)" % (u_index, v_index)
        for side, got in ((0, ctx.get_q(2)), (1, ctx.get_p(2))):
            ao.check_bits(got, ao.ref_multisecant(x[1][side], u[u_index][side], [vv[side] for vv in v], v_index, ca, cb), what + " QP"[side + 1])


# ------------------------------------------------------------------------------------------------------------------ 2
def run_forms(ctx, shape, lb, seed, forms):
    ao.install(ctx, shape, 1, lb)
    for n, (form, s, pattern, to, base) in enumerate(forms):
        c = ao.projection_case(shape, lb, form, s, seed + n, pattern)
        got_q, got_p = ao.run_case(ctx, c, to, base)
        assert np.isfinite(got_q).all() and np.isfinite(got_p).all()
        ao.check_projection(got_q, got_p, c, "%s %s s %r" % (ao.shape_id(shape), form, s))


@pytest.mark.parametrize("K", range(1, 65))
def test_projection_of_off_simplex_rows_at_every_k(ctx, K):
    shape = ao.make_shape(K, 70, [2, 3, 9, 33])
    run_forms(ctx, shape, bound_of(shape), 100 * K, [("squarem", -2.5, None, 2, 0), ("qn", -37.25, None, 1, 1),
                                                      ("multi", 0.0, ao.MULTI_PATTERNS[K % 5], 2, 0)])


@pytest.mark.parametrize("model", ["admix_c", "mix"])
@pytest.mark.parametrize("K", [1, 8, 33, 64])
def test_projection_of_the_shared_row(ctx, model, K):
    shape = ao.make_shape(K, 12, [2, 3, 9, 33], model)
    forms = [(("squarem", -2.5), ("qn", -37.25))[n % 2] + (None, 2, 0) for n in range(7)]      # seven seeds: each family in turn
    run_forms(ctx, shape, bound_of(shape), 7 * K, forms + [("multi", 0.0, ao.MULTI_PATTERNS[2], 2, 0)])


@pytest.mark.parametrize("flags", [0, 1], ids=["bitmask", "byteflags"])
@pytest.mark.parametrize("K", [1, 5, 64])
def test_projection_of_p_blocks_on_every_path(ctx, K, flags):
    shape = ao.p_side_shapes(K)[flags]
    run_forms(ctx, shape, bound_of(shape), 31 * K + flags, [("squarem", -2.5, None, 2, 0), ("multi", 0.0, ao.MULTI_PATTERNS[3], 2, 0)])


def test_projection_at_a_tiny_bound(ctx):
    shape = ao.make_shape(40, 70, [2, 9, 33, 65, 100])
    run_forms(ctx, shape, 1e-75, 75, [("squarem", -2.5, None, 2, 0), ("qn", -1e-3, None, 2, 0)])


def test_update_into_a_slot_an_m_step_wrote_reads_back_finite(ctx):
    """the slot's "rows of individuals without data read as NaN" state follows the base's: finite base, finite result"""
    shape = ao.make_shape(3, 40, [2, 3, 4, 2])
    lb = bound_of(shape)
    ao.install(ctx, shape, 1, lb)
    c = ao.projection_case(shape, lb, "squarem", -2.5, 9)
    q0 = ao.project_q(shape, np.abs(c["x0"][0]) + 0.1, lb)
    p0 = ao.project_p(shape, np.abs(c["x0"][1]) + 0.1, lb)
    ctx.set_q(0, q0)
    ctx.set_p(0, p0)
    ctx.em_step(0, 1)
    got_q, got_p = ao.run_case(ctx, c, 1, 0)
    assert np.isfinite(got_q).all() and np.isfinite(got_p).all()
    ao.check_projection(got_q, got_p, c, "into an M step's slot")


# ------------------------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("family", ["unit", "tiny", "wide"])
@pytest.mark.parametrize("shape", ao.dots_shapes(), ids=ao.shape_id)
def test_dot_products_against_long_double(ctx, shape, family):
    ao.install(ctx, shape, 0, 1e-8)
    u, v = ao.dots_operands(shape, family, 11)
    for j in range(3):
        ctx.set_secant(0, j, u[j][1], u[j][0])
        ctx.set_secant(1, j, v[j][1], v[j][0])
    worst, failures = 0.0, []
    for j in range(3):
        got, again = ctx.step_dots(j), ctx.step_dots(j)
        if np.array(got).tobytes() != np.array(again).tobytes():
            failures.append("step_dots(%d) twice: %r, %r" % (j, got, again))
        try:
            worst = max(worst, ao.check_dots(got, ao.dots_reference(ao.step_terms(u[j], v[j])), shape, "%s step_dots(%d)" % (family, j)))
        except AssertionError as e:
            failures.append(str(e))
    for j1 in range(3):
        for j2 in range(3):
            got, again = ctx.secant_dots(j1, j2), ctx.secant_dots(j1, j2)
            if np.array(got).tobytes() != np.array(again).tobytes():
                failures.append("secant_dots(%d, %d) twice: %r, %r" % (j1, j2, got, again))
            try:
                worst = max(worst, ao.check_dots(got, ao.dots_reference(ao.secant_terms(u[j1], u[j2], v[j2])), shape,
                                                 "%s secant_dots(%d, %d)" % (family, j1, j2)))
            except AssertionError as e:
                failures.append(str(e))
    print("WORST-CASE %s %s %.3g" % (ao.shape_id(shape), family, worst))
    assert not failures, failures


# ------------------------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("I,L,scheme", [(12, 43, 1), (12, 43, 2), (12, 43, 3), (12, 43, 4), (12, 10928, 3), (12, 10928, 4), (140, 43, 3)])
def test_batched_cycle_equals_cycle_by_cycle_with_many_blocks(I, L, scheme, monkeypatch):
    """test_dual_individual_pass_equals_the_two_passes's comparison where k_dots_slots, k_reduce_dots_step and block_ordered_sum
    index more than one block: gp = 3 or the 512-block cap with its grid-stride tail, gq = 1 or 3.  (The fits start from a drawn
    interior point: a random partition of so few individuals into 64 clusters leaves (locus, cluster) cells empty, 0 / 0 here as
    in the reference.)"""
    from multiclust_amd import host
    from synth import make_dataset, random_params
    K = 64
    ua, geno = make_dataset(I, L, K, ploidy=2, max_alleles=4, seed=901)
    KT = K * int(ua.sum())
    assert (8192 < KT <= 8192 + 4 * K) if L == 43 else (2097152 < KT <= 2097152 + 4 * K)
    assert ao.grid_of(KT) in (3, 512) and ao.grid_of(I * K) == (3 if I == 140 else 1)
    out = []
    for nobatch in (False, True):
        monkeypatch.delenv("MC_NO_BATCH", raising=False)
        if nobatch:
            monkeypatch.setenv("MC_NO_BATCH", "1")
        fit = host.Fit(ua, geno, K, admixture=1, accel_scheme=scheme, verbosity=1, max_iter=6)
        fit.set_params(*random_params(I, ua, K, seed=4242, lower_bound=fit.opt.lower_bound))
        fit.em()
        m = fit.mod
        assert m.fatal == 0 and m.n_iter >= 6
        out.append((m.n_iter, m.converged, m.iter_stop, m.logL, fit.get_q(m.pindex), fit.get_p(m.pindex)))
        fit.close()
    a, b = out
    assert a[:3] == b[:3] and np.float64(a[3]).tobytes() == np.float64(b[3]).tobytes(), (a[:4], b[:4])
    ao.check_bits(a[4], b[4], "Q, batched against cycle by cycle")
    ao.check_bits(a[5], b[5], "P, batched against cycle by cycle")
