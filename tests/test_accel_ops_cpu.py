"""The CPU side of the acceleration vector-op tests (tests/accel_ops.py; the GPU side is tests/test_gpu_accel_ops.py): the
references are sound, the inputs reach what they are meant to reach, and the checkers fail on mutants.

Michelot against exact arithmetic: |ob.michelot - exact projection onto {x >= lb, sum x = 1}| <= c eps len max(1, |x|_inf) with
eps = 2^-53.  Measured over the families (a)-(g), 35 rows at each of K = 1 .. 64, 65, 100: the worst c is 0.77 (family (e) at
K = 11; per family a 0.25, b 0.28, c 0.42, d 0.07, e 0.77, f 0.50, g 0.005); the test holds 8 times that, c = 6.2.

The oracle's serial dot products: a serial chain of n terms has depth n, not the device's D = kernel_depth(n) (about 20 to 40), and
a serial sum of n positive terms really is worse than the device's tree: measured |error| / device bound up to 1.9 at n = 4097, 19
at 2.1 M ("unit", "tiny") and 252 for "wide".  So the oracle is held to the bound of its own depth, (n + 3) eps sum |a||b|
(worst ratio measured: 0.47, at n = 1), and the device's bound is kept for the device.
"""
from fractions import Fraction

import numpy as np
import pytest

import accel_ops as ao
import oracle_bind as ob

LB = ob.lib.mco_lower_bound(1e-8, 70, 2)
C_MICHELOT = 6.2
ALL_K = list(range(1, 65)) + [65, 100]
DOT_FAMILIES = ("unit", "tiny", "wide")


def test_michelot_against_the_exact_projection():
    worst = 0.0
    for K in ALL_K:
        rows, labels = ao.target_rows(35, K, LB, K)
        for r, lab in zip(rows, labels):
            got, exact = ob.michelot(r, LB), ao.exact_projection(r, LB)
            assert sum(exact) == 1 and min(exact) >= Fraction(LB)
            err = max(abs(Fraction(float(g)) - e) for g, e in zip(got, exact))
            c = float(err) / (ao.EPS * K * max(1.0, np.abs(r).max()))
            worst = max(worst, c)
            assert c <= C_MICHELOT, (K, lab, c)
            assert ao.michelot_restated(r, LB)[0].tobytes() == got.tobytes(), (K, lab)       # the round counter is the same algorithm
    print("michelot: worst c %.3g" % worst)


def test_long_double_dot_reference_against_exact_sums():
    """the pairwise long-double sums against Dekker products + math.fsum, at the small shapes: within 2^-58 sum |a||b|"""
    for shape in ao.dots_shapes()[:4]:
        for fam in DOT_FAMILIES:
            u, v = ao.dots_operands(shape, fam, 5)
            for side in (0, 1):
                a, b = ao._ld(u[0][side]), ao._ld(v[1][side])
                s, sc, _ = ao._dot(a, b)
                assert abs(s - ao.LD(ao.exact_dot_fsum(u[0][side], v[1][side]))) <= sc * ao.LD(2.0) ** -58 + abs(s) * ao.LD(2.0) ** -52


@pytest.mark.parametrize("shape", ao.dots_shapes(), ids=ao.shape_id)
def test_oracle_serial_dots_and_the_dropped_element_condition(shape):
    """Every case of the GPU test: the oracle's serial sums within the bound at their own depth; in the "unit" family every
    single term is more than 1000 times the DEVICE's bound, so a sum that drops one element is outside it.  (The large shapes take
    three of the nine secant pairs here; the GPU test takes all nine.)"""
    nq, KT = shape["nq"], shape["K"] * shape["T"]
    pairs = [(a, b) for a in range(3) for b in range(3)] if nq + KT < 100000 else [(0, 1), (1, 2), (2, 0)]
    for fam in DOT_FAMILIES:
        u, v = ao.dots_operands(shape, fam, 11)
        checks = [(ob.step_dots(u[j][0], v[j][0], u[j][1], v[j][1]), ao.dots_reference(ao.step_terms(u[j], v[j]))) for j in range(3)]
        checks += [(ob.secant_dots(u[a][0], u[b][0], v[b][0], u[a][1], u[b][1], v[b][1]),
                    ao.dots_reference(ao.secant_terms(u[a], u[b], v[b]))) for a, b in pairs]
        for got, ref in checks:
            for g, (exact, scales, smallest) in zip(got, ref):
                assert abs(ao.LD(g) - exact) <= ao.dots_bound(scales, nq + KT, nq + KT), (fam, g, exact)
                if fam == "unit":
                    assert smallest > 1000 * ao.dots_bound(scales, ao.kernel_depth(nq), ao.kernel_depth(KT))


def test_kernel_depth_and_grids_reach_every_edge():
    n = [s["K"] * s["T"] for s in ao.dots_shapes()[:6]]
    assert n[:4] == [1, 255, 4096, 4097] and [ao.grid_of(x) for x in n] == [1, 1, 1, 2, 258, 512]
    assert n[5] > 2097152 and n[5] % (512 * 256) != 0 and -(-n[5] // (512 * 256)) == 17
    nq = [s["nq"] for s in ao.dots_shapes()]
    assert nq[:4] == [1, 255, 4096, 4097] and [ao.grid_of(x) for x in nq[6:]] == [258, 512]
    assert ao.kernel_depth(1) == 1 + 8 + 1 + 8 + 1 and ao.kernel_depth(n[4]) == 16 + 8 + 2 + 8 + 1 and ao.kernel_depth(n[5]) == 17 + 8 + 2 + 8 + 1


def test_the_inputs_have_teeth():
    """round counts, high indices fixed early, real ties: what the projection families are for"""
    most = {}
    for K in ALL_K:
        rows, labels = ao.target_rows(70, K, LB, K)
        assert set(labels) >= set("abce") and (K < 3 or "f" in labels) and (K < 2 or "d" in labels) and (K <= 32 or "g" in labels)
        rounds, high_early = 0, False
        for r, lab in zip(rows, labels):
            _, n, fixed_in, ties = ao.michelot_restated(r, LB)
            rounds = max(rounds, n)
            high_early |= any(j >= 32 for now in fixed_in[:-1] for j in now) and any(j < 32 for now in fixed_in[1:] for j in now)
            if lab == "f":                      # the tie: on the bound, not below it, so not fixed in that round
                assert len(ties[0]) == 1 and ties[0][0] not in fixed_in[0] and fixed_in[0] and ties[0][0] in fixed_in[1]
            if lab == "e":
                assert sum(len(now) for now in fixed_in) == K - 1
            if lab == "a":
                assert n == 1
        most[K] = rounds
        assert K < 4 or rounds >= 3, (K, rounds)
        assert K <= 32 or high_early, K
    assert most[64] >= 8, most[64]
    assert ao.tie_row(2, LB, 0) is None and ao.tie_row(8, 1e-75, 0) is None


def test_projection_cases_land_in_their_families():
    """the secants are solved for the target rows: numpy's unprojected update is the target (the tie rows bit for bit)"""
    for form, s, pat in (("squarem", -2.5, None), ("qn", -37.25, None), ("multi", 0.0, ao.MULTI_PATTERNS[3])):
        c = ao.projection_case(ao.make_shape(40, 70, [2, 3, 9, 40]), LB, form, s, 3, pat)
        xq, xp = ao.unprojected(c)
        yq, yp, lq, lp = ao.targets(c["shape"], LB, 3)
        np.testing.assert_allclose(xq, yq, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(xp, yp, rtol=1e-9, atol=1e-9)
        ties = [i for i, lab in enumerate(lq) if lab == "f"]
        assert len(ties) == 10 and xq[ties].tobytes() == yq[ties].tobytes() and "f" in lp and "g" in lp
        pq, pp = ao.projected(c)
        assert np.all(pq >= LB) and np.all(pp >= LB) and np.abs(pq.sum(axis=1) - 1).max() < 1e-9


# ------------------------------------------------------------------------------------------------------------------ mutants
def projection_mutant(c, **kw):
    return ao.projected(c, michelot=lambda row, lb: ao.michelot_restated(row, lb, **kw)[0])


@pytest.mark.parametrize("mutant", [dict(mask_bits=32), dict(max_rounds=1), dict(le=True)], ids=["mask32", "one-round", "le"])
def test_projection_checker_fails_on_mutants(mutant):
    shape = ao.make_shape(64, 70, [2, 9, 33, 64])
    c = ao.projection_case(shape, LB, "squarem", -2.5, 64)
    good = projection_mutant(c)
    ao.check_projection(good[0], good[1], c, "restated")              # the restatement itself passes
    bad = projection_mutant(c, **mutant)
    with pytest.raises(AssertionError):
        ao.check_bits(bad[0], ao.projected(c)[0], "Q")
    with pytest.raises(AssertionError):
        ao.check_bits(bad[1], ao.projected(c)[1], "P")
    if "mask_bits" in mutant:                                             # a 32-bit mask is right up to 32 entries and wrong above
        c32 = ao.projection_case(ao.make_shape(32, 70, [2, 9, 32]), LB, "squarem", -2.5, 32)
        ok = projection_mutant(c32, **mutant)
        ao.check_projection(ok[0], ok[1], c32, "mask32 at 32")
        c33 = ao.projection_case(ao.make_shape(33, 70, [2, 9, 33]), LB, "qn", -37.25, 33)
        bad = projection_mutant(c33, **mutant)
        with pytest.raises(AssertionError):
            ao.check_bits(bad[0], ao.projected(c33)[0], "Q")


def test_update_checker_fails_on_fused_multiply_add():
    shape = ao.make_shape(17, 241, ao.ua_for(241))
    st = ao.random_state(shape, 2)
    for qn in (0, 1):
        for side in (0, 1):
            x0, u, v = st["x"][0][side], st["u"][1][side], st["v"][1][side]
            want = ao.ref_accel(x0, u, v, -2.5, qn)
            fused = ao.fma_accel(x0, u, v, -2.5, qn)
            np.testing.assert_allclose(fused, want, rtol=1e-9, atol=1e-300)
            with pytest.raises(AssertionError):
                ao.check_bits(fused, want, "fused")


def test_secant_checker_fails_on_a_transposed_layout():
    shape = ao.make_shape(17, 241, ao.ua_for(241))
    st = ao.random_state(shape, 3)
    want = st["x"][1][1] - st["x"][0][1]
    ao.check_bits(want.copy(), want, "secant")
    K, T = want.shape
    with pytest.raises(AssertionError):                                   # stored [T][K], read as [K][T]
        ao.check_bits(np.ascontiguousarray(want.T).reshape(K, T), want, "secant")
    with pytest.raises(AssertionError):                                   # shifted by one element
        ao.check_bits(np.roll(want.ravel(), 1).reshape(K, T), want, "secant")


@pytest.mark.parametrize("index", [3, 4, 5])
def test_dots_checker_fails_on_mutants(index, capsys):
    shape = ao.dots_shapes()[index]
    u, v = ao.dots_operands(shape, "unit", 7)
    step, sec = ao.step_terms(u[0], v[0]), ao.secant_terms(u[0], u[1], v[1])
    ref_step, ref_sec = ao.dots_reference(step), ao.dots_reference(sec)
    ao.check_dots(ao.emulate_device_dots(step), ref_step, shape, "model step")
    ao.check_dots(ao.emulate_device_dots(sec), ref_sec, shape, "model secant")
    mutants = [dict(drop="last"), dict(drop="block"), dict(drop="trip"), dict(acc=np.float32)]
    if ao.grid_of(shape["nq"]) != ao.grid_of(shape["K"] * shape["T"]):
        mutants.append(dict(swap_parts=True))
    for m in mutants:
        with pytest.raises(AssertionError):
            ao.check_dots(ao.emulate_device_dots(step, **m), ref_step, shape, "mutant %r" % m)
        with pytest.raises(AssertionError):
            ao.check_dots(ao.emulate_device_dots(sec, **m), ref_sec, shape, "mutant %r" % m)
    with pytest.raises(AssertionError):                                   # u[j2] read where v[j2] belongs
        ao.check_dots(ao.emulate_device_dots(ao.secant_terms(u[0], u[1], u[1])), ref_sec, shape, "mutant u for v")
    with pytest.raises(AssertionError):                                   # j1 and j2 mixed up
        ao.check_dots(ao.emulate_device_dots(ao.secant_terms(u[1], u[0], v[0])), ref_sec, shape, "mutant j1 <-> j2")
    assert "WORST" in capsys.readouterr().out
