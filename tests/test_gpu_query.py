"""-m gpu: mchip_fit_q_rows (multiclust_amd/csrc/mchip_query.hip) through the C-ABI, with drawn parameters put in place by
mchip_set_p / mchip_set_q: one update against the Q side of mchip_em_step, trajectories and stopping against the numpy restatement
(tests/query_util.py), the state it must leave alone, and its error returns."""
import numpy as np
import pytest

from bits import bits
from device_util import ctx, status_of
import query_util as qu
from multiclust_amd import hip

pytestmark = pytest.mark.gpu
ROWS = np.arange(qu.I_ROWS, dtype=np.int32)


def install(ctx, ua, geno, K, q=None, p=None, do_projection=1, slot=0):
    ctx.set_genotypes(ua, geno)
    ctx.set_model(K, admixture=1, do_projection=do_projection, lower_bound=qu.LOWER_BOUND)
    if p is not None:
        ctx.set_p(slot, p)
    if q is not None:
        ctx.set_q(slot, q)


def check_rows(got, want, copies, K, what):
    """proportions within q_tolerance (its derivation is there), entry by entry; NaN rows and 1 / K rows exactly"""
    tol = qu.q_tolerance(copies, K)[:, None]
    diff = np.abs(got - want)
    print("%s: largest difference / tolerance = %.3g" % (what, np.nanmax(diff / tol)))
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    assert (diff[~np.isnan(want)] <= np.broadcast_to(tol, diff.shape)[~np.isnan(want)]).all(), (what, np.nanmax(diff / tol))


# ---------------------------------------------------------------- one update against the existing path
# The Q side of mchip_em_step computes q_k sum_c n_c p_kc / t_c over allele columns with their counts, normalises and projects;
# mchip_fit_q_rows computes the same quantity copy by copy.  The two differ in the order of summation only.  A sum of n_i
# positive terms, each a few roundings, is within (n_i + K + 8) 2^-52 relative of the exact sum on either side; the quotient
# S_k / sum S of two such pairs differs by at most four times that; q <= 1 makes it absolute; the projection does not expand
# differences: 4 (n_i + K + 8) 2^-52 per entry (query_util.q_tolerance).
@pytest.mark.parametrize("name", qu.CASE_NAMES)
def test_one_update_is_the_em_steps_q_side(name, ctx):
    ua, geno, q, p = qu.case(name)
    K = p.shape[0]
    copies = qu.copies_per_row(geno)
    install(ctx, ua, geno, K, q, p)
    got, ll, it, conv = ctx.fit_q_rows(0, ROWS, 1, from_slot=True)
    ll_em = ctx.em_step(0, 1)
    want = ctx.get_q(1)                       # (rows of individuals without an observed copy come back as NaN)
    assert np.array_equal(np.isnan(want).all(axis=1), copies == 0)
    live = copies > 0
    check_rows(got[live], want[live], copies[live], K, name)
    assert (got[~live] == 1.0 / K).all() and (ll[~live] == 0).all() and (it[~live] == 0).all()
    assert (it[live] == 1).all() and (conv == 0).all()
    # the rows' log likelihoods are those of q(1)
    ref = qu.fit_rows(ua, geno, p, ROWS, 1, q0=q, lb=qu.LOWER_BOUND)
    abs_logs = np.array([r["abs_logs"] for r in ref[4]])
    assert (np.abs(ll - ref[1]) <= (copies + K + 8) * qu.EPS * abs_logs).all()
    assert np.isfinite(ll_em)


# ---------------------------------------------------------------- trajectories against the restatement
@pytest.mark.parametrize("name", qu.CASE_NAMES)
def test_trajectories(name, ctx):
    ua, geno, _, p = qu.case(name)
    K = p.shape[0]
    copies = qu.copies_per_row(geno)
    install(ctx, ua, geno, K, None, p)
    for updates in (1, 5, 20):
        q, ll, it, conv = ctx.fit_q_rows(0, ROWS, updates)
        rq, rll, rit, rconv, res = qu.fit_rows(ua, geno, p, ROWS, updates, lb=qu.LOWER_BOUND)
        assert np.array_equal(it, rit) and np.array_equal(conv, rconv) and (conv == 0).all()
        check_rows(q, rq, copies, K, "%s, %d updates" % (name, updates))
        abs_logs = np.array([r["abs_logs"] for r in res])
        assert (np.abs(ll - rll) <= (copies + K + 8) * qu.EPS * abs_logs).all()
    # the last call once more: the same bits; a single row: the bits it has among all of them
    again = ctx.fit_q_rows(0, ROWS, 20)
    assert all(bits(a) == bits(b) for a, b in zip(again, (q, ll, it, conv)))
    for i in (0, qu.I_ROWS - 1):
        one = ctx.fit_q_rows(0, [i], 20)
        assert all(bits(a) == bits(b[i:i + 1]) for a, b in zip(one, (q, ll, it, conv)))
    # rows in another order: every row's bits go with the row
    perm = ROWS[::-1].copy()
    back = ctx.fit_q_rows(0, perm, 20)
    assert all(bits(a[::-1]) == bits(b) for a, b in zip(back, (q, ll, it, conv)))


def test_without_projection_and_from_a_slot(ctx):
    ua, geno, q, p = qu.case("k9")
    K = 9
    copies = qu.copies_per_row(geno)
    install(ctx, ua, geno, K, q, p, do_projection=0, slot=2)
    got = ctx.fit_q_rows(2, ROWS, 5, from_slot=True)
    want = qu.fit_rows(ua, geno, p, ROWS, 5, q0=q, do_projection=False)
    check_rows(got[0], want[0], copies, K, "k9, no projection, from the slot")
    assert np.array_equal(got[2], want[2])


# ---------------------------------------------------------------- stopping
@pytest.mark.parametrize("rule", sorted(qu.STOP_RULES))
@pytest.mark.parametrize("name", sorted(qu.STOP_CASES))
def test_stopping(name, rule, ctx):
    ua, geno, p = qu.stop_case(name)
    K = p.shape[0]
    copies = qu.copies_per_row(geno)
    rq, rll, rit, rconv, res = qu.stop_reference(name, rule)
    # the seeds are chosen so that no deciding difference lies within one part in 10^3 of its threshold (query_util)
    margin = qu.stop_margin(res, **qu.STOP_RULES[rule])
    print("%s, %s: iterations %d .. %d, margin %.3g" % (name, rule, rit.min(), rit.max(), margin))
    assert margin > 1e-3
    assert (rconv[copies > 0] == 1).all() and rit.max() < qu.STOP_MAX_ITER
    install(ctx, ua, geno, K, None, p)
    q, ll, it, conv = ctx.fit_q_rows(0, ROWS, qu.STOP_MAX_ITER, **qu.STOP_RULES[rule])
    assert np.array_equal(it, rit) and np.array_equal(conv, rconv)
    check_rows(q, rq, copies, K, "%s, %s" % (name, rule))
    abs_logs = np.array([r["abs_logs"] for r in res])
    assert (np.abs(ll - rll) <= (copies + K + 8) * qu.EPS * abs_logs).all()
    # the cap comes first where it is lower: not converged
    cap = int(rit.max()) - 1
    _, _, it2, conv2 = ctx.fit_q_rows(0, ROWS, cap, **qu.STOP_RULES[rule])
    assert np.array_equal(it2, np.minimum(rit, cap)) and np.array_equal(conv2, np.where(rit <= cap, rconv, 0))


# ---------------------------------------------------------------- a frequency of zero: the non-finite row
def test_zero_frequency_gives_the_non_finite_row(ctx):
    ua, geno, q, p = qu.case("k8")
    K = 8
    col = qu.row_columns(ua, geno[3])[0]
    carriers = np.array([col in qu.row_columns(ua, geno[i]) for i in range(qu.I_ROWS)])
    assert carriers[3] and not carriers.all()
    pz = p.copy()
    pz[:, col] = 0.0
    install(ctx, ua, geno, K, None, pz, do_projection=0)
    got, ll, it, conv = ctx.fit_q_rows(0, ROWS, 5)
    want, rll, rit, rconv, _ = qu.fit_rows(ua, geno, pz, ROWS, 5, do_projection=False)
    assert np.array_equal(np.isnan(got).all(axis=1), carriers) and np.array_equal(np.isnan(want).all(axis=1), carriers)
    assert (ll[carriers] == -np.inf).all() and (it[carriers] == 0).all() and (conv == 0).all()
    assert np.array_equal(it, rit)
    check_rows(got, want, qu.copies_per_row(geno), K, "zero column")


# ---------------------------------------------------------------- state
def test_the_call_changes_nothing(ctx):
    ua, geno, q, p = qu.case("many3")
    K = 3
    install(ctx, ua, geno, K)
    rng = np.random.default_rng(8)
    for slot in range(3):
        ctx.set_p(slot, np.maximum(p * rng.uniform(0.5, 1.5, p.shape), 1e-8))
        ctx.set_q(slot, q[rng.permutation(qu.I_ROWS)])
    before = [(bits(ctx.get_q(s)), bits(ctx.get_p(s))) for s in range(3)]
    first = ctx.fit_q_rows(1, ROWS, 7)
    assert [(bits(ctx.get_q(s)), bits(ctx.get_p(s))) for s in range(3)] == before
    ll_after = ctx.em_step(1, 2)
    after = (bits(ctx.get_q(2)), bits(ctx.get_p(2)), bits(ctx.expected_counts()))
    for slot in range(3):                      # the same state again, this time without the call in between
        ctx.set_p(slot, np.frombuffer(before[slot][1]).reshape(K, -1))
        ctx.set_q(slot, np.frombuffer(before[slot][0]).reshape(qu.I_ROWS, K))
    assert ctx.em_step(1, 2) == ll_after
    assert (bits(ctx.get_q(2)), bits(ctx.get_p(2)), bits(ctx.expected_counts())) == after
    # between a log likelihood that keeps its S-side sums and the EM step that uses them
    for slot in range(3):
        ctx.set_p(slot, np.frombuffer(before[slot][1]).reshape(K, -1))
        ctx.set_q(slot, np.frombuffer(before[slot][0]).reshape(qu.I_ROWS, K))
    ctx.loglik_prefetch(1)
    second = ctx.fit_q_rows(1, ROWS, 7)
    assert ctx.em_step(1, 2) == ll_after
    assert (bits(ctx.get_q(2)), bits(ctx.get_p(2)), bits(ctx.expected_counts())) == after
    assert all(bits(a) == bits(b) for a, b in zip(first, second))


def test_under_a_hold_out_it_reads_the_full_data_set(ctx):
    ua, geno, q, p = qu.case("k17")
    K = 17
    install(ctx, ua, geno, K, q, p)
    full = ctx.fit_q_rows(0, ROWS, 6)
    mask = (np.arange(qu.I_ROWS) % 3 == 1)
    folds = np.repeat(mask.astype(np.uint8)[:, None], geno.shape[1], axis=1)
    ctx.cv_set_folds(folds, 2)
    ctx.cv_hold_out(1)
    masked = geno.copy()
    masked[mask] = qu.MISSING
    assert np.array_equal(ctx.get_genotypes(), masked)
    ctx.set_q(0, q)
    ctx.set_p(0, p)
    held = ctx.fit_q_rows(0, ROWS, 6)
    assert all(bits(a) == bits(b) for a, b in zip(full, held))
    assert np.array_equal(ctx.get_genotypes(), masked) and ctx.empty_individuals()[0] == int(mask.sum())
    assert np.array_equal(ctx.cv_get_folds(), folds)
    ctx.cv_hold_out(-1)                        # ... and the installed data set when none is in force
    assert np.array_equal(ctx.get_genotypes(), geno)
    ctx.set_q(0, q)
    ctx.set_p(0, p)
    assert all(bits(a) == bits(b) for a, b in zip(full, ctx.fit_q_rows(0, ROWS, 6)))


# ---------------------------------------------------------------- error returns
def test_error_returns_leave_the_arrays_alone():
    ua, geno, q, p = qu.case("k3")
    K = 3
    c = hip.Context(0)
    lib = c.lib
    out = (np.full((qu.I_ROWS, K), 7.0), np.full(qu.I_ROWS, 7.0), np.full(qu.I_ROWS, 7, np.int32), np.full(qu.I_ROWS, 7, np.uint8))
    untouched = [bits(a) for a in out]

    def call(slot=0, rows=ROWS, n=None, max_iter=5, abs_error=0.0, rel_error=0.0):
        r = np.ascontiguousarray(rows, dtype=np.int32)
        rc = lib.mchip_fit_q_rows(c.h, slot, r.ctypes.data, len(r) if n is None else n, 0, max_iter, abs_error, rel_error,
                                  out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, out[3].ctypes.data)
        assert [bits(a) for a in out] == untouched
        return status_of(rc)

    try:
        assert call() == "STATE"                                   # no data set
        c.set_genotypes(ua, geno)
        assert call() == "STATE"                                   # no model
        c.set_model(K, admixture=1, lower_bound=qu.LOWER_BOUND)
        c.set_p(0, p)
        c.set_q(0, q)
        assert call(slot=3) == "INVALID" and call(slot=-1) == "INVALID"
        assert call(n=0) == "INVALID" and call(n=-1) == "INVALID"
        assert call(rows=[0, 13]) == "INVALID" and call(rows=[-1]) == "INVALID"
        assert call(rows=[4, 5, 4]) == "INVALID"
        assert call(max_iter=0) == "INVALID" and call(abs_error=-1.0) == "INVALID" and call(rel_error=float("nan")) == "INVALID"
        assert lib.mchip_fit_q_rows(c.h, 0, None, 1, 0, 5, 0.0, 0.0, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data,
                                    out[3].ctypes.data) == 1
        c.set_model(K, admixture=1, eta_constrained=1, lower_bound=qu.LOWER_BOUND)
        assert call() == "UNSUPPORTED"                             # shared mixing proportions
        c.set_model(K, admixture=0, lower_bound=qu.LOWER_BOUND)
        assert call() == "UNSUPPORTED"                             # the mixture model
        c.set_model(K, admixture=1, lower_bound=qu.LOWER_BOUND)
        c.set_p(0, p)
        c.fit_q_rows(0, ROWS, 5, out=out)                          # and the call that succeeds fills them
        assert all(bits(a) != u for a, u in zip(out, untouched))
    finally:
        c.close()
