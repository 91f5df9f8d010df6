"""The mixture worst-case inputs of tests/mixture_worstcase.py are where they claim to be, their long-double reference is sound,
and the bounds have room for a correct float64 implementation and none for a subtly wrong one (no GPU needed).

  * test_reference_against_decimal: `reference` against 60-digit decimal arithmetic (stdlib ln and exp) on a few individuals
    and loci, with missing copies and with a p == 0 cell (0 in the E step, -inf in the log likelihood).
  * test_oracle_within_bounds: mco_em_step, mco_e_step and mco_log_likelihood against `reference` within `bounds` at every
    (family, regime) and worstcase.K_VALUES; test_window_oracle_and_inputs: the same on the window cases, where the oracle's
    log likelihood is +inf as soon as someone sits on the overflow edge and the long-double value is finite.  That assertion
    is the record that +inf is the reference's own arithmetic (log_likelihood.c:203-228) and not the oracle's.
  * test_float64_restatements_within_bounds: the step restated in float64 in three summation orders (loci and individuals in
    order, reversed, and in chunks of 8 added in chunk order) stays within 0.25 of every bound; the ratios are printed.
  * test_mutants_are_caught: eight float64 mutants each exceed a bound in the regime named beside them, and pass the
    rtol = 1e-7, atol = 1e-13 of today's vik / eta / P comparisons.  That second half is shown on `ordinary` wherever the
    mutant's effect there is small.  A dropped, a doubled copy and a skipped chunk change v by whole nats on Dirichlet(1)
    parameters, which any tolerance sees; their small form is on a near-fixed allele, so they are shown to pass the old
    array tolerance on `fixed`, where v moves by 1e-8 for every k alike and only the log likelihood's bound (1e-10) sees it.
  * test_inputs_are_where_they_claim: dominance gaps beyond 745 nats for every k, subnormal runners-up, tied rows (every K;
    the subnormal window and the overflow edge of the window cases are asserted in test_window_oracle_and_inputs).
  * test_case_list_reaches_every_mixture_kernel: `reach` of test_gpu_kernel_matrix.py over the GPU case list, K by K."""
import math
from decimal import Decimal, getcontext

import numpy as np
import pytest

import mixture_worstcase as mw
import oracle_bind as ob
import worstcase as wc
from test_gpu_kernel_matrix import count_bits, geometry, reach

LD = mw.LD
CPU_CASES = [(mw.make_case(fam, K), regime) for fam in mw.FAMILIES for K in wc.K_VALUES for regime in mw.REGIMES]
RESTATE_K = (1, 2, 6, 13, 28, 64)
RESTATE_CASES = [(mw.make_case(fam, K), regime) for fam in mw.FAMILIES for K in RESTATE_K for regime in mw.REGIMES]
ORDERS = ("sequential", "reversed", "chunks")


def pair_id(cr):
    return "%s-%s" % (mw.case_id(cr[0]), cr[1])


# --------------------------------------------------------------------------------------------------------------- decimal
def test_reference_against_decimal():
    getcontext().prec = 60
    rs = np.random.default_rng(11)
    I, L, K, pl, lb = 4, 5, 3, 2, 1e-8
    ua = np.array([2, 3, 2, 4, 3], dtype=np.int32)
    toff = mw.offsets(ua)
    geno = np.stack([rs.integers(0, ua[l], size=(I, pl)) for l in range(L)], axis=1).astype(np.uint8)
    geno[1, 2, 0] = geno[3, 0, 1] = mw.MISSING
    p = mw.dirichlet_blocks(ua, K, rs, lb)
    eta = np.array([0.2, 0.5, 0.3])
    ref = mw.reference(ua, geno, eta, p, lb)
    v = [[Decimal(float(eta[k])).ln() + sum(Decimal(float(p[k, toff[l] + g])).ln() for l in range(L) for g in geno[i, l] if g != mw.MISSING)
          for k in range(K)] for i in range(I)]
    w = [[(x - max(row)).exp() for x in row] for row in v]
    vik = [[x / sum(row) for x in row] for row in w]
    ll = sum(sum(row).ln() + max(vr) for row, vr in zip(w, v))
    n = wc.counts(ua, geno)
    num = [[Decimal(lb) + sum(vik[i][k] * int(n[i, c]) for i in range(I)) for c in range(int(ua.sum()))] for k in range(K)]
    col = [sum(vik[i][k] for i in range(I)) for k in range(K)]

    def close(got, want):
        # long double carries 64 bits: split it into two doubles, both exact in decimal
        hi = float(got)
        lo = float(LD(got) - LD(hi))
        return abs(Decimal(hi) + Decimal(lo) - want) <= Decimal(2e-17) * abs(want)
    assert close(ref["ll"], ll)
    for i in range(I):
        for k in range(K):
            assert close(ref["v"][i, k], v[i][k]) and close(ref["vik"][i, k], vik[i][k]), (i, k)
    for k in range(K):
        assert close(ref["eta_u"][k], col[k] / sum(col))
        for l in range(L):
            s = sum(num[k][toff[l]:toff[l + 1]])
            for c in range(toff[l], toff[l + 1]):
                assert close(ref["num"][k, c], num[k][c]) and close(ref["p_u"][k, c], num[k][c] / s), (k, c)
    # a p == 0 cell: skipped by the E step, -inf in the log likelihood of whoever carries it
    p0 = p.copy()
    p0[:, toff[1] + int(geno[0, 1, 0])] = 0.0
    z = mw.reference(ua, geno, eta, p0, lb)
    carriers = (geno[:, 1, :] == geno[0, 1, 0]).any(axis=1)
    assert np.isfinite(z["v"].astype(np.float64)).all() and (np.isneginf(z["ll_i"].astype(np.float64)) == carriers).all()
    skipped = [Decimal(float(eta[k])).ln() + sum(Decimal(float(p0[k, toff[l] + g])).ln() for l in range(L) for g in geno[0, l]
                                                   if g != mw.MISSING and p0[k, toff[l] + g] != 0.0) for k in range(K)]
    assert all(close(z["v"][0, k], skipped[k]) for k in range(K))


# ---------------------------------------------------------------------------------------------------------------- oracle
def oracle_point(c, ua, geno, eta, p, lb):
    """(ll of em_step, vik, eta', P', e_step, log_likelihood) of the oracle at a point"""
    opt = ob.make_options(admixture=0, do_projection=1, lower_bound=lb, fused=1, abs_error=0.0)
    mod = ob.Model(ob.Data(c["I"], c["L"], c["ploidy"], ua, geno), opt, c["K"])
    mod.q(0)[...] = eta
    mod.p(0)[...] = p
    ll1, e = mod.loglik(0), mod.e_step()
    mod.em_step()
    return mod.logL, mod.sik().copy(), mod.q(mod.pindex).copy(), mod.p(mod.pindex).copy(), e, ll1


def all_ratios(ref, tol, out):
    ll, vik, eta1, p1, e, ll1 = out
    return mw.step_ratios(ref, tol, ll, vik, eta1, p1) + (mw.ratio(e, ref["ll"], tol["ll0"]), mw.ratio(ll1, ref["ll"], tol["ll1"]))


@pytest.mark.parametrize("cr", CPU_CASES, ids=pair_id)
def test_oracle_within_bounds(cr):
    c, regime = cr
    ua, geno, eta, p, lb = mw.build(c, regime)
    assert (p >= lb).all() and (eta >= lb).all() and abs(eta.sum() - 1.0) < 1e-14
    ref = mw.reference(ua, geno, eta, p, lb)
    tol = mw.bounds(ref, ua, 1)
    r = all_ratios(ref, tol, oracle_point(c, ua, geno, eta, p, lb))
    print("%s: oracle / long double over the bound: ll %.3g vik %.3g eta %.3g P %.3g e_step %.3g loglik %.3g" % ((pair_id(cr),) + r))
    assert max(r) <= 1.0, r


@pytest.mark.parametrize("c", mw.window_cases(), ids=mw.case_id)
def test_window_oracle_and_inputs(c):
    K = c["K"]
    ua, geno, eta, p, lb = mw.build_window(c)
    assert c["I"] * c["L"] <= 65 * 260
    ref = mw.reference(ua, geno, eta, p, lb)
    tol = mw.bounds(ref, ua, 1)
    edge, S = mw.overflow_edge(ref)
    sub = mw.subnormal_window(ref)
    kappa = tol["kappa"].astype(np.float64)
    # (a) exp(max) subnormal and not 0 for at least 4 individuals, kappa <= 2^-20 for everyone
    assert sub.sum() >= 4 and (kappa <= 2.0 ** -20).all() and (kappa[sub] > 2.0 ** -52).all(), (sub.sum(), kappa.max())
    # (b) the overflow edge with two tied clusters and with all K of them
    if K >= 2:
        assert (edge & (np.abs(S - 2.0) < 1e-6)).sum() >= (4 if K >= 3 else 0) and (edge & (np.abs(S - K) < 1e-6)).sum() >= 4, (edge.sum(), S[edge])
    else:
        assert not edge.any()                   # one cluster: exp(h) <= DBL_MAX is the whole sum
    mx = ref["mx"].astype(np.float64)
    assert (mx < mw.LOG_HALF_DENORM).sum() >= 30 and (mx > math.log(mw.TINY)).sum() >= 8      # rescaled ones and plain ones besides
    out = oracle_point(c, ua, geno, eta, p, lb)
    r = all_ratios(ref, tol, out)
    print("%s: oracle / long double over the bound: ll %.3g vik %.3g eta %.3g P %.3g e_step %.3g loglik %.3g; %d on the edge"
          % ((mw.case_id(c),) + r + (edge.sum(),)))
    assert max(r[:5]) <= 1.0, r
    assert np.isfinite(float(ref["ll"])) and np.isfinite(tol["ll1"])
    if edge.any():
        assert out[5] == math.inf, out[5]       # the reference's own arithmetic: logL_mixture's rescaled sum overflows
    else:
        assert r[5] <= 1.0, r
    # and the float64 restatement with the branch k_mix_finalize takes there is finite and within the mode 1 bound
    got = f64_step(ua, geno, eta, p, lb, "chunks")
    assert mw.ratio(got[5], ref["ll"], tol["ll1"]) <= 0.25
    if edge.any():
        assert f64_step(ua, geno, eta, p, lb, "chunks", "no_overflow_branch")[5] == math.inf


# ----------------------------------------------------------------------------------------------- float64 restatements
MUTANTS = {             # name: (regime in which it has to exceed a bound, regime on which it passes today's array tolerance)
    "drop_last_copy": ("fixed", "fixed"),           # last copy of the last (partial) block of 8 loci
    "double_copy": ("fixed", "fixed"),              # copy 0 of locus 0 counted twice
    "no_add_lb": ("tied", "tied"),                  # numerators of 1 / K and more: 6e-8 of them; a rare allele's would show at 1e-7
    "log_1e-9": ("ordinary", "ordinary"),
    "exp_1e-9": ("ordinary", "ordinary"),
    "max_without_last_k": ("dominant", "ordinary"),
    "no_shift_last_k": ("deep", "ordinary"),        # mode 1's rescaling leaves the last k alone
    "eta_first_chunk_skipped": ("fixed", "fixed"),  # mode 1 with log eta in front and the last chunk's sums left out
}


def f64_step(ua, geno, eta, p, lb, order, mutant=None):
    """The mixture step as the device kernels state it, in float64: (ll, vik, eta', P', e_step, loglik).  `order`: loci and
    individuals in order, reversed, or in chunks of 8 whose sums are added in chunk order."""
    I, L, pl = geno.shape
    K = p.shape[0]
    toff = mw.offsets(ua)
    logp = np.log(p)
    alt = np.where((np.arange(K)[:, None] + np.arange(p.shape[1])[None, :]) % 2 == 0, 1.0, -1.0)
    if mutant == "log_1e-9":
        logp = logp * (1.0 + 1e-9 * alt)
    loge = np.log(eta)

    def seq(n):
        if order == "sequential":
            return [list(range(n))]
        if order == "reversed":
            return [list(range(n - 1, -1, -1))]
        return [list(range(a, min(n, a + 8))) for a in range(0, n, 8)]

    def gather(loci):
        acc = np.zeros((I, K))
        for l in loci:
            for b in range(pl):
                reps = 1
                if mutant == "drop_last_copy" and l == L - 1 and b == pl - 1:
                    reps = 0
                if mutant == "double_copy" and l == 0 and b == 0:
                    reps = 2
                g = geno[:, l, b]
                ok = g != mw.MISSING
                add = np.where(ok[:, None], logp[:, toff[l] + np.where(ok, g, 0)].T, 0.0)
                for _ in range(reps):
                    acc += add
        return acc
    parts = [gather(loci) for loci in seq(L)]
    v = np.tile(loge, (I, 1))
    for part in parts:
        v = v + part
    # mode 0 (k_mix_finalize, e_step_mixture)
    mx = (v[:, :K - 1] if (mutant == "max_without_last_k" and K > 1) else v).max(axis=1)
    with np.errstate(over="ignore", invalid="ignore"):
        w = np.exp(v - mx[:, None])
        if mutant == "exp_1e-9":
            w = w * (1.0 + 1e-9 * alt[:, 0][None, :])
        temp = np.zeros(I)
        for k in range(K):
            temp = temp + w[:, k]
        vik = w / temp[:, None]
        ll = float(np.sum(np.log(temp) + mx))
    # mode 1 (logL_mixture's form, with k_mix_finalize's branch for a rescaled sum that overflows)
    v1 = np.zeros((I, K))
    if mutant == "eta_first_chunk_skipped":
        v1 = v1 + loge[None, :]
        for part in parts[:-1]:
            v1 = v1 + part
    else:
        for part in parts:
            v1 = v1 + part
        v1 = v1 + loge[None, :]
    m1 = v1.max(axis=1)
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        te = np.exp(m1)
        need = (te == 0.0) | (te == np.inf)
        s = np.where(te == np.inf, m1, -m1)
        active = need.copy()
        while active.any():
            s = np.where(active, s * 0.5, s)
            active &= np.exp(s) == np.inf
        scale = np.where(need, m1 - s, 0.0)
        shifted = v1 - scale[:, None]
        if mutant == "no_shift_last_k":
            shifted[:, K - 1] = v1[:, K - 1]
        t1 = np.zeros(I)
        for k in range(K):
            t1 = t1 + np.exp(shifted[:, k])
        ll_i = np.log(t1) + scale
        over = t1 == np.inf
        if over.any() and mutant != "no_overflow_branch":
            top = m1 - scale
            t2 = np.zeros(I)
            for k in range(K):
                t2 = t2 + np.exp(shifted[:, k] - top)
            ll_i = np.where(over, np.log(t2) + m1, ll_i)
        ll1 = float(np.sum(ll_i))
    # M step
    n = wc.counts(ua, geno).astype(np.float64)
    eta_num, num = np.zeros(K), np.zeros((K, p.shape[1]))
    for chunk in seq(I):
        e_part, n_part = np.zeros(K), np.zeros((K, p.shape[1]))
        for i in chunk:
            e_part = e_part + vik[i]
            n_part = n_part + vik[i][:, None] * n[i][None, :]
        eta_num, num = eta_num + e_part, num + n_part
    if mutant != "no_add_lb":
        num = num + lb
    with np.errstate(invalid="ignore"):
        eta1 = eta_num / np.sum(eta_num)
        eta1 = ob.michelot(eta1, lb) if np.isfinite(eta1).all() else eta1
        p1 = np.empty_like(num)
        for l in range(L):
            blk = slice(toff[l], toff[l + 1])
            temp = np.zeros(K)
            for c in range(toff[l], toff[l + 1]):
                temp = temp + num[:, c]
            q = num[:, blk] / temp[:, None]
            for k in range(K):
                p1[k, blk] = ob.michelot(q[k], lb) if np.isfinite(q[k]).all() else q[k]
    return ll, vik, eta1, p1, ll, ll1


@pytest.mark.parametrize("cr", RESTATE_CASES, ids=pair_id)
def test_float64_restatements_within_bounds(cr):
    c, regime = cr
    ua, geno, eta, p, lb = mw.build(c, regime)
    ref = mw.reference(ua, geno, eta, p, lb)
    tol = mw.bounds(ref, ua, -(-c["L"] // 8))
    worst = 0.0
    for order in ORDERS:
        r = all_ratios(ref, tol, f64_step(ua, geno, eta, p, lb, order))
        print("%s %s: float64 / long double over the bound: ll %.3g vik %.3g eta %.3g P %.3g e_step %.3g loglik %.3g" % ((pair_id(cr), order) + r))
        worst = max(worst, max(r))
    assert worst <= 0.25, worst


def passes_old_tolerance(got, clean):
    return all(np.allclose(a, b, rtol=1e-7, atol=1e-13) for a, b in zip(got[1:4], clean[1:4]))


@pytest.mark.parametrize("name", sorted(MUTANTS), ids=str)
def test_mutants_are_caught(name):
    caught_in, quiet_in = MUTANTS[name]
    c = mw.make_case("mix_2bit", 6)
    assert c["L"] % 8 != 0
    seen = {}
    for regime in {caught_in, quiet_in}:
        ua, geno, eta, p, lb = mw.build(c, regime)
        ref = mw.reference(ua, geno, eta, p, lb)
        tol = mw.bounds(ref, ua, -(-c["L"] // 8))
        clean, got = f64_step(ua, geno, eta, p, lb, "chunks"), f64_step(ua, geno, eta, p, lb, "chunks", name)
        seen[regime] = (max(all_ratios(ref, tol, clean)), all_ratios(ref, tol, got), passes_old_tolerance(got, clean))
        print("%s on %s: over the bound (ll, vik, eta, P, e_step, loglik) %r, unmutated %.3g, passes rtol 1e-7: %s"
              % (name, regime, tuple(float("%.3g" % x) for x in seen[regime][1]), seen[regime][0], seen[regime][2]))
    assert seen[caught_in][0] <= 0.25 and max(seen[caught_in][1]) > 1.0, seen[caught_in]
    assert seen[quiet_in][2], "today's tolerance would have caught it on %s" % quiet_in


# ------------------------------------------------------------------------------------------------------------ the inputs
@pytest.mark.parametrize("K", mw.K_ALL)
def test_inputs_are_where_they_claim(K):
    for fam in mw.FAMILIES:
        c = mw.make_case(fam, K)
        assert c["I"] <= 129 and c["L"] <= 45 and c["L"] % 8 != 0 and c["I"] % 64 in (1, 63)
        # dominant: every k (every k that has an individual) dominates someone by more than 745 nats, the first and the last always
        ua, geno, eta, p, lb = mw.build(c, "dominant")
        ref = mw.reference(ua, geno, eta, p, lb)
        rows, win = mw.exactly_one_hot(ref)
        owners = set(int(k) for k in win[rows])
        assert owners >= set(range(min(K, c["I"] - 1))) | {0, K - 1}, (fam, sorted(set(range(K)) - owners))
        if K > 1:
            assert mw.runner_up_gap(ref)[rows].min() > 746.0
        # deep: |v| of 1e4 and more, and someone whose runner-up is 700 to 745 nats behind (exp(v - max) subnormal)
        ua, geno, eta, p, lb = mw.build(c, "deep")
        assert lb == 1e-120 and (p >= lb).all()
        ref = mw.reference(ua, geno, eta, p, lb)
        assert float(-ref["mx"].max()) > 2000.0 and float(-ref["mx"].min()) > 1e4
        if K > 1:
            gap = mw.runner_up_gap(ref)
            gaps = [i for i in range(c["I"]) if mw.is_gap_individual(i)]
            assert len(gaps) >= 4 and all(700.0 < gap[i] < 745.0 for i in gaps), (fam, gap[gaps])
            sub = ref["vik"][gaps].astype(np.float64)
            assert ((sub > 0) & (sub < mw.TINY)).any(axis=1).all()
        # tied: identical rows, uniform eta
        ua, geno, eta, p, lb = mw.build(c, "tied")
        assert (p == p[0]).all() and (eta == 1.0 / K).all()
        # fixed: one allele per block off the bound
        ua, geno, eta, p, lb = mw.build(c, "fixed")
        assert ((p > lb).sum(axis=1) == c["L"]).all()


# -------------------------------------------------------------------------------------------------------------- coverage
def test_case_list_reaches_every_mixture_kernel():
    cases = mw.all_cases()
    assert len(cases) == 64 * len(mw.FAMILIES) and len({mw.case_id(c) for c in cases}) == len(cases)
    assert len(mw.window_cases()) == 2 * len(wc.K_VALUES)
    for K in mw.K_ALL:
        have, chunks, slabs = set(), 0, 0
        for c in (x for x in cases if x["K"] == K):
            ua = mw.case_ua(c)
            have |= reach(dict(c, ua=ua, lb=mw.regime_bound(c, "ordinary")))
            assert reach(dict(c, ua=mw.case_ua(c, "deep"), lb=mw.DEEP_BOUND)) == reach(dict(c, ua=ua, lb=mw.regime_bound(c, "ordinary")))
            cbits = count_bits(c["ploidy"], c["knobs"])
            g = geometry(K, c["I"], c["L"], int(ua.sum()), c["ploidy"], int(ua.max()), False, cbits, c["knobs"])
            chunks = max(chunks, g["n_lchunks"])
            slabs = max(slabs, -(-g["n_ichunks"] // 4) if cbits else g["n_ichunks"])      # plan()'s mix_col_slabs (mchip_kernels_k.hip)
        want = {"k_mix_gather<2,true>", "k_mix_gather<0,true>", "k_mix_gather<2,false>", "k_mix_gather<0,false>",
                "k_column_counts<2,true,false>", "k_column_counts<4,true,false>", "k_mix_column<2>", "k_mix_column<0>",
                "k_finalize_p_tile", "k_finalize_p", "k_mix_finalize", "finalize_shared_eta"}
        assert want <= have, (K, sorted(want - have))
        assert chunks > 1 and slabs > 8, (K, chunks, slabs)
