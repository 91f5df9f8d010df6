"""-m gpu: the paired E step (k_estep_pair: the column pass's and the S-side pass's workgroups in one launch) against the two
launches it replaces (MCHIP_NO_PAIR=1).

Both kinds of block run the stand-alone kernels' bodies, so nothing may differ by a bit.  Shapes: I = 130 is three tiles of 64
individuals, the last one partial; L = 70 ends on a partial block of 8 loci, L = 9 leaves two of a workgroup's four waves
without loci; K = 3, 8, 12 are the smallest, the benchmark's and the largest K the pair exists at; two and up to four alleles
per locus, with and without missing copies, and one case with projection off (the reciprocal-per-cell instances).

  1. one EM step and three SQUAREM-3 cycles: Q, P, S_ik, log L and n_iter with the pair and with MCHIP_NO_PAIR=1, bit for bit;
  2. the same with the pair twice (run-to-run reproducibility);
  3. whole fits: batched cycles (mchip_accel_run) against the cycle-by-cycle host loop, pair on, bit for bit;
  4. profiled runs: both passes report a duration and one launch per working E step, a cached E step no individual launch.
"""
import ctypes as C

import numpy as np
import pytest

import multiclust_amd as mc
from multiclust_amd import host
from synth import make_dataset, random_params

pytestmark = pytest.mark.gpu

I = 130
KERN_P, KERN_Q, KERN_LOGLIK, KERN_DUAL = 0, 1, 2, 3        # MCHIP_KERN_* (mchip_internal.h)
ENV = ("MCHIP_NO_PAIR", "MC_NO_BATCH")

CASES = [dict(K=K, maxal=maxal, missing=missing, L=L, projection=1)
         for K in (3, 8, 12) for maxal in (2, 4) for missing in (0.0, 0.05) for L in (70, 9)]
CASES.append(dict(K=8, maxal=4, missing=0.05, L=70, projection=0))


def case_id(c):
    return "K%d-a%d-%s-L%d%s" % (c["K"], c["maxal"], "miss" if c["missing"] else "nomiss", c["L"], "" if c["projection"] else "-noproj")


def data_of(c):
    ua, geno = make_dataset(I, c["L"], c["K"], ploidy=2, max_alleles=c["maxal"], seed=1000 + 7 * c["K"] + c["L"], missing=c["missing"])
    q0, p0 = random_params(I, ua, c["K"], seed=5 + c["K"], lower_bound=1e-8)
    return ua, geno, q0, p0


def set_env(monkeypatch, env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def start(ctx, c, ua, geno, q0, p0):
    ctx.set_genotypes(ua, geno)
    ctx.set_model(c["K"], do_projection=c["projection"], lower_bound=1e-8, n_secants=1)
    ctx.set_q(0, q0)
    ctx.set_p(0, p0)


def accel_run(ctx, cycles):
    st = mc.hip.RunState(logL=-np.inf, abs_error=1e-300, n_iter=0)
    rc = ctx.lib.mchip_accel_run(ctx.h, 0, 3, cycles, C.byref(st))
    assert rc == 0, rc
    return st


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


_RUNS = {}


def run(monkeypatch, c, mode):
    """(after one EM step, after three SQUAREM-3 cycles) of the case: every number as bytes.  mode: 'pair', 'again' (the pair a
    second time, in a context of its own) or 'nopair'; computed once per (case, mode)"""
    key = (case_id(c), mode)
    if key in _RUNS:
        return _RUNS[key]
    set_env(monkeypatch, {"MCHIP_NO_PAIR": "1"} if mode == "nopair" else {})
    ua, geno, q0, p0 = data_of(c)
    ctx = mc.Context(0)
    try:
        start(ctx, c, ua, geno, q0, p0)
        ll = ctx.em_step(0, 1)
        step = (bits(ll), bits(ctx.get_q(1)), bits(ctx.get_p(1)), bits(ctx.expected_counts()))
        st = accel_run(ctx, 3)
        cycles = (bits(st.logL), st.n_iter, st.stopped, st.fatal, bits(ctx.get_q(0)), bits(ctx.get_p(0)), bits(ctx.expected_counts()))
        finite = bool(np.isfinite(ll)) and bool(np.isfinite(st.logL))
    finally:
        ctx.close()
    _RUNS[key] = (step, cycles, finite)
    return _RUNS[key]


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_pair_equals_the_two_launches(c, monkeypatch):
    pair, two = run(monkeypatch, c, "pair"), run(monkeypatch, c, "nopair")
    assert pair[0] == two[0], "one EM step: (logL, Q, P, S_ik) differ"
    assert pair[1][:4] == two[1][:4], "three cycles: (logL, n_iter, stopped, fatal) differ"
    assert pair[1][4:] == two[1][4:], "three cycles: (Q, P, S_ik) differ"
    if c["projection"]:
        assert pair[2] and pair[1][1] >= 2      # finite log likelihoods, and the cycles ran


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_pair_is_reproducible(c, monkeypatch):
    assert run(monkeypatch, c, "pair") == run(monkeypatch, c, "again")


@pytest.mark.parametrize("K,maxal,missing,L", [(3, 4, 0.0, 70), (8, 4, 0.05, 70), (8, 2, 0.0, 9), (12, 4, 0.05, 70), (12, 2, 0.0, 70)])
def test_batched_cycles_equal_the_host_loop_with_the_pair(K, maxal, missing, L, monkeypatch):
    ua, geno = make_dataset(I, L, K, ploidy=2, max_alleles=maxal, seed=300 + K, missing=missing)
    out = []
    for env in ({}, {"MC_NO_BATCH": "1"}):
        set_env(monkeypatch, env)
        fit = host.Fit(ua, geno, K, admixture=1, accel_scheme=3, verbosity=1, max_iter=12)
        try:
            fit.initialize(4242)
            fit.em()
            m = fit.mod
            assert m.fatal == 0
            out.append((m.n_iter, m.converged, m.iter_stop, bits(m.logL), bits(fit.get_q(m.pindex)), bits(fit.get_p(m.pindex)),
                        bits(fit.expected_counts())))
        finally:
            fit.close()
    assert out[0] == out[1], (out[0][:3], out[1][:3])


@pytest.mark.parametrize("K", [3, 8, 12])
def test_profiled_pair_reports_both_passes(K, monkeypatch):
    """Up to four alleles per locus: the dual pass exists at these K, so a cycle's only S-side launches are its E steps'."""
    set_env(monkeypatch, {})
    c = dict(K=K, maxal=4, missing=0.05, L=70, projection=1)
    ua, geno, q0, p0 = data_of(c)
    ctx = mc.Context(0)
    try:
        start(ctx, c, ua, geno, q0, p0)
        # a working E step: one launch of each kind, each with a duration inside the region's
        ctx.profile_begin()
        ctx.em_step(0, 1)
        total, ms, n = ctx.profile_end()
        print("PAIR K=%d em_step total %.4f ms column %.4f ms individual %.4f ms" % (K, total, ms[KERN_P], ms[KERN_Q]))
        assert (n[KERN_P], n[KERN_Q]) == (1, 1), n
        assert 0.0 < ms[KERN_P] <= total + 0.1 and 0.0 < ms[KERN_Q] <= total + 0.1, (ms, total)
        # sums cached on the host's side (mchip_loglik_prefetch): the column pass alone
        ctx.loglik_prefetch(0)
        ctx.profile_begin()
        ctx.em_step(0, 1)
        total, ms, n = ctx.profile_end()
        assert (n[KERN_P], n[KERN_Q]) == (1, 0) and ms[KERN_P] > 0.0 and ms[KERN_Q] == 0.0, (n, ms)
        # a cycle: two working E steps
        ctx.profile_begin()
        st = accel_run(ctx, 1)
        total, ms, n = ctx.profile_end()
        assert st.n_iter == 2 and not st.stopped
        assert (n[KERN_P], n[KERN_Q], n[KERN_DUAL]) == (2, 2, 1), n
        assert ms[KERN_P] > 0.0 and ms[KERN_Q] > 0.0
        # a cycle whose first E step finds its sums cached (the device flag): its individual blocks return at once
        ctx.set_q(0, q0)
        ctx.set_p(0, p0)
        ctx.loglik_prefetch(0)
        ctx.profile_begin()
        st = accel_run(ctx, 1)
        total, ms, n = ctx.profile_end()
        assert st.n_iter == 2 and not st.stopped
        assert (n[KERN_P], n[KERN_Q], n[KERN_DUAL]) == (2, 1, 1), n
        assert ms[KERN_P] > 0.0 and ms[KERN_Q] > 0.0
    finally:
        ctx.close()
