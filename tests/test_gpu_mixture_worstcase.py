"""The mixture model's passes at every K against a long-double step (tests/mixture_worstcase.py), on the GPU.

One test per (K, family), K = 1 to 64: k_logp, k_mix_gather<PL,STAGED>, k_mix_finalize (modes 0 and 1), k_mix_column<PL> or
the MIX instance of k_column_counts, finalize_shared_eta and the add_lb branch of k_finalize_p / k_finalize_p_tile, each
compiled once per K.  Families: mix_2bit (diploid, 3 % missing), mix_4bit (tetraploid), mix_p3 (triploid, the generic PL),
mix_nocounts_p2 (MCHIP_NO_COUNTS), mix_dense (one allele more than the sparse edge: the unstaged gather), mix_geom
(MCHIP_SLAB_FRAC=1000 and MCHIP_NO_COUNTS on 129 x 45 triploids with one locus of 65 alleles or more: six locus chunks, seventeen
column slabs, the unstaged generic gather, k_mix_column<0>, k_finalize_p).  tests/test_mixture_worstcase_cpu.py asserts that
this list reaches every one of them at every K.

Each test runs the regimes ordinary, fixed, tied, dominant and deep in turn (what each is for: the module docstring of
mixture_worstcase.py).  Per regime: set_model(K, admixture=0, lower_bound=...), set_q, set_p, em_step(0, 1); ll, vik
(expected_counts), eta' and P' against `reference` within `bounds`; e_step(0) (mode 0 again) within the mode 0 bound, loglik(0)
and loglik_prefetch(0) (mode 1) within the mode 1 bound; tied: vik == 1 / K and the K rows of P' equal, as bits; dominant: vik
exactly 0 or 1 wherever the runner-up is more than 746 nats behind; everything finite.  The bounds are functions of the case
(about 1e-11 relative on ordinary data, against the 1e-7 of the oracle comparisons); a result outside one is a finding about
a kernel or about the derivation, not a reason for a factor.

The window tests (mix_2bit and mix_4bit at worstcase.K_VALUES; k_mix_finalize is the only kernel that sees the difference)
put individuals where logL_mixture's rescaling has its edges: exp(max v) subnormal but not 0 (the kappa term of the mode 1
bound), and max v = -2 h with h just below log DBL_MAX, where the reference's rescaled sum overflows for two tied clusters and
its log likelihood is +inf (asserted of the oracle in the CPU module).  mchip_loglik has to be finite there and within the
mode 1 bound of the long-double value: k_mix_finalize takes such a term in mode 0's form (documented departures).

Every test prints one MIXWORST line per regime: the largest |difference| / tolerance of ll, vik, eta', P', e_step, loglik and
loglik_prefetch."""
import numpy as np
import pytest

from device_util import knob_contexts, set_knobs
import mixture_worstcase as mw
from test_gpu_kernel_matrix import KNOBS

pytestmark = pytest.mark.gpu

CASES = mw.all_cases()
WINDOW = mw.window_cases()


def run_point(ctx, c, name, ua, geno, eta, p, lb):
    """one step and the three log likelihoods of a point against the long-double step; returns (failures, ref, results)"""
    K = c["K"]
    ref = mw.reference(ua, geno, eta, p, lb)
    tol = mw.bounds(ref, ua, mw.n_lchunks(c, ua))
    ctx.set_genotypes(ua, geno)
    ctx.set_model(K, admixture=0, eta_constrained=0, do_projection=1, lower_bound=lb)
    ctx.set_q(0, eta)
    ctx.set_p(0, p)
    ll = ctx.em_step(0, 1)
    vik, eta1, p1 = ctx.expected_counts(), ctx.get_q(1), ctx.get_p(1)
    e, a, d = ctx.e_step(0), ctx.loglik(0), ctx.loglik_prefetch(0)
    r = mw.step_ratios(ref, tol, ll, vik, eta1, p1) + (mw.ratio(e, ref["ll"], tol["ll0"]), mw.ratio(a, ref["ll"], tol["ll1"]),
                                                      mw.ratio(d, ref["ll"], tol["ll1"]))
    print("MIXWORST %s %s ll %.3g vik %.3g eta %.3g P %.3g e_step %.3g loglik %.3g prefetch %.3g" % ((mw.case_id(c), name) + r))
    failures = []
    assert np.isfinite(float(ref["ll"])) and np.isfinite(ref["p1"]).all() and np.isfinite(tol["ll1"])
    if not (np.isfinite([ll, e, a, d]).all() and np.isfinite(vik).all() and np.isfinite(eta1).all() and np.isfinite(p1).all()):
        failures.append("%s: not finite: em_step %r e_step %r loglik %r prefetch %r (long double %r)" % (name, ll, e, a, d, float(ref["ll"])))
    if max(r) > 1.0:
        failures.append("%s: (ll, vik, eta, P, e_step, loglik, prefetch) over the bound: %r; ll %r e_step %r loglik %r prefetch %r, "
                        "long double %r, bounds %.3g (mode 0) %.3g (mode 1)" % (name, r, ll, e, a, d, float(ref["ll"]), tol["ll0"], tol["ll1"]))
    if e != ll:
        failures.append("%s: e_step %r != em_step's log likelihood %r of the same point" % (name, e, ll))
    return failures, ref, (vik, eta1, p1)


@pytest.mark.parametrize("c", CASES, ids=mw.case_id)
def test_mixture_step_vs_longdouble(knob_contexts, monkeypatch, c):
    set_knobs(monkeypatch, c["knobs"], KNOBS)
    ctx = knob_contexts(c["knobs"])
    K = c["K"]
    failures = []
    for regime in mw.REGIMES:
        bad, ref, (vik, eta1, p1) = run_point(ctx, c, regime, *mw.build(c, regime))
        failures += bad
        if regime == "tied":
            if not (vik == 1.0 / K).all():
                failures.append("tied: vik is not 1 / K exactly: %r" % (np.unique(vik)[:8],))
            if not ((p1 == p1[0]).all() and (eta1 == eta1[0]).all()):
                failures.append("tied: the K rows of P' (or the entries of eta') are not bitwise equal: rows %r"
                                % (np.nonzero((p1 != p1[0]).any(axis=1))[0][:8],))
        if regime == "dominant":
            rows, win = mw.exactly_one_hot(ref)
            assert len(rows) >= min(K, c["I"]) // 2
            want = np.zeros((len(rows), K))
            want[np.arange(len(rows)), win[rows]] = 1.0
            if not (vik[rows] == want).all():
                failures.append("dominant: vik is not exactly 0 or 1: individuals %r" % (rows[(vik[rows] != want).any(axis=1)][:8],))
    assert not failures, failures


@pytest.mark.parametrize("c", WINDOW, ids=mw.case_id)
def test_mixture_loglik_window_vs_longdouble(knob_contexts, monkeypatch, c):
    set_knobs(monkeypatch, c["knobs"], KNOBS)
    failures, _, _ = run_point(knob_contexts(c["knobs"]), c, "window", *mw.build_window(c))
    assert not failures, failures
