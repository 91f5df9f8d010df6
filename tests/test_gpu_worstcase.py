"""The EM passes at worst-case parameters (tests/worstcase.py) against a long-double reference, on the GPU.

Every other GPU test draws Q and P from Dirichlet(1): no t is near the bound, the running product loses a decade per
multiplication, and neither the look cadence of the log-likelihood product (`flush_blocks`) nor the
shared reciprocals are near their limits.  Here each case is one upload and one EM step on 131 x 130 (longer where flush_blocks = 3
needs it to hold whole periods of the pattern, at most 171 x 291) from a point with

  * allele columns whose P is the bound for every k next to ordinary ones (one t at the bound shares a reciprocal with one of
    order 1; four t of the bound share the column side's), Q rows at a vertex,
  * rows (and, in the dense family, columns) that take the product to just above 1e-100 at a look, unrescaled, and then
    through two looks' worth of tiny factors: the largest legal fall with the right interval, 0 with a doubled one,

at the smallest bound of flush_blocks = 1, 2, 3 (`edge_bound`), at 1e-75 (shared reciprocals on the packed-count column side,
the individual side looking after every copy) and at the suite's usual 1e-8 (the control: tests/test_worstcase_cpu.py shows
that a look half as often is -inf on every edge case and goes unnoticed at the control).  No (K, b) pair is dropped: med >= lb holds for all of them.

K covers both sides of every K-dependent switch: NJ of k_column_counts (12/13, 20/21), bial_pays (6, 10), the dual limit
(12), ind_split (27/28, 48/49), col_split (36/37).  Families: diploid general, diploid all-biallelic (k_individual_bial),
tetraploid, diploid with MCHIP_FORCE_DENSE=1 (k_column_pass<2,...> carries the log likelihood), shared mixing proportions at
K = 8, 28, 64; each with and without missing copies (the NOMISS instances differ).  tests/test_worstcase_cpu.py asserts that
every case's chunk spans a whole period of the pattern and that it reaches the instances it is meant for.

Checks per case (tolerances: the suite's step-1 ones, test_em_steps_vs_oracle_paths): em_step(0, 1) -> logL, Q1, P1, S against
`reference_step` and against the oracle, all finite; loglik / e_step / loglik_prefetch of the worst point itself (ACCUM false
and true instances) within the logL tolerance, loglik == e_step as bits; the same with MCHIP_FORCE_SAFE=1 in a second
context (a reciprocal per cell, a look after every copy: none of the contracts needed), so a failure says which side broke.

Not covered, deliberately: the dual individual pass's second parameter set (prod2).  It only ever sees the second EM iterate
of an accelerated cycle; one EM step moves every carried tiny allele far off the bound, so no worst point survives to it,
and the slots cannot be staged otherwise through the C-ABI.

A correct kernel's error budget is 2.5 ulp per reciprocal and about 1e-16 |logL| for the products, orders of magnitude inside
these tolerances; a finite result outside one is a finding, not a reason to widen it.  Largest |difference| / tolerance of
the oracle (CPU, double) against the long-double reference, all 670 cases: logL 0.45, Q1 0.17, P1 0.09, S 1.6e-4.  The test
prints one WORST line per case and path with the same ratios of the GPU result."""
import numpy as np
import pytest

from device_util import knob_contexts, set_knobs
import worstcase as wc
from test_gpu_kernel_matrix import KNOBS

pytestmark = pytest.mark.gpu

CASES = wc.all_cases()


def gpu_step(knob_contexts, monkeypatch, c, knobs, ua, geno, q, p):
    """(logL, Q1, P1, S) of em_step(0, 1), and loglik / e_step / loglik_prefetch of slot 0"""
    set_knobs(monkeypatch, knobs, KNOBS)
    ctx = knob_contexts(knobs)
    ctx.set_genotypes(ua, geno)
    ctx.set_model(c["K"], admixture=1, eta_constrained=int(c["model"] == "admix_c"), do_projection=1, lower_bound=c["lb"])
    ctx.set_q(0, q)
    ctx.set_p(0, p)
    ll = ctx.em_step(0, 1)
    step = (ll, ctx.get_q(1), ctx.get_p(1), ctx.expected_counts())
    return step, (ctx.loglik(0), ctx.e_step(0), ctx.loglik_prefetch(0))


@pytest.mark.parametrize("c", CASES, ids=wc.case_id)
def test_worst_case_step_vs_longdouble(knob_contexts, monkeypatch, c):
    ua, geno, q, p = wc.build(c)
    ref = wc.reference_step(ua, geno, q, p, c["lb"], c["model"])
    orc = wc.oracle_step(c, ua, geno, q, p)
    tol = max(1e-8, 1e-12 * abs(ref[0]))
    failures = []
    for path, knobs in (("fast", c["knobs"]), ("safe", dict(c["knobs"], MCHIP_FORCE_SAFE="1"))):
        step, lls = gpu_step(knob_contexts, monkeypatch, c, knobs, ua, geno, q, p)
        finite = all(np.isfinite(x).all() for x in step) and all(np.isfinite(x) for x in lls)
        r_ref, r_orc = wc.ratios(step, ref), wc.ratios(step, orc)
        r_ll = max(abs(x - ref[0]) for x in lls) / tol
        print("WORST %s %s ref %.3g %.3g %.3g %.3g orc %.3g %.3g %.3g %.3g ll3 %.3g" % ((wc.case_id(c), path) + r_ref + r_orc + (r_ll,)))
        if not finite:
            failures.append("%s path: not finite: logL %r, loglik/e_step/prefetch %r" % (path, step[0], lls))
            continue
        if max(r_ref) > 1.0:
            failures.append("%s path: (logL, Q1, P1, S) over tolerance against the long-double reference: %r" % (path, r_ref))
        if max(r_orc) > 1.0:
            failures.append("%s path: (logL, Q1, P1, S) over tolerance against the oracle: %r" % (path, r_orc))
        if r_ll > 1.0:
            failures.append("%s path: loglik / e_step / loglik_prefetch of the worst point %r, reference %r" % (path, lls, ref[0]))
        if lls[0] != lls[1]:
            failures.append("%s path: loglik %r != e_step %r" % (path, lls[0], lls[1]))
    assert not failures, failures
