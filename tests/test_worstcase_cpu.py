"""The worst-case inputs of tests/worstcase.py have teeth, and their long-double reference is sound (no GPU needed).

  * test_product_rule_simulation: a pure-Python simulation of the running-product rule (multiply, look every n slots, move the
    exponent out below 1e-100) over the per-copy t sequence of every worst row (and, in the dense family, every worst
    column) of every case.  With the right interval the product never goes below DBL_MIN, reaches what legal parameters can
    reach, and the log equals the long-double sum within 1e-9.  With the interval doubled the result is -inf for at least one
    row (column) of every edge-bound case; at the customary 1e-8 bound, with the plain pattern the control keeps, a doubled
    interval goes unnoticed (25 safe multiplications, 16 used), which is why the edge bounds exist.
  * test_geometry_and_instances: with the cases' knobs a chunk spans a whole period of the pattern (a chunk restarts the
    product), and each case reaches the template instances it is meant for (`geometry`, `reach` of test_gpu_kernel_matrix.py).
  * test_oracle_against_longdouble_reference: one fused em_step of the oracle against `reference_step` at the suite's step-1
    tolerances (test_em_steps_vs_oracle_paths).  Measured on all 670 cases: logL at most 0.45 of its tolerance, Q1 0.17, P1 0.09,
    S 1.6e-4: the reference alone stays well inside every tolerance.

How deep legal parameters reach.  The host sizes the look interval for t >= lb / K, but the q_k sum to 1, so every t is >= lb:
at lb = edge_bound(K, b) the largest fall between two looks is n (-log10 lb) = 200 - 16 b log10(1.001 K) decades from just
above 1e-100.  The smallest product is therefore below 1e-280 only where 16 b log10(1.001 K) < 20 (`reaches_1e280`: b = 1 to
K = 13, b = 2 and 3 to K = 2); that is asserted there, and every edge case is asserted to reach its own deepest legal product.
A doubled interval is -inf at every edge bound: two looks' worth of tiny factors behind a product that stands just above
1e-100 unrescaled is 100 + 2 n (-log10 lb) >= 326 decades."""
import math
import sys

import numpy as np
import pytest

import worstcase as wc
from test_gpu_kernel_matrix import count_bits, flush_blocks, geometry, reach

CASES = wc.all_cases()
DBL_MIN = sys.float_info.min


def test_edge_bounds():
    assert abs(wc.edge_bound(1, 1) / 3.17e-13 - 1) < 0.01 and abs(wc.edge_bound(1, 2) / 5.6e-7 - 1) < 0.01
    assert abs(wc.edge_bound(1, 3) / 6.8e-5 - 1) < 0.01 and abs(wc.edge_bound(64, 3) / 4.4e-3 - 1) < 0.01
    for K in range(1, 65):
        for b in (1, 2, 3):
            lb = wc.edge_bound(K, b)            # asserts flush_blocks == b, and b - 1 just below, for ploidy 2 and 4
            assert lb <= wc.medium(16 * b), (K, b)
            assert flush_blocks(K, 2, 1, lb) == flush_blocks(K, 4, 1, lb) == (False, b)     # the kernel matrix's restatement agrees
    assert wc.host_flush_blocks(13, 1e-75) == (False, 0) and wc.host_flush_blocks(13, 0.99e-75) == (True, 0)
    for K in wc.K_VALUES + wc.K_SHARED:
        assert wc.host_flush_blocks(K, 1e-8, 2) == wc.host_flush_blocks(K, 1e-8, 4) == (False, 1)
    # a doubled interval behind a product just above 1e-100 is past the smallest subnormal at every edge bound
    for K in range(1, 65):
        for b in (1, 2, 3):
            assert 100 + 2 * 16 * b * -math.log10(wc.edge_bound(K, b)) > 326
    deep = {(b, K) for b in (1, 2, 3) for K in wc.K_VALUES if wc.reaches_1e280(wc.make_case("dip", K, "edge%d" % b, False))}
    assert deep == {(1, K) for K in wc.K_VALUES if K <= 13} | {(b, K) for b in (2, 3) for K in (1, 2)}


def test_case_list():
    ids = [wc.case_id(c) for c in CASES]
    assert len(ids) == len(set(ids)) == 4 * 16 * 5 * 2 + 3 * 5 * 2
    assert {c["K"] for c in CASES if c["family"] != "shared"} == set(wc.K_VALUES)


@pytest.mark.parametrize("c", CASES, ids=wc.case_id)
def test_inputs_are_legal_and_carry_the_pattern(c):
    ua, geno, q, p = wc.build(c)
    K, lb, med, pl = c["K"], c["lb"], c["med"], c["ploidy"]
    assert (p >= lb).all() and (q >= lb).all() and np.allclose(q.sum(axis=-1), 1.0, rtol=0, atol=1e-14)
    off = 0
    for M in ua:
        assert np.allclose(p[:, off:off + M].sum(axis=1), 1.0, rtol=0, atol=1e-14)
        off += M
    assert ((geno == wc.MISSING).mean() > 0.005) == bool(c["missing"])
    if c["model"] == "admix":
        vertex = q[2::wc.VERTEX_EVERY]
        assert ((vertex == lb).sum(axis=1) == K - 1).all()
    t = np.array(wc.full_q(q, c["I"])) @ p
    if c["family"] != "bial":
        assert np.allclose(t[:, 0::4], lb, rtol=1e-14, atol=0) and np.allclose(t[:, 1::4], med, rtol=1e-14, atol=0)
        # one t at the bound beside one of order 1 under a shared reciprocal: heterozygotes tiny / ordinary
        g = geno.astype(int)
        assert (((g[:, :, 0] == 0) & (g[:, :, 1] >= 2)) | ((g[:, :, 1] == 0) & (g[:, :, 0] >= 2))).sum() > 100
    else:
        assert (np.isclose(t, lb, rtol=1e-14, atol=0).all(axis=0).sum()) >= 3 * (c["n"] // pl)      # columns at the bound for everyone
    # four t of the bound in one group of the packed-count column pass: every individual of such a column
    assert np.isclose(t, lb, rtol=1e-14, atol=0).all(axis=0).any()


@pytest.mark.parametrize("c", CASES, ids=wc.case_id)
def test_product_rule_simulation(c):
    ua, geno, q, p = wc.build(c)
    if c["family"] == "dense":      # the column side carries the log likelihood: the columns of the tiny and the medium allele
        seqs = [wc.col_slots(c, ua, geno, q, p, l, m) for l in wc.worst_cols(c) for m in (0, 1)]
    else:
        seqs = [wc.row_slots(c, ua, geno, q, p, i) for i in wc.worst_rows(c)]
    assert len(seqs) >= 19
    n = c["n"] if c["flush_blocks"] else 1      # flush_blocks == 0: a look after every copy
    assert n == 16 * c["flush_blocks"] or not c["flush_blocks"]
    low, n_inf, worst2 = 1.0, 0, 0.0
    for s in seqs:
        exact = float(np.log(np.array(s, dtype=np.longdouble)).sum())
        got, lo = wc.simulate_product(s, n)
        assert lo >= DBL_MIN and abs(got - exact) <= 1e-9, (lo, got, exact)
        low = min(low, lo)
        got2, _ = wc.simulate_product(s, 2 * n)
        n_inf += got2 == -math.inf
        if got2 != -math.inf:
            worst2 = max(worst2, abs(got2 - exact))
    print("%s: smallest product %.3g (deepest legal 1e%.1f), doubled interval: %d of %d -inf, else off by %.3g"
          % (wc.case_id(c), low, wc.deepest_log10(c["lb"], c["n"]), n_inf, len(seqs), worst2))
    if wc.is_edge(c):
        # the deepest legal product is reached: by the rows to the 1.001^n headroom of the medium factors, by a column (whose
        # head of the tiny run is a whole number of factors) to within one factor
        slack = 0.1 + (-math.log10(c["lb"]) if c["family"] == "dense" else 0.0)
        assert math.log10(low) < wc.deepest_log10(c["lb"], c["n"]) + slack
        if c["K"] == 1 or (wc.reaches_1e280(c) and c["family"] != "dense"):
            assert low < 1e-280
        assert n_inf >= 1                       # a look that comes half as often is -inf
    elif c["bound"] == "1e-8":
        # the control: a doubled interval is NOT detected at the customary bound
        assert n_inf == 0 and worst2 <= 1e-9 and low > 1e-260


@pytest.mark.parametrize("c", CASES, ids=wc.case_id)
def test_geometry_and_instances(c):
    K, I, L, pl = c["K"], c["I"], c["L"], c["ploidy"]
    M = 2 if c["family"] == "bial" else 4
    ua = np.full(L, M, dtype=np.int32)
    cbits = count_bits(pl, c["knobs"])
    g = geometry(K, I, L, int(ua.sum()), pl, M, True, cbits, c["knobs"])
    period = 4 * (c["n"] // pl)                 # loci (individuals, for a column) of four looks' worth of homozygotes
    assert g["lchunk"] >= period and L >= period, (g, period)
    if c["family"] == "dense":
        assert g["n_ichunks"] == 1 and I >= period and not g["sparse"]
    got = reach(dict(c, ua=ua, projection=1))
    B = {True: "true", False: "false"}
    nomiss, ind_safe = not c["missing"], c["flush_blocks"] < 1
    assert ind_safe == (c["bound"] == "1e-75") and not c["safe_rcp"]
    want = set()
    if c["family"] == "dense":
        want |= {"k_column_pass<2,true,%s,true>" % B[ind_safe], "k_column_pass<2,false,%s,true>" % B[ind_safe], "k_individual_pass<2>"}
    else:
        # shared reciprocals on the column side at every bound of the list, 1e-75 included
        want.add("k_column_counts_split<%d,false>" % cbits if K > 36 else "k_column_counts<%d,false,false>" % cbits)
        for accum in (True, False):
            if c["family"] == "bial" and not ind_safe and (10 if accum else 6) <= K <= 27:
                want.add("k_individual_bial<%s,%s>" % (B[accum], B[nomiss]))
            else:
                want.add("%s<%d,%s,%s,%s,false>" % ("k_individual_sparse_w" if K <= 27 else "k_individual_sparse", pl, B[accum],
                                                    B[ind_safe], B[nomiss and not ind_safe]))
    assert want <= got, (sorted(want - got), sorted(got))
    # and with MCHIP_FORCE_SAFE=1, the second path of the GPU test, none of them
    safe = reach(dict(c, ua=ua, projection=1, knobs=dict(c["knobs"], MCHIP_FORCE_SAFE="1")))
    assert not any(",false,true>" in x and x.startswith("k_column_pass<2") for x in safe)
    assert not any(x.startswith("k_individual_bial") or x.startswith("k_column_counts<%d,false,false" % cbits)
                   or x.startswith("k_column_counts_split<%d,false" % cbits) for x in safe), sorted(safe)
    assert not any(x.startswith("k_individual_sparse") and x.split(",")[2] == "false" for x in safe), sorted(safe)


@pytest.mark.parametrize("c", CASES, ids=wc.case_id)
def test_oracle_against_longdouble_reference(c):
    ua, geno, q, p = wc.build(c)
    ref = wc.reference_step(ua, geno, q, p, c["lb"], c["model"])
    orc = wc.oracle_step(c, ua, geno, q, p)
    assert all(np.isfinite(x).all() for x in ref) and all(np.isfinite(x).all() for x in orc)
    r = wc.ratios(orc, ref)
    print("%s: oracle / long double, difference over tolerance: logL %.3g Q1 %.3g P1 %.3g S %.3g" % ((wc.case_id(c),) + r))
    assert max(r) <= 1.0, r
