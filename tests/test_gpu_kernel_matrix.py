"""Every K instance of every EM kernel variant against the oracle.

Each K from 1 to 64 is its own translation unit (Makefile: -DMCHIP_K=K), and inside it plan() of mchip_kernels_k.hip picks
one of about thirty template instances by ploidy, allele counts, missing data, the reciprocal-per-cell condition, the LDS budget,
the testing knobs and the launch geometry.  One such instance (K = 52, tetraploid, reciprocal per cell) once came out of hipcc
miscompiled.  This module visits every (K, instance) cell the dispatch can reach:

  * DISPATCH RULE: a Python statement of which kernels a case reaches (`reach`), each condition citing the C it restates;
    tests/test_kernel_plan_cpu.py holds it against the library's own account (mchip_describe_plan), without a GPU;
  * CASES: a fixed case list, per K and per variant family, on small data sets around the tile edges (I = 64 n +- 1, L not a
    multiple of 8);
  * test_the_case_list_covers_every_reachable_cell (CPU): every (K, kernel) cell the rule can reach over a grid of
    configurations has at least one case, so an edit that shrinks the matrix fails here;
  * test_kernel_matrix_em_step_vs_oracle (-m gpu): one EM step from fixed (Q0, P0), logL, Q1, P1 and S_ik against the oracle
    (fused order), then loglik / e_step / loglik_prefetch of the new point against the oracle's log likelihood;
  * test_kernel_matrix_dual_cycle_vs_oracle (-m gpu): one batched SQUAREM-3 cycle (the dual individual pass, K <= 12) against
    the oracle's accelerated_em_step and bit for bit against the same cycle with MCHIP_NO_DUAL=1.

Tolerances are the suite's own for the same quantities (tests/test_gpu_parity.py, tests/test_gpu_fuzz.py)."""
import ctypes as C
import math

import numpy as np
import pytest

from device_util import knob_contexts, set_knobs
import multiclust_amd as mc
import oracle_bind as ob
from synth import make_dataset, random_params

# ---------------------------------------------------------------------------------------------------------------- DISPATCH RULE
# Constants of the build (mchip_internal.h, mchip_finalize.h) and of the device (MI355X: 256 compute units).
MAX_K = 64                  # MCHIP_MAX_K (include/multiclust_hip.h)
SPARSE_MAX_M = 32           # MCHIP_SPARSE_MAX_M
QBLOCK = 128                # MCHIP_QBLOCK
COL_WAVES = 4               # MCHIP_COL_WAVES = MCHIP_BLOCK / 64
IND_WAVES_MAX = 4           # MCHIP_IND_WAVES_MAX
COL_SPLIT2_ABOVE = 36       # MCHIP_COL_SPLIT2_ABOVE
FP_TILE = 1024              # mchip_finalize.h
N_CU = 256
# the knobs read_knobs() takes (mchip.hip); every test starts from none of them
KNOBS = ("MCHIP_NO_BIAL", "MCHIP_NO_COUNTS", "MCHIP_FORCE_DENSE", "MCHIP_FORCE_SAFE", "MCHIP_NO_GRAPH", "MCHIP_NO_DUAL",
         "MCHIP_NO_SLAB_SUM", "MCHIP_NO_FUSED_FINALIZE", "MCHIP_NO_PAIR", "MCHIP_NO_COL_SPLIT", "MCHIP_PART_NO_TILE", "MCHIP_SIM_NO_TILE",
         "MCHIP_BLOCKS_PER_CU", "MCHIP_BLOCKS_PER_CU_COL", "MCHIP_BLOCKS_PER_CU_IND", "MCHIP_SLAB_FRAC", "MCHIP_NO_CHUNK_ROUNDUP")


def cdiv(a, b):
    return -(-a // b)


def ind_split(K):            # mchip_ind_split (mchip_internal.h)
    return 1 if K <= 27 else (2 if K <= 48 else 4)


def col_split(K):            # mchip_col_split (mchip_internal.h)
    return 2 if K > COL_SPLIT2_ABOVE else 1


def qblock(K):               # mchip_qblock (mchip_internal.h)
    return 2 * QBLOCK if K > 48 else QBLOCK


def ind_pstride(K):          # mchip_ind_pstride, mchip_parts_conflict (mchip_internal.h)
    split = ind_split(K)
    stride = ((cdiv(K, split)) + 1) & ~1

    def conflict(st):
        return any((2 * st * (b - a)) % 64 < 4 or (2 * st * (b - a)) % 64 > 60 for a in range(split) for b in range(a + 1, split))
    while split > 1 and conflict(stride):
        stride += 2
    return stride


def kp(K):                   # mchip_kp (mchip_internal.h): LDS row stride of a staged P row
    base = max(ind_pstride(K) * ind_split(K), (K + 1) & ~1)
    return base + (2 if base % 16 == 0 else 0)


def ind_waves_for(K, tile_cols):     # mchip_ind_waves (mchip_internal.h)
    per_wave = (4 if K <= 12 else 2) * cdiv(tile_cols * kp(K), 128) * 128 * 8
    w = IND_WAVES_MAX
    while w > 1:
        if w * per_wave <= 48 * 1024:
            return w
        w >>= 1
    return 1


def lds_sparse(K, max_M):    # model_geometry's sparse (mchip_plan.hip): two staged tiles of 8 loci fit 64 KiB
    return max_M <= SPARSE_MAX_M and (2 * 8 * max_M * kp(K) + qblock(K)) * 8 <= 65536


def sparse_edge(K):          # the largest max_M that still takes the sparse pass
    return max(m for m in range(1, SPARSE_MAX_M + 1) if lds_sparse(K, m))


def count_bits(ploidy, knobs):       # count_bits_for (mchip_plan.hip)
    if "MCHIP_NO_COUNTS" in knobs:
        return 0
    return 2 if ploidy <= 3 else (4 if ploidy <= 15 else 0)


def finalize_p_loci(K, max_M):       # finalize_p_loci (mchip_plan.hip)
    if max_M > 64 or max_M < 1:
        return 0
    n = FP_TILE // (max_M * K)
    return n if n >= 4 else 0


def flush_blocks(K, ploidy, projection, p_lb):
    """(safe_rcp, flush_blocks) of model_geometry (mchip_plan.hip).  The column passes on packed counts take the
    reciprocal per cell where safe_rcp; the individual-side passes and the dense pair wherever flush_blocks < 1 (sparse_instance:
    `safe = a.flush_blocks < 1`), which a lower bound such as 1e-40 gives without safe_rcp."""
    safe = (not projection) or not (p_lb >= 1e-75)
    tmin = p_lb / K
    blocks = 0
    if projection and 0 < tmin < 1:
        mults = math.floor(200.0 / -math.log10(tmin))
        blocks = min(int(mults / (16.0 if ploidy == 4 else 8.0 * ploidy)), 1 << 16)
    return safe, (0 if safe else blocks)


def geometry(K, I, L, T, ploidy, max_M, admixture, cbits, knobs, n_cu=N_CU):
    """model_geometry (mchip_plan.hip): chunks of either pass, waves of the cooperating sparse pass"""
    def num(name, dflt):
        v = int(knobs.get(name, "0"))
        return v if v > 0 else dflt
    both = num("MCHIP_BLOCKS_PER_CU", 64)
    per_cu_col, per_cu_ind = num("MCHIP_BLOCKS_PER_CU_COL", both), num("MCHIP_BLOCKS_PER_CU_IND", both)
    slab_frac = float(knobs.get("MCHIP_SLAB_FRAC", "0.3"))
    given = any(k in knobs for k in ("MCHIP_BLOCKS_PER_CU", "MCHIP_BLOCKS_PER_CU_COL", "MCHIP_SLAB_FRAC"))
    col_tiles, iblocks, lblocks = cdiv(T, 256), cdiv(I, 8), cdiv(L, 8)
    min_ichunk = math.ceil(8.0 * K * T / (slab_frac * L * ploidy))
    want = cdiv(per_cu_col * n_cu, col_tiles)
    cap = I // (min_ichunk if min_ichunk > 0 else 1)
    soft = max(cap // 2, min(cdiv(2 * 8 * n_cu, col_tiles), cap))
    if not given and want > soft:
        want = soft
    want = min(max(min(want, cap), 1), iblocks)
    if cbits and "MCHIP_NO_CHUNK_ROUNDUP" not in knobs:
        up = cdiv(want, COL_WAVES) * COL_WAVES
        if up <= cap and up <= iblocks:
            want = up
    gran = 128 // cbits if cbits else 8
    ichunk = cdiv(cdiv(I, want), gran) * gran
    n_ichunks = cdiv(I, ichunk)
    ind_tiles = cdiv(I, qblock(K) // (ind_split(K) if admixture else 1))
    min_lchunk = math.ceil(8.0 * K / (slab_frac * ploidy))
    want = cdiv(per_cu_ind * n_cu, ind_tiles)
    cap = L // (min_lchunk if min_lchunk > 0 else 1)
    want = min(max(min(want, cap), 1), lblocks)
    sparse = lds_sparse(K, max_M) and "MCHIP_FORCE_DENSE" not in knobs
    coop = bool(admixture and sparse and ind_split(K) == 1)
    waves = ind_waves_for(K, 8 * max_M) if coop else 1
    if coop:
        up8, up1 = cdiv(want, 8 * waves) * 8 * waves, cdiv(want, waves) * waves
        if up8 <= cap and up8 <= lblocks:
            want = up8
        elif up1 <= cap and up1 <= lblocks:
            want = up1
    lchunk = cdiv(lblocks, want) * 8
    n_lchunks = cdiv(L, lchunk)
    xcd_rows = coop and cdiv(n_lchunks, waves) % 8 == 0
    return dict(n_ichunks=n_ichunks, lchunk=lchunk, n_lchunks=n_lchunks, sparse=sparse, coop=coop, waves=waves, xcd_rows=xcd_rows)


def bial_pays(K, accum):     # sparse_instance (mchip_kernels_k.hip): SPLIT == 1 && (accum ? K >= 10 : K >= 6)
    return ind_split(K) == 1 and (K >= 10 if accum else K >= 6)


def dual_available(K, sparse, ind_safe, ploidy, biallelic, waves, max_M):     # plan()'s dual (mchip_kernels_k.hip)
    if K > 12 or not sparse or ind_safe or ploidy != 2:
        return False
    if biallelic and K >= 6:                                                   # either half would run k_individual_bial
        return False
    tc, p = 8 * max_M, kp(K)
    stride = cdiv(tc * p, 128) * 128 if (p == K and K % 2 == 0 and ind_split(K) == 1) else tc * p
    return max(waves * 2 * 2 * stride, (K + 2) * 64) * 8 <= 64 * 1024


def pair_available(K, sparse, cbits, ploidy, waves, col_safe, ind_safe, biallelic, col_blocks, ind_blocks):
    """plan()'s pair (mchip_kernels_k.hip): col is k_column_counts<2,false,SAFE>, sside k_individual_sparse_w<2,true,SAFE,NOMISS>
    with four waves and the same SAFE; col_blocks / ind_blocks = workgroups of the two (counts_grid, coop_rows)"""
    if K > 12 or ind_split(K) != 1 or col_split(K) != 1:
        return False
    if not sparse or cbits != 2 or ploidy != 2 or waves * 64 != 256:
        return False
    if col_safe != ind_safe:
        return False
    if biallelic and K >= 10 and not ind_safe:                                 # sside would be k_individual_bial
        return False
    col_runs, ind_runs = cdiv(col_blocks, 8), cdiv(ind_blocks, 8)              # MCHIP_PAIR_RUN
    return col_runs > 0 and ind_runs > 0 and (col_runs + ind_runs) * ind_runs < 1 << 32


def B(x):
    return "true" if x else "false"


def sparse_instances(K, ploidy, accum, nomiss, safe, biallelic):
    """sparse_instance (mchip_kernels_k.hip)"""
    if ind_split(K) == 1:
        if bial_pays(K, accum) and biallelic and ploidy == 2 and not safe:
            return "k_individual_bial<%s,%s>" % (B(accum), B(nomiss))
        name = "k_individual_sparse_w"
    else:
        name = "k_individual_sparse"
    if ploidy in (2, 4):
        return "%s<%d,%s,%s,%s,false>" % (name, ploidy, B(accum), B(safe), B(nomiss and not safe))
    return "%s<0,%s,true,false,false>" % (name, B(accum))


def reach(case):
    """The kernels (and geometry facts) one case reaches: an EM step from slot 0 into slot 1 (mchip_em_step), then mchip_loglik,
    mchip_e_step and mchip_loglik_prefetch of slot 1; for `accel` cases one batched SQUAREM cycle (mchip_accel_run) instead.
    Nothing where that call is unsupported (a cycle on the dense pair)."""
    K, I, L, pl, knobs = case["K"], case["I"], case["L"], case["ploidy"], case["knobs"]
    ua, missing = case["ua"], case["missing"]
    min_M, max_M, T = int(ua.min()), int(ua.max()), int(ua.sum())
    admixture, constrained = case["model"] != "mix", case["model"] == "admix_c"
    accel = bool(case.get("accel"))
    cbits = count_bits(pl, knobs)
    g = geometry(K, I, L, T, pl, max_M, admixture, cbits, knobs)
    sparse = g["sparse"]
    safe, flush = flush_blocks(K, pl, case["projection"], case["lb"])
    if "MCHIP_FORCE_SAFE" in knobs:
        safe, flush = True, 0
    ind_safe = flush < 1
    biallelic = min_M == 2 and max_M == 2 and "MCHIP_NO_BIAL" not in knobs      # shape_args (mchip_plan.hip)
    nomiss = not missing
    out = set()
    p_loci = finalize_p_loci(K, max_M)
    if max_M > 64:
        out.add("byte_flag_projection")          # k_finalize_p / k_project_p with d_flags (mchip_plan.hip: needs_byte_flags)
    if not admixture:
        # run_mixture (mchip_em.hip): k_logp, mix_gather, k_mix_finalize, shared eta, mix_column, finalize_p; plan()'s mix_gather, mix_col
        out.add("k_mix_gather<%d,%s>" % (2 if pl == 2 else 0, B(sparse)))
        out |= {"k_mix_finalize", "finalize_shared_eta"}
        out.add("k_column_counts<%d,true,false>" % cbits if cbits else "k_mix_column<%d>" % (2 if pl == 2 else 0))
        out.add("k_finalize_p_tile" if p_loci else "k_finalize_p")
        if (cdiv(g["n_ichunks"], COL_WAVES) if cbits else g["n_ichunks"]) > 8:  # plan()'s mix_col_slabs
            out.add("col_slabs>8")
        if g["n_lchunks"] > 8:
            out.add("ind_slabs>8")
        return out
    if accel and not sparse:
        return set()                             # mchip_accel_run: MCHIP_ERR_UNSUPPORTED
    split_ok = col_split(K) > 1 and "MCHIP_NO_COL_SPLIT" not in knobs
    # plan()'s col (mchip_kernels_k.hip)
    if sparse and cbits and split_ok:
        col = "k_column_counts_split<%d,%s>" % (cbits, B(safe))
    elif sparse and cbits:
        col = "k_column_counts<%d,false,%s>" % (cbits, B(safe))
    elif sparse:
        col = "k_column_pass<%d,true,false,false>" % (2 if pl == 2 else 0)
    elif pl == 2:
        col = "k_column_pass<2,true,%s,true>" % B(flush < 1)
    else:
        col = "k_column_pass<0,true,true,true>"
    if sparse:              # plan()'s sside and ll
        sside = sparse_instances(K, pl, True, nomiss, ind_safe, biallelic)
        ll = sparse_instances(K, pl, False, nomiss, ind_safe, biallelic)
    else:
        sside = "k_individual_pass<%d>" % (2 if pl == 2 else 0)
        ll = "k_column_pass<2,false,%s,true>" % B(flush < 1) if pl == 2 else "k_column_pass<0,false,true,true>"
    # plan()'s col_slabs, ind_slabs, pair and dual
    n_slabs = cdiv(g["n_ichunks"], COL_WAVES) if (sparse and cbits and not split_ok) else g["n_ichunks"]
    s_slabs = cdiv(g["n_lchunks"], g["waves"]) if (sparse and ind_split(K) == 1) else g["n_lchunks"]
    pair = "MCHIP_NO_PAIR" not in knobs and pair_available(K, sparse, cbits, pl, g["waves"], safe, ind_safe, biallelic,
                                                           cdiv(T, 64) * n_slabs, cdiv(I, 64) * s_slabs)
    dual = "MCHIP_NO_DUAL" not in knobs and dual_available(K, sparse, ind_safe, pl, biallelic, g["waves"], max_M)
    # run_estep (mchip_em.hip) with the M step: the two passes, where the pair exists as one launch that runs the bodies of both
    # (mchip_describe_plan lists all three), then the finalisers (finish_for)
    out |= {col, sside}
    if pair:
        out.add("k_estep_pair<2,2,%s,%s>" % (B(ind_safe), B(nomiss and not ind_safe)))
    slab_sum = n_slabs > 8 and "MCHIP_NO_SLAB_SUM" not in knobs
    if not constrained and p_loci and not slab_sum and "MCHIP_NO_FUSED_FINALIZE" not in knobs:
        out.add("k_finalize_qp")
    else:
        out.add("k_finalize_q")
        if slab_sum:
            out.add("k_sum_slabs")
        out.add("k_finalize_p_tile" if p_loci else "k_finalize_p")
    if constrained:
        out.add("finalize_shared_eta")
    if accel:               # accel_cycle_enqueue (mchip_accel.hip): log L of the second iterate and of the extrapolated point
        out |= {"k_individual_sparse_w<2,true,false,%s,true>" % B(nomiss)} if dual else {ll, sside}
    else:                   # mchip_loglik; mchip_e_step (run_estep without the M step: k_finalize_q); mchip_loglik_prefetch
        out |= {ll, sside, "k_finalize_q"}
    if n_slabs > 8:
        out.add("col_slabs>8")
    if s_slabs > 8:
        out.add("ind_slabs>8")
    if g["xcd_rows"]:
        out.add("xcd_rows")
    return out


# pseudo-cell of reach -> the same statement about the key=value lines of mchip_describe_plan
PSEUDO = {
    "col_slabs>8": lambda f: f["col_slabs"] > 8,
    "ind_slabs>8": lambda f: f["ind_slabs"] > 8,
    "xcd_rows": lambda f: f["xcd_rows"],
    "byte_flag_projection": lambda f: f["byte_flags"],
    "finalize_shared_eta": lambda f: f["shared_eta"],
}


def plan_query(c, n_cu=N_CU):
    """the case as mchip_describe_plan takes it (multiclust_amd.hip.describe_plan)"""
    ua = c["ua"]
    return dict(K=c["K"], I=c["I"], L=c["L"], T=int(ua.sum()), ploidy=c["ploidy"], min_alleles=int(ua.min()),
                max_alleles=int(ua.max()), has_missing=int(bool(c["missing"])), admixture=int(c["model"] != "mix"),
                eta_constrained=int(c["model"] == "admix_c"), do_projection=c["projection"], p_lb=c["lb"], n_cu=n_cu,
                accel_cycle=int(bool(c.get("accel"))))


# ---------------------------------------------------------------------------------------------------------------------- CASES
FAMILIES = ["dip_nomiss", "dip_miss", "tet_nomiss", "tet_miss", "triploid", "hexaploid", "haploid", "bial_nomiss", "bial_miss",
            "noproj_p2", "noproj_p4", "bound40_p2", "bound40_p4", "ploidy16", "nocounts_p2", "edge_sparse", "edge_dense",
            "dense_flush", "dense_noflush", "dense_p3", "alleles_gt64", "shared_eta", "mix_2bit", "mix_4bit", "mix_nocounts",
            "mix_nocounts_p2", "mix_dense", "mix_dense_p3", "geom_slabs", "geom_xcd", "nocolsplit_p2", "nocolsplit_p4", "nocolsplit_noproj_p2",
            "nocolsplit_noproj_p4"]
GEOM = {"MCHIP_SLAB_FRAC": "1000"}        # slab caps out of the way: as many chunks as the data set has blocks of 8


def alleles(L, spec, rs):
    """allele counts per locus: `spec` = (low, high) drawn, with low and high both present"""
    lo, hi = spec
    ua = rs.integers(lo, hi + 1, size=L).astype(np.int32)
    ua[0], ua[L // 2] = lo, hi
    return ua


def small_shape(K, fam):
    j = (K + FAMILIES.index(fam)) % 4
    return (63, 65, 127, 129)[j], (21, 29, 37, 45)[(K // 4 + j) % 4]


def geometry_shape(c, want):
    """the smallest of a few candidate shapes (I = 64 n + 1) on which the case's geometry does what `want` asks"""
    for I in (65, 129, 577, 1089, 2113):
        for L in (45, 77, 141, 269, 509):
            c.update(I=I, L=L)
            ua = case_ua(c)[0]
            if want(reach(case_dict(c, ua)), geometry(c["K"], I, L, int(ua.sum()), c["ploidy"], int(ua.max()), True,
                                                      count_bits(c["ploidy"], c["knobs"]), c["knobs"])):
                return I, L
    raise AssertionError("no candidate shape for K = %d" % c["K"])


def make_case(fam, K):
    seed = 1000 * K + FAMILIES.index(fam)
    rs = np.random.default_rng(seed)
    I, L = small_shape(K, fam)
    c = dict(family=fam, K=K, I=I, L=L, ploidy=2, spec=(2, 4), missing=0.0, model="admix", projection=1, bound=1e-8, knobs={},
             seed=seed, wide=None)
    if fam == "dip_miss" or fam == "shared_eta" or fam == "geom_xcd":
        c["missing"] = 0.03
    if fam.startswith("tet"):
        c["ploidy"] = 4
        c["missing"] = 0.03 if fam == "tet_miss" else 0.0
    if fam in ("triploid", "hexaploid", "haploid"):
        c["ploidy"] = {"triploid": 3, "hexaploid": 6, "haploid": 1}[fam]
        c["missing"] = 0.0 if fam == "hexaploid" else 0.03
    if fam.startswith("bial"):
        c["spec"], c["missing"] = (2, 2), (0.03 if fam == "bial_miss" else 0.0)
    if fam.startswith("noproj"):
        c["projection"], c["missing"], c["ploidy"] = 0, 0.03, int(fam[-1])
    if fam.startswith("bound40"):
        c["bound"], c["ploidy"] = 1e-40, int(fam[-1])
    if fam == "ploidy16":
        c["ploidy"], c["projection"], c["missing"] = 16, 0, 0.03
    if fam == "nocounts_p2":
        c["knobs"] = {"MCHIP_NO_COUNTS": "1"}
    if fam == "edge_sparse":
        c["spec"] = (2, sparse_edge(K))
    if fam == "edge_dense":
        c["spec"] = (2, sparse_edge(K) + 1)
    if fam.startswith("dense_"):
        c["spec"], c["knobs"] = (2, 3), {"MCHIP_FORCE_DENSE": "1"}
        if fam == "dense_noflush":
            c["bound"] = 1e-20                    # below ~3e-13 K: no log-product check between blocks, still shared reciprocals
        if fam == "dense_p3":
            c["ploidy"] = 3
    if fam == "alleles_gt64":
        c["wide"] = 65 + int(rs.integers(0, 56))  # one locus with 65-120 alleles
    if fam == "shared_eta":
        c["model"] = "admix_c"
    if fam.startswith("mix"):
        c["model"] = "mix"
        c["ploidy"] = {"mix_2bit": 2, "mix_4bit": 4, "mix_nocounts": 16, "mix_nocounts_p2": 2, "mix_dense": 2, "mix_dense_p3": 3}[fam]
        if fam.startswith("mix_dense"):
            c["spec"] = (2, sparse_edge(K) + 1)
        if fam == "mix_nocounts_p2":
            c["knobs"] = {"MCHIP_NO_COUNTS": "1"}
        if fam == "mix_2bit":
            c["missing"] = 0.03
    if fam.startswith("nocolsplit"):
        c["knobs"], c["ploidy"] = {"MCHIP_NO_COL_SPLIT": "1"}, int(fam[-1])
        if "noproj" in fam:
            c["projection"], c["missing"] = 0, 0.03
    if fam == "geom_slabs":                       # both axes leave more than eight slabs, the S side not whole groups of 8 rows
        c["knobs"] = dict(GEOM)
        c["I"], c["L"] = geometry_shape(c, lambda r, g: "col_slabs>8" in r and "ind_slabs>8" in r and not g["xcd_rows"])
    if fam == "geom_xcd":                         # the S side ends on whole groups of eight rows: one row, one XCD
        c["knobs"] = dict(GEOM)
        c["I"], c["L"] = geometry_shape(c, lambda r, g: "xcd_rows" in r and "ind_slabs>8" in r)
    return c


def applies(fam, K):
    if fam == "geom_xcd":
        return ind_split(K) == 1                  # only the cooperating sparse pass (K <= 27) maps rows to XCDs
    if fam.startswith("nocolsplit"):
        return col_split(K) > 1
    return True


def case_ua(c):
    rs = np.random.default_rng(c["seed"] + 7)
    ua = alleles(c["L"], c["spec"], rs)
    if c["wide"]:
        ua[c["L"] // 3] = c["wide"]
    return ua, rs


def build_data(c):
    I, L, pl, K = c["I"], c["L"], c["ploidy"], c["K"]
    ua, rs = case_ua(c)
    ua0, geno = make_dataset(I, L, max(K, 2), ploidy=pl, max_alleles=2, seed=c["seed"], missing=c["missing"])
    # redraw the copies at loci that have more than the two alleles make_dataset drew (missing copies stay missing)
    for l in np.nonzero(ua != ua0)[0]:
        keep = geno[:, l, :] == 0xFF
        geno[:, l, :] = np.where(keep, 0xFF, rs.integers(0, ua[l], size=(I, pl))).astype(np.uint8)
    return ua, np.ascontiguousarray(geno)


def case_dict(c, ua):
    lb = ob.lib.mco_lower_bound(c["bound"], c["I"], c["ploidy"])
    return dict(c, ua=ua, lb=lb)


def all_cases():
    out = []
    for K in range(1, MAX_K + 1):
        for fam in FAMILIES:
            if applies(fam, K):
                out.append(make_case(fam, K))
    return out


def dual_cases():
    out = []
    for K in range(1, 13):
        for miss in (0.0, 0.03):
            c = make_case("dip_miss" if miss else "dip_nomiss", K)
            c.update(family="dual_" + ("miss" if miss else "nomiss"), accel=True, seed=c["seed"] + 500)
            out.append(c)
    return out


CASES = all_cases()
DUAL = dual_cases()


def case_id(c):
    return "%s-K%d-%dx%dx%d" % (c["family"], c["K"], c["I"], c["L"], c["ploidy"])


# ------------------------------------------------------------------------------------------------------------------ CPU test
def grid_configs(K):
    """the grid of configurations (cases as `reach` takes them) of grid_reach"""
    rs = np.random.default_rng(K)
    specs = [(2, 2), (2, 4), (2, sparse_edge(K)), (2, sparse_edge(K) + 1), (2, 100)]
    bounds = [(1, 1e-8), (1, 1e-20), (1, 1e-40), (0, 1e-8)]
    knobsets = [{}, {"MCHIP_NO_COUNTS": "1"}, {"MCHIP_FORCE_DENSE": "1"}, {"MCHIP_NO_COL_SPLIT": "1"}]
    shapes = [(65, 45, {}), (2113, 269, GEOM), (65, 509, GEOM), (577, 77, GEOM)]
    uas = {(spec, L): alleles(L, spec, rs) for spec in specs for _, L, _ in shapes}
    for pl in (1, 2, 3, 4, 16):
        for spec in specs:
            for I, L, geo in shapes:
                ua = uas[(spec, L)]
                for missing in (0.0, 0.03):
                    for proj, bound in bounds:
                        for model in ("admix", "admix_c", "mix"):
                            for kn in knobsets:
                                if geo and (kn or model != "admix" or bound != 1e-8 or spec[1] > 4 or pl != 2):
                                    continue
                                c = dict(K=K, I=I, L=L, ploidy=pl, knobs=dict(kn, **geo), ua=ua, missing=missing, model=model,
                                         projection=proj, lb=min(bound, 0.5 / (I * pl)))
                                yield c
                                if model == "admix" and not kn and not geo:
                                    yield dict(c, accel=True)


def grid_reach(K):
    """every (kernel, geometry fact) the rule gives at this K over a grid of configurations"""
    cells = set()
    for c in grid_configs(K):
        cells |= reach(c)
    return cells


def test_sparse_edge_table():
    """the LDS edge (model_geometry's sparse) as derived from mchip_kp: the largest max_M of the sparse pass, K by K"""
    want = {1: 32, 14: 32, 15: 28, 18: 28, 19: 25, 20: 25, 21: 22, 22: 22, 23: 21, 24: 21, 25: 19, 26: 19, 27: 18, 28: 18,
            29: 14, 36: 14, 37: 12, 40: 12, 41: 11, 44: 11, 45: 10, 48: 10, 49: 8, 56: 8, 57: 6, 64: 6}
    assert {K: sparse_edge(K) for K in want} == want
    assert all(sparse_edge(K) >= sparse_edge(K + 1) for K in range(1, MAX_K))


def test_the_case_list_covers_every_reachable_cell():
    have = {}
    for c in CASES + DUAL:
        for cell in reach(case_dict(c, case_ua(c)[0])):
            have.setdefault(c["K"], set()).add(cell)
    missing = {K: sorted(grid_reach(K) - have.get(K, set())) for K in range(1, MAX_K + 1)}
    missing = {K: m for K, m in missing.items() if m}
    assert not missing, missing
    # the family table of the issue, K by K
    for K in range(1, MAX_K + 1):
        h = have[K]
        assert "k_sum_slabs" in h and "col_slabs>8" in h and "ind_slabs>8" in h and "k_finalize_p" in h, K
        assert ("xcd_rows" in h) == (K <= 27), K
        assert any(x.startswith("k_column_counts_split<") for x in h) == (K > 36), K
        assert ("k_individual_bial<true,true>" in h) == (10 <= K <= 27) and ("k_individual_bial<false,false>" in h) == (6 <= K <= 27), K
        assert "k_individual_pass<2>" in h and "k_individual_pass<0>" in h and "k_column_pass<2,true,true,true>" in h, K
        assert ("k_individual_sparse_w<2,true,false,true,true>" in h) == (K <= 12), K
        # the pair (plan(): K <= 12; two to four alleles stage 32 columns of at most 12 doubles, four waves' tiles fill the 48 KiB
        # of mchip_ind_waves exactly at K = 11 and 12), with shared reciprocals without and with missing data, and without them
        for inst in ("false,true", "false,false", "true,false"):
            assert ("k_estep_pair<2,2,%s>" % inst in h) == (K <= 12), (K, inst)
    ids = [case_id(c) for c in CASES + DUAL]
    assert len(ids) == len(set(ids))
    assert {c["K"] for c in CASES} == set(range(1, MAX_K + 1))


# ------------------------------------------------------------------------------------------------------------------ GPU tests
def finite_except_empty(a, empty):
    keep = np.ones(a.shape[0], dtype=bool)
    keep[empty] = False
    return np.isfinite(a[keep]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_kernel_matrix_em_step_vs_oracle(knob_contexts, monkeypatch, c):
    ua, geno = build_data(c)
    K, I, L, pl = c["K"], c["I"], c["L"], c["ploidy"]
    cd = case_dict(c, ua)
    lb = cd["lb"]
    admixture, con = int(c["model"] != "mix"), int(c["model"] == "admix_c")
    q0, p0 = random_params(I, ua, K, seed=c["seed"] + 1, lower_bound=max(lb, 1e-12))
    if not admixture:
        q0 = np.full(K, 1.0 / K)
    elif con:
        q0 = np.ascontiguousarray(q0[0])
    opt = ob.make_options(admixture=admixture, eta_constrained=con, do_projection=c["projection"], lower_bound=lb, fused=1,
                          abs_error=0.0)
    mod = ob.Model(ob.Data(I, L, pl, ua, geno), opt, K)
    mod.q(0)[...] = q0
    mod.p(0)[...] = p0
    set_knobs(monkeypatch, c["knobs"], KNOBS)
    ctx = knob_contexts(c["knobs"])
    ctx.set_genotypes(ua, geno)
    ctx.set_model(K, admixture=admixture, eta_constrained=con, do_projection=c["projection"], lower_bound=lb)
    n_cu = ctx.device_info()[1]
    if n_cu == N_CU:        # what the library launches on this device is what the rule (and so the coverage proof) says
        cd["missing"] = bool((geno == 0xFF).any())
        rc, kernels, facts = mc.hip.describe_plan(**plan_query(cd, n_cu))
        want = reach(cd)
        assert rc == 0 and kernels == want - set(PSEUDO), (rc, sorted(kernels ^ (want - set(PSEUDO))))
        assert all((cell in want) == bool(says(facts)) for cell, says in PSEUDO.items()), (facts, sorted(want))
    ctx.set_q(0, q0)
    ctx.set_p(0, p0)
    ll = ctx.em_step(0, 1)
    mod.em_step()
    empty = np.nonzero((geno == 0xFF).all(axis=(1, 2)))[0] if (admixture and not con) else []
    q1, p1, sik = ctx.get_q(1), ctx.get_p(1), ctx.expected_counts()
    assert np.isfinite(ll) and np.isfinite(p1).all() and finite_except_empty(sik, empty)
    assert (finite_except_empty(q1, empty) if q1.ndim == 2 else np.isfinite(q1).all())
    qo, po = mod.q(mod.pindex), mod.p(mod.pindex)
    ll_o = mod.loglik(mod.pindex)
    if admixture:
        assert abs(ll - mod.logL) <= max(1e-8, 1e-12 * abs(mod.logL)), (ll, mod.logL)
        np.testing.assert_allclose(q1, qo, rtol=1e-11, atol=1e-15)
        np.testing.assert_allclose(p1, po, rtol=1e-11, atol=1e-15)
        np.testing.assert_allclose(sik, mod.sik(), rtol=1e-11, atol=1e-12)
        tol = max(1e-8, 1e-12 * abs(ll_o))
    else:
        # the mixture model's documented bounds (tests/test_gpu_fuzz.py: test_random_shapes_mixture_vs_oracle)
        assert abs(ll - mod.logL) <= max(1e-8, 1e-12 * abs(mod.logL)), (ll, mod.logL)
        np.testing.assert_allclose(q1, qo, rtol=1e-7, atol=1e-13)
        np.testing.assert_allclose(p1, po, rtol=1e-7, atol=1e-13)
        np.testing.assert_allclose(sik, mod.sik(), rtol=1e-7, atol=1e-12)
        tol = max(1e-8, 1e-11 * abs(ll_o))
    a, b, d = ctx.loglik(1), ctx.e_step(1), ctx.loglik_prefetch(1)
    assert np.isfinite(a) and np.isfinite(b) and np.isfinite(d), (a, b, d)
    # The mixture model's E step returns e_step_mixture's log likelihood (em_alg.c), its log likelihood logL_mixture's
    # (log_likelihood.c), and the reference's two differ where exp(max_k v_ik) is subnormal (logL_mixture rescales only once it
    # is 0): 1.04 in 97 000 on 129 individuals of ploidy 16.  Each is checked against its own counterpart.
    b_o = ll_o if admixture else mod.e_step()
    assert abs(a - ll_o) <= tol and abs(b - b_o) <= tol and abs(d - ll_o) <= tol, (a, b, d, ll_o, b_o)


@pytest.mark.gpu
@pytest.mark.parametrize("c", DUAL, ids=case_id)
def test_kernel_matrix_dual_cycle_vs_oracle(knob_contexts, monkeypatch, c):
    """One batched SQUAREM-3 cycle (mchip_accel_run; the dual individual pass where the plan has one) against the oracle's
    accelerated_em_step from the same point, and bit for bit against the same cycle with the dual pass off (MCHIP_NO_DUAL=1)."""
    ua, geno = build_data(c)
    K, I, L, pl = c["K"], c["I"], c["L"], c["ploidy"]
    lb = ob.lib.mco_lower_bound(1e-8, I, pl)
    q0, p0 = random_params(I, ua, K, seed=c["seed"] + 1, lower_bound=lb)
    opt = ob.make_options(lower_bound=lb, fused=1, accel_scheme=3, abs_error=1e-300)
    mod = ob.Model(ob.Data(I, L, pl, ua, geno), opt, K)
    mod.q(0)[...] = q0
    mod.p(0)[...] = p0
    stop_o, trace = mod.accelerated_em_step()
    out = []
    for knobs in ({}, {"MCHIP_NO_DUAL": "1"}):
        set_knobs(monkeypatch, knobs, KNOBS)
        ctx = knob_contexts(knobs)
        ctx.set_genotypes(ua, geno)
        ctx.set_model(K, lower_bound=lb, n_secants=1)
        ctx.set_q(0, q0)
        ctx.set_p(0, p0)
        st = mc.hip.RunState(logL=-np.inf, abs_error=1e-300, n_iter=0)
        rc = ctx.lib.mchip_accel_run(ctx.h, 0, 3, 1, C.byref(st))
        assert rc == 0 and st.fatal == 0, (rc, st.fatal)
        out.append((st.logL, st.n_iter, st.stopped, st.converged, ctx.get_q(0), ctx.get_p(0)))
    (ll, n_iter, stopped, conv, q, p), other = out
    assert (ll, n_iter, stopped, conv) == other[:4]
    assert np.array_equal(q, other[4]) and np.array_equal(p, other[5])
    assert stop_o == 0 and n_iter == mod.n_iter == 2
    assert np.isfinite(ll) and np.isfinite(q).all() and np.isfinite(p).all()
    assert abs(ll - mod.logL) <= max(1e-8, 1e-12 * abs(mod.logL)), (ll, mod.logL)
    np.testing.assert_allclose(q, mod.q(mod.pindex), rtol=1e-8, atol=1e-13)
    np.testing.assert_allclose(p, mod.p(mod.pindex), rtol=1e-8, atol=1e-13)
