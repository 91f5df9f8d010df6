"""Query individuals on the CPU (TEST INFRASTRUCTURE): the numpy restatement of mchip_fit_q_rows -- update, simplex projection as
michelot_strided does it, stopping rule, empty row, non-finite row -- in any float type, and the inputs tests/test_gpu_query.py and
tests/test_query_cpu.py share."""
import functools

import numpy as np

from cv_util import cv_dataset
from synth import make_dataset, random_params

MISSING = 0xFF
EPS = 2.0 ** -52


def michelot(x, mn):
    """michelot_strided (multiclust_amd/csrc/mchip_finalize.h), operation for operation, in x's own float type"""
    x = x.copy()
    one = x.dtype.type(1)
    fixed = np.zeros(len(x), dtype=bool)
    n = len(x)
    while n:
        csum = x.dtype.type(0)
        for v in x:
            csum = csum + v
        shift = (csum - one) / x.dtype.type(n)
        can_terminate = True
        for j in range(len(x)):
            if fixed[j]:
                continue
            v = x[j] - shift
            if v < mn:
                v = x.dtype.type(mn)
                fixed[j] = True
                n -= 1
                can_terminate = False
            x[j] = v
        if can_terminate:
            break
    return x


def row_columns(ua, g):
    """allele columns of the observed copies of one individual's genotype g [L][ploidy], in l, a order"""
    toff = np.concatenate(([0], np.cumsum(ua)))[:-1]
    ll, _ = np.nonzero(g != MISSING)
    return toff[ll] + g[g != MISSING].astype(np.int64)


def fit_row(ua, g, p, q0, max_iter, abs_error=0.0, rel_error=0.0, do_projection=True, lb=1e-8, dtype=np.float64):
    """One row of mchip_fit_q_rows as include/multiclust_hip.h defines it.  g [L][ploidy], p [K][T], q0 [K] or None (1 / K).
    Returns dict(q, logL, n, converged, copies, abs_logs = sum |log t| of the stopping evaluation, deltas = |l_n - l_(n-1)| of
    every evaluation n >= 1, prevs = the l_(n-1) beside them)."""
    K = p.shape[0]
    cols = row_columns(ua, g)
    out = dict(copies=len(cols), deltas=[], prevs=[], abs_logs=0.0)
    if not len(cols):
        out.update(q=np.full(K, 1.0 / K), logL=0.0, n=0, converged=0)
        return out
    pc = p[:, cols].astype(dtype)                       # [K][copies]
    q = (np.full(K, 1.0 / K) if q0 is None else np.asarray(q0)).astype(dtype)
    prev = None
    n = 0
    while True:
        with np.errstate(divide="ignore", invalid="ignore"):
            t = q @ pc
            logs = np.log(t)
            ll = logs.sum()
        out["abs_logs"] = float(np.abs(logs).sum())
        if not np.isfinite(ll):
            out.update(q=np.full(K, np.nan), logL=float(ll), n=n, converged=0)
            return out
        conv = 0
        if n >= 1 and (abs_error != 0 or rel_error != 0):
            d = abs(ll - prev)
            out["deltas"].append(float(d))
            out["prevs"].append(float(prev))
            conv = 1
            if abs_error != 0 and d > abs_error:
                conv = 0
            if rel_error != 0 and d / abs(prev) > rel_error:
                conv = 0
        if conv or n == max_iter:
            out.update(q=q.astype(np.float64), logL=float(ll), n=n, converged=conv)
            return out
        s = q * (pc / t).sum(axis=1)
        temp = s.sum()
        if temp == 0:
            q = np.full(K, 1.0 / K).astype(dtype)
        else:
            q = s / temp
            if do_projection:
                q = michelot(q, lb)
        prev = ll
        n += 1


def fit_rows(ua, geno, p, rows, max_iter, q0=None, **kw):
    """fit_row for every listed individual: (q [n][K], logL [n], iter [n], converged [n], list of the per-row dicts)"""
    res = [fit_row(ua, geno[i], p, None if q0 is None else q0[i], max_iter, **kw) for i in rows]
    return (np.array([r["q"] for r in res]), np.array([r["logL"] for r in res]), np.array([r["n"] for r in res], dtype=np.int32),
            np.array([r["converged"] for r in res], dtype=np.uint8), res)


def q_tolerance(copies, K):
    """4 (n_i + K + 8) 2^-52 absolute per entry: S_k and sum_k S_k are sums of n_i (and K) positive terms, each term a few
    roundings (the reciprocal, the product, the fma chain of t behind it), so each is within (n_i + K + 8) 2^-52 relative of the
    exact value whatever the order of summation; the quotient of two such results from two orders differs by at most four times
    that relative, q <= 1 makes it absolute, and the projection onto the simplex does not expand differences."""
    return 4.0 * (np.asarray(copies, dtype=np.float64) + K + 8) * EPS


# ---- the inputs: (name, K, L, ploidy, kind, special); I = 13 everywhere (not a multiple of the 8-individual groups of gtA).
# K covers 1, 2, 3 and both sides of the kernel's K buckets (8 | 9, 16 | 17, 32 | 33, 64); L has fewer loci than a workgroup has
# lanes (1, 7, 9, 255), one more than that (257) and several walks (1000); the kernel's loop over k sits inside its loop over the
# loci and neither knows of the other, so the small L go with the small K.  special: individual 0 has no observed copy and
# individual 1 a single one.
# Why not every L with every K, and the special rows only up to K = 3: a row with far fewer copies than clusters is an
# underdetermined problem.  Its likelihood is flat along whole directions, rounding differences along them are not contracted by
# the update and add up linearly with the number of updates, while the tolerance is a bound for one update.  Measured on the
# float64 restatement against long double, as a fraction of 1 / 16 of q_tolerance: a single-copy row at K = 8, 17, 32, 33, 64
# gave 0.47, 0.04, 0.24, 0.14, 0.38 after 20 updates and 1.41, 1.77, 2.88, 1.90, 1.48 after 100 (at K <= 3 it runs into a vertex
# within a few updates and stays under 0.2); an 18-copy row at K = 33 gave 0.07 and 1.32; every row of the cases below stays
# under 0.25 through 100 updates (tests/test_query_cpu.py prints the figures).
I_ROWS = 13
CASES = [
    ("k1", 1, 7, 2, "plain", True), ("k2", 2, 1, 1, "plain", True), ("k3", 3, 9, 4, "plain", True),
    ("k8", 8, 255, 2, "plain", False), ("k9", 9, 257, 2, "plain", False), ("k16", 16, 1000, 1, "plain", False),
    ("k17", 17, 255, 4, "plain", False), ("k32", 32, 257, 2, "plain", False), ("k33", 33, 1000, 1, "plain", False),
    ("k64", 64, 1000, 2, "plain", False), ("many3", 3, 1000, 2, "many", True), ("many8", 8, 64, 4, "many", False),
]
CASE_NAMES = [c[0] for c in CASES]
LOWER_BOUND = 1e-8


@functools.lru_cache(maxsize=None)
def case(name):
    """(ua, geno [13][L][ploidy], q [13][K], p [K][T]) of a case: drawn parameters, not a fit"""
    _, K, L, pl, kind, special = CASES[CASE_NAMES.index(name)]
    seed = 1000 + CASE_NAMES.index(name)
    if kind == "many":     # a 35-allele locus, up to 4 alleles elsewhere, 3 % missing
        ua, geno = cv_dataset(I_ROWS, L, pl, seed, missing=0.03)
    else:
        ua, geno = make_dataset(I_ROWS, L, K, ploidy=pl, max_alleles=4 if L > 1 else 2, seed=seed)
    geno = geno.copy()
    real = ua - ((geno == MISSING).any(axis=(0, 2)) if kind == "many" else 0)      # (cv_dataset has added the phantom slots)
    if special:
        geno[0] = MISSING
        keep = geno[1, 0, 0] if geno[1, 0, 0] != MISSING else 0
        geno[1] = MISSING
        geno[1, 0, 0] = keep
    # the phantom allele slot the reader gives every locus that has a missing copy
    ua = (real + (geno == MISSING).any(axis=(0, 2))).astype(np.int32)
    q, p = random_params(I_ROWS, ua, K, seed=seed + 500, lower_bound=LOWER_BOUND)
    for a in (ua, geno, q, p):
        a.setflags(write=False)
    return ua, geno, q, p


def copies_per_row(geno):
    return (geno != MISSING).sum(axis=(1, 2))


# ---- the inputs of the stopping tests.  The iteration at which a row stops is compared exactly, so the deciding |l_n - l_(n-1)|
# of the stopping evaluation and of the one before it must stand clear of the threshold: by more than one part in 10^3, in the
# float64 restatement, for every row (stop_margin; asserted by the tests).  Successive differences of a row shrink by the row's
# rate of convergence, so the last one above the threshold and the first one below it lie within that factor of each other: only
# rows that converge faster than 0.999 per iteration can keep the margin on both sides.  Drawn parameters with a data set drawn
# from another model (CASES) take thousands of iterations from K = 8 on; here the genotypes are drawn from the very P the fit holds
# fixed, with mixing proportions Dirichlet(alpha) -- interior (alpha = 20) where K is large, so that no component creeps towards
# zero -- and the seeds are those for which the margin holds (searched on the CPU).
def model_dataset(I, L, K, ploidy, seed, alpha):
    """(ua, geno, p): up to 4 alleles per locus, p drawn, every copy drawn from sum_k q_ik p_k with q_i ~ Dirichlet(alpha)"""
    rng = np.random.default_rng(seed)
    ua = rng.integers(2, 5, size=L).astype(np.int32)
    _, p = random_params(I, ua, K, seed=seed + 1, lower_bound=LOWER_BOUND)
    toff = np.concatenate(([0], np.cumsum(ua)))
    qt = rng.dirichlet(np.full(K, alpha), size=I)
    geno = np.empty((I, L, ploidy), np.uint8)
    for i in range(I):
        z = rng.choice(K, size=(L, ploidy), p=qt[i])
        u = rng.random((L, ploidy))
        for l in range(L):
            for a in range(ploidy):
                c = np.cumsum(p[z[l, a], toff[l]:toff[l + 1]])
                geno[i, l, a] = min(int((u[l, a] * c[-1] > c).sum()), ua[l] - 1)
    return ua, geno, p


STOP_CASES = {          # name: (K, L, ploidy, seed, alpha), or a case of CASES
    "s2": (2, 257, 2, 1, 0.3), "s3": (3, 255, 4, 1, 0.3), "s8": (8, 1000, 4, 2, 20.0), "k2": "k2", "many3": "many3",
}
STOP_RULES = {"abs": dict(abs_error=1e-6), "rel": dict(rel_error=1e-9)}
STOP_MAX_ITER = 3000


@functools.lru_cache(maxsize=None)
def stop_case(name):
    spec = STOP_CASES[name]
    if isinstance(spec, str):
        ua, geno, _, p = case(spec)
        return ua, geno, p
    K, L, pl, seed, alpha = spec
    ua, geno, p = model_dataset(I_ROWS, L, K, pl, seed, alpha)
    for a in (ua, geno, p):
        a.setflags(write=False)
    return ua, geno, p


@functools.lru_cache(maxsize=None)
def stop_reference(name, rule):
    """the float64 restatement of a stopping case under a rule: what fit_rows returns"""
    ua, geno, p = stop_case(name)
    return fit_rows(ua, geno, p, range(I_ROWS), STOP_MAX_ITER, lb=LOWER_BOUND, **STOP_RULES[rule])


def stop_margin(res, abs_error=0.0, rel_error=0.0):
    """the smallest relative distance from its threshold of a deciding difference: the last two evaluations of every row"""
    worst = np.inf
    for r in res:
        for d, prev in list(zip(r["deltas"], r["prevs"]))[-2:]:
            if abs_error:
                worst = min(worst, abs(d / abs_error - 1))
            if rel_error:
                worst = min(worst, abs(d / abs(prev) / rel_error - 1))
    return worst
