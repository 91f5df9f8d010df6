"""Worst-case inputs for the mixture model's passes, a long-double reference of one mixture EM step and of the log
likelihood, and error bounds that are functions of the case.

The mixture kernels (k_logp, k_mix_gather<PL,STAGED>, k_mix_finalize modes 0 and 1, k_mix_column<PL>, the MIX instance of
k_column_counts, the add_lb branch of k_finalize_p / k_finalize_p_tile) are compared elsewhere against the oracle at
rtol = 1e-7 on Dirichlet(1) parameters.  Here they are compared against `reference` (numpy.longdouble; it shares no code with
oracle/, only the projection, applied to the rounded result as worstcase.reference_step does) within `bounds`.

THE STEP (em_alg.c:763-1011, kernels_k/mixture.h "mixture model", mchip_em.hip run_mixture).  n_ic = copies of allele column c
individual i carries (missing copies are skipped), eta = shared mixing proportions, p = (K, T):
    v_ik  = log eta_k + sum_c n_ic log p_kc          (a cell with p == 0 adds 0 in the E step, -inf in the log likelihood: k_logp)
    vik   = exp(v_ik - max_k v_ik) / sum_k exp(v_ik - max_k v_ik),      ll = sum_i ll_i,  ll_i = log sum_k exp(v_ik)
    eta'  = project(sum_i vik / sum_ik vik),         p'_kc = project(N_kc / sum_{c' of the locus} N_kc'),  N_kc = lb + sum_i vik n_ic
mchip_e_step / mchip_em_step return ll in e_step_mixture's form (mode 0: log sum_k exp(v - max) + max); mchip_loglik and
mchip_loglik_prefetch in logL_mixture's (mode 1: log sum_k exp(v_k - scale) + scale, scale != 0 only once exp(max) is exactly 0
or inf).  Both are the same number in exact arithmetic, which is what `reference` returns.

THE BOUNDS.  eps = 2^-52, n_i = observed copies of individual i, A_ik = |log eta_k| + sum_copies |log p_kc| (long double).
  * v.  Each log is good to 1 ulp (|log p| eps per term, A_ik eps in all) and a sum of m terms in any order is off by at most
    (m - 1) eps sum |terms|; the device adds n_i + 1 terms in n_lchunks partial sums.  delta_i = (n_i + n_lchunks + 16) eps
    max_k A_ik bounds |v_dev - v_exact| for every k, with 15 roundings of the size of |v| to spare (mode 1's scale).
  * vik = 1 / sum_j exp(v_ij - v_ik): a shift of all v cancels, each exponent is off by at most 2 delta_i, so the relative
    error from v is 2 delta_i.  The arithmetic adds: the exp argument x = v_ik - max is rounded (|x| eps relative in exp), exp
    itself, K additions, one division.  rho_ik = 2 delta_i + (K + 8 + |v_ik - max_k v_ik|) eps, relative; entries whose exact
    value is below 2^-1022 (subnormal or 0) get an absolute 2^-1022 on top (exp's result there has fewer bits or none).
  * ll, mode 0.  ll_i = log(sum) + max with sum in [1, K]: delta_i from v, (K + 8) eps (1 + |ll_i|) for the arithmetic; summing I
    terms in any order adds (I + 8) eps sum |ll_i|.  tol = sum_i [delta_i + (K + 8) eps (1 + |ll_i|)] + (I + 8) eps sum_i |ll_i|.
  * ll, mode 1: the same (the exp arguments are at most 745 + the gap in size, and |ll_i| >= 708 wherever they are that
    large, so (K + 8) eps |ll_i| covers them), plus 2 kappa_i per individual where exp(max) is a non-zero double:
    kappa_i = (K + 1) 2^-1074 / sum_k exp(v_ik).  The reference rescales only once exp(max) is exactly 0, so between -745.13
    and -708.4 it adds subnormals, each a multiple of 2^-1074: the sum is off by up to K 2^-1074, relatively kappa_i, and
    |log(1 +- kappa)| <= 2 kappa for kappa <= 1/2 (no bound above that: inf).  The project keeps the reference's form there
    (documented departures), so the term belongs to the bound and not to the code.
  * eta' and p'.  A numerator is a sum of non-negative terms, so its absolute error is at most sum_i tol(vik) n_ic (the
    vik-weighted mean of rho, relatively) plus (I + 8) eps of itself for the additions in any order (lb is exact).  A quotient
    a_c / s, s = sum of the block's numerators, is off relatively by r_c + r_s + (M + 8) eps, r_s = sum_c |error a_c| / s being a
    weighted mean of the block's r_c: at most twice the block's largest r_c ("the quotient doubles it").  The projection is the
    Euclidean projection onto a convex set and so non-expansive in the 2-norm: every entry of a projected block is within the
    2-norm of the block's unprojected tolerances.  The projection's own arithmetic (the reference's and the device's, in
    double) adds (M + 2) eps per pass per side -- a sum of M entries that total 1, one division, one subtraction -- and a pass
    that is not the last fixes at least one entry at the bound, so passes <= 1 + entries on the bound: 2 (M + 2) eps passes.

THE REGIMES (`build`).  Each gives (ua, geno, eta0, P0, lb) for a case (K, I, L, ploidy, allele spec, missing):
  ordinary  Dirichlet(1) blocks floored at the bound, drawn genotypes: the suite's usual inputs under the tightened tolerance.
  fixed     every (l, k) block has one allele at 1 - (M - 1) lb and the rest at lb; the same allele for every k except at loci
            l = 5 mod 8; individuals carry mostly that allele.  A_ik is small, so are the bounds: a dropped or double-counted
            copy (1e-8 in v, the same for every k: only ll shows it) and a lost add_lb are far outside them.
  tied      all K rows of P identical, eta uniform: vik is 1 / K exactly and the K rows of P' are bitwise equal (every k runs
            the same chain of operations): any k-indexing, LDS-stride or staging mix-up breaks that.
  dominant  lb = 1e-120; cluster k's allele at locus l is bit (l mod 6) of k, p = 1 - (M - 1) lb there and lb elsewhere, and
            individual i carries the alleles of cluster i mod K (the last individual those of cluster K - 1): two clusters
            differ in at least one bit, at least three loci, 276 nats per copy, so the gap is far beyond 745 nats and vik is
            exactly 0 or 1; every k dominates someone where I >= K, the first and the last always.
  deep      lb = 1e-120 (the tinybound fixture's bound); allele 0 of every locus is on the bound for every k and is what
            individuals mostly carry, so |v| is 1e4 to 1e5 (several halvings in mode 1); individuals i = 4 mod 9 carry it
            everywhere except at loci 1 and 2, where clusters 0 and K - 1 each own an allele and every other cluster is
            722 to 725 nats behind: exp(v - max) is subnormal.
  window    (`build_window`) biallelic loci whose P is the same for every k: 16 fine copies (a = 0.45, steps of 0.2 nats)
            and the rest coarse (a = 0.05, steps of 2.9 nats) put each individual's max v on a target: 13 in the subnormal
            window [-725, -709.5] (kappa <= 2^-20), 13 on the overflow edge (max v = -2 h, h in [709.2, 709.65]: one halving
            leaves the shifted maximum within ln 2 of log DBL_MAX), 13 rescaled and far from it, 13 just below the point where
            exp(max) becomes 0, 13 above -708.  Three signature loci split the individuals into those for whom all K clusters
            tie (S = K) and those for whom clusters 0 and 1 tie and the rest are 110 nats and more behind (S = 2)."""
import math

import numpy as np

import oracle_bind as ob                    # the projection only
import worstcase as wc
from synth import make_dataset
from test_gpu_kernel_matrix import GEOM, count_bits, geometry, small_shape, sparse_edge

LD = np.longdouble
MISSING = 0xFF
EPS = 2.0 ** -52
TINY = 2.0 ** -1022
LOG_DBL_MAX = math.log(1.7976931348623157e308)          # 709.782712893384
LOG_HALF_DENORM = -1075.0 * math.log(2.0)               # exp(x) rounds to 0 below it: -745.1332191019412
DEEP_BOUND = 1e-120
REGIMES = ("ordinary", "fixed", "tied", "dominant", "deep")
FAMILIES = ("mix_2bit", "mix_4bit", "mix_p3", "mix_nocounts_p2", "mix_dense", "mix_geom")
WINDOW_FAMILIES = ("mix_2bit", "mix_4bit")
K_ALL = tuple(range(1, 65))
# whose entry of the kernel matrix's shape table a family takes (small_shape indexes that module's family list)
SHAPE_OF = {"mix_2bit": "mix_2bit", "mix_4bit": "mix_4bit", "mix_p3": "mix_dense_p3", "mix_nocounts_p2": "mix_nocounts_p2",
            "mix_dense": "mix_dense"}
GAP_EVERY, GAP_LOCI, GAP_NATS = 9, (1, 2), 722.0
WINDOW_I, WINDOW_SIG, WINDOW_FINE_COPIES, A_COARSE, A_FINE = 65, 3, 16, 0.05, 0.45


def lower_bound(lb, I, ploidy):
    """multiclust.c:812-813"""
    return min(lb, 1.0 / I / ploidy - 0.5 / I / ploidy)


# ------------------------------------------------------------------------------------------------------------------- the cases
def make_case(fam, K):
    """mix_geom: with packed counts an individual chunk is 64 wide, so more than eight column slabs on 129 individuals need
    MCHIP_NO_COUNTS; it is also the family of k_mix_gather<0,false>, k_mix_column<0> and, through one locus of 65 alleles or
    more, of k_finalize_p at the K whose sparse edge still fits the tiled form."""
    c = dict(family=fam, K=K, ploidy=2, spec=(2, 4), missing=0.0, knobs={}, wide=None, model="mix", projection=1,
             seed=5000 * K + FAMILIES.index(fam))
    if fam == "mix_geom":
        c.update(I=129, L=45, ploidy=3, knobs=dict(GEOM, MCHIP_NO_COUNTS="1"), wide=65 + K % 8)
    else:
        c["I"], c["L"] = small_shape(K, SHAPE_OF[fam])
    if fam == "mix_2bit":
        c["missing"] = 0.03
    if fam == "mix_4bit":
        c["ploidy"] = 4
    if fam == "mix_p3":
        c["ploidy"] = 3
    if fam == "mix_nocounts_p2":
        c["knobs"] = {"MCHIP_NO_COUNTS": "1"}
    if fam == "mix_dense":
        c["spec"] = (2, sparse_edge(K) + 1)
    return c


def window_case(fam, K):
    pl = 4 if fam == "mix_4bit" else 2
    return dict(family=fam, K=K, ploidy=pl, I=WINDOW_I, L=520 // pl, spec=(2, 2), missing=0.03 if fam == "mix_2bit" else 0.0,
                knobs={}, wide=None, model="mix", projection=1, seed=9000 * K + FAMILIES.index(fam))


def all_cases():
    return [make_case(fam, K) for K in K_ALL for fam in FAMILIES]


def window_cases():
    return [window_case(fam, K) for K in wc.K_VALUES for fam in WINDOW_FAMILIES]


def case_id(c):
    return "%s-K%d-%dx%dx%d" % (c["family"], c["K"], c["I"], c["L"], c["ploidy"])


def case_ua(c, regime="ordinary"):
    rs = np.random.default_rng(c["seed"] + 7)
    lo, hi = c["spec"]
    ua = rs.integers(lo, hi + 1, size=c["L"]).astype(np.int32)
    ua[0], ua[c["L"] // 2] = lo, hi
    if c["wide"]:
        ua[c["L"] // 3] = c["wide"]
    if regime == "deep":
        ua[list(GAP_LOCI)] = 3
    return ua


def n_lchunks(c, ua):
    return geometry(c["K"], c["I"], c["L"], int(ua.sum()), c["ploidy"], int(ua.max()), False, count_bits(c["ploidy"], c["knobs"]),
                    c["knobs"])["n_lchunks"]


def offsets(ua):
    return np.concatenate(([0], np.cumsum(ua))).astype(np.int64)


def regime_bound(c, regime):
    return DEEP_BOUND if regime in ("dominant", "deep") else lower_bound(1e-8, c["I"], c["ploidy"])


def drawn_genotypes(c, ua, rs):
    I, L, pl = c["I"], c["L"], c["ploidy"]
    _, geno = make_dataset(I, L, max(c["K"], 2), ploidy=pl, max_alleles=2, seed=c["seed"])
    for l in np.nonzero(ua != 2)[0]:
        geno[:, l, :] = rs.integers(0, ua[l], size=(I, pl)).astype(np.uint8)
    return geno


def dirichlet_blocks(ua, rows, rs, lb):
    p = np.empty((rows, int(ua.sum())))
    off = 0
    for M in ua:
        p[:, off:off + M] = rs.dirichlet(np.ones(M), size=rows)
        off += M
    return np.maximum(p, lb)


def random_eta(K, rs, lb):
    return wc.bounded_simplex(rs.dirichlet(np.ones(K)), lb)


def dominant_cluster(i, I, K):
    return K - 1 if i == I - 1 else i % K


def is_gap_individual(i):
    return i % GAP_EVERY == 4


def build(c, regime):
    """(ua, geno, eta0, P0, lb) of one regime of a case"""
    K, I, L, pl = c["K"], c["I"], c["L"], c["ploidy"]
    rs = np.random.default_rng(c["seed"] + 31 * (REGIMES.index(regime) + 1))
    ua = case_ua(c, regime)
    toff = offsets(ua)
    lb = regime_bound(c, regime)
    keep = np.zeros((I, L), dtype=bool)            # genotypes no missing copy may touch
    if regime == "ordinary":
        geno = drawn_genotypes(c, ua, rs)
        p, eta = dirichlet_blocks(ua, K, rs, lb), random_eta(K, rs, lb)
    elif regime == "tied":
        geno = drawn_genotypes(c, ua, rs)
        p, eta = np.repeat(dirichlet_blocks(ua, 1, rs, lb), K, axis=0), np.full(K, 1.0 / K)
    elif regime == "fixed":
        p = np.full((K, int(ua.sum())), lb)
        geno = np.empty((I, L, pl), dtype=np.uint8)
        for l in range(L):
            M = int(ua[l])
            own = l % 8 == 5                        # the clusters disagree here
            fav = (np.arange(K) + l) % M if own else np.full(K, l % M)
            p[np.arange(K), toff[l] + fav] = 1.0 - (M - 1) * lb
            carried = fav[np.arange(I) % K]
            other = rs.random((I, pl)) < (0.1 if own else 0.03)
            geno[:, l, :] = np.where(other, rs.integers(0, M, size=(I, pl)), carried[:, None])
        eta = random_eta(K, rs, lb)
    elif regime == "dominant":
        p = np.full((K, int(ua.sum())), lb)
        geno = np.empty((I, L, pl), dtype=np.uint8)
        ks = np.arange(K)
        who = np.array([dominant_cluster(i, I, K) for i in range(I)])
        for l in range(L):
            bit = (ks >> (l % 6)) & 1
            p[ks, toff[l] + bit] = 1.0 - (int(ua[l]) - 1) * lb
            geno[:, l, :] = bit[who][:, None]
        for i in range(3, I, 5):                    # one copy of the other allele: the winner's v is -276, not 0
            geno[i, (7 * i) % L, 0] ^= 1
        eta = random_eta(K, rs, lb)
    elif regime == "deep":
        p = np.empty((K, int(ua.sum())))
        geno = np.empty((I, L, pl), dtype=np.uint8)
        for l in range(L):
            M = int(ua[l])
            blockp = np.concatenate((np.zeros((K, 1)), rs.dirichlet(np.ones(M - 1), size=K)), axis=1)
            p[:, toff[l]:toff[l] + M] = wc.bounded_simplex(blockp, lb)
            rare = rs.random((I, pl)) < 0.2
            geno[:, l, :] = np.where(rare, rs.integers(1, M, size=(I, pl)), 0)
        d = GAP_NATS / (len(GAP_LOCI) * pl)         # nats per copy between the owner of a gap allele and the runners-up
        h = math.exp(-d)
        assert h > lb
        for l in GAP_LOCI:
            for k in range(K):
                hk = h * math.exp(-0.3 * k / K)
                p[k, toff[l]:toff[l] + 3] = (hk, hk, 1.0 - 2.0 * hk)
            p[K - 1, toff[l]:toff[l] + 3] = (h, 1.0 - 2.0 * h, h)
            p[0, toff[l]:toff[l] + 3] = (1.0 - 2.0 * h, h, h)
            geno[:, l, :] = rs.integers(0, 3, size=(I, pl))
        for i in range(I):
            if is_gap_individual(i):
                geno[i] = 0
                geno[i, list(GAP_LOCI), :] = (i // GAP_EVERY) % 2 if K > 1 else 0
                keep[i] = True
        eta = random_eta(K, rs, lb)
    else:
        raise ValueError(regime)
    if c["missing"]:
        hit = (rs.random(geno.shape) < c["missing"]) & ~keep[:, :, None]
        geno[hit] = MISSING
    return ua, np.ascontiguousarray(geno.astype(np.uint8)), np.ascontiguousarray(eta), np.ascontiguousarray(p), lb


def window_targets(c):
    """(target of max v, whether clusters 0 and 1 alone tie) per individual; group = i mod 5, place in the group = i // 5"""
    t, pair = np.empty(c["I"]), np.zeros(c["I"], dtype=bool)
    for i in range(c["I"]):
        g, j = i % 5, i // 5
        t[i] = (-725.0 + j * 15.5 / 12, -2.0 * (709.2 + 0.45 * j / 12), -760.0 - 50.0 * j, -745.8 - 0.5 * j, -708.0 + 9.0 * j)[g]
        pair[i] = j % 2 == 1 and c["K"] >= 3
    return t, pair


def build_window(c):
    """(ua, geno, eta0, P0, lb): loci 0-2 signature, then 16 / ploidy fine tuning loci, the rest coarse ones"""
    K, I, L, pl = c["K"], c["I"], c["L"], c["ploidy"]
    rs = np.random.default_rng(c["seed"])
    lb = lower_bound(1e-8, I, pl)
    ua = np.full(L, 2, dtype=np.int32)
    n_fine = WINDOW_FINE_COPIES // pl
    fine, coarse = np.arange(WINDOW_SIG, WINDOW_SIG + n_fine), np.arange(WINDOW_SIG + n_fine, L)
    p = np.empty((K, L, 2))
    p[:, :WINDOW_SIG, 0] = np.where(np.arange(K) < 2, 1.0 - lb, lb)[:, None]
    p[:, fine, 0], p[:, coarse, 0] = A_FINE, A_COARSE
    p[:, :, 1] = 1.0 - p[:, :, 0]
    p[:, :WINDOW_SIG, 1] = np.where(np.arange(K) < 2, lb, 1.0 - lb)[:, None]      # the same two numbers, swapped: exact ties
    eta = np.full(K, 1.0 / K)
    target, pair = window_targets(c)
    geno = np.ones((I, L, pl), dtype=np.uint8)
    miss = rs.random(geno.shape) < c["missing"]
    miss[:, :WINDOW_SIG + n_fine, :] = False           # all 16 fine copies: 3.2 nats of them bridge a coarse step of 2.94
    steps = (math.log(A_COARSE), math.log(1.0 - A_COARSE), math.log(A_FINE), math.log(1.0 - A_FINE))
    for i in range(I):
        if pair[i]:
            geno[i, :WINDOW_SIG, :] = 0                                     # clusters 0 and 1 own it, the others are at lb
            base = WINDOW_SIG * pl * math.log(1.0 - lb)
        else:
            geno[i, :WINDOW_SIG, :pl // 2] = 0                              # half and half: the same product for every cluster
            base = WINDOW_SIG * (pl // 2) * (math.log(1.0 - lb) + math.log(lb))
        base -= math.log(K)
        slots_c = [(l, b) for l in coarse for b in range(pl) if not miss[i, l, b]]
        slots_f = [(l, b) for l in fine for b in range(pl) if not miss[i, l, b]]
        nc, nf = np.arange(len(slots_c) + 1)[:, None], np.arange(len(slots_f) + 1)[None, :]
        v = base + nc * steps[0] + (len(slots_c) - nc) * steps[1] + nf * steps[2] + (len(slots_f) - nf) * steps[3]
        best_c, best_f = np.unravel_index(np.abs(v - target[i]).argmin(), v.shape)
        assert abs(v[best_c, best_f] - target[i]) < 0.11, (i, v[best_c, best_f], target[i])
        for l, b in slots_c[:best_c] + slots_f[:best_f]:
            geno[i, l, b] = 0
    geno[miss] = MISSING
    return ua, geno, eta, np.ascontiguousarray(p.reshape(K, 2 * L)), lb


# ------------------------------------------------------------------------------------------------------------- the reference
def reference(ua, geno, eta, p, lb):
    """One mixture EM step and the log likelihood in numpy.longdouble.  Returns a dict: v (I, K) as the E step has it, ll_i and
    ll as the log likelihood has it (p == 0 cells), vik, the numerators and unprojected quotients of the M step, eta1 and p1
    (rounded to double and projected), A (I, K), n (I, T)."""
    assert np.finfo(LD).eps < 2.0 ** -60, "this platform's long double is no wider than double"
    K = p.shape[0]
    n = wc.counts(ua, geno)
    nl = n.astype(LD)
    P, le = np.asarray(p).astype(LD), np.log(np.asarray(eta).astype(LD))
    zero = P == 0
    with np.errstate(divide="ignore"):
        lp = np.log(P)
    lpe = np.where(zero, LD(0), lp)
    v = le[None, :] + nl @ lpe.T
    A = np.abs(le)[None, :] + nl @ np.abs(lpe).T
    vl = v if not zero.any() else v + np.where((n[:, None, :] > 0) & zero[None, :, :], -np.inf, 0.0).sum(axis=2)
    mx = v.max(axis=1)
    w = np.exp(v - mx[:, None])
    vik = w / w.sum(axis=1, keepdims=True)
    mxl = vl.max(axis=1)
    safe = np.where(np.isfinite(mxl), mxl, LD(0))
    with np.errstate(divide="ignore"):
        ll_i = np.log(np.exp(vl - safe[:, None]).sum(axis=1)) + safe
    eta_num = vik.sum(axis=0)
    eta_u = eta_num / eta_num.sum()
    eta1 = ob.michelot(eta_u.astype(np.float64), lb)
    num = LD(lb) + vik.T @ nl
    p_u = np.empty(num.shape, dtype=LD)
    p1 = np.empty(num.shape, dtype=np.float64)
    toff = offsets(ua)
    for l in range(len(ua)):
        blk = slice(toff[l], toff[l + 1])
        p_u[:, blk] = num[:, blk] / num[:, blk].sum(axis=1, keepdims=True)
        for k in range(K):
            p1[k, blk] = ob.michelot(p_u[k, blk].astype(np.float64), lb)
    return dict(v=v, vl=vl, mx=mx, vik=vik, ll_i=ll_i, ll=ll_i.sum(), eta_num=eta_num, eta_u=eta_u, eta1=eta1, num=num, p_u=p_u,
                p1=p1, A=A, n=n, lb=lb)


def bounds(ref, ua, lchunks=1):
    """tolerances of a case (module docstring): vik (I, K) absolute, ll0 and ll1 absolute, eta (K,) and p (K, T) absolute,
    kappa (I,)"""
    v, mx, vik, n = ref["v"], ref["mx"], ref["vik"], ref["n"]
    I, K = v.shape
    nl = n.astype(LD)
    n_i = nl.sum(axis=1)
    delta = (n_i + lchunks + 16) * EPS * ref["A"].max(axis=1)
    rho = 2 * delta[:, None] + (K + 8 + np.abs(v - mx[:, None])) * EPS
    t_vik = rho * vik + np.where(vik < TINY, LD(TINY), LD(0))
    absll = np.abs(ref["ll_i"])
    ll0 = (delta + (K + 8) * EPS * (1 + absll)).sum() + (I + 8) * EPS * absll.sum()
    mxl = ref["vl"].max(axis=1)
    sumexp = np.exp(ref["vl"]).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        kappa = np.where(mxl > LOG_HALF_DENORM, (K + 1) * LD(2.0) ** -1074 / sumexp, LD(0))
    ll1 = ll0 + np.where(kappa > 0.5, LD(np.inf), 2 * kappa).sum()

    def projected(a, ta, u, p1):
        """absolute tolerance of projected blocks, one per row: numerators, their tolerances, unprojected quotients, the
        projected blocks"""
        M = a.shape[1]
        t_u = u * (ta / a + ta.sum(axis=1, keepdims=True) / a.sum(axis=1, keepdims=True) + (M + 8) * EPS)
        passes = 1 + (p1 == ref["lb"]).sum(axis=1)
        return (np.sqrt((t_u * t_u).sum(axis=1)) + 2 * (M + 2) * EPS * passes).astype(np.float64)

    t_eta_num = t_vik.sum(axis=0) + (I + 8) * EPS * ref["eta_num"]
    t_eta = np.full(K, projected(ref["eta_num"][None, :], t_eta_num[None, :], ref["eta_u"][None, :], ref["eta1"][None, :])[0])
    t_num = t_vik.T @ nl + (I + 8) * EPS * ref["num"]
    t_p = np.empty(ref["p1"].shape)
    toff = offsets(ua)
    for l in range(len(ua)):
        blk = slice(toff[l], toff[l + 1])
        t_p[:, blk] = projected(ref["num"][:, blk], t_num[:, blk], ref["p_u"][:, blk], ref["p1"][:, blk])[:, None]
    return dict(vik=t_vik, ll0=float(ll0), ll1=float(ll1), eta=t_eta, p=t_p, kappa=kappa, delta=delta)


def ratio(got, want, tol):
    """largest |difference| / tolerance; a non-finite entry where the reference is finite counts as inf"""
    got, want, tol = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD), np.asarray(tol, dtype=LD)
    bad = ~np.isfinite(got) & np.isfinite(want)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(bad, np.inf, np.abs(got - want) / tol)
    r = np.where(np.isnan(r), np.inf, r)
    return float(np.max(r))


def step_ratios(ref, tol, ll, vik, eta1, p1):
    """(ll, vik, eta, P) of a mode 0 step against the reference"""
    return (ratio(ll, ref["ll"], tol["ll0"]), ratio(vik, ref["vik"], tol["vik"]), ratio(eta1, ref["eta1"], tol["eta"]),
            ratio(p1, ref["p1"], tol["p"]))


# --------------------------------------------------------------------------------------------------- where the inputs are
def exactly_one_hot(ref):
    """individuals whose runner-up is more than 746 nats behind: vik has to be exactly 0 or 1 (rows, winning k)"""
    v = ref["v"]
    win = v.argmax(axis=1)
    rest = np.where(np.arange(v.shape[1])[None, :] == win[:, None], -np.inf, v)
    gap = ref["mx"] - (rest.max(axis=1) if v.shape[1] > 1 else np.full(v.shape[0], -np.inf))
    return np.nonzero(gap > 746.0)[0], win


def runner_up_gap(ref):
    v = np.sort(ref["v"], axis=1)
    return (v[:, -1] - v[:, -2]).astype(np.float64) if v.shape[1] > 1 else np.full(v.shape[0], np.inf)


def overflow_edge(ref):
    """(mask, S): individuals for whom logL_mixture's rescaled sum overflows -- exp(max) is 0, -max halved until exp() is
    finite leaves h, and S exp(h) > DBL_MAX with S = sum_k exp(v_k - max) -- in long double"""
    mx = ref["vl"].max(axis=1)
    S = np.exp(ref["vl"] - mx[:, None]).sum(axis=1)
    edge = np.zeros(len(mx), dtype=bool)
    for i, m in enumerate(mx):
        if not m < LOG_HALF_DENORM:
            continue
        h = -m * LD(0.5)
        while h > LOG_DBL_MAX:
            h = h * LD(0.5)
        edge[i] = h + np.log(S[i]) > LOG_DBL_MAX
    return edge, S.astype(np.float64)


def subnormal_window(ref):
    """individuals whose exp(max v) is a subnormal double and not 0"""
    mx = ref["vl"].max(axis=1)
    return (mx > LOG_HALF_DENORM) & (mx < math.log(TINY))
