"""Divergence of the fitted clusters on the CPU (TEST INFRASTRUCTURE): the long-double reference of every quantity that
include/multiclust_hip.h defines for mchip_divergence, the parameter sets the tests use, float64 restatements (and deliberate
mutants) of the sums, and the checker that holds a set of sums to the bounds.

The bounds (u = 2^-53).  A sum of n non-negative terms, each a product or square formed with at most three roundings, added in any
order, is within ((n - 1) + 3) u (1 + O(n u)) <= (n + 8) u of its exact value, relatively:
    h_a, s_ab      n = T columns;
    HT_l           n = M_l, given pbar_lm -- which the definition fixes as the fma chain's double, so it carries no error;
    V_l            n = K M_l, given the same pbar;     sum_l HT_l: n = T;     sum_l V_l: n = K T.
Against V_l of the EXACT weighted mean pbar* the chain's pbar = pbar* + delta, |delta| <= e pbar*, e = K u / (1 - K u), adds
    V(pbar) - V(pbar*) = sum_m [ -2 delta_m sum_k w_k (p_klm - pbar*_lm) + delta_m^2 W ],  W = sum_k w_k,
in size at most  2 e A_l + e^2 W sum_m pbar*_lm^2  with  A_l = sum_m sum_k w_k |p_klm - pbar*_lm|: the absolute part of V_l's bound.

When run as a program it prints the bits of one fixed case: tests/test_gpu_divergence.py starts it as a fresh process under
different launch-geometry knobs."""
import sys
from fractions import Fraction

import numpy as np

from synth import random_params

LD = np.longdouble
U = 2.0 ** -53


def offsets(ua):
    return np.concatenate(([0], np.cumsum(np.asarray(ua, dtype=np.int64))))


def rel_bound(n):
    return (n + 8) * U


def fma_chain(w, P):
    """pbar [T] as the definition has it: acc = fma(w_k, p_k, acc) in k order from 0, every step rounded once (exact rationals,
    rounded to nearest even by float())"""
    K, T = P.shape
    acc = [Fraction(0)] * T
    for k in range(K):
        wk = Fraction(float(w[k]))
        acc = [Fraction(float(wk * Fraction(float(x)) + a)) for x, a in zip(P[k], acc)]
    return np.array([float(a) for a in acc], dtype=np.float64).reshape(T)


def reference(ua, P, w, exact_pbar=False):
    """every quantity of the definitions from ua [L], P [K][T] and w [K], in long double.  pbar is the fma chain's double (the
    definition), or with exact_pbar the weighted mean itself in long double."""
    ua = np.asarray(ua, dtype=np.int64)
    P = np.asarray(P, dtype=np.float64)
    K, T = P.shape
    L, off = len(ua), offsets(ua)
    assert off[-1] == T
    Pl, wl = P.astype(LD), np.asarray(w, dtype=np.float64).astype(LD)
    L1 = int((ua > 0).sum())
    h = (Pl * (1 - Pl)).sum(axis=1)
    s = np.zeros((K, K), dtype=LD)
    for a in range(K):
        d = Pl[a][None, :] - Pl
        s[a] = (d * d).sum(axis=1)
        s[a, a] = 0
    pbar = (wl[:, None] * Pl).sum(axis=0) if exact_pbar else fma_chain(w, P).astype(LD)
    ht_c = pbar * (1 - pbar)
    dev = Pl - pbar[None, :]
    v_c = (wl[:, None] * dev * dev).sum(axis=0)
    a_c = (wl[:, None] * np.abs(dev)).sum(axis=0)
    HT, V, A, PB2 = (np.zeros(L, dtype=LD) for _ in range(4))
    for l in range(L):
        c0, c1 = off[l], off[l + 1]
        if c1 > c0:
            HT[l], V[l], A[l], PB2[l] = ht_c[c0:c1].sum(), v_c[c0:c1].sum(), a_c[c0:c1].sum(), (pbar[c0:c1] ** 2).sum()
    H = h / L1
    D = s / (2 * L1)
    den = D + (H[:, None] + H[None, :]) / 2
    with np.errstate(invalid="ignore", divide="ignore"):
        F = np.where(den != 0, D / np.where(den != 0, den, 1), np.nan)
        Fl = np.where((ua > 0) & (HT != 0), V / np.where(HT != 0, HT, 1), np.nan)
    sum_v, sum_ht = V.sum(), HT.sum()
    return dict(K=K, L=L, T=T, n_loci=L1, het=h, sqdiff=s, H=H, D=D, F=F, pbar=pbar, locus_ht=HT, locus_v=V, locus_abs=A,
                locus_pbar2=PB2, locus_f=Fl, sum_v=sum_v, sum_ht=sum_ht, f_all=(sum_v / sum_ht if sum_ht != 0 else LD("nan")),
                W=wl.sum())


def weights_from_q(q, K):
    """the command line's weights: column means of Q [I][K] over the rows without a NaN, 1 / K without one; Q [K] itself"""
    q = np.asarray(q, dtype=np.float64)
    if q.ndim == 1:
        return q.copy()
    ok = ~np.isnan(q).any(axis=1)
    if not ok.any():
        return np.full(K, 1.0 / K)
    w = np.zeros(K)
    for row in q[ok]:                                           # (row order, as mc_divergence_weights adds them)
        w += row
    return w / ok.sum()


# ---- parameter sets: (P [K][T], w [K]) ----
def ordinary(ua, K, seed):
    _, p = random_params(1, ua, K, seed=seed)
    return p, np.random.default_rng(seed + 1000).dirichlet(np.ones(K))


def near_fixed(ua, K, seed):
    """every other locus with two or more columns: the first column at 1 - 1e-12 in every cluster, the rest shares what is left"""
    p, w = ordinary(ua, K, seed)
    off = offsets(ua)
    for l in range(0, len(ua), 2):
        M = int(ua[l])
        if M >= 2:
            p[:, off[l]] = 1 - 1e-12
            p[:, off[l] + 1:off[l + 1]] = 1e-12 / (M - 1)
    return p, w


def twin_clusters(ua, K, seed):
    """cluster 1 = cluster 0 with every entry moved by a relative 1e-9 at most, renormalised per locus"""
    p, w = ordinary(ua, K, seed)
    if K < 2:
        return p, w
    rng = np.random.default_rng(seed + 2000)
    p[1] = p[0] * (1 + 1e-9 * rng.uniform(-1, 1, size=p.shape[1]))
    off = offsets(ua)
    for l in range(len(ua)):
        if ua[l] > 0:
            p[1, off[l]:off[l + 1]] /= p[1, off[l]:off[l + 1]].sum()
    return p, w


def zero_weight(ua, K, seed):
    p, w = ordinary(ua, K, seed)
    if K >= 2:
        w[0] = 0.0
        w /= w.sum()
    return p, w


MAKERS = (ordinary, near_fixed, twin_clusters, zero_weight)


# ---- float64 restatements of the sums, and mutants ----
def _sum(x, order):
    """a float64 sum of the 1-d array x: 'forward' and 'backward' one term at a time, 'pairwise' numpy's"""
    x = np.asarray(x, dtype=np.float64)
    if order == "pairwise":
        return float(np.sum(x))
    acc = 0.0
    for v in (x if order == "forward" else x[::-1]):
        acc += float(v)
    return acc


def restate(ua, P, w, order="forward", mutant=None):
    """what mchip_divergence returns, in float64 with the given summation order.  mutant: 'gram' (s_ab from sums of squares and a
    dot product), 'no_phantom' (the last column of every locus with three or more is left out), 'all_loci' (L for L1),
    'unweighted' (pbar and V with 1 / K for the weights)"""
    ua = np.asarray(ua, dtype=np.int64)
    P = np.asarray(P, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    K, T = P.shape
    L, off = len(ua), offsets(ua)
    keep = np.ones(T, dtype=bool)
    if mutant == "no_phantom":
        for l in range(L):
            if ua[l] >= 3:
                keep[off[l + 1] - 1] = False
    if mutant == "unweighted":
        w = np.full(K, 1.0 / K)
    het = np.array([_sum((P[a] * (1 - P[a]))[keep], order) for a in range(K)])
    sq = np.zeros((K, K))
    for a in range(K):
        for b in range(a + 1, K):
            if mutant == "gram":
                sq[a, b] = _sum((P[a] * P[a])[keep], order) + _sum((P[b] * P[b])[keep], order) - 2 * _sum((P[a] * P[b])[keep], order)
            else:
                d = P[a] - P[b]
                sq[a, b] = _sum((d * d)[keep], order)
            sq[b, a] = sq[a, b]
    pbar = fma_chain(w, P)
    ht_c = pbar * (1 - pbar)
    v_c = np.array([_sum(w * (P[:, c] - pbar[c]) ** 2, order) for c in range(T)])
    lv, lht = np.zeros(L), np.zeros(L)
    for l in range(L):
        sel = np.arange(off[l], off[l + 1])[keep[off[l]:off[l + 1]]]
        lv[l], lht[l] = _sum(v_c[sel], order), _sum(ht_c[sel], order)
    return dict(het=het, sqdiff=sq, locus_v=lv, locus_ht=lht, sum_v=_sum(lv, order), sum_ht=_sum(lht, order),
                n_loci=L if mutant == "all_loci" else int((ua > 0).sum()))


# ---- the checker ----
def _ratio(got, want, bound):
    """largest |got - want| / bound over the entries (0 where both the error and the bound are 0)"""
    err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - want)
    bound = np.asarray(bound, dtype=LD)
    r = np.where(err == 0, 0, err / np.where(bound > 0, bound, 1))
    r = np.where((err > 0) & (bound <= 0), np.inf, r)
    return float(np.max(r)) if np.size(r) else 0.0


def ratios(got, ua, P, w):
    """error / bound of every group of sums of `got` (het, sqdiff, locus_v, locus_ht, sum_v, sum_ht, n_loci as mchip_divergence
    gives them): a dict of the largest ratio per group; all <= 1 means every bound holds"""
    ua = np.asarray(ua, dtype=np.int64)
    ref, exact = reference(ua, P, w), reference(ua, P, w, exact_pbar=True)
    K, T = ref["K"], ref["T"]
    M = ua.astype(np.float64)
    off_diag = ~np.eye(K, dtype=bool)
    e = K * U / (1 - K * U)
    v_abs = 2 * e * exact["locus_abs"] + e * e * exact["W"] * exact["locus_pbar2"]
    sq = np.asarray(got["sqdiff"])
    out = dict(
        het=_ratio(got["het"], ref["het"], rel_bound(T) * ref["het"]),
        sqdiff=_ratio(sq[off_diag], ref["sqdiff"][off_diag], rel_bound(T) * ref["sqdiff"][off_diag]),
        locus_ht=_ratio(got["locus_ht"], ref["locus_ht"], rel_bound(M) * np.abs(ref["locus_ht"])),
        locus_v=_ratio(got["locus_v"], ref["locus_v"], rel_bound(K * M) * ref["locus_v"]),
        locus_v_exact=_ratio(got["locus_v"], exact["locus_v"], rel_bound(K * M) * (exact["locus_v"] + v_abs) + v_abs),
        sum_ht=_ratio(got["sum_ht"], ref["sum_ht"], rel_bound(T) * abs(ref["sum_ht"])),
        sum_v=_ratio(got["sum_v"], ref["sum_v"], rel_bound(K * T) * ref["sum_v"]),
    )
    out["shape"] = 0.0 if (np.array_equal(sq, sq.T) and not np.diag(sq).any() and got["n_loci"] == ref["n_loci"]
                           and not np.asarray(got["locus_v"])[ua == 0].any() and not np.asarray(got["locus_ht"])[ua == 0].any()) else np.inf
    return out


def check(got, ua, P, w):
    r = ratios(got, ua, P, w)
    bad = {k: v for k, v in r.items() if not v <= 1}
    assert not bad, "error / bound above 1: %r (all: %r)" % (bad, r)
    return r


def derived_bound(T):
    """H, D, F_ab, F_l and F are quotients of sums held to rel_bound: two such sums and at most eight more roundings"""
    return 2 * rel_bound(T) + 8 * U


# ---- shapes for the GPU tests ----
def shaped_ua(L, T=None):
    """allele counts for L loci: two alleles and the phantom slot mostly, some with two columns, and where there is room a
    monomorphic locus (1 column), one with 35 and one with 254 columns, and a locus without a column in the middle and at the
    end.  T: the total the counts are stretched to (by widening the plain loci, 200 columns at most each)."""
    ua = np.where(np.arange(L) % 3 == 1, 2, 3).astype(np.int32)
    if L >= 8:
        ua[1], ua[2], ua[L // 2], ua[5], ua[L - 1] = 1, 35, 0, 254, 0
    if T is not None:
        need = T - int(ua.sum())
        assert need >= 0
        for l in range(L):
            if ua[l] in (2, 3) and need:
                add = min(need, 200 - int(ua[l]))
                ua[l] += add
                need -= add
        assert need == 0
    return ua


def random_genotypes(ua, I, ploidy=2, seed=0, missing=0.1):
    """valid allele indices for every locus (a locus without a column is all missing)"""
    rng = np.random.default_rng(seed)
    L = len(ua)
    g = np.full((I, L, ploidy), 0xFF, dtype=np.uint8)
    for l in range(L):
        if ua[l] > 0:
            g[:, l, :] = rng.integers(0, ua[l], size=(I, ploidy))
    g[(rng.random(g.shape) < missing)] = 0xFF
    return g


def hexbits(res):
    """the bits of everything mchip_divergence returned, as text"""
    parts = [np.ascontiguousarray(res[k]).tobytes().hex() for k in ("het", "sqdiff", "locus_v", "locus_ht")]
    parts += [np.float64(res["sum_v"]).tobytes().hex(), np.float64(res["sum_ht"]).tobytes().hex(), "%d" % res["n_loci"]]
    return " ".join(parts)


def fixed_case(ctx, K=8):
    """one case on a context, the same every time: several pair-kernel chunks, several workgroups of the locus kernel"""
    ua = shaped_ua(700, T=2600)
    geno = random_genotypes(ua, 8, seed=5)
    p, w = ordinary(ua, K, seed=17)
    q = np.random.default_rng(3).dirichlet(np.ones(K), size=8)
    ctx.set_genotypes(ua, geno)
    ctx.set_model(K)
    ctx.set_q(0, q)
    ctx.set_p(0, p)
    return ctx.divergence(0, w)


if __name__ == "__main__":
    from multiclust_amd import hip
    c = hip.Context(0)
    print(hexbits(fixed_case(c, int(sys.argv[1]) if len(sys.argv) > 1 else 8)))
    c.close()
