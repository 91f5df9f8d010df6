"""Residual correlation of the admixture fit on the CPU (TEST INFRASTRUCTURE): the long-double reference of every quantity that
include/multiclust_hip.h defines for mchip_residual_products, the residual as the device forms it (exact-rational fma), float64
restatements (and deliberate mutants) of the sums, and the checker that holds G and D to the bounds.

The definitions.  a_il observed copies, n_ic copies carrying allele m, t_ic = sum_k q_ik p_kc, r_ic = n_ic - a_il t_ic,
s_il = sum_m r_ilm^2, o_il = [a_il > 0], G_ij = sum_c r_ic r_jc, D_ij = sum_l s_il o_jl, cor_ij = G_ij / sqrt(D_ij D_ji).

The bounds (u = 2^-53; starred quantities are exact, computed here in long double with t exact).
  The device's residual.  t is an fma chain of K non-negative terms: |t - t*| <= K u t* (1 + O(K u)).  r = fma(-a, t, n) is rounded
  once: r = (n - a t)(1 + d), |d| <= u, so |r - r*| <= a |t - t*| + u |r| <= K u a t* + u |r*| + second-order terms, which the step
  from K to K + 1 covers:   e_ic = (K + 1) u a_il t*_ic + u |r*_ic|.
  G.  The device adds the T products r_ic r_jc in some order with at most two roundings per term (a product rounded and added, or
  fused): for ANY order of T terms, |fl(sum) - sum| <= (T - 1 + 2) u (1 + O(T u)) sum |terms| <= (T + 8) u sum_c |r_ic r_jc|.
  The terms themselves are off by |r_i r_j - r*_i r*_j| <= e_i |r*_j| + |r*_i| e_j + e_i e_j.  Together
      |G_ij - G*_ij| <= (T + 8) u sum_c |r*_ic r*_jc| + sum_c (e_ic |r*_jc| + |r*_ic| e_jc + e_ic e_jc).
  D.  Its terms are non-negative: s_il is a chain of M_l squares, then at most L of them are added: a relative (M_l + L + 8) u on
  every locus's share; the squares are off by |r^2 - r*^2| <= 2 e |r*| + e^2 and o is exact:
      |D_ij - D*_ij| <= sum_l o_jl [ (M_l + L + 8) u s*_il + sum_m (2 e_ilm |r*_ilm| + e_ilm^2) ].
  Where the data set has no missing copy the definition makes D_ij = G_ii bit for bit, and the checker asks for that.

When run as a program it prints the bits of one fixed case: tests/test_gpu_resid.py starts it as a fresh process under different
launch-geometry knobs."""
import sys
from fractions import Fraction

import numpy as np

from divergence_util import fma_chain, offsets

LD = np.longdouble
U = 2.0 ** -53
MISSING = 0xFF


def counts(ua, geno):
    """a [I][L] observed copies and n [I][T] copies carrying each allele, as int64"""
    ua = np.asarray(ua, dtype=np.int64)
    geno = np.asarray(geno, dtype=np.uint8)
    I, L, pl = geno.shape
    off = offsets(ua)
    a = (geno != MISSING).sum(axis=2).astype(np.int64)
    n = np.zeros((I, int(off[-1])), dtype=np.int64)
    for l in range(L):
        for m in range(int(ua[l])):
            n[:, off[l] + m] = (geno[:, l, :] == m).sum(axis=1)
    return a, n


def rows_of(Q, I):
    Q = np.asarray(Q, dtype=np.float64)
    return Q if Q.ndim == 2 else np.broadcast_to(Q, (I, Q.shape[0]))


def col_locus(ua):
    return np.repeat(np.arange(len(ua)), np.asarray(ua, dtype=np.int64))


def _per_locus(x, ua):
    """sum over the columns of every locus of x [I][T] -> [I][L] (a locus without a column: 0)"""
    off = offsets(ua)
    out = np.zeros((x.shape[0], len(ua)), dtype=x.dtype)
    for l in range(len(ua)):
        if off[l + 1] > off[l]:
            out[:, l] = x[:, off[l]:off[l + 1]].sum(axis=1)
    return out


def reference(ua, geno, Q, P):
    """every quantity of the definitions in long double, t exact, and the bounds of the module's docstring"""
    ua = np.asarray(ua, dtype=np.int64)
    P = np.asarray(P, dtype=np.float64)
    K, T = P.shape
    I, L = geno.shape[0], len(ua)
    a, n = counts(ua, geno)
    cl = col_locus(ua)
    ac = a[:, cl].astype(LD)                                    # a_il of every column
    t = rows_of(Q, I).astype(LD) @ P.astype(LD)
    r = n.astype(LD) - ac * t
    o = (a > 0).astype(LD)
    s = _per_locus(r * r, ua)
    G = r @ r.T
    D = s @ o.T
    ar = np.abs(r)
    e = (K + 1) * U * ac * t + U * ar
    g_bound = (T + 8) * U * (ar @ ar.T) + e @ ar.T + ar @ e.T + e @ e.T
    es = _per_locus(2 * e * ar + e * e, ua)
    d_bound = (((ua + L + 8) * U).astype(LD)[None, :] * s + es) @ o.T
    with np.errstate(invalid="ignore", divide="ignore"):
        den = np.sqrt(D * D.T)
        cor = np.where((D > 0) & (D.T > 0), G / np.where(den > 0, den, 1), np.nan)
    cor[np.diag_indices(I)] = np.nan
    return dict(I=I, L=L, T=T, K=K, a=a, n=n, t=t, r=r, s=s, o=o, e=e, G=G, D=D, g_bound=g_bound, d_bound=d_bound, cor=cor,
                no_missing=bool((a == geno.shape[2]).all()))


def device_residuals(ua, geno, Q, P, ploidy_for_a=False):
    """r [I][T] as the definition fixes its bits: t by the fma chain in k order from 0, r = fma(-a, t, n), 0 where a = 0 -- every fma
    exact in rationals and rounded once (small shapes: I T K rational operations).  ploidy_for_a: the mutant that predicts from the
    ploidy where copies are missing"""
    ua = np.asarray(ua, dtype=np.int64)
    P = np.asarray(P, dtype=np.float64)
    I = geno.shape[0]
    a, n = counts(ua, geno)
    cl = col_locus(ua)
    q = rows_of(Q, I)
    r = np.zeros((I, P.shape[1]))
    for i in range(I):
        t = fma_chain(q[i], P)
        for c in range(P.shape[1]):
            ai = int(a[i, cl[c]]) if not ploidy_for_a else geno.shape[2]
            r[i, c] = float(Fraction(int(n[i, c])) - ai * Fraction(float(t[c]))) if ai else 0.0
    return r


def exact(ua, geno, Q, P):
    """G and D in exact rationals from exact residuals (tiny shapes): object arrays of Fractions"""
    ua = np.asarray(ua, dtype=np.int64)
    I, (K, T) = geno.shape[0], np.asarray(P).shape
    a, n = counts(ua, geno)
    cl = col_locus(ua)
    q = rows_of(Q, I)
    r = [[Fraction(int(n[i, c])) - int(a[i, cl[c]]) * sum(Fraction(float(q[i, k])) * Fraction(float(P[k][c])) for k in range(K))
          for c in range(T)] for i in range(I)]
    G = [[sum(r[i][c] * r[j][c] for c in range(T)) for j in range(I)] for i in range(I)]
    D = [[sum(r[i][c] ** 2 for c in range(T) if a[j, cl[c]] > 0) for j in range(I)] for i in range(I)]
    return r, G, D


# ---- float64 restatements of the sums, and mutants ----
def _products(X, Y, order):
    """sum_c X[:, c] Y[:, c]^T in float64, every product rounded, then added: 'forward' / 'backward' one column at a time, 'mfma'
    four columns to a group -- the group's products added to each other first, then to the accumulator (one of the orders a
    16 x 16 x 4 instruction may use; tiles of 16 x 16 outputs do not change the order inside an element)"""
    n = X.shape[1]
    acc = np.zeros((X.shape[0], Y.shape[0]))
    if order == "mfma":
        for c0 in range(0, n, 4):
            grp = np.zeros_like(acc)
            for c in range(c0, min(n, c0 + 4)):
                grp = grp + np.outer(X[:, c], Y[:, c])
            acc = acc + grp
        return acc
    for c in (range(n) if order == "forward" else range(n - 1, -1, -1)):
        acc = acc + np.outer(X[:, c], Y[:, c])
    return acc


def restate(ua, geno, Q, P, order="forward", mutant=None, r=None, chunk=512):
    """(G, D) as mchip_residual_products returns them, in float64 with the given summation order, from the device's residuals (r:
    device_residuals when the caller has them already).  mutant: 'diag_norms' (G_ii for the pairwise-complete D), 'ploidy' (the
    ploidy for a_il), 'drop_chunk' (the columns behind the last multiple of `chunk` left out), 'transposed' (D^T)"""
    ua = np.asarray(ua, dtype=np.int64)
    a, n = counts(ua, geno)
    if mutant == "ploidy":
        r = device_residuals(ua, geno, Q, P, ploidy_for_a=True)
    elif r is None:
        r = device_residuals(ua, geno, Q, P)
    T = r.shape[1]
    keep = T if mutant != "drop_chunk" else (T - 1) // chunk * chunk
    G = _products(r[:, :keep], r[:, :keep], order)
    off = offsets(ua)
    s = np.zeros((r.shape[0], len(ua)))
    for l in range(len(ua)):
        for c in range(off[l], off[l + 1]):
            s[:, l] = s[:, l] + r[:, c] * r[:, c]
    o = (a > 0).astype(np.float64)
    if mutant == "diag_norms" or (mutant is None and (a == geno.shape[2]).all()):
        D = np.repeat(np.diag(G)[:, None], r.shape[0], axis=1)
    else:
        D = _products(s, o, order)
    return G, (D.T.copy() if mutant == "transposed" else D)


# ---- the checker ----
def _ratio(got, want, bound):
    err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - want)
    r = np.where(err == 0, 0, err / np.where(bound > 0, bound, 1))
    r = np.where((err > 0) & (bound <= 0), np.inf, r)
    r = np.where(np.isnan(err), np.inf, r)
    return float(np.max(r)) if np.size(r) else 0.0


def ratios(G, D, ref):
    """error / bound of G and of D (None: not asked for) against reference(): the largest ratio of each; 'shape' is 0 when G is
    symmetric bit for bit and, on a data set without a missing copy, D_ij is G_ii bit for bit, else inf"""
    G = np.asarray(G, dtype=np.float64)
    out = dict(gram=_ratio(G, ref["G"], ref["g_bound"]))
    ok = G.shape == (ref["I"], ref["I"]) and np.array_equal(G, G.T)
    if D is not None:
        D = np.asarray(D, dtype=np.float64)
        out["norms"] = _ratio(D, ref["D"], ref["d_bound"])
        if ref["no_missing"]:
            ok = ok and np.array_equal(D, np.repeat(np.diag(G)[:, None], ref["I"], axis=1))
    out["shape"] = 0.0 if ok else np.inf
    return out


def check(G, D, ref, limit=1.0):
    r = ratios(G, D, ref)
    bad = {k: v for k, v in r.items() if not v <= limit}
    assert not bad, "error / bound above %g: %r (all: %r)" % (limit, bad, r)
    return r


def correlation(G, D):
    """cor from the sums in float64, as mc_residual_ratios forms it"""
    G, D = np.asarray(G, dtype=np.float64), np.asarray(D, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        den = np.sqrt(D * D.T)
        cor = np.where((D > 0) & (D.T > 0), G / np.where(den > 0, den, 1), np.nan)
    cor[np.diag_indices(G.shape[0])] = np.nan
    return cor


# ---- shapes and parameters for the tests ----
def biallelic(I, T, ploidy=2, seed=0, missing=0.0):
    """loci of two columns (one of three where T is odd, one of one where T = 1) with T columns in all"""
    assert T >= 1
    ua = np.full(T // 2, 2, dtype=np.int32)
    if T % 2:
        ua = np.concatenate((ua[:-1], [3])) if T >= 3 else np.array([1], dtype=np.int32)
    ua = ua.astype(np.int32)
    assert int(ua.sum()) == T
    return ua, genotypes(ua, I, ploidy, seed, missing)


def genotypes(ua, I, ploidy=2, seed=0, missing=0.0):
    """valid allele indices for every locus (a locus without a column is all missing), `missing` of the copies missing"""
    rng = np.random.default_rng(seed)
    g = np.full((I, len(ua), ploidy), MISSING, dtype=np.uint8)
    for l in range(len(ua)):
        if ua[l] > 0:
            g[:, l, :] = rng.integers(0, ua[l], size=(I, ploidy))
    if missing:
        g[rng.random(g.shape) < missing] = MISSING
    return g


def parameters(ua, I, K, seed=0):
    """Q [I][K] rows on the simplex, P [K][T] with every locus's columns summing to 1 in every cluster"""
    rng = np.random.default_rng(seed + 500)
    Q = rng.dirichlet(np.ones(K), size=I)
    off = offsets(ua)
    P = np.zeros((K, int(off[-1])))
    for l in range(len(ua)):
        if ua[l] > 0:
            P[:, off[l]:off[l + 1]] = rng.dirichlet(np.full(int(ua[l]), 0.7), size=K)
    return Q, P


def hexbits(G, D):
    return np.ascontiguousarray(G).tobytes().hex() + " " + ("-" if D is None else np.ascontiguousarray(D).tobytes().hex())


def fixed_case(ctx, K=8):
    """one case on a context, the same every time: three chunks of columns, two tiles of individuals a side, missing copies"""
    ua, geno = biallelic(70, 1300, seed=5, missing=0.1)
    Q, P = parameters(ua, 70, K, seed=17)
    ctx.set_genotypes(ua, geno)
    ctx.set_model(K)
    ctx.set_q(0, Q)
    ctx.set_p(0, P)
    return ctx.residual_products(0)


if __name__ == "__main__":
    from multiclust_amd import hip
    c = hip.Context(0)
    print(hexbits(*fixed_case(c, int(sys.argv[1]) if len(sys.argv) > 1 else 8)))
    c.close()
