"""Kinship under the fitted admixture model on the CPU (TEST INFRASTRUCTURE): the long-double reference of the two sums that
include/multiclust_hip.h defines for mchip_kinship_products, float64 restatements (and deliberate mutants) of them, the checker that
holds G and V to the bounds, the host's rules (multiclust_amd/host/mc_kinship.c) restated down to the text of its line and its two
files, and a pedigree with admixed founders.

The definitions.  a_il observed copies, n_ic copies carrying allele m, t_ic = sum_k q_ik p_kc, r_ic = n_ic - a_il t_ic (all as
tests/resid_util.py has them), v_ic = t_ic max(1 - t_ic, 0), w_ic = a_il sqrt(v_ic), G_ij = sum_c r_ic r_jc, V_ij = sum_c w_ic w_jc,
phi_ij = G_ij / V_ij (NaN where V_ij = 0).

The bounds (u = 2^-53; starred quantities are exact, computed here in long double with t exact).
  G.  resid_util's: the operand and the kernel are the same.
  The device's w.  t^ is an fma chain of K non-negative terms: |t^ - t| <= K u t.  d^ = fl(1 - t^), one rounded subtraction, is off
  1 - t by at most K u t + u (1 - t) <= K u t + u; the fmax changes nothing where the difference is positive and takes a negative
  one, which lies inside that error of the non-negative 1 - t, to 0, nearer still.  v^ = fl(t^ d^), to first order:
  |v^ - v| <= |t^ - t| (1 - t) + t |d^ - (1 - t)| + u v <= K u v + (K u t^2 + u v) + u v = (K + 2) u v + K u t^2 =: e_v.
  The square root: for v > 0 the mean
  value theorem gives |sqrt(v^) - sqrt(v)| <= e_v / sqrt(v) (first order), and always |sqrt(v^) - sqrt(v)| <= sqrt(|v^ - v|) <=
  sqrt(e_v), which is the smaller one near v = 0: the minimum of the two.  Two further u relative cover a square root that is not
  correctly rounded.  Times a_il:   e_ic = a_il (min(e_v / sqrt(v), sqrt(e_v)) + 2 u sqrt(v)).
  V.  As G: any order of T terms, at most two roundings per term, and the terms off by e_i w_j + w_i e_j + e_i e_j:
      |V_ij - V*_ij| <= (T + 8) u sum_c w_ic w_jc + sum_c (e_ic w_jc + w_ic e_jc + e_ic e_jc).

When run as a program it prints the bits of one fixed case: tests/test_gpu_kinship.py starts it as a fresh process under different
launch knobs."""
import sys

import numpy as np

import bedfiles
import resid_util as ru
from divergence_util import fma_chain, offsets

LD = np.longdouble
U = ru.U
MISSING = ru.MISSING
CUTS = (0.354, 0.177, 0.0884, 0.0442)                          # duplicate / MZ, first, second, third degree


def reference(ua, geno, Q, P):
    """resid_util.reference's dict (G, g_bound, a, n, t, r, ...) with w, V, e_w, v_bound and phi added"""
    ref = ru.reference(ua, geno, Q, P)
    K, T = ref["K"], ref["T"]
    ac = ref["a"][:, ru.col_locus(ua)].astype(LD)
    t = ref["t"]
    v = t * np.maximum(1 - t, 0)
    sv = np.sqrt(v)
    e_v = (K + 2) * U * v + K * U * t * t
    with np.errstate(divide="ignore", invalid="ignore"):
        by_slope = np.where(sv > 0, e_v / np.where(sv > 0, sv, 1), np.inf)
    e = ac * (np.minimum(by_slope, np.sqrt(e_v)) + 2 * U * sv)
    w = ac * sv
    V = w @ w.T
    ref.update(v=v, w=w, e_w=e, V=V, v_bound=(T + 8) * U * V + e @ w.T + w @ e.T + e @ e.T)
    with np.errstate(divide="ignore", invalid="ignore"):
        ref["phi"] = np.where(V > 0, ref["G"] / np.where(V > 0, V, 1), np.nan)
    return ref


def pooled_frequencies(ua, geno):
    """the homogeneous estimator's frequencies: per column the share of the observed copies of the whole sample that carry the allele,
    as a one-cluster P [1][T]"""
    a, n = ru.counts(ua, geno)
    tot = a.sum(axis=0)[ru.col_locus(ua)].astype(np.float64)
    return (n.sum(axis=0) / np.where(tot > 0, tot, 1))[None, :]


def device_operands(ua, geno, Q, P, mutant=None):
    """(r, w) [I][T] in float64 as the device forms them: t by the fma chain (exact rationals, rounded once a step), r = fma(-a, t, n),
    v = t fmax(1 - t, 0), w = a sqrt(v).  mutant: 'no_fmax' (v = t (1 - t)), 'no_copies' (w = sqrt(v) wherever a > 0), 'pooled' (the
    pooled sample frequencies in place of t)"""
    ua = np.asarray(ua, dtype=np.int64)
    I = geno.shape[0]
    if mutant == "pooled":
        Q, P = np.ones((I, 1)), pooled_frequencies(ua, geno)
    r = ru.device_residuals(ua, geno, Q, P)
    a, _ = ru.counts(ua, geno)
    ac = a[:, ru.col_locus(ua)].astype(np.float64)
    q = ru.rows_of(Q, I)
    t = np.stack([fma_chain(q[i], np.asarray(P, dtype=np.float64)) for i in range(I)])
    one_minus = 1.0 - t
    with np.errstate(invalid="ignore"):
        v = t * (one_minus if mutant == "no_fmax" else np.maximum(one_minus, 0.0))
        w = (ac if mutant != "no_copies" else (ac > 0).astype(np.float64)) * np.sqrt(v)
    return r, np.where(ac > 0, w, 0.0)


def restate(ua, geno, Q, P, order="forward", mutant=None):
    """(G, V) as mchip_kinship_products returns them, in float64 with resid_util's summation orders.  mutant: those of
    device_operands, and 'gram_diag' (sqrt(G_ii G_jj), the correlation's denominator, in place of V)"""
    r, w = device_operands(ua, geno, Q, P, mutant if mutant != "gram_diag" else None)
    G, V = ru._products(r, r, order), ru._products(w, w, order)
    if mutant == "gram_diag":
        d = np.diag(G)
        V = np.sqrt(np.outer(d, d))
    return G, V


def ratios(G, V, ref):
    """error / bound of G and V against reference(): the largest ratio of each; 'shape' is 0 when both are symmetric bit for bit"""
    G, V = np.asarray(G, dtype=np.float64), np.asarray(V, dtype=np.float64)
    ok = G.shape == V.shape == (ref["I"], ref["I"]) and np.array_equal(G, G.T) and np.array_equal(V, V.T, equal_nan=True)
    return dict(gram=ru._ratio(G, ref["G"], ref["g_bound"]), scale=ru._ratio(V, ref["V"], ref["v_bound"]), shape=0.0 if ok else np.inf)


def check(G, V, ref, limit=1.0):
    r = ratios(G, V, ref)
    bad = {k: v for k, v in r.items() if not v <= limit}
    assert not bad, "error / bound above %g: %r (all: %r)" % (limit, bad, r)
    return r


# ---- the host's rules (mc_kinship.c), restated ----
def kinship(G, V):
    G, V = np.asarray(G, dtype=np.float64), np.asarray(V, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(V > 0, G / np.where(V > 0, V, 1), np.nan)


def degree(phi):
    for d, cut in enumerate(CUTS):
        if phi > cut:
            return d
    return 4


def _num(v):
    return "NaN" if np.isnan(v) else "%.6f" % v


def report(G, V, ploidy, t, K):
    """what mc_kinship_from_sums, mc_kinship_line and mc_write_kinship make of the sums: dict with pairs [(i, j, phi, G, V, degree)],
    n_degree [5], n_finite, mean, max, max_pair, per individual self, inbreeding, count, ind_max, partner, and the texts line, kin0
    and ind"""
    phi = kinship(G, V)
    I = phi.shape[0]
    pairs, n_degree, total, n_finite, hi, max_pair = [], [0] * 5, 0.0, 0, -np.inf, (-1, -1)
    self_, inb, cnt, big, partner = np.full(I, np.nan), np.full(I, np.nan), np.zeros(I, dtype=int), np.full(I, np.nan), np.full(I, -1)
    for i in range(I):
        m, who = -np.inf, -1
        for j in range(I):
            x = phi[i, j]
            if j == i:
                self_[i] = x
                inb[i] = 2.0 * x - 1.0 if ploidy == 2 else np.nan
                continue
            if not np.isfinite(x):
                continue
            if x > m:
                m, who = x, j
            cnt[i] += x > t
            if j < i:
                continue
            total += x
            n_finite += 1
            if x > hi:
                hi, max_pair = x, (i, j)
            if x > t:
                pairs.append((i, j, x, G[i, j], V[i, j], degree(x)))
                n_degree[degree(x)] += 1
        if who >= 0:
            big[i], partner[i] = m, who
    mean = total / n_finite if n_finite else np.nan
    line = "Kinship (K=%d): " % K
    if n_finite:
        line += ("%d pairs above %g (%d duplicates, %d first, %d second, %d third degree); largest %.6f (%d, %d); mean over %d pairs %.6f"
                 % (len(pairs), t, n_degree[0], n_degree[1], n_degree[2], n_degree[3], hi, max_pair[0], max_pair[1], n_finite, mean))
    else:
        line += "no pairs"
    kin0 = "i\tj\tphi\tG\tV\tdegree\n" + "".join("%d\t%d\t%s\t%s\t%s\t%d\n" % (i, j, _num(x), _num(g), _num(v), d)
                                                  for i, j, x, g, v, d in pairs)
    ind = "i\tself\tinbreeding\tn_above\tmax\tpartner\n" + "".join(
        "%d\t%s\t%s\t%d\t%s\t%d\n" % (i, _num(self_[i]), _num(inb[i]), cnt[i], _num(big[i]), partner[i]) for i in range(I))
    return dict(phi=phi, pairs=pairs, n_degree=n_degree, n_finite=n_finite, mean=mean, max=hi if n_finite else np.nan, max_pair=max_pair,
                self=self_, inbreeding=inb, count=cnt, ind_max=big, partner=partner, line=line, kin0=kin0, ind=ind)


# ---- a pedigree with admixed founders ----
def pedigree(seed, L, founders=40, missing=0.05, fst=0.15):
    """king_util.pedigree with per-individual admixture: two Balding-Nichols populations, `founders` (>= 9) founders whose share of
    population 0 is Beta(1/2, 1/2) and whose every allele copy comes from population 0 with that probability, a duplicate of founder
    2, two children of founders 0 and 1 (a trio with two sibs), a child of 3 and 4, three children of 5 and 6; a child's share is the
    mean of its parents'.  The individuals are shuffled.  Returns dict: codes [I][L] (.bed codes), dup (the duplicate pair), first (the
    parent-child and sib pairs), planted = both, Q [I][2] and P [2][2 L] the true parameters (column 2 l + 1 is allele A2 of locus l)"""
    assert founders >= 9
    rng = np.random.default_rng(seed)
    anc = rng.uniform(0.1, 0.9, size=L)
    freq = np.stack([rng.beta(anc * (1 - fst) / fst, (1 - anc) * (1 - fst) / fst) for _ in range(2)])
    hap, share = {}, {}

    def founder(x):
        share[x] = float(rng.beta(0.5, 0.5))
        src = (rng.random((2, L)) >= share[x]).astype(int)      # the population each copy comes from
        hap[x] = (rng.random((2, L)) < freq[src, np.arange(L)]).astype(np.uint8)

    def child(x, mother, father):
        pick_m, pick_f = rng.integers(0, 2, size=L), rng.integers(0, 2, size=L)
        hap[x] = np.stack([hap[mother][pick_m, np.arange(L)], hap[father][pick_f, np.arange(L)]])
        share[x] = 0.5 * (share[mother] + share[father])

    F = founders
    for x in range(F):
        founder(x)
    hap[F], share[F] = hap[2].copy(), share[2]
    child(F + 1, 0, 1)
    child(F + 2, 0, 1)
    child(F + 3, 3, 4)
    for x in (F + 4, F + 5, F + 6):
        child(x, 5, 6)
    dup = {(2, F)}
    first = {(0, F + 1), (1, F + 1), (0, F + 2), (1, F + 2), (F + 1, F + 2), (3, F + 3), (4, F + 3)}
    first |= {(p, c) for p in (5, 6) for c in (F + 4, F + 5, F + 6)} | {(F + 4, F + 5), (F + 4, F + 6), (F + 5, F + 6)}
    n = len(hap)
    dosage = np.stack([hap[x].sum(axis=0) for x in range(n)])
    codes = np.array([bedfiles.HOM1, bedfiles.HET, bedfiles.HOM2], dtype=np.uint8)[dosage]
    codes[rng.random(codes.shape) < missing] = bedfiles.MISS
    order = rng.permutation(n)                                   # file position x holds individual order[x]
    place = np.argsort(order)

    def placed(pairs):
        return {tuple(sorted((int(place[a]), int(place[b])))) for a, b in pairs}

    s = np.array([share[int(x)] for x in order])
    P = np.zeros((2, 2 * L))
    P[:, 1::2], P[:, 0::2] = freq, 1 - freq
    return dict(codes=codes[order], dup=placed(dup), first=placed(first), planted=placed(dup | first), Q=np.stack([s, 1 - s], axis=1), P=P)


def genotypes_of(codes):
    """(ua, geno) of .bed codes with two columns a locus: HOM1 = (0, 0), HET = (0, 1), HOM2 = (1, 1), a missing call two missing copies"""
    table = np.array([[0, 0], [MISSING, MISSING], [0, 1], [1, 1]], dtype=np.uint8)
    return np.full(codes.shape[1], 2, dtype=np.int32), table[codes]


def margins(phi, ped):
    """(smallest phi of the duplicate pairs, smallest of the first-degree pairs, largest of all other pairs i < j)"""
    I = phi.shape[0]
    other = [phi[i, j] for i in range(I) for j in range(i + 1, I) if (i, j) not in ped["planted"]]
    return min(phi[p] for p in ped["dup"]), min(phi[p] for p in ped["first"]), float(np.nanmax(other))


# ---- one fixed case for the knob runs ----
def hexbits(G, V):
    return np.ascontiguousarray(G).tobytes().hex() + " " + np.ascontiguousarray(V).tobytes().hex()


def fixed_case(ctx, K=8):
    """resid_util.fixed_case's state: three chunks of columns, two tiles of individuals a side, missing copies"""
    ru.fixed_case(ctx, K)
    return ctx.kinship_products(0)


if __name__ == "__main__":
    from multiclust_amd import hip
    c = hip.Context(0)
    print(hexbits(*fixed_case(c, int(sys.argv[1]) if len(sys.argv) > 1 else 8)))
    c.close()
