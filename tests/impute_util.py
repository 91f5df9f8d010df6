"""Filling missing genotypes on the CPU (TEST INFRASTRUCTURE): the numpy float64 form of the rule of mchip_impute_missing
(include/multiclust_hip.h) -- the predictive t, the greedy mode of the multinomial, the confidence c -- a brute-force mode over all
multisets, the data sets of tests/test_gpu_impute.py and the scores of the accuracy tests."""
import itertools
import math

import numpy as np

MISSING = 0xFF


def impute_dataset(I, L, ploidy, alleles, missing, seed, specials=True):
    """(uniquealleles, n_real, geno): 2..`alleles` real alleles per locus (locus 0 has `alleles`), `missing` of the copies
    missing, and the phantom slot the reader gives every locus that has a missing copy.  specials, where the shape has room:
    individual 1 without a single copy, locus 2 without a call but with its candidates (as under a hold-out), locus 4 without a
    call and without an allele column (uniquealleles = 0, the reader's locus with no call)."""
    rng = np.random.default_rng(seed)
    n_real = rng.integers(2, alleles + 1, size=L).astype(np.int32)
    n_real[0] = alleles
    geno = rng.integers(0, n_real[None, :, None], size=(I, L, ploidy)).astype(np.uint8)
    geno[rng.random(geno.shape) < missing] = MISSING
    if specials and I >= 3:
        geno[1] = MISSING
    if specials and L >= 7:
        geno[:, 2, :] = MISSING
        geno[:, 4, :] = MISSING
        n_real[4] = 0
    has_missing = (geno == MISSING).any(axis=(0, 2))
    ua = (n_real + (has_missing & (n_real > 0))).astype(np.int32)
    return ua, n_real, geno


def missing_genotypes(geno):
    """(i, l, r) of every genotype with r >= 1 missing copies, in i, l order"""
    miss = geno == MISSING
    ii, ll = np.nonzero(miss.any(axis=2))
    return ii, ll, miss[ii, ll].sum(axis=1)


def predictive(ua, n_real, ii, ll, q, p):
    """t [n][M] of the listed genotypes over the candidates of their loci (0 behind the last candidate) and the mask of the
    candidates.  q: [I][K] or [K]; p: [K][T]."""
    toff = np.concatenate(([0], np.cumsum(ua)))[:-1]
    nr = np.asarray(n_real)[ll]
    M = max(1, int(nr.max())) if len(ll) else 1
    valid = np.arange(M)[None, :] < nr[:, None]
    cols = np.where(valid, toff[ll][:, None] + np.arange(M)[None, :], 0)
    qq = q[ii] if q.ndim == 2 else np.broadcast_to(q, (len(ii), q.shape[0]))
    t = np.einsum("nk,knm->nm", qq, p[:, cols]) if len(ii) else np.zeros((0, M))
    return np.where(valid, t, 0.0), valid


def fillable(t, valid):
    """a candidate with t > 0 (NaN is not)"""
    with np.errstate(invalid="ignore"):
        return (valid & (t > 0)).any(axis=1)


def greedy_counts(t, valid, r):
    """c [n][M]: copy j = 1 .. r goes to the first m with the largest t_m / (c_m + 1); rows that are not fillable keep 0"""
    c = np.zeros(t.shape, dtype=np.int64)
    ok = fillable(t, valid)
    rows = np.arange(len(t))
    for j in range(int(r.max()) if len(r) else 0):
        with np.errstate(invalid="ignore"):
            v = np.where(valid & (t > 0), t / (c + 1), -np.inf)
        am = np.argmax(v, axis=1)                       # the first of equal maxima
        act = ok & (j < r)
        c[rows[act], am[act]] += 1
    return c


FACT = np.array([math.factorial(n) for n in range(21)], dtype=np.float64)


def multiset_prob(t, valid, c):
    """r! / prod c_m! prod x_m^c_m with x = t / sum_cand t, per row"""
    s = t.sum(axis=1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        x = np.where(valid, t / s, 1.0)
        terms = np.where(c > 0, x ** c, 1.0)
    coef = FACT[c.sum(axis=1)] / np.prod(FACT[c], axis=1)
    return coef * np.prod(terms, axis=1)


def filled_counts(geno, out, ii, ll, M):
    """c [n][M] of what `out` holds in the positions that are missing in `geno`; -1 rows where a filled position is still missing"""
    miss = geno[ii, ll] == MISSING
    vals = out[ii, ll].astype(np.int64)
    c = np.zeros((len(ii), max(M, 1)), dtype=np.int64)
    bad = np.zeros(len(ii), dtype=bool)
    for a in range(geno.shape[2]):
        sel = miss[:, a]
        left = sel & (vals[:, a] == MISSING)
        bad |= left
        put = sel & ~left
        over = put & (vals[:, a] >= c.shape[1])
        bad |= over
        put &= ~over
        np.add.at(c, (np.flatnonzero(put), vals[put, a]), 1)
    c[bad] = -1
    return c


def impute_reference(ua, n_real, geno, q, p):
    """the rule on the CPU: dict with the genotypes with missing copies (ii, ll, r), t, valid, whether each is fillable, the greedy
    counts c, their probability conf, and `filled`: geno with the multisets written ascending into the missing positions"""
    ii, ll, r = missing_genotypes(geno)
    t, valid = predictive(ua, n_real, ii, ll, q, p)
    ok = fillable(t, valid)
    c = greedy_counts(t, valid, r)
    conf = np.where(ok, multiset_prob(t, valid, np.where(ok[:, None], c, 0)), 0.0)
    filled = geno.copy()
    for n in np.flatnonzero(ok):
        vals = np.repeat(np.arange(c.shape[1]), c[n])
        g = filled[ii[n], ll[n]]
        g[g == MISSING] = vals
    return dict(ii=ii, ll=ll, r=r, t=t, valid=valid, ok=ok, c=c, conf=conf, filled=filled)


def brute_mode(x, r):
    """(largest probability, its multiset as counts) over all multisets of r copies of len(x) alleles; of equal ones the first in
    lexicographic order of the sorted allele lists"""
    best, best_c = -1.0, None
    for combo in itertools.combinations_with_replacement(range(len(x)), r):
        c = np.bincount(combo, minlength=len(x))
        pr = math.factorial(r) / np.prod([math.factorial(int(v)) for v in c]) * np.prod(np.asarray(x, dtype=np.float64) ** c)
        if pr > best:
            best, best_c = pr, c
    return best, best_c


def sorted_pairs(geno):
    return np.sort(geno, axis=2)


def concordance(truth, filled, hidden):
    """share of the hidden genotypes [I][L] (all copies hidden) whose filled multiset is the true one"""
    same = (sorted_pairs(truth) == sorted_pairs(filled)).all(axis=2)
    return float(same[hidden].mean())


def modal_baseline(truth, hidden):
    """the same for filling in every locus's most frequent observed (not hidden) genotype"""
    I, L, pl = truth.shape
    base = 1 + int(truth.max())
    code = np.zeros((I, L), dtype=np.int64)
    for a in range(pl):
        code = code * base + sorted_pairs(truth)[:, :, a]
    hits = 0
    for l in range(L):
        obs = code[~hidden[:, l], l]
        if not len(obs):
            continue
        vals, cnt = np.unique(obs, return_counts=True)
        hits += int((code[hidden[:, l], l] == vals[np.argmax(cnt)]).sum())
    return hits / float(hidden.sum())
