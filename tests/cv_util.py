"""Cross-validation on the CPU (TEST INFRASTRUCTURE): the data sets, the numpy mask and the numpy form of the held-out score that
tests/test_gpu_cv*.py compare mchip_cv_* and mc_cross_validate with."""
import math

import numpy as np

import rand_window as rw
from synth import make_dataset

MISSING = 0xFF


def cv_dataset(I, L, ploidy, seed, missing=0.02, many=35):
    """make_dataset with up to 4 alleles per locus and `missing` of the copies missing, plus: locus 0 with `many` alleles, locus 1
    without a missing call, and the phantom allele slot the reader gives every locus that has a missing copy"""
    ua, geno = make_dataset(I, L, 3, ploidy=ploidy, max_alleles=4, seed=seed, missing=missing)
    rng = np.random.default_rng(seed + 1)
    ua = ua.copy()
    ua[0] = many
    geno[:, 0, :] = rng.integers(0, many, size=(I, ploidy))
    geno[:, 0, :][rng.random((I, ploidy)) < missing] = MISSING
    geno[:, 1, :] = rng.integers(0, ua[1], size=(I, ploidy))
    has_missing = (geno == MISSING).any(axis=(0, 2))
    assert not has_missing[1]
    return (ua + has_missing).astype(np.int32), geno


def clustered_dataset(I, L, n_clusters, seed):
    """diploid, biallelic, no missing data: every individual belongs to one of n_clusters clusters whose allele frequencies are
    drawn far apart (Beta(0.3, 0.3): most loci nearly fixed one way or the other in a cluster)"""
    rng = np.random.default_rng(seed)
    f = rng.beta(0.3, 0.3, size=(n_clusters, L))
    z = np.arange(I) % n_clusters
    geno = (rng.random((I, L, 2)) < f[z][:, :, None]).astype(np.uint8)
    return np.full(L, 2, np.int32), geno


def serial_folds(window, I, L, n_folds):
    return (rw.draws(window, I * L) % n_folds).astype(np.uint8).reshape(I, L)


def masked(geno, folds, f):
    out = geno.copy()
    if f >= 0:
        out[folds == f] = MISSING
    return out


def empty_individuals(geno):
    e = np.flatnonzero((geno == MISSING).all(axis=(1, 2)))
    return len(e), (int(e[0]) if len(e) else -1)


def heldout_terms(ua, geno, folds, f, q, p, floor):
    """t' = max(t, floor) of every observed copy of fold f, in i, l, a order, and which of them were floored (t < floor or NaN).
    q: [I][K] or [K]; p: [K][T]."""
    I, L, pl = geno.shape
    toff = np.concatenate(([0], np.cumsum(ua)))[:-1]
    sel = (folds == f)[:, :, None] & (geno != MISSING)
    ii, ll, _ = np.nonzero(sel)
    cols = toff[ll] + geno[sel].astype(np.int64)
    qq = q[ii] if q.ndim == 2 else np.broadcast_to(q, (len(ii), q.shape[0]))
    t = np.einsum("nk,kn->n", qq, p[:, cols]) if len(ii) else np.zeros(0)
    floored = ~(t >= floor)
    return np.where(floored, floor, t), floored


def heldout_score(ua, geno, folds, f, q, p, floor):
    """(exact sum of log t', copies, floored copies, sum |log t'|)"""
    tp, floored = heldout_terms(ua, geno, folds, f, q, p, floor)
    logs = np.log(tp)
    return math.fsum(logs), len(tp), int(floored.sum()), math.fsum(np.abs(logs))
