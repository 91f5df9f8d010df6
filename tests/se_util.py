"""The bootstrap over loci on the CPU (TEST INFRASTRUCTURE): the data sets, the numpy forms of the selection, of the stream
convention and of the accumulation that tests/test_gpu_resample.py and tests/test_gpu_se*.py compare mchip_resample_loci and
mc_locus_bootstrap with."""
import ctypes as C

import numpy as np

import cv_util as cu
from multiclust_amd import hip

MISSING = cu.MISSING


def resample_dataset(I, L, ploidy, seed):
    """cv_util.cv_dataset (a 35-allele locus 0, locus 1 without a missing call, phantom slots, 2 % missing) in which individual 3
    has no observed copy at every third locus from locus 2 on; a locus that gains its first missing copy that way gains the
    phantom slot the reader would give it"""
    ua, geno = cu.cv_dataset(I, L, ploidy, seed)
    before = (geno == MISSING).any(axis=(0, 2))
    geno[3, 2::3, :] = MISSING
    after = (geno == MISSING).any(axis=(0, 2))
    assert not after[1] and (geno[3] != MISSING).any()
    return (ua + (after & ~before)).astype(np.int32), geno


def with_phantoms(ua, before, after):
    """ua with the phantom slot the reader gives a locus that has a missing copy, for the loci that gained their first one between
    the genotypes `before` and `after`"""
    had, has = (before == MISSING).any(axis=(0, 2)), (after == MISSING).any(axis=(0, 2))
    return (ua + (has & ~had)).astype(np.int32)


def toff(ua):
    return np.concatenate(([0], np.cumsum(ua))).astype(np.int64)


def gather_columns(ua, src):
    """columns of the base's [K][T] table that make up the selection's, in its order"""
    t = toff(ua)
    return np.concatenate([np.arange(t[l], t[l + 1]) for l in src]) if len(src) else np.zeros(0, np.int64)


def data_counts(geno):
    """(cells (i, allele column) with a count above zero, observed copies)"""
    g = np.sort(geno, axis=2)
    obs = g != MISSING
    distinct = obs.copy()
    distinct[:, :, 1:] &= g[:, :, 1:] != g[:, :, :-1]
    return int(distinct.sum()), int(obs.sum())


def locus_lists(draws, L, block, n_replicates):
    """the stream convention of mc_locus_bootstrap (mc_host.h) on the draws of rand(): nb = ceil(L / block) blocks; replicate r
    takes the next nb draws, each draw b = rand() % nb appends the loci of block b"""
    nb = -(-L // block)
    draws = np.asarray(draws, dtype=np.int64)
    assert len(draws) >= nb * n_replicates
    out = []
    for r in range(n_replicates):
        b = draws[r * nb:(r + 1) * nb] % nb
        out.append(np.concatenate([np.arange(x * block, min(L, (x + 1) * block)) for x in b]).astype(np.int32))
    return out


class Welford:
    """n++; d = x - mean; mean += d / n; M2 += d (x - mean), per entry, NaN entries skipped -- numpy float64 operations are the
    IEEE operations of the C loop, one rounding each, in the same order"""

    def __init__(self, shape):
        self.mean, self.m2, self.n = np.zeros(shape), np.zeros(shape), np.zeros(shape, dtype=np.int32)

    def add(self, x):
        ok = ~np.isnan(x)
        n = self.n[ok] + 1
        d = x[ok] - self.mean[ok]
        mean = self.mean[ok] + d / n
        self.m2[ok] = self.m2[ok] + d * (x[ok] - mean)
        self.mean[ok], self.n[ok] = mean, n

    def result(self):
        mean = np.where(self.n >= 1, self.mean, np.nan)
        with np.errstate(invalid="ignore", divide="ignore"):
            se = np.where(self.n >= 2, np.sqrt(self.m2 / (self.n - 1)), np.nan)
        return mean, se, self.n


def summary(se):
    """(mean, max) over the entries that have a standard error, added up in index order as the C loop does"""
    v = se.ravel()[~np.isnan(se.ravel())]
    total = 0.0
    for x in v:
        total += float(x)
    return (total / len(v), float(v.max())) if len(v) else (float("nan"), float("nan"))


def device_of(fit):
    """the model's own context, seen through the C-ABI wrappers"""
    ctx = hip.Context.__new__(hip.Context)
    ctx.lib = hip.load()
    ctx.h = C.c_void_p(fit.mod.dev)
    ctx.I, ctx.L, ctx.ploidy = fit.geno.shape
    ctx.T, ctx.K, ctx.indiv_q = fit.T, fit.K, fit.indiv_q
    ctx._ua, ctx._rs_ua = fit.ua.copy(), None
    ctx.close = lambda: None                                        # the Fit owns it
    return ctx


def cpu_locus_bootstrap(ua, geno, K, seed, n_replicates, block, accel_scheme=3):
    """mc_locus_bootstrap's definition on the CPU, admixture model with individual mixing proportions: the oracle's EM
    (tests/oracle_bind.py) from the random allele partition of srand(seed), then every replicate of the stream convention fitted by
    the oracle from that estimate; returns (mean, se, count)"""
    import oracle_bind as ob
    import rand_window as rw
    I, L, pl = geno.shape
    opt = ob.make_options(accel_scheme=accel_scheme, fused=1)
    full = ob.Model(ob.Data(I, L, pl, ua, geno), opt, K)
    full.init_random(seed)
    full.em()
    assert full.fatal == 0
    q, p = full.q(full.pindex).copy(), full.p(full.pindex).copy()
    nb = -(-L // block)
    acc = Welford(q.shape)
    for src in locus_lists(rw.draws(ob.glibc_window(seed)[0], nb * n_replicates), L, block, n_replicates):
        rep = ob.Model(ob.Data(I, len(src), pl, ua[src], np.ascontiguousarray(geno[:, src, :])), opt, K)
        rep.q(0)[...] = q
        rep.p(0)[...] = p[:, gather_columns(ua, src)]
        rep.em()
        assert rep.fatal == 0
        acc.add(rep.q(rep.pindex).copy())
    return acc.result()
