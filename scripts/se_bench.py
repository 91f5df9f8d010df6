"""What a replicate of the bootstrap over loci costs (profiles/locus_bootstrap.txt):
    python scripts/se_bench.py [I L K T]        default 10000 100000 8 300 (config-3 size), SQUAREM-3, at most T iterations per fit
One process: the full-data fit, the three forms of mchip_resample_loci (the first one, which saves the base; a later one; NULL),
one whole replicate step by step as mc_locus_bootstrap runs it, and -- for comparison -- the hold-outs of cross-validation on the
same data.  The data set is drawn on the host: K clusters, 2-4 alleles per locus, every individual in one cluster, no missing
copy.  Every fit stops after T iterations at the latest: with the default tolerance (1e-4 absolute on a log likelihood of 1e9) a
fit at this size runs for tens of thousands of iterations, which says nothing more about what a replicate costs.  "stream ms" is mchip_profile_begin/end's total: HIP events on the context's stream around the call, host work between the
launches included; "wall ms" is the host's clock around the call."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multiclust_amd import hip, host          # noqa: E402


def dataset(I, L, seed, n_clusters=3, chunk=500):
    rng = np.random.default_rng(seed)
    ua = rng.integers(2, 5, size=L).astype(np.int32)
    f = rng.dirichlet(np.full(4, 0.3), size=(n_clusters, L))
    f *= np.arange(4)[None, None, :] < ua[None, :, None]
    f /= f.sum(axis=2, keepdims=True)
    # cumulative thresholds on a byte: allele = number of thresholds the byte reaches
    thr = np.minimum(np.round(np.cumsum(f, axis=2)[:, :, :3] * 256), 255).astype(np.uint8)
    thr[np.broadcast_to(np.arange(3)[None, None, :] >= (ua[None, :, None] - 1), thr.shape)] = 255
    geno = np.empty((I, L, 2), dtype=np.uint8)
    for i0 in range(0, I, chunk):
        i1 = min(I, i0 + chunk)
        t = thr[np.arange(i0, i1) % n_clusters]                       # (n, L, 3)
        r = rng.integers(0, 255, size=(i1 - i0, L, 2), dtype=np.uint8)
        geno[i0:i1] = sum((r >= t[:, :, m, None]).view(np.uint8) for m in range(3))
    assert (geno < ua[None, :, None]).all()
    return ua, geno


def device_of(fit):
    ctx = hip.Context.__new__(hip.Context)
    ctx.lib = hip.load()
    ctx.h = C.c_void_p(fit.mod.dev)
    ctx.I, ctx.L, ctx.ploidy = fit.geno.shape
    ctx.T, ctx.K, ctx.indiv_q = fit.T, fit.K, fit.indiv_q
    ctx._ua, ctx._rs_ua = fit.ua.copy(), None
    ctx.close = lambda: None
    return ctx


def timed(ctx, fn):
    ctx.synchronize()
    ctx.profile_begin()
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    total, _, _ = ctx.profile_end()
    return out, total, wall


def set_model(fit, ctx):
    o = fit.opt
    rc = ctx.lib.mchip_set_model(ctx.h, fit.K, o.admixture, o.eta_constrained, o.do_projection, o.eta_lower_bound, o.p_lower_bound,
                                 o.q if o.accel_scheme else 0)
    assert rc == 0
    ctx.K = fit.K


def gather_columns(ua, src):
    off = np.concatenate(([0], np.cumsum(ua)))
    n = ua[src]
    start = np.repeat(off[src], n)
    within = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    return start + within


def main():
    I, L, K, T = [int(v) for v in sys.argv[1:5]] if len(sys.argv) >= 5 else (10000, 100000, 8, 300)
    seed = 20261017
    t0 = time.perf_counter()
    ua, geno = dataset(I, L, seed, n_clusters=K)
    print("data set: %d x %d, diploid, 2-4 alleles, one cluster per individual, drawn on the host in %.1f s; genotype %.2f GB" % (I, L, time.perf_counter() - t0, geno.size / 1e9), flush=True)
    fit = host.Fit(ua, geno, K, admixture=1, accel_scheme=3, seed=seed, max_iter=T)
    ctx = device_of(fit)
    print("%s, %d CUs; admixture K = %d, SQUAREM-3, at most %d iterations per fit" % (ctx.device_info()[:2] + (K, T)), flush=True)
    t0 = time.perf_counter()
    fit.fit_unit(seed, 0)
    wall = time.perf_counter() - t0
    print("full-data fit (initialisation + mc_em): %d iterations, logL %.3f, %s, %.2f s wall: %.3f ms per iteration" %
          (fit.mod.n_iter, fit.mod.logL, "converged" if fit.mod.converged else "not converged", wall, 1e3 * wall / max(fit.mod.n_iter, 1)), flush=True)
    slot = fit.mod.pindex
    q, p = fit.get_q(slot), fit.get_p(slot)
    lists = fit.locus_lists(3, 1)

    ctx.profile_begin()
    for _ in range(3):
        ctx.em_step(slot, slot)
    _, km, kl = ctx.profile_end()
    print("EM step of the same process: column pass %.3f ms, S-side (individual) pass %.3f ms per launch" % (km[0] / max(kl[0], 1), km[1] / max(kl[1], 1)))

    # cross-validation's hold-outs, for comparison (profiles/cv_passes.txt)
    window = np.random.default_rng(3).integers(0, 1 << 32, 31, dtype=np.uint64).astype(np.uint32)
    ctx.cv_draw_folds(window, 5)
    for f, note in ((0, " (first: saves the full set)"), (1, ""), (-1, "")):
        _, total, wall = timed(ctx, lambda: ctx.cv_hold_out(f))
        print("mchip_cv_hold_out(%d)%-32s stream %9.3f ms   wall %9.3f ms" % (f, note, total, wall))

    # the three forms of a resample
    for r, note in ((0, " (first: saves the base)"), (1, ""), (2, "")):
        _, total, wall = timed(ctx, lambda: ctx.resample_loci(lists[r]))
        print("mchip_resample_loci(list %d)%-26s stream %9.3f ms   wall %9.3f ms   L2 = %d, T2 = %d" % (r, note, total, wall, ctx.L, ctx.T))
    _, total, wall = timed(ctx, lambda: ctx.resample_loci(None))
    print("mchip_resample_loci(NULL)%-29s stream %9.3f ms   wall %9.3f ms" % ("", total, wall), flush=True)

    # one whole replicate, step by step as mc_locus_bootstrap runs it
    src = lists[0]
    t_all = time.perf_counter()
    _, total, wall = timed(ctx, lambda: ctx.resample_loci(src))
    print("replicate: mchip_resample_loci                         stream %9.3f ms   wall %9.3f ms" % (total, wall))
    _, total, wall = timed(ctx, lambda: set_model(fit, ctx))
    print("replicate: mchip_set_model                             stream %9.3f ms   wall %9.3f ms" % (total, wall))
    fit.reset()
    t0 = time.perf_counter()
    p2 = np.ascontiguousarray(p[:, gather_columns(ua, src)])
    host_ms = (time.perf_counter() - t0) * 1e3
    _, total, wall = timed(ctx, lambda: (ctx.set_q(0, q), ctx.set_p(0, p2)))
    print("replicate: set q, p (columns gathered on the host in %.1f ms)   stream %9.3f ms   wall %9.3f ms" % (host_ms, total, wall))
    ua2 = np.ascontiguousarray(ua[src])
    keep = (fit.dat.L, fit.dat.uniquealleles, fit.dat.geno)
    fit.dat.L, fit.dat.uniquealleles, fit.dat.geno = len(src), ua2.ctypes.data, None
    t0 = time.perf_counter()
    fit.em()
    ctx.synchronize()
    fit_ms = (time.perf_counter() - t0) * 1e3
    fit.dat.L, fit.dat.uniquealleles, fit.dat.geno = keep
    print("replicate: mc_em from the warm start                   %d iterations, %s, logL %.3f   wall %9.3f ms: %.3f ms per iteration" %
          (fit.mod.n_iter, "converged" if fit.mod.converged else "not converged", fit.mod.logL, fit_ms, fit_ms / max(fit.mod.n_iter, 1)))
    x = fit.get_q(fit.mod.pindex)
    print("replicate: whole (install, model, parameters, fit, Q)   wall %9.3f ms;  max |q - q_hat| = %.4f" %
          ((time.perf_counter() - t_all) * 1e3, float(np.nanmax(np.abs(x - q)))))
    ctx.resample_loci(None)
    fit.close()


if __name__ == "__main__":
    main()
