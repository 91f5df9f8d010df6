"""Times of the cross-validation passes beside the EM passes of the same process (profiles/cv_passes.txt):
    python scripts/cv_passes.py [I L K F]          default 10000 100000 8 5 (config-3 size)
The data set is generated on the device (mchip_simulate_genotypes).  "stream ms" is mchip_profile_begin/end's total: HIP events
on the context's stream around the call, host work between the launches included; "wall ms" is the host's clock around the call."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from multiclust_amd import hip          # noqa: E402
from synth import random_params         # noqa: E402


def timed(ctx, fn):
    ctx.synchronize()
    ctx.profile_begin()
    t0 = time.perf_counter()
    out = fn()
    wall = (time.perf_counter() - t0) * 1e3
    total, _, _ = ctx.profile_end()
    return out, total, wall


def main():
    I, L, K, F = [int(v) for v in sys.argv[1:5]] if len(sys.argv) >= 5 else (10000, 100000, 8, 5)
    rng = np.random.default_rng(3)
    ua = rng.integers(2, 5, size=L).astype(np.int32)
    q, p = random_params(I, ua, K, seed=1)
    window = rng.integers(0, 1 << 32, 31, dtype=np.uint64).astype(np.uint32)
    ctx = hip.Context(0)
    print("%s, %d CUs" % ctx.device_info()[:2])
    ctx.simulate_genotypes(I, L, 2, ua, window, K, q, p)
    ctx.set_model(K)
    ctx.set_q(0, q)
    ctx.set_p(0, p)
    print("data set: %d x %d, diploid, 2-4 alleles, K = %d, %d folds; genotype %.2f GB, folds %.2f GB" % (I, L, K, F, I * L * 2 / 1e9, I * L / 1e9))
    ctx.em_step(0, 0)
    ctx.profile_begin()
    for _ in range(3):
        ctx.em_step(0, 0)
    _, km, kl = ctx.profile_end()
    print("EM step of the same process: column pass %.3f ms, S-side (individual) pass %.3f ms per launch" % (km[0] / max(kl[0], 1), km[1] / max(kl[1], 1)))
    _, total, wall = timed(ctx, lambda: ctx.cv_draw_folds(window, F))
    print("mchip_cv_draw_folds:              stream %9.3f ms   wall %9.3f ms" % (total, wall))
    for rep in range(2):
        _, total, wall = timed(ctx, lambda: ctx.cv_hold_out(rep))
        print("mchip_cv_hold_out(%d)%s  stream %9.3f ms   wall %9.3f ms" % (rep, " (first: saves the full set)" if rep == 0 else "                            ", total, wall))
    ctx.em_step(0, 0)
    for rep in range(4):
        (s, n, nf), total, wall = timed(ctx, lambda: ctx.cv_heldout_loglik(0, 1.0 / (2 * I + 1)))
        bytes_read = I * L * 3 / F + I * L          # fold bytes of every genotype, genotype bytes of the fold's
        print("mchip_cv_heldout_loglik (run %d):  stream %9.3f ms   wall %9.3f ms   sum %.6f over %d copies, %d floored;  %.2f GB if every fold byte and the fold's genotype bytes are read once: %.0f GB/s"
              % (rep, total, wall, s, n, nf, bytes_read / 1e9, bytes_read / 1e9 / (total / 1e3)))
    _, total, wall = timed(ctx, lambda: ctx.cv_hold_out(-1))
    print("mchip_cv_hold_out(-1)             stream %9.3f ms   wall %9.3f ms" % (total, wall))
    ctx.close()


if __name__ == "__main__":
    main()
