#!/usr/bin/env python3
"""Time of mchip_impute_missing beside the S-side pass of the same process (profiles/impute.txt).

    python scripts/impute_bench.py [-I 10000 -L 100000 -K 8] [--missing 0.01 0.05 0.2] [--rounds 3]

A diploid biallelic data set of uniformly drawn alleles (the pass does not care how the alleles are distributed, and the clustered
generator of tests/synth.py takes minutes at this size) with the given share of the copies missing, the phantom slot at every locus
that has a missing copy, and drawn parameters.  Per share: the call is timed on the host (wall seconds around the entry point: the
unlayout into the scratch, the kernel, the reduction, the copy of I L ploidy bytes back) without the confidences, `rounds` times,
the smallest kept.  S-side pass = kernel kind [1] of mchip_profile_end over five EM steps of the same data set.
One JSON line per share on stdout."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from multiclust_amd import hip            # noqa: E402
from synth import random_params      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-I", type=int, default=10000)
    ap.add_argument("-L", type=int, default=100000)
    ap.add_argument("-K", type=int, default=8)
    ap.add_argument("--missing", type=float, nargs="+", default=[0.01, 0.05, 0.2])
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    ctx = hip.Context(0)
    for share in a.missing:
        rng = np.random.default_rng(20261018)
        geno = rng.integers(0, 2, size=(a.I, a.L, 2), dtype=np.uint8)
        for i0 in range(0, a.I, 500):                                # (in slices: a mask of the whole set is 8 GB of doubles)
            geno[i0:i0 + 500][rng.random(geno[i0:i0 + 500].shape, dtype=np.float32) < share] = 0xFF
        n_real = np.full(a.L, 2, np.int32)
        ua = (n_real + (geno == 0xFF).any(axis=(0, 2))).astype(np.int32)
        q, p = random_params(a.I, ua, a.K, seed=3)
        ctx.set_genotypes(ua, geno)
        ctx.set_model(a.K, admixture=1)
        ctx.set_q(0, q)
        ctx.set_p(0, p)
        ctx.em_step(0, 1)                        # warm-up
        ctx.profile_begin()
        for _ in range(5):
            ctx.em_step(0, 1)
        _, kernel_ms, launches = ctx.profile_end()
        out = (np.empty(geno.shape, dtype=np.uint8), None)
        res = ctx.impute_missing(0, n_real, conf=False, out=out)      # warm-up
        best = np.inf
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            res = ctx.impute_missing(0, n_real, conf=False, out=out)
            best = min(best, time.perf_counter() - t0)
        print(json.dumps({"I": a.I, "L": a.L, "K": a.K, "missing": share, "call_ms": round(best * 1e3, 3),
                          "copies_filled": res[2], "copies_left": res[3], "genotypes_filled": res[4],
                          "s_side_pass_ms": round(kernel_ms[1] / max(launches[1], 1), 4)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
