#!/usr/bin/env python3
"""Time of mchip_divergence beside the S-side pass of the same process (profiles/divergence.txt).

    python scripts/divergence_bench.py [-I 10000 -L 100000] [-K 8 64] [--rounds 5]

A diploid biallelic data set of uniformly drawn alleles without missing copies (the call reads the allele-frequency table alone:
the data set only gives the S-side pass beside it something to do) and drawn parameters.  Per K: the call is timed on the host
(wall seconds around the entry point: three kernels, the two reductions, K (K + 1) / 2 + 2 L + 2 doubles back), `rounds` times, the
smallest kept.  S-side pass = kernel kind [1] of mchip_profile_end over five EM steps of the same data set.
One JSON line per K on stdout."""
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
    ap.add_argument("-K", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    ctx = hip.Context(0)
    rng = np.random.default_rng(20261019)
    geno = rng.integers(0, 2, size=(a.I, a.L, 2), dtype=np.uint8)
    ua = np.full(a.L, 2, np.int32)
    ctx.set_genotypes(ua, geno)
    for K in a.K:
        q, p = random_params(a.I, ua, K, seed=3)
        w = q.mean(axis=0)
        ctx.set_model(K, admixture=1)
        ctx.set_q(0, q)
        ctx.set_p(0, p)
        ctx.em_step(0, 1)                        # warm-up
        ctx.profile_begin()
        for _ in range(5):
            ctx.em_step(0, 1)
        _, kernel_ms, launches = ctx.profile_end()
        res = ctx.divergence(0, w)               # warm-up
        best = np.inf
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            res = ctx.divergence(0, w)
            best = min(best, time.perf_counter() - t0)
        print(json.dumps({"I": a.I, "L": a.L, "K": K, "table_MB": round(8e-6 * K * int(ua.sum()), 1), "call_ms": round(best * 1e3, 3),
                          "fst_among": res["sum_v"] / res["sum_ht"],
                          "s_side_pass_ms": round(kernel_ms[1] / max(launches[1], 1), 4)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
