#!/usr/bin/env python3
"""Time of mchip_fit_q_rows beside the S-side pass of the same process (profiles/query_fit.txt).

    python scripts/query_fit_bench.py [-I 10000 -L 100000 -K 8] [--rows 16 256 4096] [--rounds 3]

A synthetic diploid biallelic data set (tests/synth.py) and drawn parameters.  Per n_rows: the first n_rows individuals are fitted
from 1/K with both errors 0, so every row runs exactly max_iter iterations; the call is timed on the host (wall seconds around the
entry point: allocation, the gather launch, the fit launch, the copies back) with max_iter = 10 and 30, `rounds` times each in
alternation, the smaller of each kept.  launch = the 30-iteration call; row-iteration = (t30 - t10) / 20 / n_rows, which leaves
the call's fixed part out.  S-side pass = kernel kind [1] of mchip_profile_end over five EM steps of the whole data set.
One JSON line per n_rows on stdout."""
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
from synth import make_dataset, random_params      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-I", type=int, default=10000)
    ap.add_argument("-L", type=int, default=100000)
    ap.add_argument("-K", type=int, default=8)
    ap.add_argument("--rows", type=int, nargs="+", default=[16, 256, 4096])
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    ua, geno = make_dataset(a.I, a.L, a.K, ploidy=2, seed=20261017)
    q, p = random_params(a.I, ua, a.K, seed=3)
    ctx = hip.Context(0)
    ctx.set_genotypes(ua, geno)
    ctx.set_model(a.K, admixture=1)
    ctx.set_q(0, q)
    ctx.set_p(0, p)
    ctx.em_step(0, 1)                        # warm-up
    ctx.profile_begin()
    for _ in range(5):
        ctx.em_step(0, 1)
    _, kernel_ms, launches = ctx.profile_end()
    s_side_ms = kernel_ms[1] / max(launches[1], 1)
    for n in a.rows:
        n = min(n, a.I)
        rows = np.arange(n, dtype=np.int32)
        ctx.fit_q_rows(0, rows, 2)           # warm-up
        best = {10: np.inf, 30: np.inf}
        for _ in range(a.rounds):
            for it in (10, 30):
                t0 = time.perf_counter()
                out = ctx.fit_q_rows(0, rows, it)
                best[it] = min(best[it], time.perf_counter() - t0)
                assert (out[2] == it).all()
        per_iter_ms = (best[30] - best[10]) / 20 * 1e3
        print(json.dumps({"I": a.I, "L": a.L, "K": a.K, "n_rows": n, "launch_30_iterations_ms": round(best[30] * 1e3, 3),
                          "launch_10_iterations_ms": round(best[10] * 1e3, 3), "iteration_all_rows_ms": round(per_iter_ms, 4),
                          "row_iteration_us": round(per_iter_ms * 1e3 / n, 4), "s_side_pass_ms": round(s_side_ms, 4)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
