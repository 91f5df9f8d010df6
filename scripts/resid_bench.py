#!/usr/bin/env python3
"""Time of mchip_residual_products beside the S-side pass of the same process (profiles/resid.txt).

    python scripts/resid_bench.py [-I 1000 4000 10000] [-L 100000] [-K 8] [--rounds 3] [--kernels]

A diploid biallelic data set of uniformly drawn alleles with 2 % of the copies missing (so the pairwise-complete denominators are
formed by the product kernel, not taken from the diagonal) and drawn parameters.  Per I: the call is timed on the host (wall seconds
around the entry point: per chunk of 512 columns the three launches, at the end the mirror and two I x I arrays of doubles back to
pageable memory), `rounds` times, the smallest kept.  S-side pass = kernel kind [1] of mchip_profile_end over five EM steps of the
same data set.  The arithmetic to hold the figures against: I^2 T + 2 I^2 L multiply-adds (padded I: a multiple of 64).
--kernels: the same run once more as a child under `rocprofv3 --kernel-trace --stats`, and from its kernel statistics the summed
time per call of k_resid_tile, k_resid_gram<true> (G) and k_resid_gram<false> (D), and the FP64 rate of the G kernel -- two flops per
multiply-add over the tiles on and above the diagonal, which is what it executes -- as a share of the 78.6 TF/s vector peak.
One JSON line per I on stdout."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from multiclust_amd import hip            # noqa: E402
from synth import random_params      # noqa: E402

PEAK_TF = 78.6
TILE = 64


def one(I, L, K, rounds):
    ctx = hip.Context(0)
    rng = np.random.default_rng(20261019)
    geno = rng.integers(0, 2, size=(I, L, 2), dtype=np.uint8)
    geno[rng.integers(0, 50, size=(I, L, 2), dtype=np.uint8) == 0] = 0xFF
    ua = np.full(L, 2, np.int32)
    ctx.set_genotypes(ua, geno)
    del geno
    q, p = random_params(I, ua, K, seed=3)
    ctx.set_model(K, admixture=1)
    ctx.set_q(0, q)
    ctx.set_p(0, p)
    ctx.em_step(0, 1)                            # warm-up
    ctx.profile_begin()
    for _ in range(5):
        ctx.em_step(0, 1)
    _, kernel_ms, launches = ctx.profile_end()
    best = np.inf
    for n in range(rounds + 1):                  # (the first is the warm-up)
        t0 = time.perf_counter()
        G, D = ctx.residual_products(0)
        if n:
            best = min(best, time.perf_counter() - t0)
    with np.errstate(invalid="ignore", divide="ignore"):
        cor = G / np.sqrt(D * D.T)
    off = cor[~np.eye(I, dtype=bool)]
    ctx.close()
    return {"I": I, "L": L, "K": K, "call_ms": round(best * 1e3, 2), "calls": rounds + 1,
            "s_side_pass_ms": round(kernel_ms[1] / max(launches[1], 1), 4), "mean_cor": float(np.nanmean(off))}


def kernel_times(I, L, K, rounds):
    """per call: the summed milliseconds of each of the three kernels, from a child run under rocprofv3"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "r", "--", sys.executable,
               os.path.abspath(__file__), "-I", str(I), "-L", str(L), "-K", str(K), "--rounds", str(rounds)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if res.returncode:
            raise RuntimeError("rocprofv3 run failed: " + res.stderr[-2000:])
        calls = json.loads(res.stdout.strip().split("\n")[-1])["calls"]
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get("Name") or row.get("KernelName") or ""
                for key, tag in (("k_resid_tile", "tile_ms"), ("k_resid_gram<true>", "gram_ms"), ("k_resid_gram<false>", "norms_ms")):
                    if key in name.replace("(bool)1", "true").replace("(bool)0", "false"):
                        out[tag] = out.get(tag, 0.0) + float(row["TotalDurationNs"]) * 1e-6 / calls
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-I", type=int, nargs="+", default=[1000, 4000, 10000])
    ap.add_argument("-L", type=int, default=100000)
    ap.add_argument("-K", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    for I in a.I:
        line = one(I, a.L, a.K, a.rounds)
        nt = (I + TILE - 1) // TILE
        line["gram_gflop"] = round(2.0 * (nt * (nt + 1) // 2) * TILE * TILE * (2 * a.L) * 1e-9, 1)
        if a.kernels:
            line.update({k: round(v, 3) for k, v in kernel_times(I, a.L, a.K, a.rounds).items()})
            if line.get("gram_ms"):
                line["gram_share_of_fp64_peak"] = round(line["gram_gflop"] / line["gram_ms"] / PEAK_TF, 4)   # (GFLOP / ms = TFLOP / s)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
