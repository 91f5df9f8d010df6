#!/usr/bin/env python3
"""Time of mchip_kinship_products, its two products of a chunk as one launch against two launches, beside
mchip_residual_products of the same process (profiles/kinship.txt).

    python scripts/kinship_bench.py [-I 1000 4000 10000] [-L 100000] [-K 8] [--rounds 3]

A diploid biallelic data set of uniformly drawn alleles with 2 % of the copies missing and drawn parameters, as scripts/resid_bench.py
has it.  Per I and per form a process of its own (`--child`), started one after the other, each under its own time limit: the form
is an environment knob (MCHIP_KIN_TWO_LAUNCHES) read when the context is made, and a fresh process starts every measurement from the
same state of the device.  In the child the two entry points are timed on the host (wall seconds around the call: per chunk of 512
columns the tile pass and the products, at the end the mirrors and two I x I arrays of doubles back to pageable memory), `rounds`
times after a warm-up, the smallest kept.  The digest is the sum of the bits of both arrays: the two forms must print the same one.
The arithmetic to hold the figures against: 2 I^2 T multiply-adds, the tiles below the diagonal skipped (padded I: a multiple of 64).
One JSON line per I and form on stdout."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KNOB = "MCHIP_KIN_TWO_LAUNCHES"
TILE = 64


def child(I, L, K, rounds):
    from multiclust_amd import hip
    from synth import random_params
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
    best = {"kinship": np.inf, "resid": np.inf}
    for n in range(rounds + 1):                  # (the first is the warm-up)
        t0 = time.perf_counter()
        G, V = ctx.kinship_products(0)
        t1 = time.perf_counter()
        G2, _ = ctx.residual_products(0)
        t2 = time.perf_counter()
        if n:
            best["kinship"] = min(best["kinship"], t1 - t0)
            best["resid"] = min(best["resid"], t2 - t1)
    digest = hashlib.sha256(G.tobytes() + V.tobytes()).hexdigest()[:16]
    with np.errstate(invalid="ignore", divide="ignore"):
        phi = G / V
    nt = (I + TILE - 1) // TILE
    ctx.close()
    return {"I": I, "L": L, "K": K, "form": "two launches" if os.environ.get(KNOB) else "one launch", "kinship_call_ms": round(best["kinship"] * 1e3, 2),
            "resid_call_ms": round(best["resid"] * 1e3, 2), "calls": rounds + 1, "gram_equals_resid": bool(np.array_equal(G, G2)),
            "products_gflop": round(2 * 2.0 * (nt * (nt + 1) // 2) * TILE * TILE * (2 * L) * 1e-9, 1),
            "mean_phi": float(np.nanmean(phi[~np.eye(I, dtype=bool)])), "digest": digest}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-I", type=int, nargs="+", default=[1000, 4000, 10000])
    ap.add_argument("-L", type=int, default=100000)
    ap.add_argument("-K", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=400, help="seconds a child may take")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.I[0], a.L, a.K, a.rounds)), flush=True)
        return 0
    for I in a.I:
        for two in (False, True):
            env = {k: v for k, v in os.environ.items() if k != KNOB}
            if two:
                env[KNOB] = "1"
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "-I", str(I), "-L", str(a.L), "-K", str(a.K),
                                  "--rounds", str(a.rounds)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env,
                                 timeout=a.timeout)
            if res.returncode:                   # nothing more is started on the device after a child that failed
                sys.stderr.write(res.stderr[-2000:])
                return res.returncode
            print(res.stdout.strip().split("\n")[-1], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
