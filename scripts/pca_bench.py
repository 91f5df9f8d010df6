#!/usr/bin/env python3
"""Time of mchip_bed_pca_apply and mchip_bed_pca, per kernel, with the achieved FP64 matrix rate and, beside it, the rate of
k_resid_gram -- the other FP64-MFMA kernel of the library -- measured in the same run (profiles/pca.txt).

    python scripts/pca_bench.py [-I 10000] [-L 100000] [--rounds 10] [--resid-L 20000] [--kernels]

Records: three populations drawn from the Balding-Nichols beta at F_ST = 0.1 around ancestral frequencies uniform in (0.1, 0.9),
individuals round-robin, 2 % of the calls missing; 4096 variants are drawn and repeated up to L (the kernels' time does not depend
on what the bits are).
Call times: wall seconds (time.perf_counter) around one call, which ends in a device synchronise and includes the records going up
and the arrays coming back to pageable memory; one warm-up, then `rounds` repeats, [median, smallest, largest].  One
mchip_bed_pca_apply at n_vec = 16, 32 and 64, and one whole mchip_bed_pca with n_pc = 10, 10 extra vectors, 200 iterations at most and
tolerance 1e-6 -- what --pca 10 runs -- once after a warm-up of 2 iterations.
--kernels: the applies and one mchip_residual_products (I individuals x --resid-L biallelic loci, K = 8) once more as a child under
`rocprofv3 --kernel-trace --stats`: the mean time of a launch of every kernel, and from it the rate -- 2 I L b flops for each of
k_pca_project and k_pca_expand (b = the padded column count; what the definition needs, the padding rows and columns not counted),
and for k_resid_gram<true> two flops per multiply-add over the tiles on and above the diagonal, as scripts/resid_bench.py counts it.
The profiler's clock is the device's; the profiled run is not the one the call times come from.
One JSON line on stdout."""
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

PEAK_TF = 78.6          # FP64 vector = FP64 matrix peak of the MI355X
DRAWN = 4096
N_VECS = (16, 32, 64)
TILE = 64


def records(I, L):
    import bedfiles
    rng = np.random.default_rng(20261021)
    n = min(L, DRAWN)
    anc = rng.uniform(0.1, 0.9, size=n)
    freq = rng.beta(anc * 9.0, (1 - anc) * 9.0, size=(3, n))          # (1 - F) / F = 9 at F_ST = 0.1
    codes = np.array([bedfiles.HOM1, bedfiles.HET, bedfiles.HOM2], dtype=np.uint8)[rng.binomial(2, freq[np.arange(I) % 3])]
    codes[rng.random((I, n)) < 0.02] = bedfiles.MISS
    bed = bedfiles.pack(codes)
    return np.ascontiguousarray(np.tile(bed, (-(-L // n), 1))[:L])


def spread(secs):
    return [round(float(v), 4) for v in (np.median(secs), min(secs), max(secs))]


def applies(ctx, I, bed, rounds):
    out = {}
    rng = np.random.default_rng(1)
    for n_vec in N_VECS:
        x = rng.standard_normal((I, n_vec))
        secs = []
        for n in range(rounds + 1):                  # (the first is the warm-up)
            t0 = time.perf_counter()
            ctx.bed_pca_apply(I, bed, x, w=False, scale=False)
            if n:
                secs.append(time.perf_counter() - t0)
        out["apply_%d_s" % n_vec] = spread(secs)
    return out


def whole(ctx, I, bed):
    ctx.bed_pca(I, bed, 10, n_extra=10, max_iter=2, tol=1e-6)
    t0 = time.perf_counter()
    r = ctx.bed_pca(I, bed, 10, n_extra=10, max_iter=200, tol=1e-6)
    secs = time.perf_counter() - t0
    return {"pca_10_s": round(secs, 3), "pca_10_iterations": r["n_iter"], "pca_10_components_converged": int((r["residuals"] <= 1e-6).sum()),
            "pca_10_largest_residual": float(r["residuals"].max()), "n_used": r["n_used"]}


def resid(I, L, K=8):
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
    ctx.residual_products(0)
    ctx.close()


def kernel_times(a):
    """mean milliseconds of a launch of every kernel named below, from a child run under rocprofv3"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "r", "--", sys.executable,
               os.path.abspath(__file__), "-I", str(a.I), "-L", str(a.L), "--rounds", "2", "--resid-L", str(a.resid_L), "--child"]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if res.returncode:
            raise RuntimeError("rocprofv3 run failed: " + res.stderr[-2000:])
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = (row.get("Name") or row.get("KernelName") or "").replace("(bool)1", "true").replace("(bool)0", "false")
                calls = float(row.get("Calls") or 0)
                if not calls:
                    continue
                for key in ["k_pca_scale", "k_pca_fold", "k_resid_gram<true>"] + ["k_pca_%s<%d>" % (k, nb) for k in ("project", "expand") for nb in (1, 2, 4)]:
                    if key in name:
                        out[key + "_ms"] = round(float(row["TotalDurationNs"]) * 1e-6 / calls, 4)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-I", type=int, default=10000)
    ap.add_argument("-L", type=int, default=100000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--resid-L", type=int, default=20000)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    from multiclust_amd import hip
    bed = records(a.I, a.L)
    ctx = hip.Context(0)
    line = {"I": a.I, "L": a.L, "record_megabytes": round(a.L * ((a.I + 3) // 4) / 1e6, 1), "clock": "time.perf_counter around a call that ends in a synchronise"}
    line.update(applies(ctx, a.I, bed, a.rounds))
    if a.child:
        ctx.close()
        resid(a.I, a.resid_L)
        return
    line.update(whole(ctx, a.I, bed))
    ctx.close()
    if a.kernels:
        k = kernel_times(a)
        line.update(k)
        for nb in (1, 2, 4):
            gflop = 2.0 * a.I * a.L * 16 * nb * 1e-9
            for which in ("project", "expand"):
                ms = k.get("k_pca_%s<%d>_ms" % (which, nb))
                if ms:
                    line["%s_%d_tflops" % (which, 16 * nb)] = round(gflop / ms, 2)          # (GFLOP / ms = TFLOP / s)
        if k.get("k_resid_gram<true>_ms"):
            nt = (a.I + TILE - 1) // TILE
            n_chunks = -(-2 * a.resid_L // 512)                                             # launches of the G kernel in one call
            gflop = 2.0 * (nt * (nt + 1) // 2) * TILE * TILE * (2 * a.resid_L) * 1e-9
            line["resid_gram_tflops"] = round(gflop / (k["k_resid_gram<true>_ms"] * n_chunks), 2)
            line["resid_L"] = a.resid_L
        line["fp64_peak_tflops"] = PEAK_TF
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
