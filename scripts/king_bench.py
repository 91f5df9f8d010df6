#!/usr/bin/env python3
"""Time of mchip_bed_king, the KING-robust kinships of all pairs of individuals (profiles/king.txt).

    python scripts/king_bench.py [-I 10000] [-L 100000] [--rounds 2] [--host-rows 2] [--kernels]

Records of uniformly drawn bytes (every code a quarter of the calls, so a quarter missing: the counting does not depend on what
the bits are).  The unit the times are held against is the word pair: one 64-bit word (64 variants) of one individual's bit planes
met with the same word of another's, I * I * ceil(L / 64) of them -- what the kernel's inner loop handles with five population
counts.
Device: the whole matrix in slabs of 1024 rows, as the host calls it (multiclust_amd/host/mc_king.c); wall seconds around the
calls, which end in a synchronise and include, per slab, the records going up, their turning into planes, and the kinships and
counts coming back to pageable memory; one warm-up, then `rounds` repeats, the smallest kept.
Host: tests/king_host_driver.c (the definition, one variant at a time; gcc -O2) on the first --host-rows rows against all
individuals, wall seconds of the whole program (it also reads the records and writes its rows), scaled by word pairs.
--kernels: the device part once more as a child under `rocprofv3 --kernel-trace --stats`: the summed times of k_king_planes,
k_king_pairs and k_king_phi per matrix.
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

SLAB = 1024
KERNELS = ("k_king_planes", "k_king_pairs", "k_king_phi")


def records(I, L):
    return np.random.default_rng(20261020).integers(0, 256, size=(L, (I + 3) // 4), dtype=np.uint8)


def word_pairs(I, L, rows=None):
    return (I if rows is None else rows) * I * ((L + 63) // 64)


def device(I, L, rounds):
    from multiclust_amd import hip
    bed = records(I, L)
    ctx = hip.Context(0)
    best, finite = np.inf, 0
    for n in range(rounds + 1):                  # (the first is the warm-up)
        t0 = time.perf_counter()
        finite = 0
        for i0 in range(0, I, SLAB):
            phi, cnt = ctx.bed_king(I, bed, i0=i0, n_rows=min(SLAB, I - i0))
            finite += int(np.isfinite(phi).sum())
        if n:
            best = min(best, time.perf_counter() - t0)
    ctx.close()
    return best, finite


def host_restatement(I, L, rows):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "king_host")
        hostdir = os.path.join(ROOT, "multiclust_amd", "host")
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-I" + os.path.join(ROOT, "include"), "-I" + hostdir, "-o", exe,
                        os.path.join(ROOT, "tests", "king_host_driver.c"), os.path.join(hostdir, "mc_king.c"), "-lm"], check=True)
        bed = records(I, L)
        bed.tofile(os.path.join(d, "bed"))
        t0 = time.perf_counter()
        subprocess.run([exe, "band", str(I), str(L), str(bed.shape[1]), "0", str(rows), "bed", "phi", "counts"], cwd=d, check=True)
        return time.perf_counter() - t0, word_pairs(I, L, rows)


def kernel_times(I, L, rounds):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "r", "--", sys.executable,
               os.path.abspath(__file__), "-I", str(I), "-L", str(L), "--rounds", str(rounds), "--host-rows", "0"]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if res.returncode:
            raise RuntimeError("rocprofv3 run failed: " + res.stderr[-2000:])
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get("Name") or row.get("KernelName") or ""
                for key in KERNELS:
                    if key in name:
                        out[key + "_ms_per_matrix"] = out.get(key + "_ms_per_matrix", 0.0) + float(row["TotalDurationNs"]) * 1e-6 / (rounds + 1)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-I", type=int, default=10000)
    ap.add_argument("-L", type=int, default=100000)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--host-rows", type=int, default=2)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    sec, finite = device(a.I, a.L, a.rounds)
    wp = word_pairs(a.I, a.L)
    line = {"I": a.I, "L": a.L, "slab": SLAB, "device_matrix_s": round(sec, 4), "word_pairs": wp, "device_word_pairs_per_s": round(wp / sec, 1),
            "finite_phi": finite}
    if a.host_rows > 0:
        hsec, hwp = host_restatement(a.I, a.L, min(a.host_rows, a.I))
        line.update(host_rows=min(a.host_rows, a.I), host_rows_s=round(hsec, 4), host_word_pairs=hwp, host_word_pairs_per_s=round(hwp / hsec, 1),
                    host_s_for_the_whole_matrix=round(hsec * wp / hwp, 1))
    if a.kernels:
        line.update({k: round(v, 3) for k, v in kernel_times(a.I, a.L, a.rounds).items()})
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
