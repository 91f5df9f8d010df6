#!/usr/bin/env python3
"""Time of mchip_bed_qc, the genotype counts of both axes and the Hardy-Weinberg exact test of every variant (profiles/qc.txt;
DESIGN.md section 7).

    python scripts/qc_bench.py [-I 10000] [-L 100000] [--rounds 20] [--kernels]

Records of Hardy-Weinberg genotypes at minor-allele frequencies drawn uniformly from (0.005, 0.5), one call in a hundred missing:
the counting does not depend on what the bits are, but the exact test walks r / 2 weights twice, r the copies of the rarer allele,
so its time is that of the allele-count distribution.  4096 variants are drawn and repeated up to L.
Device: one call with all three outputs, and one without hwe_p, as wall seconds around the call, which ends in a synchronise and
includes the records going up and the arrays coming back to pageable memory; one warm-up, then `rounds` repeats, the median kept and
the smallest and largest shown.
--kernels: the full call once more as a child under `rocprofv3 --kernel-trace --stats`: the summed times of the four kernels per call.
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

KERNELS = ("k_qc_mask", "k_qc_variants", "k_qc_individuals", "k_qc_hwe")
DRAWN = 4096


def records(I, L):
    import bedfiles
    rng = np.random.default_rng(20261021)
    n = min(L, DRAWN)
    f = rng.uniform(0.005, 0.5, size=n)
    a2 = rng.binomial(2, f, size=(I, n))
    codes = np.array([bedfiles.HOM1, bedfiles.HET, bedfiles.HOM2], dtype=np.uint8)[a2]
    codes[rng.random((I, n)) < 0.01] = bedfiles.MISS
    bed = bedfiles.pack(codes)
    return np.ascontiguousarray(np.tile(bed, (-(-L // n), 1))[:L])


def device(I, L, rounds):
    from multiclust_amd import hip
    bed = records(I, L)
    ctx = hip.Context(0)
    out = {}
    for name, hwe in (("all_outputs", True), ("without_hwe_p", False)):
        secs = []
        for n in range(rounds + 1):                  # (the first is the warm-up)
            t0 = time.perf_counter()
            ind, var, p = ctx.bed_qc(I, bed, hwe=hwe)
            if n:
                secs.append(time.perf_counter() - t0)
        out[name + "_s"] = [round(float(x), 4) for x in (np.median(secs), min(secs), max(secs))]
    out["mean_minor_allele_copies"] = round(float(np.minimum(2 * var[:, 0] + var[:, 2], 2 * var[:, 3] + var[:, 2]).mean()), 1)
    ctx.close()
    return out


def kernel_times(I, L, rounds):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "r", "--", sys.executable,
               os.path.abspath(__file__), "-I", str(I), "-L", str(L), "--rounds", str(rounds)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if res.returncode:
            raise RuntimeError("rocprofv3 run failed: " + res.stderr[-2000:])
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get("Name") or row.get("KernelName") or ""
                for key in KERNELS:
                    if key in name:
                        calls = 2 * (rounds + 1) if key != "k_qc_hwe" else rounds + 1
                        out[key + "_ms_per_call"] = out.get(key + "_ms_per_call", 0.0) + float(row["TotalDurationNs"]) * 1e-6 / calls
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-I", type=int, default=10000)
    ap.add_argument("-L", type=int, default=100000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    line = {"I": a.I, "L": a.L, "record_megabytes": round(a.L * ((a.I + 3) // 4) / 1e6, 1)}
    line.update(device(a.I, a.L, a.rounds))
    if a.kernels:
        line.update({k: round(v, 3) for k, v in kernel_times(a.I, a.L, a.rounds).items()})
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
