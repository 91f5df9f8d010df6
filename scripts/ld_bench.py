#!/usr/bin/env python3
"""Time of mchip_bed_ld_band beside a plain-C restatement of the same band on one core (profiles/ld.txt).

    python scripts/ld_bench.py [-I 10000] [-L 100000] [-W 50] [--rounds 3] [--host-first 200] [--reader] [--kernels]

Records of uniformly drawn bytes (every code a quarter of the calls, so a quarter missing: the counting does not depend on what
the bits are).  The unit both times are held against is the word pair: one 64-bit word (32 individuals) of one variant met with the
same word of another, pairs * ceil(I / 32) of them -- what the kernel's inner loop handles with nine population counts.
Device: the band of all L variants in slabs of 65 536 first variants, as the host calls it (multiclust_amd/host/mc_ld.c); wall
seconds around the calls, which end in a synchronise and include the records going up and the band coming back to pageable memory;
one warm-up, then `rounds` repeats, the smallest kept.
Host: tests/ld_host_driver.c (the definition, one individual at a time; gcc -O2) on the first --host-first variants with the same
window, the seconds it reports for the band alone.
--reader: the same records as a fileset in a temporary directory, read and pruned (t = 0.5) by mc_read_bed in a child process under
MC_READER_TIMING: the seconds of the read and of the pruning (band, greedy walk, compaction) as the reader reports them.
--kernels: the device part once more as a child under `rocprofv3 --kernel-trace --stats`: the summed time of k_ld_band and k_ld_r2.
One JSON line on stdout."""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SLAB = 65536


def records(I, L):
    return np.random.default_rng(20261020).integers(0, 256, size=(L, (I + 3) // 4), dtype=np.uint8)


def word_pairs(I, L, W, first=None):
    first = L if first is None else first
    pairs = sum(min(W, L - 1 - l) for l in range(first))
    return pairs * ((I + 31) // 32)


def device(I, L, W, rounds):
    from multiclust_amd import hip
    bed = records(I, L)
    ctx = hip.Context(0)
    best, finite = np.inf, 0
    for n in range(rounds + 1):                  # (the first is the warm-up)
        t0 = time.perf_counter()
        finite = 0
        for l0 in range(0, L, SLAB):
            r2 = ctx.bed_ld_band(I, bed, l0=l0, n_first=min(SLAB, L - l0), window=W)
            finite += int(np.isfinite(r2).sum())
        if n:
            best = min(best, time.perf_counter() - t0)
    ctx.close()
    return best, finite


def host_restatement(I, L, W, first):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "ld_host")
        hostdir = os.path.join(ROOT, "multiclust_amd", "host")
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-I" + os.path.join(ROOT, "include"), "-I" + hostdir, "-o", exe,
                        os.path.join(ROOT, "tests", "ld_host_driver.c"), os.path.join(hostdir, "mc_ld.c"), "-lm"], check=True)
        n = min(L, first + W)
        bed = records(I, L)[:n]
        bed.tofile(os.path.join(d, "bed"))
        out = subprocess.run([exe, "band", str(I), str(n), str(bed.shape[1]), str(W), "0", str(min(first, n)), "bed", "-"], cwd=d, check=True,
                             stdout=subprocess.PIPE, text=True).stdout
        return float(out), word_pairs(I, n, W, min(first, n))


def reader_child(prefix, W):
    from multiclust_amd import host
    rc, dat = host.read_bed(prefix, decode=False, prune=0.5, prune_window=W)
    print(json.dumps({"rc": rc, "kept": dat["L"] if dat else -1}))


def reader(I, L, W):
    with tempfile.TemporaryDirectory() as d:
        prefix = os.path.join(d, "data")
        with open(prefix + ".bed", "wb") as f:
            f.write(b"\x6c\x1b\x01")
            f.write(records(I, L).tobytes())
        with open(prefix + ".bim", "w") as f:
            f.write("".join("1\tsnp%d\t0\t%d\tA\tC\n" % (l, l + 1) for l in range(L)))
        with open(prefix + ".fam", "w") as f:
            f.write("".join("f i%d 0 0 0 -9\n" % i for i in range(I)))
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--reader-child", prefix, "-W", str(W)], stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, text=True, env=dict(os.environ, MC_READER_TIMING="1"))
        if res.returncode:
            raise RuntimeError("reader run failed: " + res.stderr[-2000:])
        t = {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"INFO \[mc_(?:bed|ld).c\]: (.+?)\s+([0-9.]+) s", res.stderr)}
        return t.get("fileset read"), t.get("LD pruning"), json.loads(res.stdout.strip().split("\n")[-1])["kept"]


def kernel_times(I, L, W, rounds):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "r", "--", sys.executable,
               os.path.abspath(__file__), "-I", str(I), "-L", str(L), "-W", str(W), "--rounds", str(rounds), "--host-first", "0"]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if res.returncode:
            raise RuntimeError("rocprofv3 run failed: " + res.stderr[-2000:])
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get("Name") or row.get("KernelName") or ""
                for key in ("k_ld_band", "k_ld_r2"):
                    if key in name:
                        out[key + "_ms_per_band"] = out.get(key + "_ms_per_band", 0.0) + float(row["TotalDurationNs"]) * 1e-6 / (rounds + 1)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-I", type=int, default=10000)
    ap.add_argument("-L", type=int, default=100000)
    ap.add_argument("-W", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-first", type=int, default=200)
    ap.add_argument("--reader", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--reader-child")
    a = ap.parse_args()
    if a.reader_child:
        return reader_child(a.reader_child, a.W)
    sec, finite = device(a.I, a.L, a.W, a.rounds)
    wp = word_pairs(a.I, a.L, a.W)
    line = {"I": a.I, "L": a.L, "W": a.W, "device_band_s": round(sec, 4), "word_pairs": wp, "device_word_pairs_per_s": round(wp / sec, 1),
            "finite_r2": finite}
    if a.host_first > 0:
        hsec, hwp = host_restatement(a.I, a.L, a.W, a.host_first)
        line.update(host_first=a.host_first, host_band_s=round(hsec, 4), host_word_pairs=hwp, host_word_pairs_per_s=round(hwp / hsec, 1),
                    host_s_for_the_whole_band=round(hsec * wp / hwp, 1))
    if a.reader:
        read_s, prune_s, kept = reader(a.I, a.L, a.W)
        line.update(fileset_read_s=read_s, ld_pruning_s=prune_s, kept=kept)
    if a.kernels:
        line.update({k: round(v, 3) for k, v in kernel_times(a.I, a.L, a.W, a.rounds).items()})
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
