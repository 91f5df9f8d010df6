#!/usr/bin/env python3
"""Time to "data set installed" of the command line through --bed and through -f on the equivalent STRUCTURE file
(profiles/bed_reader.txt).

    python scripts/bed_reader_bench.py --workdir DIR [-I 2000 -L 20000] [--rounds 3]     alternated A/B, wall seconds from
                                                                                         process start to the first upload
    python scripts/bed_reader_bench.py --workdir DIR --write-only                        only writes the files (for a profiler run)
    python scripts/bed_reader_bench.py --workdir DIR -I 10000 -L 100000 --fit ...        one --bed fit, reader seconds + peak RSS

The files are drawn locus block by locus block (Hardy-Weinberg genotypes from a per-locus allele frequency, 3 % missing), so
the headline size needs no I x L array in memory.  Every program is started once; the first failure ends the script."""
import argparse
import os
import resource
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "multiclust_amd", "bin", "multiclust")
BLOCK = 512          # loci per block


def write_files(workdir, I, L, stru, seed=1):
    prefix, stru_path = os.path.join(workdir, "panel"), os.path.join(workdir, "equivalent.stru")
    rng = np.random.default_rng(seed)
    rb = (I + 3) // 4
    rows = [[] for _ in range(2 * I)] if stru else None
    with open(prefix + ".bed", "wb") as f:
        f.write(b"\x6c\x1b\x01")
        for l0 in range(0, L, BLOCK):
            n = min(BLOCK, L - l0)
            fr = rng.uniform(0.05, 0.95, size=(n, 1))
            a2 = (rng.random((n, I)) < fr).astype(np.uint8) + (rng.random((n, I)) < fr).astype(np.uint8)
            codes = np.array([0, 2, 3], dtype=np.uint8)[a2]                  # hom A1, het, hom A2
            codes[rng.random((n, I)) < 0.03] = 1                             # missing
            full = np.zeros((n, rb * 4), dtype=np.uint8)
            full[:, :I] = codes
            q = full.reshape(n, rb, 4)
            f.write((q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).astype(np.uint8).tobytes())
            if stru:
                first = np.array(["1", "-9", "1", "2"])[codes.T]
                second = np.array(["1", "-9", "2", "2"])[codes.T]
                for i in range(I):
                    rows[2 * i].append(" ".join(first[i]))
                    rows[2 * i + 1].append(" ".join(second[i]))
    with open(prefix + ".bim", "w") as f:
        f.writelines("1\tsnp%d\t0\t%d\tA\tC\n" % (l, l + 1) for l in range(L))
    with open(prefix + ".fam", "w") as f:
        f.writelines("pop%d ind%d 0 0 0 -9\n" % (i % 5, i) for i in range(I))
    if stru:
        with open(stru_path, "w") as f:
            f.write(" ".join("snp%d" % l for l in range(L)) + "\n")
            for i in range(I):
                for h in (0, 1):
                    f.write("ind%d pop%d %s\n" % (i, i % 5, " ".join(rows[2 * i + h])))
    return prefix, stru_path


def time_to_install(data_args, outdir, fit_args):
    """(seconds from process start to the first "data set installed", reader lines, whole run seconds, peak RSS of the child in MB)"""
    env = dict(os.environ, MC_READER_TIMING="1")
    t0 = time.perf_counter()
    proc = subprocess.Popen([BIN] + data_args + fit_args + ["-o", "bench", "-d", os.path.join(outdir, "")], stdout=subprocess.DEVNULL,
                            stderr=subprocess.PIPE, text=True, env=env)
    installed, reader = None, []
    for line in proc.stderr:
        if "data set installed" in line and installed is None:
            installed = time.perf_counter() - t0
        elif line.startswith("INFO [mc_reader.c]") or line.startswith("INFO [mc_bed.c]"):
            reader.append(line.strip())
        elif not line.startswith("INFO"):
            sys.stderr.write(line)
    rc = proc.wait()
    total = time.perf_counter() - t0
    if rc or installed is None:
        sys.exit("multiclust %s left with status %d" % (" ".join(data_args), rc))
    return installed, reader, total, resource.getrusage(resource.RUSAGE_CHILDREN).ru_maxrss / 1024.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workdir", required=True)
    ap.add_argument("-I", type=int, default=2000)
    ap.add_argument("-L", type=int, default=20000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--write-only", action="store_true")
    ap.add_argument("--fit", nargs=argparse.REMAINDER, help="arguments of one --bed fit (no -f run, no STRUCTURE file)")
    a = ap.parse_args()
    os.makedirs(a.workdir, exist_ok=True)
    t0 = time.perf_counter()
    prefix, stru = write_files(a.workdir, a.I, a.L, stru=a.fit is None)
    print("files for %d x %d written in %.1f s: .bed %d bytes%s" % (a.I, a.L, time.perf_counter() - t0, os.path.getsize(prefix + ".bed"),
          "" if a.fit is not None else ", equivalent STRUCTURE file %d bytes" % os.path.getsize(stru)), flush=True)
    if a.write_only:
        return
    if a.fit is not None:
        inst, reader, total, rss = time_to_install(["--bed", prefix], a.workdir, a.fit)
        print("--bed %s: installed after %.3f s, whole run %.3f s, peak RSS %.0f MB; %s" % (" ".join(a.fit), inst, total, rss, "; ".join(reader)))
        return
    fit = ["-a", "-k", "5", "-n", "1", "-T", "1", "-r", "1"]
    for r in range(a.rounds):
        for name, data in (("--bed", ["--bed", prefix]), ("-f", ["-f", stru])):
            inst, reader, total, rss = time_to_install(data, a.workdir, fit)
            print("round %d %-5s installed after %.3f s; %s" % (r, name, inst, "; ".join(reader)), flush=True)


if __name__ == "__main__":
    main()
