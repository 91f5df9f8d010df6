#!/usr/bin/env python3
"""A/B timing of a mixture-model bootstrap run (`multiclust -b` without -a) between two builds of the command line.

    python scripts/mixture_bootstrap_ab.py --new multiclust_amd/bin/multiclust --old <other tree>/multiclust_amd/bin/multiclust \
        [--pairs 3] [--I 2000 --L 20000 --ploidy 4 --maxal 4 -k 4 -b 4 -T 20] [--data <file>] [--out profiles/mixture_bootstrap_ab.txt]

Draws a data set of K clusters (bench.gen_dataset), writes it as a STRUCTURE file (bench.write_structure) unless --data names one that exists,
and runs `multiclust -f <file> -k K -n N -b B -T T -r R -d <dir>` with the two programs in turn, `--pairs` times, profiler off.
A run in which the null model is not beaten ends early (status 13, as in the reference) and times no replicate: every timed run
must print all B " test statistics" lines or the helper fails.  With one initialisation of T iterations that depends on the
seed, so the new program (cheap) first probes -r 1, 2, ... and then -n 2, 3 with -r 1 for a command line that completes; the
one used is in the report (`--argv-out` writes it to a file, for a profiler run of the same command).
Reported per run: wall time of the whole command, time until the first replicate starts (reading the file, the two fits of the
observed data), and the time of every replicate (between the arrivals of the " test statistics" lines on stdout, which the program
writes line by line; the first replicate from the last line of the observed-data fits).  The text the two programs print from "Bootstrap dataset 1" on has to be the same.  Summary: the ratio old /
new of every pair, and the spread (max - min) of the old program's own repeats, which a difference has to exceed to mean anything."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(exe, args):
    t0 = time.perf_counter()
    proc = subprocess.Popen([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    marks, lines = [], []
    for line in proc.stdout:
        marks.append(time.perf_counter() - t0)
        lines.append(line)
    err = proc.stderr.read()
    rc = proc.wait()
    wall = time.perf_counter() - t0
    if rc not in (0, 13):       # 13: the null model was not beaten, the run ended early (the caller counts the replicates)
        raise SystemExit("%s left with status %d: %s" % (exe, rc, err[-2000:]))
    # replicate b ends with its " test statistics" line and starts where the previous one ended; the first starts at the line
    # before the one that carries "Bootstrap dataset 1" (the last line of the fits of the observed data)
    at = [x for x, l in enumerate(lines) if "test statistics" in l]
    first = next((x for x, l in enumerate(lines) if "Bootstrap dataset 1 " in l), 0)
    before = marks[first - 1] if first > 0 else 0.0
    ends = [before] + [marks[x] for x in at]
    reps = [ends[x + 1] - ends[x] for x in range(len(at))]
    text = "".join(lines)
    return wall, before, reps, (text[text.index("Bootstrap dataset 1"):] if "Bootstrap dataset 1" in text else text) + "status %d\n" % rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", required=True)
    ap.add_argument("--old", required=True)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--I", type=int, default=2000)
    ap.add_argument("--L", type=int, default=20000)
    ap.add_argument("--ploidy", type=int, default=4)
    ap.add_argument("--maxal", type=int, default=4)
    ap.add_argument("-k", type=int, default=4)
    ap.add_argument("-b", type=int, default=4)
    ap.add_argument("-T", type=int, default=20)
    ap.add_argument("--data", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--argv-out", default=None)
    a = ap.parse_args()
    work = tempfile.mkdtemp(prefix="mixture_ab_")
    data = a.data or os.path.join(work, "mixture_ab.stru")
    if not os.path.exists(data):
        import bench
        try:
            import torch
            device = "cuda:0" if torch.cuda.is_available() else "cpu"
        except ImportError:
            device = "cpu"
        t0 = time.perf_counter()
        ua, geno = bench.gen_dataset(a.I, a.L, a.k, a.ploidy, a.maxal, 20250118, device)     # K clusters: HA beats H0
        bench.write_structure(data, ua, geno)
        print("data set drawn and written in %.1f s: %s" % (time.perf_counter() - t0, data), flush=True)
    def argv(n, r):
        return ["-f", data, "-k", str(a.k), "-n", str(n), "-b", str(a.b), "-T", str(a.T), "-r", str(r), "-p", str(a.ploidy), "-d", os.path.join(work, "")]
    args = None
    for n, r in [(1, r) for r in range(1, 9)] + [(2, 1), (3, 1)]:
        wall, before, reps, _ = run(a.new, argv(n, r))
        print("probe -n %d -r %d: %d of %d replicates in %.2f s" % (n, r, len(reps), a.b, wall), flush=True)
        if len(reps) == a.b:
            args, used = argv(n, r), (n, r)
            break
    if args is None:
        raise SystemExit("no probed command line completed all %d replicates" % a.b)
    if a.argv_out:
        with open(a.argv_out, "w") as f:
            f.write("\n".join(args) + "\n")
    rows, texts = [], {}
    for pair in range(a.pairs):
        for name, exe in (("old", a.old), ("new", a.new)):
            wall, before, reps, text = run(exe, args)
            if len(reps) != a.b:
                raise SystemExit("%s printed %d of %d replicates" % (exe, len(reps), a.b))
            rows.append((pair, name, wall, before, reps))
            texts.setdefault(name, text)
            print("pair %d %s: wall %.2f s, before the replicates %.2f s, replicates %s" %
                  (pair, name, wall, before, " ".join("%.3f" % r for r in reps)), flush=True)
    out = ["mixture bootstrap A/B: multiclust -k %d -n %d -b %d -T %d -r %d (mixture model, H0: K = %d) on %d %d-ploid individuals x %d loci, "
           "2-%d alleles" % (a.k, used[0], a.b, a.T, used[1], a.k - 1, a.I, a.ploidy, a.L, a.maxal),
           "old = %s" % a.old, "new = %s" % a.new, "wall time of the whole command, profiler off, the two programs alternated", ""]
    out.append("%-5s %-4s %9s %12s  %s" % ("pair", "prog", "wall s", "pre-repl. s", "seconds per replicate"))
    for pair, name, wall, before, reps in rows:
        out.append("%-5d %-4s %9.2f %12.2f  %s" % (pair, name, wall, before, " ".join("%.3f" % r for r in reps)))
    old = [r for r in rows if r[1] == "old"]
    new = [r for r in rows if r[1] == "new"]
    spread = max(r[2] for r in old) - min(r[2] for r in old)
    out.append("")
    for o, n in zip(old, new):
        out.append("pair %d: old / new = %.2f (wall), old - new = %.2f s; replicates alone: %.3f against %.3f s each, ratio %.1f" %
                   (o[0], o[2] / n[2], o[2] - n[2], sum(o[4]) / a.b, sum(n[4]) / a.b, sum(o[4]) / sum(n[4])))
    rep_old = [sum(o[4]) / a.b for o in old]
    out.append("spread of the old program's own repeats, per replicate (max - min of its mean replicate time): %.3f s" % (max(rep_old) - min(rep_old)))
    out.append("spread of the old program's own repeats (max - min wall): %.2f s" % spread)
    faster = all(o[2] - n[2] > spread for o, n in zip(old, new))
    out.append("new faster in every pair by more than that spread: %s" % ("yes" if faster else "NO"))
    out.append("text from 'Bootstrap dataset 1' on identical between the two programs: %s" % ("yes" if texts["old"] == texts["new"] else "NO"))
    if texts["old"] != texts["new"]:
        for lo, ln in zip(texts["old"].split("\n"), texts["new"].split("\n")):
            if lo != ln:
                out += ["first line that differs:", "  old: " + lo, "  new: " + ln]
                break
    report = "\n".join(out) + "\n"
    print(report)
    if a.out:
        with open(a.out, "w") as f:
            f.write(report)
    return 0 if faster and texts["old"] == texts["new"] else 1


if __name__ == "__main__":
    sys.exit(main())
