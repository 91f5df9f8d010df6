"""What the `multiclust` binary given by path prints and writes, as SHA-256 digests, over a matrix of command lines that reaches every
route of its front end (multiclust_amd/host/mc_main.c and mc_cli_*.c): run it for two builds of the binary and diff the two outputs.

    python3 scripts/diag/cli_digests.py <binary> <work directory> [<first>-<last>]  >  digests.txt

(with a range, those command lines of the matrix alone, and their masked stdout and stderr are kept as <work directory>/<number>.out
and .err: for looking at a difference)

Every command line runs in a fresh process under its own time limit, in a directory of its own under the work directory, with
relative result paths, so two builds see the same arguments.  One line per command line: its number, exit status, and the digests of
stdout, of stderr and of every file written (names and bytes); the last line is the digest of all masked outputs one after the other.
Only wall-clock fields are masked: the HH:MM:SS groups, and the `esec` and `esec/n` numbers of the -w lines.  The matrix stops at the
first command line that ends on a signal, a device fault or at its time limit: nothing more is started on the device after that.

Fixtures: tests/golden/data/multi.stru (diploid: admixture K = 4, mixture K = 3), tetra.stru (tetraploid admixture K = 3) and the
fileset of the filter tests (tests/qc_util.py: cli_case).  -t and -w t with a positive time are left out: the number of
initialisations or repetitions, and so the lines, follow the clock."""
import hashlib
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bedfiles as bf
import ld_util as lu
import qc_util as qu

DATA = os.path.join(ROOT, "tests", "golden", "data")
CLOCK = re.compile(r"\d\d:\d\d:\d\d")
# a repetition's line of -w: the model state ends "HH:MM:SS <4 counts>[ <target> <2 counts>][ time]", then esec and esec/n
W_LINE = re.compile(r"(HH:MM:SS(?: -?\d+){4}(?: -?\d+\.\d+ \d+ \d+)?(?: time)?) \d+\.\d+ \d+\.\d+ ")
W_TIME = re.compile(r"^Average time: \S+ \(total: \S+;", re.M)
TIME_LIMIT = 120


def mask(text):
    return W_TIME.sub("Average time: T (total: T;", W_LINE.sub(r"\1 T T ", CLOCK.sub("HH:MM:SS", text)))


def individuals(path, ploidy):
    return (sum(1 for ln in open(path) if ln.strip()) - 1) // ploidy       # one header line, a line per copy of an individual


def matrix(work):
    def labels(name, ploidy, what, label):
        """a file of one label per individual of the data file: a partition for -A, the query individuals for --query"""
        path = os.path.join(work, "%s.%s.txt" % (name, what))
        open(path, "w").write(" ".join(label(i) for i in range(individuals(os.path.join(DATA, name), ploidy))) + "\n")
        return path

    def A(base):
        return ["-A", labels(os.path.basename(base[1]), 4 if "-p" in base else 2, "partition", lambda i: str(i % 3 + 1))]

    query = labels("missing.stru", 2, "query", lambda i: "1" if i % 7 == 3 else "0")
    D = ["-f", os.path.join(DATA, "multi.stru"), "-a", "-k", "4", "-r", "7", "-n", "3", "-T", "30"]
    T = ["-f", os.path.join(DATA, "tetra.stru"), "-p", "4", "-a", "-k", "3", "-r", "11", "-n", "2", "-T", "30"]
    M = ["-f", os.path.join(DATA, "multi.stru"), "-k", "3", "-r", "5", "-n", "2", "-T", "30"]
    PQ = ["-f", os.path.join(DATA, "c1_tiny.stru"), "-a", "-k", "3", "-r", "1234567", "-n", "1", "-T", "30", "-P", os.path.join(DATA, "c1_P.txt"),
          "-Q", os.path.join(DATA, "c1_Q.txt")]
    BED = ["--bed", "data", "-a", "-k", "3", "-s", "3", "-n", "2", "-r", "7", "-T", "30"]
    forced, s2, s3 = ({"MC_FORCE_SHARDED": "1", "MC_TRACE_EXCHANGE": "1"}, ["--gpus", "1"]), ({}, ["--streams", "2"]), ({}, ["--streams", "3"])
    serial = ({}, [])
    runs = []
    for base, routes in ((D, (serial, forced, s2, s3)), (T, (serial, s2)), (M, (serial, s2))):
        plain = [[], ["-1", "2", "-2", "4"], ["-s", "3"]] + ([["-c"]] if base is not M else [])
        for more in plain:
            for env, extra in routes:
                runs.append((env, base + more + extra))
                runs.append((env, base + more + A(base) + extra))
    runs.append(({}, PQ))
    runs.append(({}, PQ + ["--streams", "2"]))                   # not shardable: the warning, then the serial route
    runs.append(({}, M + ["--streams", "2", "-b", "2"]))         # the mixture model's replicates split: the other warning
    # (-u with targets that are reached: the loop over the initialisations has no other end.  A log likelihood every fit exceeds; a
    # revisit of the maximum by the first fit that converges, which -E 10 lets every fit do)
    for more in (["-u", "l", "-1e9"], ["-u", "n", "1", "-E", "10", "-T", "2000"], ["-u", "n", "2", "l", "-1e9"], ["-t", "0"], ["-w", "n", "3"], ["-w", "t", "0", "n", "2"],
                 ["-w", "n", "2", "m", "1"], ["-w", "n", "3", "-1", "2", "-2", "3"], ["-w", "n", "2"] + A(D), ["-M"], ["-n", "0"], ["-k", "1"]):
        for env, extra in (serial, s2):
            runs.append((env, D + more + extra))
    for v in ("0", "1", "3"):
        for env, extra in (serial, forced):
            runs.append((env, D + ["-v", v] + extra))
            runs.append((env, D + ["-v", v, "-b", "2", "-k", "3"] + extra))
    # the bootstrap: serial, host-drawn, by replicate, by unit (fewer replicates than workers), both models, with -A and result files on
    for base in (D, M):
        for more in ([], A(base)):
            b = base + ["-k", "3", "-n", "2", "-s", "3"] + more + ["-b", "3"]
            runs.append(({}, b))
            runs.append(({"MC_HOST_BOOTSTRAP": "1"}, b))
            runs.append((forced[0], b + forced[1]))
            runs.append(({}, b + ["--streams", "2"]))
            runs.append(({}, b + ["--streams", "4"]))
            runs.append((forced[0], b + ["-b", "1", "--streams", "2"] + forced[1]))
    # the post-fit analyses, singly and together
    post = {"--fst": [], "--resid": [], "--cv": ["3"], "--se": ["4"], "--fill": [], "--query": [query]}
    Dm = [os.path.join(DATA, "missing.stru") if x.endswith("multi.stru") else x for x in D[:4]] + ["3", "-r", "7", "-n", "2", "-T", "30"]
    for opt, val in post.items():
        for env, extra in ((serial,) if opt == "--query" else (serial, s2)):
            runs.append((env, Dm + [opt] + val + extra))
            runs.append((env, Dm + ["-1", "2", "-2", "3", opt] + val + extra))
    together = [x for opt, val in post.items() if opt != "--query" for x in [opt] + val]
    for env, extra in (serial, s2, forced):
        runs.append((env, Dm + together + extra))
        runs.append((env, Dm + ["-1", "1", "-2", "3"] + together + A(Dm) + extra))
    runs.append(({}, Dm + ["--fst", "--resid", "--query", query]))
    runs.append(({}, M + ["--fst", "--se", "4"]))
    runs.append(({}, M + ["--fst", "--se", "4", "--streams", "2"]))
    # the fileset: plain, every filter and --pca together, with a post-fit analysis behind them
    C = qu.CLI
    filters = ["--mind", repr(C["mind"]), "--geno", repr(C["geno"]), "--maf", repr(C["maf"]), "--hwe", repr(C["hwe"]), "--prune", repr(C["prune_t"]),
               "--prune-window", str(C["prune_window"]), "--king-cutoff", repr(C["king_t"]), "--pca", "3"]
    for env, extra in (serial, s2):
        runs.append((env, BED + extra))
        runs.append((env, BED + filters + extra))
        runs.append((env, BED + filters + ["--fill", "--fst"] + extra))
    runs.append(({}, BED + ["--mind", repr(C["mind"])]))
    runs.append(({}, BED + ["--pca", "2"]))
    runs.append(({}, BED + ["--mind", "0", "--geno", "0", "--maf", "0.5", "--hwe", "0.999"]))      # an emptied data set ends the run
    # what check_setup refuses
    runs += [({}, D + ["-k", "1000"]), ({}, D + ["-b", "2", "-k", "1"]), ({}, D + ["--se", "3", "--se-block", "100000"]), ({}, D + ["-1", "3", "-2", "2"])]
    # -w with fits that converge (-E 10 lets every fit): the sums of initialisations and iterations are not zero
    runs += [({}, D + ["-w", "n", "3", "-E", "10", "-T", "2000"] + extra) for env, extra in (serial, s2)]
    return runs


def main():
    binary, work = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
    os.makedirs(work)
    codes, fids, iids, chrom = qu.cli_case()
    L = codes.shape[1]
    first, last = [int(x) for x in sys.argv[3].split("-")] if len(sys.argv) > 3 else (0, 10 ** 9)
    whole = hashlib.sha256()
    for n, (env, args) in enumerate(matrix(work)):
        if not first <= n <= last:
            continue
        d = os.path.join(work, "%03d" % n)
        os.makedirs(d)
        if "--bed" in args:
            bf.write_fileset(os.path.join(d, "data"), codes, padding=1, fids=fids, iids=iids)
            lu.write_bim(os.path.join(d, "data"), list(chrom), ["rs%d" % (7 * l) for l in range(L)], [1000 + 13 * l for l in range(L)])
        before = set(os.listdir(d))
        try:
            res = subprocess.run([binary] + args + ["-o", "stem"], cwd=d, env=dict(os.environ, **env), capture_output=True, text=True, timeout=TIME_LIMIT)
        except subprocess.TimeoutExpired:
            print("%03d TIME LIMIT: %s" % (n, " ".join(args)))
            return 1
        out, err = mask(res.stdout).replace(work, "WORK"), mask(res.stderr).replace(work, "WORK")
        if len(sys.argv) > 3:
            open(d + ".out", "w").write(out)
            open(d + ".err", "w").write(err)
        files = hashlib.sha256()
        names = sorted(set(os.listdir(d)) - before)
        for f in names:
            files.update(f.encode() + b"\0" + open(os.path.join(d, f), "rb").read())
        for part in (out, err, files.hexdigest()):
            whole.update(part.encode())
        shown = " ".join("%s=%s" % kv for kv in sorted(env.items())) + " " + " ".join(a.replace(DATA + os.sep, "").replace(work, "WORK") for a in args)
        print("%03d status %d stdout %s (%d lines) stderr %s (%d lines) files %s (%d): %s" % (
            n, res.returncode, hashlib.sha256(out.encode()).hexdigest()[:16], out.count("\n"), hashlib.sha256(err.encode()).hexdigest()[:16],
            err.count("\n"), files.hexdigest()[:16], len(names), shown.strip()), flush=True)
        if res.returncode < 0 or res.returncode in (124, 134, 137, 139) or "illegal memory access" in res.stderr:
            print("stopped: command line %03d ended on a signal or a device fault\n%s" % (n, res.stderr[-2000:]))
            return 1
    print("all %d command lines: %s" % (min(last, n) - first + 1, whole.hexdigest()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
