"""Running the command-line program from the tests: where it is, one launch with its status checked and the files it wrote
collected, a memo of launches for the modules that share runs, and the inputs and result-file readers the command-line tests of
more than one feature use.  Every launch goes through procutil.run_program: one launch, a watchdog, never a second try.

pytest does not rewrite the asserts of a helper module, so each carries its evidence in its message."""
import os
import re

import numpy as np

import bedfiles as bf
import ld_util
import procutil
from conftest import ROOT

BIN = os.path.join(ROOT, "multiclust_amd", "bin", "multiclust")
DATA = os.path.join(ROOT, "tests", "golden", "data")
CLOCK = re.compile(r"\d\d:\d\d:\d\d")       # elapsed CPU time of a fit: the one thing two runs of one program differ in


def normalise(stdout):
    """the lines of stdout, the clock replaced"""
    return CLOCK.sub("HH:MM:SS", stdout).split("\n")


def result_files(d):
    return {f: open(os.path.join(str(d), f), "rb").read() for f in sorted(os.listdir(str(d)))}


def split_own(lines, own):
    """(the other lines, the option's own): own is a line prefix, or a compiled regex, whose matches then stand for the lines"""
    if isinstance(own, str):
        return [ln for ln in lines if not ln.startswith(own)], [ln for ln in lines if ln.startswith(own)]
    return [ln for ln in lines if not own.match(ln)], [own.match(ln) for ln in lines if own.match(ln)]


def run_cli(args, cwd, expect=0, timeout=300, own=None):
    """the program with these arguments in directory cwd: (stdout lines, the bytes of every file that appeared in cwd, the completed
    process), or with own= (other lines, own lines, files)"""
    cwd = str(cwd)
    before = set(os.listdir(cwd))
    res = procutil.run_program([BIN] + list(args), cwd=cwd, timeout=timeout)
    assert res.returncode == expect, (list(args), res.returncode, "expected %d" % expect, res.stderr[-2000:])
    lines = normalise(res.stdout)
    files = {f: open(os.path.join(cwd, f), "rb").read() for f in sorted(set(os.listdir(cwd)) - before)}
    if own is None:
        return lines, files, res
    return split_own(lines, own) + (files,)


def run_fresh(args, d, own=None):
    """the program in the directory d, made if need be, which also receives its results as `stem.*`"""
    os.makedirs(str(d), exist_ok=True)
    return run_cli(list(args) + ["-o", "stem", "-d", os.path.join(str(d), "")], d, own=own)


class Runs:
    """the launches a test module shares: one per distinct command line, each in a directory of its own from new_dir()"""

    def __init__(self, new_dir, own=None, launch=run_fresh):
        self.new_dir, self.own, self.launch, self.done = new_dir, own, launch, {}

    def __call__(self, args):
        key = tuple(args)
        if key not in self.done:
            self.done[key] = self.launch(list(args), self.new_dir(), own=self.own)
        return self.done[key]


def option_is_there(text):
    """the usage text (status 1) names the option"""
    res = procutil.run_program([BIN, "-h"], timeout=60)
    assert res.returncode == 1 and text in res.stdout, (text, res.returncode, res.stdout[-2000:], res.stderr[-2000:])


# ---- filesets ----
def write_fileset_inputs(d, case, rows=None, cols=None, chrom=None, ids=None, padding=None):
    """the fileset `data` in the new directory d: everything, or the individuals `rows` (what `plink --keep` would write) at the
    variants `cols` (`plink --extract`).  The whole set of individuals has its padding bits set; a kept subset is as plink writes
    it, with padding bits 0."""
    d.mkdir(parents=True)
    I, L = case["codes"].shape
    if padding is None:
        padding = 1 if rows is None else 0
    rows = np.arange(I) if rows is None else np.asarray(rows)
    cols = np.arange(L) if cols is None else np.asarray(cols)
    prefix = os.path.join(str(d), "data")
    named = "fids" in case
    bf.write_fileset(prefix, case["codes"][np.ix_(rows, cols)], padding=padding, fids=[case["fids"][i] for i in rows] if named else None,
                     iids=[case["iids"][i] for i in rows] if named else None)
    ld_util.write_bim(prefix, [chrom[l] if chrom else "1" for l in cols], [ids[l] if ids else "rs%d" % (7 * l) for l in cols],
                      [1000 + 13 * l for l in cols])
    return d


def id_lines(case, which):
    """the `FID<tab>IID` lines of the individuals of the mask"""
    return "".join("%s\t%s\n" % (case["fids"][i], case["iids"][i]) for i in range(len(which)) if which[i])


# ---- fits ----
def clustered_codes(I, L, clusters, seed=6, missing=0.05, empty_locus=17):
    """clustered diploid biallelic data as .bed codes, `missing` of the calls missing, one locus without a call"""
    import cv_util
    _, geno = cv_util.clustered_dataset(I, L, clusters, 4)
    n = geno.astype(np.int64).sum(axis=2)
    c = np.array([bf.HOM1, bf.HET, bf.HOM2], dtype=np.uint8)[n]
    c[np.random.default_rng(seed).random((I, L)) < missing] = bf.MISS
    c[:, empty_locus] = bf.MISS
    return c


def fit_inputs(tmp_path_factory, name, codes):
    """a STRUCTURE file, the fileset it stands for and a query file with every ninth individual marked"""
    from multiclust_amd import host
    d = str(tmp_path_factory.mktemp(name))
    stru = os.path.join(d, "data.stru")
    bf.write_equivalent_stru(stru, codes)
    bf.write_fileset(os.path.join(d, "data"), codes, padding=1)
    query = os.path.join(d, "query.txt")
    with open(query, "w") as f:
        f.write(" ".join("1" if i % 9 == 4 else "0" for i in range(codes.shape[0])) + "\n")
    rc, data = host.read_structure(stru)
    assert rc == 0, (stru, rc)
    return dict(dir=d, stru=stru, bed=os.path.join(d, "data"), query=query, ua=data["ua"], geno=data["geno"], tmp=tmp_path_factory)


def table(text, skip=1):
    return [ln.split("\t") for ln in text.decode().split("\n")[skip:] if ln.strip()]


def written_fit(files, ua, I, K, mdl="admix"):
    """Q ([I][K], or [K] where the proportions are shared) and P [K][T] as the result files print them"""
    import divergence_util
    T, off = int(ua.sum()), divergence_util.offsets(ua)
    P = np.full((K, T), np.nan)
    for k, l, m, v in table(files["stem.%s.K=%d.pklm.txt" % (mdl, K)]):
        P[int(k), off[int(l)] + int(m)] = float(v)
    assert not np.isnan(P).any(), ("a cell of P is absent", mdl, K, np.argwhere(np.isnan(P))[:5].tolist())
    name = "stem.%s.K=%d.etaik.txt" % (mdl, K)
    if name in files:
        q = np.full((I, K), np.nan)
        for i, k, v in table(files[name]):
            q[int(i), int(k)] = float(v)
    else:
        q = np.array([float(v) for _, v in table(files["stem.%s.K=%d.etak.txt" % (mdl, K)])])
        assert q.shape == (K,), (q.shape, K)
    return q, P
