"""Filling missing genotypes, without a GPU: the greedy mode against brute force, the accuracy of the rule on clustered data with the
oracle's fit, the two writers of --fill on hand-made files (through host.py and, under the sanitizers, through a C program of their
own), and the command line's refusals."""
import os
import subprocess

import numpy as np
import pytest

import bedfiles as bf
from cli_util import BIN, DATA, ROOT
import cv_util as cu
import host_driver
import impute_util as iu
from multiclust_amd import host

MULTI = os.path.join(ROOT, "tests", "golden", "data", "multi.stru")


# ---- the rule ----
def test_greedy_is_the_mode_of_the_multinomial():
    rng = np.random.default_rng(3)
    n = 0
    for M in (1, 2, 3, 4):
        for r in (1, 2, 3, 4):
            for _ in range(40):
                x = rng.dirichlet(np.full(M, rng.choice([0.3, 1.0, 5.0])))
                t = x * rng.uniform(0.1, 1.0)                    # the rule takes t, not x: unnormalised
                c = iu.greedy_counts(t[None, :], np.ones((1, M), dtype=bool), np.array([r]))[0]
                best, best_c = iu.brute_mode(t / t.sum(), r)
                assert c.sum() == r and np.array_equal(c, best_c), (x, r, c, best_c)
                pr = iu.multiset_prob(t[None, :], np.ones((1, M), dtype=bool), c[None, :])[0]
                assert abs(pr - best) <= 8 * 2.0 ** -52 * best
                n += 1
    assert n == 640


def test_ties_go_to_the_lowest_index_and_the_heterozygote_threshold():
    one = np.ones((1, 2), dtype=bool)
    # two equal alleles: one copy takes the first, two copies one of each
    assert iu.greedy_counts(np.array([[0.5, 0.5]]), one, np.array([1])).tolist() == [[1, 0]]
    assert iu.greedy_counts(np.array([[0.5, 0.5]]), one, np.array([2])).tolist() == [[1, 1]]
    # a fully missing diploid genotype is heterozygous when the larger x is below 2 / 3, homozygous from 2 / 3 on
    assert iu.greedy_counts(np.array([[0.66, 0.34]]), one, np.array([2])).tolist() == [[1, 1]]
    assert iu.greedy_counts(np.array([[2.0 / 3.0, 1.0 / 3.0]]), one, np.array([2])).tolist() == [[2, 0]]
    assert iu.greedy_counts(np.array([[0.3, 0.7]]), one, np.array([2])).tolist() == [[0, 2]]
    # no positive candidate, NaN included: not fillable
    t = np.array([[0.0, 0.0], [np.nan, 0.0], [0.0, 0.25]])
    assert iu.fillable(t, np.ones((3, 2), dtype=bool)).tolist() == [False, False, True]
    assert iu.multiset_prob(np.array([[0.5, 0.5]]), one, np.array([[1, 1]]))[0] == 0.5


# ---- accuracy: the yardstick of the issue, with the oracle's fit ----
# (I, L, clusters, seed) of cv_util.clustered_dataset; 15 % of the genotypes hidden (rng of seed + 100).  Measured with the oracle's
# fit (random start from seed 7, SQUAREM 3, defaults otherwise), K = clusters:
#     case                concordance   modal genotype   mean c
#     (72, 400, 3, 11)    0.7985        0.5912           0.8020
#     (72, 400, 3, 12)    0.7865        0.5912           0.7986
#     (150, 300, 3, 5)    0.7932        0.6019           0.7999
#     (96, 400, 4, 7)     0.7940        0.5586           0.8004
ACCURACY_CASES = [(72, 400, 3, 11), (72, 400, 3, 12), (150, 300, 3, 5), (96, 400, 4, 7)]


@pytest.mark.parametrize("I,L,clusters,seed", ACCURACY_CASES)
def test_accuracy_on_clustered_data_with_the_oracle_fit(I, L, clusters, seed):
    import oracle_bind as ob
    ua, truth = cu.clustered_dataset(I, L, clusters, seed)
    hidden = np.random.default_rng(seed + 100).random((I, L)) < 0.15
    geno = truth.copy()
    geno[hidden] = iu.MISSING
    mod = ob.Model(ob.Data(I, L, 2, ua, geno), ob.make_options(accel_scheme=3), clusters)
    mod.init_random(7)
    mod.em()
    assert mod.fatal == 0
    q, p = mod.q(mod.pindex).copy(), mod.p(mod.pindex).copy()
    ref = iu.impute_reference(ua, ua, geno, q, p)
    assert ref["ok"].all() and np.array_equal(ref["filled"][~hidden], truth[~hidden])
    conc, base, mean_c = iu.concordance(truth, ref["filled"], hidden), iu.modal_baseline(truth, hidden), float(ref["conf"].mean())
    print("concordance %.4f, modal genotype %.4f, mean confidence %.4f" % (conc, base, mean_c))
    assert conc >= base + 0.10
    assert abs(mean_c - conc) <= 0.05


# ---- the writers, through host.py ----
def structure_text(codes, layout, header_extra=(), minus1=False, sep="\t", eol="\n", trailer=None, ragged=False, last_eol=True):
    """A STRUCTURE file of codes [I][L][ploidy] (integers as they stand in the file).  layout "lines": `ploidy` consecutive lines
    per individual; "one": one line per individual, the copies of a locus side by side.  ragged: white space of varying width
    around the tokens.  trailer: one more line behind the data."""
    I, L, pl = codes.shape
    pad = (lambda n: " " * (n % 3)) if ragged else (lambda n: "")
    lines = [sep.join(list(header_extra) + ["loc%d" % l for l in range(L)])]
    if minus1:
        lines.append(sep.join(["-1"] + ["%d" % (10 * l) for l in range(1, L)]))
    for i in range(I):
        rows = [codes[i].reshape(-1)] if layout == "one" else [codes[i, :, a] for a in range(pl)]
        for a, row in enumerate(rows):
            toks = ["ind%d" % i, "pop%d" % (i % 2)] + ["%d" % v for v in row]
            lines.append(pad(i + a) + sep.join(t + pad(i + n) for n, t in enumerate(toks)))
    if trailer is not None:
        lines.append(trailer)
    return (eol.join(lines) + (eol if last_eol else "")).encode()


def choose_fills(geno, n_real):
    """a filled copy of geno: every missing copy takes a real allele of its locus, by position; nothing where a locus has none, and
    every fifth genotype stays as it is"""
    filled = geno.copy()
    I, L, pl = geno.shape
    for i in range(I):
        for l in range(L):
            if n_real[l] == 0 or (i + 2 * l) % 5 == 4:
                continue
            for a in range(pl):
                if geno[i, l, a] == iu.MISSING:
                    filled[i, l, a] = (i + l + a) % n_real[l]
    return filled


STRUCTURE_CASES = {
    # consecutive lines, tabs and CRLF, the "-1" line (with it the reader takes one data line fewer: the trailer is that line), a
    # locus with no call
    "lines_tabs_crlf_minus1": dict(ploidy=2, layout="lines", minus1=True, sep="\t", eol="\r\n", trailer="ind9\tpop0\t1\t1\t1\t1\t1\t1",
                                   missing=-9),
    # one line per individual, -R (two more names in the header), --missing 0, ragged blanks, no line end behind the last line
    "one_R_missing0_ragged": dict(ploidy=2, layout="one", header_extra=("name", "pop"), r_format=1, sep=" ", ragged=True,
                                  last_eol=False, missing=0),
    "haploid": dict(ploidy=1, layout="lines", sep=" ", missing=-9),
    "tetraploid_lines": dict(ploidy=4, layout="lines", sep="\t", ragged=True, missing=-9),
    "tetraploid_one": dict(ploidy=4, layout="one", sep=" ", eol="\r\n", missing=-9),
}


@pytest.mark.parametrize("name", sorted(STRUCTURE_CASES))
def test_structure_writer(name, tmp_path):
    case = dict(STRUCTURE_CASES[name])
    pl, missing, r_format = case.pop("ploidy"), case.pop("missing"), case.pop("r_format", 0)
    I, L = 6, 6
    rng = np.random.default_rng(len(name))
    alleles = np.array([[101, 105, 250], [7, 3, 12], [1, 2, 2], [40, 40, 41], [5, 6, 7], [9, 8, 8]])       # labels of every locus
    codes = alleles[np.arange(L)[None, :, None], rng.integers(0, 3, size=(I, L, pl))]
    codes[rng.random((I, L, pl)) < 0.35] = missing
    codes[:, 3, :] = missing                                    # a locus with no call
    codes[0, 0, :] = missing
    text = structure_text(codes, **case)
    src, out = str(tmp_path / "in.stru"), str(tmp_path / "out.stru")
    with open(src, "wb") as f:
        f.write(text)
    rc, d = host.read_structure(src, ploidy=pl, missing=missing, r_format=r_format)
    assert rc == 0 and (d["I"], d["L"]) == (I, L) and d["ua"][3] == 0
    n_real = host.impute_n_real(d["ua"], geno=d["geno"])
    assert n_real.tolist() == [len(a) for a in d["L_alleles"]]
    filled = choose_fills(d["geno"], n_real)
    changed = (filled != d["geno"])
    assert changed.any() and ((filled == iu.MISSING) & (d["geno"] == iu.MISSING)).any()
    assert host.write_filled_structure(src, out, filled, ploidy=pl, missing=missing, r_format=r_format) == 0
    # byte for byte the file built from the same tokens with the filled ones replaced by their labels
    want = codes.copy()
    for i, l, a in zip(*np.nonzero(changed)):
        want[i, l, a] = d["L_alleles"][l][filled[i, l, a]]
    assert open(out, "rb").read() == structure_text(want, **case)
    # read again: the filled genotype (no allele is new, so the indices stand)
    rc2, d2 = host.read_structure(out, ploidy=pl, missing=missing, r_format=r_format)
    assert rc2 == 0 and np.array_equal(d2["geno"], filled) and d2["L_alleles"] == d["L_alleles"]
    # nothing filled: the file itself
    same = str(tmp_path / "same.stru")
    assert host.write_filled_structure(src, same, d["geno"], ploidy=pl, missing=missing, r_format=r_format) == 0
    assert open(same, "rb").read() == text


@pytest.mark.parametrize("I,padding", [(7, 1), (9, 3), (8, 0)])
def test_bed_writer(I, padding, tmp_path):
    L = 11
    codes = bf.draw_codes(I, L, missing=0.3, seed=I, plant=True)
    src, out = str(tmp_path / "in"), str(tmp_path / "out")
    bf.write_fileset(src, codes, padding=padding)
    rc, d = host.read_bed(src)
    assert rc == 0 and d["geno_is_null"]
    n_real = host.impute_n_real(d["ua"], bed=d["bed"], I=I)
    assert n_real.tolist() == [len(a) for a in d["L_alleles"]]
    assert np.array_equal(n_real, host.impute_n_real(d["ua"], geno=d["geno"]))
    filled = choose_fills(d["geno"], n_real)
    assert (filled != d["geno"]).any() and (n_real == 0).any()
    assert host.write_filled_bed(src, out, filled) == 0
    # the records: a missing call whose copies were filled spells homozygous A1 / heterozygous / homozygous A2
    want = codes.copy()
    for i, l in zip(*np.nonzero((filled != d["geno"]).all(axis=2))):
        labels = sorted(d["L_alleles"][l][m] for m in filled[i, l])
        want[i, l] = {(1, 1): bf.HOM1, (1, 2): bf.HET, (2, 2): bf.HOM2}[tuple(labels)]
    assert open(out + ".bed", "rb").read() == b"\x6c\x1b\x01" + bf.pack(want, padding).tobytes()
    for ext in (".bim", ".fam"):
        assert open(out + ext, "rb").read() == open(src + ext, "rb").read()
    rc2, d2 = host.read_bed(out)
    # (a record holds a genotype, not an order of copies: the reader spells a heterozygote 0, 1)
    assert rc2 == 0 and np.array_equal(d2["geno"], np.sort(filled, axis=2)) and d2["L_alleles"] == d["L_alleles"]


# ---- the command line ----
@pytest.mark.parametrize("args", [
    ["-k", "2", "--fill"],                                  # needs the admixture model
    ["-a", "-k", "2", "--fill", "-b", "2"],
    ["-a", "-k", "2", "--fill", "-w", "n", "2"],
    ["-a", "-k", "2", "--fill", "-M"],
    ["-a", "-k", "2", "--fill", "--gpus", "2"],
    ["-a", "-k", "2", "--fill", "--query", "/nonexistent/query.txt"],
    ["-a", "-k", "2", "--impute"],                          # the reference's option stays refused
    ["-a", "-k", "2", "--cv", "3", "-b", "2"],              # what another extension gives its refusals
])
def test_refused_combinations(args, tmp_path):
    res = subprocess.run([BIN, "-f", MULTI] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, cwd=str(tmp_path))
    assert res.returncode == 10, (args, res.returncode, res.stderr[-500:])
    assert "ERROR [mc_main.c::parse_options]" in res.stderr


# ---- the writers under AddressSanitizer + UBSan, as a program of their own ----
def test_writers_are_sanitizer_clean(tmp_path):
    exe = host_driver.build(tmp_path, "impute_writers", ["tests/impute_writers_driver.c"] +
                            ["multiclust_amd/host/" + f for f in ("mc_impute.c", "mc_reader.c", "mc_bed.c")], libs=("-lm", "-lpthread"), werror=True)
    runs = [["stru", os.path.join(DATA, fn), str(pl), str(miss), "0", str(tmp_path / ("out%d.stru" % n))]
            for n, (fn, pl, miss) in enumerate((("missing.stru", 2, -9), ("tetra.stru", 4, -9), ("multi_interleaved.stru", 2, -9),
                                                ("missing99.stru", 2, 99), ("multi.stru", 2, -9)))]
    for I in (7, 8):
        codes = bf.draw_codes(I, 13, missing=0.3, seed=I)
        bf.write_fileset(str(tmp_path / ("set%d" % I)), codes, padding=1)
        runs.append(["bed", str(tmp_path / ("set%d" % I)), str(tmp_path / ("filled%d" % I))])
    for args in runs:
        res = host_driver.run(exe, args, cwd=tmp_path)
        assert "wrote 0" in res.stdout, args
    # what the program wrote is what the library writes: the filled file reads back without a missing copy where a locus has alleles
    rc, d = host.read_structure(runs[0][-1])
    rc0, d0 = host.read_structure(runs[0][1])
    assert rc == 0 and rc0 == 0 and (d["geno"] == iu.MISSING).sum() < (d0["geno"] == iu.MISSING).sum()
