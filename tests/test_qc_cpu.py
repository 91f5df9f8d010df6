"""Quality control on the CPU (no GPU): the float restatement of the Hardy-Weinberg exact test in tests/qc_util.py against exact
rationals, the four rules and their order, the composition of the maps of chained filters against a brute-force restatement,
multiclust_amd/host/mc_qc.c -- and mc_ld.c and mc_king.c on an axis that quality control thinned -- as a program of its own
(tests/qc_host_driver.c, plain and under AddressSanitizer + UBSan) against qc_util, the launch geometry, the mutants of the
definition and of the rules that the cases of the tests have to tell from the real thing, and the fixture of the command-line tests.

The counts are integers and have no tolerance.  The one tolerance of this file, of the float restatement against the rationals, is
derived at the test from the number of roundings of the walk."""
import os
from fractions import Fraction

import numpy as np
import pytest

import bedfiles
from cli_util import ROOT
import host_driver
import king_util
import qc_util as qu

U = Fraction(1, 2 ** 53)        # unit roundoff of float64


@pytest.fixture(autouse=True, scope="module")
def the_feature_is_there():
    """every test of this file is about quality control: the restatements and fixtures below are held to something only in a tree
    that has the entry point and the host unit they restate"""
    from multiclust_amd import hip
    assert "mchip_bed_qc" in hip.ABI_SYMBOLS and os.path.exists(os.path.join(ROOT, "multiclust_amd", "host", "mc_qc.c"))


# ---- the exact test: the float restatement against exact rationals ----
def tolerance(n0, n2, n3):
    """relative, as a multiple of 2^-53: a weight k steps from mid carries at most 4 k roundings (two conversions, one multiply, one
    divide a step; the conversions are exact below 2^53 and counted all the same), the two sums of at most n positive terms n - 1
    each, the quotient one; k < n = r // 2 + 1.  To first order (1 + u)^m - 1 <= 1.01 m u for m u < 0.01.  No weight is subnormal at
    N <= 400: the smallest is above e^-400."""
    n = qu.hwe_steps(n0, n2, n3)
    m = 2 * (4 * n + n) + 1
    assert m * U < Fraction(1, 100)
    return Fraction(101, 100) * m * U


def check_tables(tables):
    skipped, worst = 0, Fraction(0)
    for n0, n2, n3 in tables:
        exact, near = qu.hwe_exact(n0, n2, n3)
        if near:
            skipped += 1
            continue
        got = Fraction(qu.hwe_p(n0, n2, n3))
        err = abs(got - exact) / exact
        assert err <= tolerance(n0, n2, n3), (n0, n2, n3, float(err), float(tolerance(n0, n2, n3)))
        worst = max(worst, err / tolerance(n0, n2, n3))
    return skipped, worst


def test_hwe_restatement_on_every_table_up_to_40():
    tables = [(n0, n2, N - n0 - n2) for N in range(0, 41) for n0 in range(N + 1) for n2 in range(N + 1 - n0)]
    skipped, worst = check_tables(tables)
    print("%d tables, %d skipped for a near tie (%.3f %%), worst error %.3f of its tolerance" % (len(tables), skipped, 100.0 * skipped / len(tables),
                                                                                                float(worst)))
    assert len(tables) == 12341 and skipped <= len(tables) // 100


def test_hwe_restatement_on_random_tables_up_to_400():
    rng = np.random.default_rng(4)
    tables = []
    for _ in range(400):
        N = int(rng.integers(41, 401))
        f = rng.uniform(0.02, 0.98)
        F = rng.uniform(-0.3, 0.5)                     # inbreeding: tables on both sides of Hardy-Weinberg proportions
        pr = np.clip([f * f + F * f * (1 - f), 2 * f * (1 - f) * (1 - F), (1 - f) ** 2 + F * f * (1 - f)], 0, None)
        n0, n2, n3 = rng.multinomial(N, pr / pr.sum())
        tables.append((int(n0), int(n2), int(n3)))
    skipped, worst = check_tables(tables)
    print("%d tables, %d skipped for a near tie (%.3f %%), worst error %.3f of its tolerance" % (len(tables), skipped, 100.0 * skipped / len(tables),
                                                                                                float(worst)))
    assert skipped <= len(tables) // 100


def test_hwe_values_at_the_edges():
    for t in ((0, 0, 0), (5, 0, 0), (0, 0, 7), (6, 1, 0), (0, 1, 9), (0, 1, 0)):       # N = 0, r = 0 and r = 1: one table, p = 1
        assert qu.hwe_p(*t) == 1.0, t
    assert qu.hwe_p(1000, 0, 1000) == 0.0 and qu.hwe_p(0, 2000, 0) == 0.0 and qu.hwe_p(5000, 0, 5000) == 0.0        # through the subnormals to zero
    for n0, n2, n3 in qu.HWE_TABLES + [(3, 5, 40), (17, 20, 1)]:
        p = qu.hwe_p(n0, n2, n3)
        assert 0.0 <= p <= 1.0 and p == qu.hwe_p(n3, n2, n0)                             # which allele is A1 shows in no bit
    N, r, mid = qu.hwe_mid(40, 42, 11)
    assert (mid - r) % 2 == 0 and 0 <= mid <= r
    assert qu.hwe_mid(25, 50, 25)[2] == 50 and (25, 50, 25) in qu.HWE_TABLES and qu.hwe_p(25, 50, 25) == 1.0      # observed at mid: T is S


# ---- the rules ----
def one_variant(n0, n1, n2, n3):
    codes = np.array([0] * n0 + [1] * n1 + [2] * n2 + [3] * n3, dtype=np.uint8).reshape(-1, 1)
    return bedfiles.pack(codes), codes.shape[0]


def test_thresholds_are_strict_and_a_rate_on_the_threshold_stays():
    bed, I = one_variant(15, 1, 3, 1)                   # missing rate 1 / 20 = 0.05 exactly as floats; MAF 5 / 38
    assert qu.decide(bed, I, geno=0.05)["reason"][0] == qu.KEPT and qu.decide(bed, I, geno=0.049)["reason"][0] == qu.GENO
    bed, I = one_variant(81, 0, 18, 1)                  # MAF 20 / 200 = 0.1
    assert qu.maf_of([81, 0, 18, 1]) == 0.1
    assert qu.decide(bed, I, maf=0.1)["reason"][0] == qu.KEPT and qu.decide(bed, I, maf=0.1000001)["reason"][0] == qu.MAF
    p = qu.hwe_p(81, 18, 1)
    assert qu.decide(bed, I, hwe=p)["reason"][0] == qu.KEPT and qu.decide(bed, I, hwe=np.nextafter(p, 2.0))["reason"][0] == qu.HWE
    # --mind: 2 of 8 variants missing = 0.25
    codes = np.array([[0, 1, 0, 1, 2, 3, 0, 0], [0] * 8], dtype=np.uint8)
    assert list(qu.decide(bedfiles.pack(codes), 2, mind=0.25)["ind_keep"]) == [True, True]
    assert list(qu.decide(bedfiles.pack(codes), 2, mind=0.2499)["ind_keep"]) == [False, True]
    assert list(qu.decide(bedfiles.pack(codes), 2, mind=0.0)["ind_keep"]) == [False, True]       # 0 is allowed: any missing call


def test_a_variant_without_a_call_falls_to_geno_or_maf_never_to_hwe():
    bed, I = one_variant(0, 12, 0, 0)
    assert qu.decide(bed, I, geno=0.5, maf=0.01, hwe=0.5)["reason"][0] == qu.GENO        # missing rate 1
    assert qu.decide(bed, I, maf=0.01, hwe=0.5)["reason"][0] == qu.MAF                    # MAF 0 by definition
    assert qu.decide(bed, I, hwe=0.5)["reason"][0] == qu.KEPT and qu.decide(bed, I, hwe=0.5)["p"][0] == 1.0


def test_the_reason_is_the_first_rule_that_fails():
    bed, I = one_variant(0, 10, 30, 0)                  # missing 0.25, all heterozygous: MAF 0.5, p tiny
    assert qu.hwe_p(0, 30, 0) < 1e-6
    assert qu.decide(bed, I, geno=0.1, maf=0.5, hwe=0.01)["reason"][0] == qu.GENO
    assert qu.decide(bed, I, geno=0.3, maf=0.5, hwe=0.01)["reason"][0] == qu.HWE
    bed, I = one_variant(0, 10, 1, 29)                  # rare and missing
    assert qu.decide(bed, I, geno=0.1, maf=0.05)["reason"][0] == qu.GENO and qu.decide(bed, I, geno=0.3, maf=0.05)["reason"][0] == qu.MAF


def test_variant_counts_ignore_the_individuals_mind_removed():
    codes = np.zeros((6, 10), dtype=np.uint8)
    codes[0, :] = bedfiles.MISS                         # the individual --mind removes is every variant's only missing call
    codes[1, 0] = bedfiles.HET
    d = qu.decide(bedfiles.pack(codes), 6, mind=0.5, geno=0.0)
    assert list(d["ind_keep"]) == [False] + [True] * 5 and (d["reason"] == qu.KEPT).all() and (d["var"][:, 1] == 0).all()
    assert (d["var"].sum(axis=1) == 5).all()
    assert (qu.decide(bedfiles.pack(codes), 6, geno=0.0)["reason"] == qu.GENO).all()         # without --mind every variant goes


def test_composition_of_maps_against_brute_force():
    """places in the fileset after two filters: by composing the maps, and by filtering ids"""
    rng = np.random.default_rng(3)
    for n in (1, 7, 64, 200):
        ids = ["v%d" % x for x in range(n)]
        keep1 = rng.random(n) < 0.7
        keep1[rng.integers(n)] = True
        first = list(np.flatnonzero(keep1))
        left = [ids[x] for x in first]
        keep2 = rng.random(len(left)) < 0.6
        second = list(np.flatnonzero(keep2))
        survivors = [v for v, k in zip(left, keep2) if k]
        assert [ids[x] for x in qu.compose(first, second)] == survivors
        assert qu.compose(None, second) == second


# ---- mc_qc.c, and the two filters behind it, as a program of their own ----
driver = host_driver.plain_and_sanitized("qc_host", ["tests/qc_host_driver.c"] + ["multiclust_amd/host/" + f for f in ("mc_qc.c", "mc_ld.c", "mc_king.c")],
                                         werror=True)


def test_driver_stub_of_the_device_is_the_reference(driver, tmp_path):
    cases = [qu.case(I, L, seed, 0.15, extra) for I, L, extra, seed in ((1, 5, 0, 1), (5, 9, 3, 2), (33, 70, 1, 3), (66, 130, 0, 4))]
    cases += [qu.tables_from_codes(*t) for t in qu.HWE_TABLES if sum(t) <= 200]
    for bed, codes in cases:
        I = codes if isinstance(codes, int) else codes.shape[0]
        bed.tofile(str(tmp_path / "bed"))
        for name, keep in qu.keep_masks(I, I).items():
            (tmp_path / "keep").write_text("".join("1" if k else "0" for k in (keep if keep is not None else [])))
            driver("counts", I, bed.shape[0], bed.shape[1], "bed", "-" if keep is None else "keep", "ind", "var", "p", cwd=tmp_path)
            ind, var, p = qu.reference(bed, I, keep)
            assert np.array_equal(np.fromfile(str(tmp_path / "ind"), dtype=np.uint32).reshape(I, 4), ind), (I, name)
            assert np.array_equal(np.fromfile(str(tmp_path / "var"), dtype=np.uint32).reshape(-1, 4), var), (I, name)
            assert np.array_equal(np.fromfile(str(tmp_path / "p"), dtype=np.float64).view(np.uint64), p.view(np.uint64)), (I, name)


def arg(t):
    return "-" if t is None else repr(float(t))


def id_lines(fids, iids, which):
    return "".join("%s\t%s\n" % (fids[i], iids[i]) for i in range(len(iids)) if which[i])


OPTIONS = [dict(mind=qu.CLI["mind"]), dict(geno=qu.CLI["geno"]), dict(maf=qu.CLI["maf"]), dict(hwe=qu.CLI["hwe"]), dict(geno=0.99),
           dict(mind=qu.CLI["mind"], geno=qu.CLI["geno"], maf=qu.CLI["maf"], hwe=qu.CLI["hwe"])]


@pytest.mark.parametrize("prune,king", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("options", OPTIONS, ids=lambda o: "+".join(sorted(o)))
def test_driver_data_set_lists_and_chained_filters(driver, tmp_path, options, prune, king):
    """mc_qc_data on the fixture of the command-line tests, the device stubbed, then mc_ld_prune_data and mc_king_data on what it left:
    the line, who and what is kept, the maps as places in the fileset, the ids and locales numbered anew, the records, and every file
    byte for byte against the restated pipeline"""
    codes, fids, iids, chrom = qu.cli_case()
    I, L = codes.shape
    bed = qu.repack(codes, 3, 0)
    bed.tofile(str(tmp_path / "bed"))
    ids = ["rs%d" % (7 * l) for l in range(L)]
    (tmp_path / "fam").write_text("".join("%s %s\n" % (f, i) for f, i in zip(fids, iids)))
    (tmp_path / "bim").write_text("".join("%s %s\n" % (c, v) for c, v in zip(chrom, ids)))
    o = dict(dict(mind=None, geno=None, maf=None, hwe=None), **options)
    driver("chain", I, L, bed.shape[1], "bed", "fam", "bim", "stem", "fields", arg(o["mind"]), arg(o["geno"]), arg(o["maf"]), arg(o["hwe"]),
           repr(qu.CLI["prune_t"]) if prune else "-", qu.CLI["prune_window"], repr(qu.CLI["king_t"]) if king else "-", cwd=tmp_path)
    want = qu.pipeline(codes, chrom, prune=prune, king=king, **o)
    qc, rows, cols = want["qc"], want["rows"], want["cols"]
    got = (tmp_path / "fields").read_text().split("\n")
    assert got[0] + "\n" == qu.line_text(qc, **o)
    n_i, n_l = int(qc["ind_keep"].sum()), int((qc["reason"] == qu.KEPT).sum())
    head = ["qc I %d L %d" % (n_i, n_l)]
    if prune:
        head.append("prune %d of %d" % (len(cols), want["seen"]["prune"]))
        assert want["seen"]["prune"] == n_l
    if king:
        n_pairs = int(king_util.related(want["phi"], qu.CLI["king_t"]).sum()) // 2
        head.append("king %d of %d pairs %d" % (len(rows), want["seen"]["king"], n_pairs))
        assert want["seen"]["king"] == n_i and n_pairs >= 1
    thin_i, thin_l = len(rows) < I, len(cols) < L
    pops = []
    for i in rows:
        if fids[i] not in pops:
            pops.append(fids[i])
    head.append("I %d I_file %d L %d L_file %d record_bytes %d numpops %d" % (len(rows), I, len(cols), L, (len(rows) + 3) // 4, len(pops)))
    head.append(" ".join(["variant_of"] + ["%d" % l for l in cols]) if thin_l else "variant_of")
    head.append(" ".join(["individual_of"] + ["%d" % i for i in rows]) if thin_i else "individual_of")
    body = ["%s %d %s" % (iids[i], pops.index(fids[i]), fids[i]) for i in rows] + ["pop %s %d" % (p, sum(fids[i] == p for i in rows)) for p in pops]
    records = bedfiles.pack(codes[np.ix_(rows, cols)], padding=0) if thin_i else bed[cols]
    assert got[1:] == head + body + [(records.tobytes() + bytes(8)).hex(), ""]
    # the files
    files = {f: (tmp_path / f).read_text() for f in os.listdir(str(tmp_path)) if f.startswith("stem.")}
    expect = {"stem.qc.var.txt": qu.var_table_text(qc, ids), "stem.qc.ind.txt": qu.ind_table_text(qc, fids, iids, L)}
    if o["mind"] is not None:
        expect["stem.mind.in"], expect["stem.mind.out"] = id_lines(fids, iids, qc["ind_keep"]), id_lines(fids, iids, ~qc["ind_keep"])
    if any(o[k] is not None for k in ("geno", "maf", "hwe")):
        expect["stem.qc.in"] = "".join(ids[l] + "\n" for l in range(L) if qc["reason"][l] == qu.KEPT)
        expect["stem.qc.out"] = "".join(ids[l] + "\n" for l in range(L) if qc["reason"][l] != qu.KEPT)
    if prune:       # the final kept ids, and everything else of the file
        expect["stem.prune.in"] = "".join(ids[l] + "\n" for l in cols)
        expect["stem.prune.out"] = "".join(ids[l] + "\n" for l in range(L) if l not in set(cols))
    if king:
        final = np.isin(np.arange(I), rows)
        expect["stem.king.cutoff.in"], expect["stem.king.cutoff.out"] = id_lines(fids, iids, final), id_lines(fids, iids, ~final)
        seen = want["rows_seen"]
        expect["stem.king.kin0"] = king_util.kin0_text(codes[np.ix_(seen, cols)], [fids[i] for i in seen], [iids[i] for i in seen], qu.CLI["king_t"])
    assert files == expect


def test_driver_ends_on_an_emptied_data_set(driver, tmp_path):
    """the message names the option that took the last variant or every individual; nothing is passed on and no file is written"""
    I, L = 40, 6
    (tmp_path / "fam").write_text("".join("f%d i%d\n" % (i % 2, i) for i in range(I)))
    (tmp_path / "bim").write_text("".join("1 rs%d\n" % l for l in range(L)))
    rb = (I + 3) // 4

    def chain(codes, *thresholds):
        qu.repack(codes, 3, 0).tofile(str(tmp_path / "bed"))
        return driver("chain", I, L, rb, "bed", "fam", "bim", "stem", "fields", *thresholds, "-", 20, "-", cwd=tmp_path)

    res = chain(np.full((I, L), bedfiles.HOM1, dtype=np.uint8), "-", "-", "0.01", "0.5")       # monomorphic: --maf takes all, --hwe nothing
    assert (tmp_path / "fields").read_text() == "emptied 11 calls 1\n" and "--maf 0.01 removes the last of the 6 variants" in res.stderr
    res = chain(np.full((I, L), bedfiles.HET, dtype=np.uint8), "-", "0.5", "0.5", "0.001")    # all heterozygous: MAF 0.5 stays, p is tiny
    assert (tmp_path / "fields").read_text() == "emptied 11 calls 1\n" and "--hwe 0.001 removes the last of the 6 variants" in res.stderr
    codes = np.full((I, L), bedfiles.HET, dtype=np.uint8)
    codes[:, 0] = bedfiles.MISS                      # everybody has a missing call: --mind 0 leaves nobody, and the second call is not made
    res = chain(codes, "0", "-", "-", "-")
    assert (tmp_path / "fields").read_text() == "emptied 11 calls 1\n" and "--mind 0 removes every one of the 40 individuals" in res.stderr
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("stem.")]


# ---- the launch geometry ----
def test_qc_geometry(tmp_path):
    exe = host_driver.build(tmp_path, "qc_geometry", ["tests/qc_geometry_driver.cpp"], cxx=True, werror=True)
    cases = [(I, L, target) for I in (1, 31, 32, 33, 256, 257, 2048, 2049, 6149, 10000, 2 ** 30 - 1)
             for L in (1, 4, 5, 64, 65, 600, 1100, 100000, 2 ** 31 - 1) for target in (1, 256, 256 * 64, 256 * 4096, 2 ** 40)]
    named = {(name, knob): (g["I"], g["L"], knob * 256) for name, g in qu.GEOMETRY.items() for knob in (1, 64, 4096)}
    cases += list(named.values())
    res = host_driver.run(exe, stdin="".join("%d %d %d\n" % c for c in cases), quiet_stderr=True)
    rows = [tuple(int(x) for x in line.split()) for line in res.stdout.splitlines()]
    assert len(rows) == len(cases)
    cut = set()
    for (I, L, target), row in zip(cases, rows):
        assert row[:3] == (qu.QC_VARIANTS, qu.QC_STEP, qu.QC_ITILE)
        n_vg, v_split, v_per, n_it, i_split, i_per = row[3:]
        assert qu.qc_geometry(I, L, target) == row[3:]                 # the restatement the GPU test reads its geometry from
        assert n_vg == -(-L // qu.QC_VARIANTS) and n_it == -(-I // qu.QC_ITILE)      # every variant in one group, every individual in one tile
        steps, words = -(-(-(-I // 32)) // qu.QC_STEP), -(-L // 64)
        for base, n_split, per, units in ((n_vg, v_split, v_per, steps), (n_it, i_split, i_per, words)):
            assert 1 <= n_split <= min(units, 65535) and per >= 1
            assert (n_split - 1) * per < units <= n_split * per            # every unit in one run, no run empty
            if n_split > 1:
                assert base * (n_split - 1) < target                       # cut only on the way to the target
            cut.add(n_split > 1)
    assert cut == {False, True}
    got = {key: (rows[cases.index(c)][4], rows[cases.index(c)][5], rows[cases.index(c)][7], rows[cases.index(c)][8]) for key, c in named.items()}
    assert got[("steps", 1)] == (2, 2, 10, 1) and got[("steps", 64)] == (4, 1, 10, 1)
    assert got[("whole", 1)] == (1, 4, 9, 2) and got[("whole", 64)] == (4, 1, 18, 1)
    assert got[("words", 1)] == (1, 1, 172, 3) and got[("words", 64)] == (1, 1, 514, 1)


# ---- mutants: each has to be told from the definition on the cases the tests use ----
def test_mutants_of_the_counts_are_caught():
    bed, codes = qu.case(33, 70, 3, 0.15, 1)
    keep = qu.keep_masks(33, 1)["drawn"]
    ind, var = qu.counts(bed, 33, keep)
    for mutant in qu.COUNT_MUTANTS:
        assert not np.array_equal(qu.counts(bed, 33, keep, mutant)[1], var), mutant
    # on the fixture of the command-line tests the decisions change as well
    codes, fids, iids, chrom = qu.cli_case()
    opts = {k: qu.CLI[k] for k in ("mind", "geno", "maf", "hwe")}
    cli_bed = qu.repack(codes, 3, 2)
    good = qu.decide(cli_bed, codes.shape[0], **opts)
    for mutant in ("padding bits counted", "keep mask ignored"):
        bad = qu.decide(cli_bed, codes.shape[0], mutant=mutant, **opts)
        assert not np.array_equal(bad["var"], good["var"]) and not np.array_equal(bad["reason"], good["reason"]), mutant


def test_mutants_of_the_walk_are_caught():
    for mutant in qu.HWE_MUTANTS:
        differ = [t for t in qu.HWE_TABLES if qu.hwe_p(*t, mutant=mutant) != qu.hwe_p(*t)]
        print("%-30s %d of %d tables differ" % (mutant, len(differ), len(qu.HWE_TABLES)))
        assert differ, mutant       # (a walk from another start has the same p up to its roundings: the bits tell it, nothing coarser would)
    codes, fids, iids, chrom = qu.cli_case()
    var = qu.counts(bedfiles.pack(codes), codes.shape[0])[1]
    for mutant in qu.HWE_MUTANTS:
        assert not np.array_equal(qu.hwe_p_of(var, mutant).view(np.uint64), qu.hwe_p_of(var).view(np.uint64)), mutant


def test_mutant_of_the_comparisons_is_caught():
    bed, I = one_variant(15, 1, 3, 1)
    assert qu.decide(bed, I, geno=0.05, mutant=qu.RULE_MUTANTS[0])["reason"][0] == qu.GENO
    codes, fids, iids, chrom = qu.cli_case()
    opts = dict(mind=0.2, geno=0.15, maf=2 / 114, hwe=qu.CLI["hwe"])      # thresholds that rates of the fixture sit on
    good, bad = (qu.decide(bedfiles.pack(codes), codes.shape[0], mutant=m, **opts) for m in (None, qu.RULE_MUTANTS[0]))
    assert not np.array_equal(good["reason"], bad["reason"])


# ---- the fixture of the command-line tests ----
def test_cli_fixture_holds_what_it_plants():
    codes, fids, iids, chrom = qu.cli_case()
    I, L = codes.shape
    assert (I, L) == (qu.CLI["I"], qu.CLI["L"])
    opts = {k: qu.CLI[k] for k in ("mind", "geno", "maf", "hwe")}
    d = qu.decide(bedfiles.pack(codes), I, **opts)
    assert list(np.flatnonzero(~d["ind_keep"])) == [0, 17, 41] and d["ind"][0, 1] == L
    n = {r: int((d["reason"] == r).sum()) for r in range(4)}
    print("kept %d, geno %d, maf %d, hwe %d" % (n[0], n[1], n[2], n[3]))
    assert n[qu.GENO] >= 15 and n[qu.MAF] >= 30 and n[qu.HWE] >= 6 and n[qu.KEPT] > L // 2
    assert (d["reason"][196:204] == qu.KEPT).all()
    alone = qu.decide(bedfiles.pack(codes), I, hwe=qu.CLI["hwe"])
    assert (alone["reason"] == qu.HWE).sum() >= n[qu.HWE]
    assert (alone["var"].sum(axis=1) == I).all() and (d["var"].sum(axis=1) == I - 3).all()
    # chained: --prune keeps 196 and, across the boundary of the chromosomes, 200; --king-cutoff removes the later of the duplicates
    full = qu.pipeline(codes, chrom, prune=True, king=True, **opts)
    assert 196 in full["cols"] and 200 in full["cols"] and not set(full["cols"]) & {197, 198, 199, 201, 202, 203}
    assert 12 in full["rows"] and 33 not in full["rows"] and 50 not in full["rows"] and len(full["rows"]) % 4 != 0
    kept_fids = [fids[i] for i in full["rows"]]
    assert "fam9" not in kept_fids and "fam8" not in kept_fids and kept_fids[0] == "fam1"      # the locales are numbered anew
