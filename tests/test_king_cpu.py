"""Removal of relatives on the CPU (no GPU): the reference kinship of tests/king_util.py against exact rationals of KING's eq. 11 in
its three-term form, the properties of the greedy rule, the libc functions of multiclust_amd/host/mc_king.c as a program of their
own (tests/king_host_driver.c, plain and under AddressSanitizer + UBSan) against king_util, the launch geometry of the pair kernel,
the mutants of the definition and of the rule that the cases of the GPU tests have to tell from the real thing, and the fixture of
the command-line tests.

There is no tolerance in this file.  The counts are integers; num and 4 m stay below 2^33 for L < 2^31, so their conversions to
double are exact and the one division is the correctly rounded quotient: float(Fraction) of the same rational, bit for bit."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import bedfiles
from cli_util import BIN, ROOT
import host_driver
import king_util as ku


@pytest.fixture(autouse=True, scope="module")
def the_feature_is_there():
    """every test of this file is about --king-cutoff: the restatements and fixtures below are held to something only in a tree that
    has the entry point and the host unit they restate"""
    from multiclust_amd import hip
    assert "mchip_bed_king" in hip.ABI_SYMBOLS and os.path.exists(os.path.join(ROOT, "multiclust_amd", "host", "mc_king.c"))


# ---- the definition ----
def pair_counts(x, y):
    """n, hh, op, h_xy, h_yx of two individuals' codes, one variant at a time"""
    n = hh = op = hxy = hyx = 0
    for a, b in zip(x, y):
        if a == bedfiles.MISS or b == bedfiles.MISS:
            continue
        n += 1
        hh += a == bedfiles.HET and b == bedfiles.HET
        op += (a, b) in ((bedfiles.HOM1, bedfiles.HOM2), (bedfiles.HOM2, bedfiles.HOM1))
        hxy += a == bedfiles.HET
        hyx += b == bedfiles.HET
    return n, hh, op, hxy, hyx


def eq11(hh, op, hxy, hyx):
    """Manichaikul et al. (2010), eq. 11, as it is printed: three terms"""
    m = min(hxy, hyx)
    return Fraction(hh - 2 * op, 2 * m) + Fraction(1, 2) - Fraction(hxy + hyx, 4 * m)


def test_reference_is_the_rounded_rational_of_eq_11():
    codes = ku.draw_codes(33, 150, seed=1, missing=0.2)
    where = ku.plant(codes, seed=1)
    phi, cnt = ku.kinship(codes)
    seen = 0
    for i in range(33):
        for j in range(33):
            n, hh, op, hxy, hyx = pair_counts(codes[i], codes[j])
            assert (n, hh, op, hxy) == tuple(int(v) for v in cnt[i, j]) and hyx == cnt[j, i, 3]
            if min(hxy, hyx) == 0:
                assert np.isnan(phi[i, j])
                continue
            assert phi[i, j] == float(eq11(hh, op, hxy, hyx)) and phi[i, j] <= 0.5
            seen += 1
    assert seen > 900 and np.isnan(phi[where["missing"]]).all() and np.isnan(phi[where["nohet"]]).all()
    assert ku.same_bits(phi, phi.T) and phi[where["dup"], where["dup_of"]] > 0.45
    assert ku.same_bits(*(ku.kinship(codes, 7, 9)[0], phi[7:16])) and np.array_equal(ku.kinship(codes, 7, 9)[1], cnt[7:16])


def test_nan_exactly_when_the_smaller_heterozygote_count_is_zero():
    H1, MS, HT, H2 = bedfiles.HOM1, bedfiles.MISS, bedfiles.HET, bedfiles.HOM2
    cases = {
        "no heterozygous call": ([H1, H2, H1, H2], [HT, HT, H1, H2], True),
        "heterozygous only where the other is missing": ([HT, H1, H2, H1], [MS, HT, HT, H2], True),
        "all missing": ([MS] * 4, [HT, HT, H1, H2], True),
        "one shared typed heterozygote each": ([HT, H1, MS, MS], [H2, HT, HT, HT], False),
        "a duplicate": ([HT, H1, H2, HT], [HT, H1, H2, HT], False),
    }
    for name, (x, y, nan) in cases.items():
        phi, _ = ku.kinship(np.array([x, y], dtype=np.uint8))
        assert np.isnan(phi[0, 1]) == np.isnan(phi[1, 0]) == nan, name
    assert phi[0, 1] == 0.5 and phi[0, 0] == 0.5


def test_kinships_of_the_planted_pedigree():
    """the estimator does what it is chosen for: a duplicate at 0.5, first-degree pairs near 0.25, unrelated pairs near 0 and
    pairs across the two populations below"""
    codes, planted, pop = ku.pedigree(3, 20000)
    phi, _ = ku.kinship(codes)
    I = len(pop)
    for i in range(I):
        for j in range(i + 1, I):
            if (i, j) in planted:
                assert phi[i, j] == 0.5 or 0.22 < phi[i, j] < 0.28, (i, j, phi[i, j])
            elif pop[i] == pop[j]:
                assert abs(phi[i, j]) < 0.03, (i, j, phi[i, j])
            else:
                assert phi[i, j] < -0.05, (i, j, phi[i, j])


# ---- the rule ----
def brute_force(rel):
    """the rule once more, with sets: nothing shared with king_util.greedy"""
    I = len(rel)
    left = set(range(I))
    while True:
        partners = {i: sum(1 for j in left if j != i and rel[i][j]) for i in left}
        most = max(partners.values())
        if most == 0:
            return np.array([i in left for i in range(I)])
        left.remove(max(i for i in left if partners[i] == most))


def graph(I, edges):
    rel = np.zeros((I, I), dtype=bool)
    for i, j in edges:
        rel[i, j] = rel[j, i] = True
    return rel


def random_graph(I, p, seed):
    rng = np.random.default_rng(seed)
    up = np.triu(rng.random((I, I)) < p, 1)
    return up | up.T


def test_rule_on_small_graphs():
    assert ku.greedy(graph(5, [])).all()                                                      # nobody related: everybody stays
    assert list(np.flatnonzero(~ku.greedy(graph(6, [(0, 3), (1, 5), (2, 4)])))) == [3, 4, 5]   # disjoint pairs lose the later member
    assert list(np.flatnonzero(~ku.greedy(graph(6, [(2, 0), (2, 1), (2, 4), (2, 5)])))) == [2]  # a star loses its centre
    assert list(np.flatnonzero(ku.greedy(graph(4, [(i, j) for i in range(4) for j in range(i)])))) == [0]   # a clique keeps the first
    assert ku.greedy(graph(1, [])).all()


@pytest.mark.parametrize("I,p,seed", [(5, 0.5, 1), (17, 0.1, 2), (17, 0.4, 3), (40, 0.05, 4), (70, 0.03, 5), (70, 0.5, 6), (130, 0.02, 7)])
def test_rule_properties_and_brute_force_on_random_graphs(I, p, seed):
    rel = random_graph(I, p, seed)
    keep = ku.greedy(rel)
    assert keep.any() and not rel[np.ix_(keep, keep)].any()         # no two kept individuals are related
    for i in np.flatnonzero(~keep):
        assert rel[i].any()                                          # nobody is removed without a relative
    assert np.array_equal(keep, brute_force(rel.tolist()))


# ---- mc_king.c as a program of its own ----
driver = host_driver.plain_and_sanitized("king_host", ["tests/king_host_driver.c", "multiclust_amd/host/mc_king.c"], werror=True,
                                         result=lambda res: res.stdout)


def test_driver_band_restatement_is_the_reference(driver, tmp_path):
    for I, L, extra, seed in ((1, 5, 0, 1), (5, 9, 3, 2), (33, 70, 1, 3), (66, 130, 0, 4)):
        codes = ku.draw_codes(I, L, seed, missing=0.2)
        ku.plant(codes, seed)
        bed = ku.repack(codes, seed, extra)
        bed.tofile(str(tmp_path / "bed"))
        for i0, n_rows in ((0, I), (I // 3, I - I // 3), (I - 1, 1)):
            driver("band", I, L, bed.shape[1], i0, n_rows, "bed", "phi", "counts", cwd=tmp_path)
            phi = np.fromfile(str(tmp_path / "phi"), dtype=np.float64).reshape(n_rows, I)
            cnt = np.fromfile(str(tmp_path / "counts"), dtype=np.uint32).reshape(n_rows, I, 4)
            want_phi, want_cnt = ku.kinship(codes, i0, n_rows)
            assert ku.same_bits(phi, want_phi) and np.array_equal(cnt, want_cnt), (I, L, i0)


def test_driver_select_is_the_rule(driver, tmp_path):
    cases = [random_graph(I, p, seed) for I, p, seed in ((1, 0.5, 1), (9, 0.4, 2), (64, 0.05, 3), (65, 0.3, 4), (130, 0.02, 5), (200, 0.01, 6))]
    cases += [graph(6, [(0, 3), (1, 5), (2, 4)]), graph(6, [(2, 0), (2, 1), (2, 4), (2, 5)]), graph(7, [])]
    for rel in cases:
        (tmp_path / "rel").write_text("".join("1" if v else "0" for v in rel.ravel()))
        driver("select", len(rel), "rel", "keep", cwd=tmp_path)
        assert (tmp_path / "keep").read_text() == "".join("1" if k else "0" for k in ku.greedy(rel)), len(rel)


def test_driver_compaction_at_every_residue_with_dirty_padding(driver, tmp_path):
    """I' = 1 ... 9 out of I = 11 and 12 (every I' mod 4 from either I mod 4), all and one kept; garbage in the padding bits and in two
    bytes behind every record: the records come out ceil(I'/4) bytes long, codes unchanged, padding bits 0, 8 zero bytes behind"""
    rng = np.random.default_rng(5)
    L = 7
    for I in (11, 12):
        codes = ku.draw_codes(I, L, seed=I, missing=0.2)
        bed = ku.repack(codes, I, 2)
        keeps = [np.ones(I, bool)] + [np.isin(np.arange(I), rng.permutation(I)[:n]) for n in range(1, 10)]
        for keep in keeps:
            (tmp_path / "keep").write_text("".join("1" if k else "0" for k in keep))
            bed.tofile(str(tmp_path / "bed"))
            out = driver("compact", I, L, bed.shape[1], "keep", "bed", "out", "map", cwd=tmp_path)
            n = int(keep.sum())
            assert int(out) == n
            want = bedfiles.pack(codes[keep], padding=0)
            assert want.shape == (L, (n + 3) // 4)
            assert (tmp_path / "out").read_bytes() == want.tobytes() + bytes(8), (I, n)
            assert [int(x) for x in (tmp_path / "map").read_text().split()] == list(np.flatnonzero(keep))


@pytest.mark.parametrize("slab", [1, 5, 24, ku.SLAB])
def test_driver_data_set_and_the_three_files(driver, tmp_path, slab):
    """mc_king_data on the fixture of the command-line tests, the device stubbed: who is kept, the ids, the locales numbered anew in
    order of first appearance among the kept, the records, and the three files byte for byte"""
    codes, planted, fids, iids = ku.cli_case()
    I, L, t = codes.shape[0], codes.shape[1], ku.CLI["t"]
    bed = ku.repack(codes, 3, 0)
    bed.tofile(str(tmp_path / "bed"))
    (tmp_path / "fam").write_text("".join("%s %s\n" % (f, i) for f, i in zip(fids, iids)))
    driver("data", I, L, bed.shape[1], t, slab, "bed", "fam", "stem", "fields", cwd=tmp_path)
    phi, cnt = ku.kinship(codes)
    keep = ku.greedy(ku.related(phi, t))
    kept = list(np.flatnonzero(keep))
    pops = []
    for i in kept:
        if fids[i] not in pops:
            pops.append(fids[i])
    file_pops = []
    for f in fids:
        if f not in file_pops:
            file_pops.append(f)
    assert pops != file_pops[:len(pops)] and len(pops) < len(file_pops)      # the case tells a re-derived numbering from the file's
    want = ["I %d I_file %d record_bytes %d numpops %d pairs %d" % (len(kept), I, (len(kept) + 3) // 4, len(pops), len(planted))]
    want += ["%d %s %d %s" % (i, iids[i], pops.index(fids[i]), fids[i]) for i in kept]
    want += ["pop %s %d" % (p, sum(fids[i] == p for i in kept)) for p in pops]
    want += [(bedfiles.pack(codes[keep], padding=0).tobytes() + bytes(8)).hex()]
    assert (tmp_path / "fields").read_text().split("\n") == want + [""]
    assert (tmp_path / "stem.king.cutoff.in").read_text() == "".join("%s\t%s\n" % (fids[i], iids[i]) for i in range(I) if keep[i])
    assert (tmp_path / "stem.king.cutoff.out").read_text() == "".join("%s\t%s\n" % (fids[i], iids[i]) for i in range(I) if not keep[i])
    kin0 = ku.kin0_text(codes, fids, iids, t)
    assert (tmp_path / "stem.king.kin0").read_text() == kin0 and kin0.count("\n") == 1 + len(planted)


def test_library_select_and_compact_through_the_python_view():
    """multiclust_amd.host.king_select and king_compact call the functions of the built library: the same answers as the driver's"""
    from multiclust_amd import host
    for I, p, seed in ((1, 0.5, 1), (63, 0.1, 2), (64, 0.1, 3), (65, 0.1, 4), (130, 0.03, 5)):
        rel = random_graph(I, p, seed)
        assert np.array_equal(host.king_select(rel, I), ku.greedy(rel)), I
    codes = ku.draw_codes(13, 9, seed=8, missing=0.2)
    keep = np.arange(13) % 3 != 1
    bed, of = host.king_compact(13, ku.repack(codes, 8, 1), keep)
    assert np.array_equal(bed, bedfiles.pack(codes[keep], padding=0)) and list(of) == list(np.flatnonzero(keep))


# ---- the launch geometry of the pair kernel ----
def test_king_geometry(tmp_path):
    exe = host_driver.build(tmp_path, "king_geometry", ["tests/king_geometry_driver.cpp"], cxx=True, werror=True)
    cases = [(I, n, L, target) for I in (1, 63, 64, 65, 130, 10000, 2 ** 29) for n in (1, 64, 65, 1024) if n <= I
             for L in (1, 256, 257, 1100, 100000, 2 ** 31 - 1) for target in (1, 256, 256 * 8, 256 * 4096, 2 ** 40)]
    # the launches of tests/test_gpu_king.py's geometry test, on 256 compute units
    named = {(name, knob): (g["I"], g["I"], g["L"], knob * 256) for name, g in ku.GEOMETRY.items() for knob in (1, 64, 4096)}
    cases += list(named.values())
    res = host_driver.run(exe, stdin="".join("%d %d %d %d\n" % c for c in cases), quiet_stderr=True)
    rows = [tuple(int(x) for x in line.split()) for line in res.stdout.splitlines()]
    assert len(rows) == len(cases)
    split_seen = set()
    for (I, n, L, target), (tile, stage, n_rt, n_ct, n_split, per) in zip(cases, rows):
        assert (tile, stage * 64) == (ku.TILE, ku.STAGE_VARIANTS)
        assert ku.king_geometry(I, n, L, target) == (n_rt, n_ct, n_split, per)       # the restatement the GPU test reads its geometry from
        assert n_rt == -(-n // tile) and n_ct == -(-I // tile)                      # every row and every column in one tile
        stages = -(-(-(-L // 64)) // stage)
        assert 1 <= n_split <= min(stages, 65535) and per >= 1
        assert (n_split - 1) * per < stages <= n_split * per                          # every stage in one run, no run empty
        if n_split > 1:
            assert n_rt * n_ct * (n_split - 1) < target                               # cut only on the way to the target
        split_seen.add(n_split > 1)
        assert n_rt * n_ct < 2 ** 31 or n > 1024
    assert split_seen == {False, True}
    got = {key: rows[cases.index(case)][4:] for key, case in named.items()}
    assert got[("fixed", 1)] == got[("fixed", 64)] == got[("fixed", 4096)] == (5, 1)      # 9 tiles: one stage a workgroup under every knob
    assert got[("whole", 1)] == (1, 5) and got[("runs", 1)] == (3, 2) and got[("runs", 64)] == got[("runs", 4096)] == (5, 1)


# ---- mutants: each has to be told from the definition on the cases the GPU tests use ----
def cases_of_the_gpu_tests():
    yield ku.cli_case()[0]
    yield ku.fixed_case()[1]


@pytest.mark.parametrize("mutant", ku.MUTANTS)
def test_mutants_of_the_definition_are_caught(mutant):
    for codes in cases_of_the_gpu_tests():
        phi, cnt = ku.kinship(codes)
        bad_phi, bad_cnt = ku.kinship(codes, mutant=mutant)
        assert not (ku.same_bits(phi, bad_phi) and np.array_equal(cnt, bad_cnt)), mutant
        rel, bad_rel = ku.related(phi, ku.CLI["t"]), ku.related(bad_phi, ku.CLI["t"])
        differ = ~((phi == bad_phi) | (np.isnan(phi) & np.isnan(bad_phi)))
        print("%-32s %d of %d kinships differ, %d edges at 0.125" % (mutant, int(differ.sum()), phi.size, int((rel != bad_rel).sum()) // 2))
        assert not ku.same_bits(phi, bad_phi), mutant


def test_the_tie_going_to_the_lowest_index_is_caught():
    codes, planted, fids, iids = ku.cli_case()
    rel = ku.related(ku.kinship(codes)[0], ku.CLI["t"])
    assert not np.array_equal(ku.greedy(rel), ku.greedy(rel, tie="lowest"))
    assert not np.array_equal(ku.greedy(graph(2, [(0, 1)])), ku.greedy(graph(2, [(0, 1)]), tie="lowest"))


# ---- the fixture of the command-line tests ----
def test_cli_fixture_relates_exactly_the_planted_pairs():
    codes, planted, fids, iids = ku.cli_case()
    I = codes.shape[0]
    assert codes.shape == (ku.CLI["I"], ku.CLI["L"]) and len(planted) == 17
    phi, cnt = ku.kinship(codes)
    rel = ku.related(phi, ku.CLI["t"])
    assert {(i, j) for i in range(I) for j in range(i + 1, I) if rel[i, j]} == planted
    dup = [(i, j) for i, j in planted if phi[i, j] > 0.4]
    assert len(dup) == 1 and all(0.18 < phi[i, j] < 0.32 for i, j in planted if (i, j) != dup[0])
    assert max(phi[i, j] for i in range(I) for j in range(i + 1, I) if (i, j) not in planted) < 0.1
    keep = ku.greedy(rel)
    assert 12 <= keep.sum() < I and keep.sum() % 4 != 0 and not rel[np.ix_(keep, keep)].any()


# ---- the command line (parse_options runs before any file or device is opened) ----
@pytest.mark.parametrize("args,why", [
    (["-f", "x.stru", "--king-cutoff", "0.125"], "--king-cutoff needs a PLINK fileset (--bed)"),
    (["--bed", "x", "--king-cutoff", "0"], "the kinship threshold of --king-cutoff must lie in (0, 0.5)"),
    (["--bed", "x", "--king-cutoff", "0.5"], "the kinship threshold of --king-cutoff must lie in (0, 0.5)"),
    (["--bed", "x", "--king-cutoff", "-0.1"], "the kinship threshold of --king-cutoff must lie in (0, 0.5)"),
    (["--bed", "x", "--king-cutoff", "nan"], "the kinship threshold of --king-cutoff must lie in (0, 0.5)"),
])
def test_refused_setups(args, why, tmp_path):
    res = subprocess.run([BIN, "-a", "-k", "2"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, cwd=str(tmp_path))
    assert res.returncode == 10, (args, res.returncode, res.stderr[-500:])       # MC_EXIT_INVALID_CMD_ARGUMENT: the usual refuse()
    assert "ERROR [mc_main.c::parse_options]: " + why + " (argument '--king-cutoff')" in res.stderr and res.stdout == ""


def test_k_keeps_its_meaning_and_the_option_is_matched_in_full(tmp_path):
    """-k <K> and anything that merely begins like the new option are still the number of clusters"""
    res = subprocess.run([BIN, "--king", "0.1", "--bed", "none", "-a"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60,
                         cwd=str(tmp_path))
    assert res.returncode == 10 and "-k" in res.stderr and "king-cutoff" not in res.stderr      # 0.1 is no number of clusters
    res = subprocess.run([BIN, "-k", "3", "--king-cutoff", "0.2", "--bed", "none", "-a"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         timeout=60, cwd=str(tmp_path))
    assert res.returncode == 5 and "king" not in res.stderr       # the fileset does not exist: the options were accepted
