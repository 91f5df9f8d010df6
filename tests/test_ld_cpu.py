"""LD pruning on the CPU (no GPU): the reference r2 of tests/ld_util.py against exact rationals, where it is NaN, its invariance under
a swap of the alleles, the properties of the forward greedy rule, the libc functions of multiclust_amd/host/mc_ld.c as a program of
their own (tests/ld_host_driver.c, plain and under AddressSanitizer + UBSan) against ld_util on the same bands, and the mutants of the
definition and of the rule that the cases of the GPU tests have to tell from the real thing.

Bounds.  r2 = (c * c) / (vx * vy) with c, vx, vy the conversions of exact integers.  While C^2 and Vx Vy stay below 2^53 the
conversions and both products are exact and the division is the correctly rounded quotient: equal to the rounded rational, bit for
bit.  Beyond that there are three conversions (c's enters squared) and three operations, seven factors (1 + e), |e| <= 2^-53: at
most 3.5 * 2^-52 relative in the worst case, and the errors of drawn cases are of both signs; the bound asserted on the drawn cases
is 2 ulp of the rounded rational, and the worst distance seen is printed."""
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import bedfiles
from cli_util import BIN
import host_driver
import ld_util as lu


def exact(n, Sx, Sy, Sxx, Syy, Sxy):
    C, Vx, Vy = lu.cvv(n, Sx, Sy, Sxx, Syy, Sxy)
    return Fraction(C * C, Vx * Vy)


# ---- the definition ----
def test_reference_is_the_rounded_rational_on_drawn_records():
    """every pair of a drawn panel: all integers far below 2^53, so equality"""
    bed, codes = lu.draw_records(37, 40, seed=1, missing=0.2)
    lu.plant(codes, seed=1)
    rows = codes.T
    seen = 0
    for a in range(40):
        for b in range(a + 1, 40):
            s = lu.sums(rows[a], rows[b])
            C, Vx, Vy = lu.cvv(*s)
            r = lu.r2_of_sums(*s)
            if Vx == 0 or Vy == 0:
                assert np.isnan(r)
                continue
            assert C * C < 2 ** 53 and Vx * Vy < 2 ** 53
            assert r == float(exact(*s)) and 0.0 <= r <= 1.0
            seen += 1
    assert seen > 500


def test_reference_within_2_ulp_with_large_integers():
    """sums of panels of up to 2^29 individuals, drawn as the nine cells of the dosage table: C^2 and Vx Vy reach 2^120"""
    rng = np.random.default_rng(2)
    worst, big = 0, 0
    for case in range(400):
        scale = int(rng.integers(1, 2 ** 25))
        cell = [[int(v) for v in row] for row in rng.integers(0, scale, size=(3, 3))]
        n = sum(map(sum, cell))
        Sx = sum(x * cell[x][y] for x in range(3) for y in range(3))
        Sy = sum(y * cell[x][y] for x in range(3) for y in range(3))
        Sxx = sum(x * x * cell[x][y] for x in range(3) for y in range(3))
        Syy = sum(y * y * cell[x][y] for x in range(3) for y in range(3))
        Sxy = sum(x * y * cell[x][y] for x in range(3) for y in range(3))
        assert n < 2 ** 29
        C, Vx, Vy = lu.cvv(n, Sx, Sy, Sxx, Syy, Sxy)
        if Vx == 0 or Vy == 0:
            continue
        assert abs(C) < 2 ** 63 and Vx < 2 ** 63 and Vy < 2 ** 63      # the int64 of the device and of the driver hold them
        big += Vx * Vy >= 2 ** 53
        want = float(exact(n, Sx, Sy, Sxx, Syy, Sxy))
        got = lu.r2_of_sums(n, Sx, Sy, Sxx, Syy, Sxy)
        if want == 0.0:
            assert got == 0.0 or got < 1e-300
            continue
        worst = max(worst, lu.ulp_distance(got, want))
    print("worst distance %d ulp over %d cases with products above 2^53" % (worst, big))
    assert big > 300 and worst <= 2


def test_nan_exactly_when_a_variance_is_zero():
    H1, MS, HT, H2 = bedfiles.HOM1, bedfiles.MISS, bedfiles.HET, bedfiles.HOM2
    poly = [H1, HT, H2, H1, HT, H2]
    cases = {
        "monomorphic": ([H2] * 6, poly, True),
        "all heterozygous": ([HT] * 6, poly, True),
        "all missing": ([MS] * 6, poly, True),
        "n = 0": ([H1, HT, MS, MS, MS, MS], [MS, MS, H1, HT, H2, H1], True),
        "n = 1": ([H1, MS, MS, MS, MS, MS], [H2, H1, HT, H2, H1, HT], True),
        "monomorphic among the typed": ([H1, H1, HT, H2, MS, MS], [MS, MS, H2, H2, H1, HT][::-1], None),
        "n = 2": ([H1, H2, MS, MS, MS, MS], [HT, H1, H2, H2, H2, H2], False),
        "polymorphic": (poly, poly[::-1], False),
    }
    for name, (x, y, nan) in cases.items():
        C, Vx, Vy = lu.cvv(*lu.sums(x, y))
        r = lu.r2_pair(x, y)
        assert np.isnan(r) == (Vx == 0 or Vy == 0), name
        if nan is not None:
            assert np.isnan(r) == nan, name
        assert np.isnan(lu.r2_pair(y, x)) == np.isnan(r)
    assert lu.r2_pair(poly, poly) == 1.0 and lu.r2_pair(poly, poly[::-1]) == 1.0


def test_swapping_the_alleles_of_either_variant_changes_no_bit():
    bed, codes = lu.draw_records(61, 30, seed=3, missing=0.15)
    swap = np.array([3, 1, 2, 0], dtype=np.uint8)
    rows = codes.T
    for a in range(0, 29):
        x, y = rows[a], rows[a + 1]
        base = lu.r2_pair(x, y)
        for xx, yy in ((swap[x], y), (x, swap[y]), (swap[x], swap[y])):
            assert lu.same_bits(lu.r2_pair(xx, yy), base)
        assert lu.same_bits(lu.r2_pair(y, x), base)


def test_vector_band_is_the_pairwise_definition():
    I, L, W = 45, 23, 27
    bed, codes = lu.draw_records(I, L, seed=4, missing=0.2, extra_bytes=2)
    assert np.array_equal(lu.codes_of(bed, I), codes.T)
    want = np.full((L, W), np.nan)
    for l in range(L):
        for d in range(1, W + 1):
            if l + d < L:
                want[l, d - 1] = lu.r2_pair(codes[:, l], codes[:, l + d])
    assert lu.same_bits(lu.band(bed, I, W), want)
    assert lu.same_bits(lu.band(bed, I, W, l0=5, n_first=9), want[5:14])
    assert lu.same_bits(lu.band(bed, I, 3, l0=20, n_first=3), want[20:23, :3])


# ---- the rule ----
def drawn_band(seed, L=120, W=9, I=60, chroms=2):
    bed, codes = lu.draw_records(I, L, seed=seed, copy=0.75, flip=0.04, missing=0.05)
    chrom = [str(1 + (l * chroms) // L) for l in range(L)]
    where = lu.plant(codes, seed=seed)
    return lu.band(lu.repack(codes), I, W + 1), chrom, where


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("W,t", [(1, 0.2), (4, 0.5), (9, 0.8)])
def test_greedy_properties(seed, W, t):
    r2, chrom, where = drawn_band(seed)
    L = r2.shape[0]
    keep = lu.greedy(r2, W, t, chrom)
    assert 0 < keep.sum() < L
    for l in range(L):
        partners = [lp for lp in range(max(0, l - W), l) if keep[lp] and chrom[lp] == chrom[l] and r2[lp, l - lp - 1] > t]
        assert keep[l] == (not partners)      # no two kept ones in LD within W; every removed one has a kept partner
    assert lu.greedy(r2, W, 1.0, chrom).all()
    for what in ("missing", "mono", "het"):   # NaN compares false: such a variant is never removed, and removes nothing
        l = where[what]
        assert keep[l] and np.isnan(r2[l, :W]).all()


def test_a_chromosome_boundary_splits_a_run_of_duplicates():
    I, L = 40, 12
    bed, codes = lu.draw_records(I, L, seed=9, copy=0.0)
    for l in range(3, 10):
        codes[:, l] = codes[:, 3]
    r2 = lu.band(lu.repack(codes), I, 11)
    assert (r2[3, :6] == 1.0).all()
    one = lu.greedy(r2, 11, 0.99)
    assert one[3] and not one[4:10].any()
    chrom = ["1"] * 6 + ["2"] * 6
    two = lu.greedy(r2, 11, 0.99, chrom)
    assert two[3] and not two[4:6].any() and two[6] and not two[7:10].any()


# ---- mc_ld.c as a program of its own ----
driver = host_driver.plain_and_sanitized("ld_host", ["tests/ld_host_driver.c", "multiclust_amd/host/mc_ld.c"], werror=True,
                                         result=lambda res: res.stdout)


def test_driver_greedy_is_ld_util_on_the_same_bands(driver, tmp_path):
    for seed, W, t in ((1, 1, 0.2), (2, 4, 0.5), (3, 9, 0.8), (3, 9, 1.0)):
        r2, chrom, _ = drawn_band(seed)
        L = r2.shape[0]
        np.ascontiguousarray(r2[:, :W]).tofile(str(tmp_path / "band"))
        (tmp_path / "chrom").write_text("".join(c + "\n" for c in chrom))
        for chrom_arg, ch in (("chrom", chrom), ("-", None)):
            want = "".join("1" if k else "0" for k in lu.greedy(r2, W, t, ch))
            for slab in (1, 7, L - 1, L, 65536):
                driver("greedy", L, W, t, slab, "band", chrom_arg, "keep", cwd=tmp_path)
                assert (tmp_path / "keep").read_text() == want, (seed, W, t, chrom_arg, slab)


def test_driver_compaction(driver, tmp_path):
    rng = np.random.default_rng(5)
    for L, rb in ((1, 1), (17, 3), (64, 11)):
        bed = rng.integers(0, 256, size=(L, rb), dtype=np.uint8)
        for keep in (np.ones(L, bool), np.zeros(L, bool), rng.random(L) < 0.5):
            (tmp_path / "keep").write_text("".join("1" if k else "0" for k in keep))
            bed.tofile(str(tmp_path / "bed"))
            out = driver("compact", L, rb, "keep", "bed", "out", "map", cwd=tmp_path)
            assert int(out) == keep.sum()
            assert (tmp_path / "out").read_bytes() == bed[keep].tobytes()
            assert [int(x) for x in (tmp_path / "map").read_text().split()] == list(np.flatnonzero(keep))


def test_driver_band_restatement_is_the_reference(driver, tmp_path):
    for I, L, W, extra, seed in ((1, 5, 3, 0, 1), (5, 9, 12, 3, 2), (33, 40, 7, 1, 3), (130, 25, 30, 0, 4)):
        bed, codes = lu.draw_records(I, L, seed=seed, missing=0.2, extra_bytes=extra)
        lu.plant(codes, seed=seed)
        bed = lu.repack(codes, seed, extra)
        bed.tofile(str(tmp_path / "bed"))
        for l0, n_first in ((0, L), (L // 3, L - L // 3), (L - 1, 1)):
            driver("band", I, L, bed.shape[1], W, l0, n_first, "bed", "r2", cwd=tmp_path)
            got = np.fromfile(str(tmp_path / "r2"), dtype=np.float64).reshape(n_first, W)
            assert lu.same_bits(got, lu.band(bed, I, W, l0, n_first)), (I, L, W, l0)


# ---- mutants: each has to be told from the definition on the cases the GPU tests use ----
def mutant_band(bed, I, window, dosage):
    keep = lu.DOSAGE
    try:
        lu.DOSAGE = dosage
        return lu.band(bed, I, window)
    finally:
        lu.DOSAGE = keep


def cases_of_the_gpu_tests():
    codes, chrom = lu.cli_case()
    yield lu.CLI["I"], lu.repack(codes)
    yield lu.FIXED["I"], lu.fixed_case()


@pytest.mark.parametrize("name,dosage", [("missing calls counted as dosage 0", [0, 0, 1, 2]), ("codes 1 and 2 swapped", [0, 1, -1, 2])])
def test_mutants_of_the_definition_are_caught(name, dosage):
    for I, bed in cases_of_the_gpu_tests():
        want = lu.band(bed, I, 8)
        assert lu.same_bits(lu.band(bed, I, 8), want)
        assert not lu.same_bits(mutant_band(bed, I, 8, np.array(dosage, dtype=np.int64)), want), name


def test_mutants_of_the_rule_are_caught():
    codes, chrom = lu.cli_case()
    W, t = lu.CLI["window"], lu.CLI["t"]
    r2 = lu.band(lu.repack(codes), lu.CLI["I"], W + 1)
    want = lu.greedy(r2, W, t, chrom)
    L = len(chrom)

    def reusing_removed():
        keep = np.ones(L, dtype=bool)
        for l in range(L):
            keep[l] = not any(chrom[lp] == chrom[l] and r2[lp, l - lp - 1] > t for lp in range(max(0, l - W), l))
        return keep

    mutants = {
        "window one short": lu.greedy(r2, W - 1, t, chrom),
        "window one long": lu.greedy(r2, W + 1, t, chrom),
        "the chromosome ignored": lu.greedy(r2, W, t, None),
        "removed variants still partners": reusing_removed(),
    }
    for name, keep in mutants.items():
        print("%-34s differs at %d variants" % (name, int((keep != want).sum())))
        assert not np.array_equal(keep, want), name
    assert 0.2 * L < want.sum() < 0.9 * L


# ---- the command line (parse_options runs before any file or device is opened) ----
@pytest.mark.parametrize("args,why,option", [
    (["-f", "x.stru", "--prune", "0.5"], "--prune and --prune-window need a PLINK fileset (--bed)", "--prune"),
    (["-f", "x.stru", "--prune-window", "10"], "--prune and --prune-window need a PLINK fileset (--bed)", "--prune-window"),
    (["--bed", "x", "--prune-window", "10"], "--prune-window needs --prune", "--prune-window"),
    (["--bed", "x", "--prune", "0"], "the r2 threshold of --prune must lie in (0, 1]", "--prune"),
    (["--bed", "x", "--prune", "1.5"], "the r2 threshold of --prune must lie in (0, 1]", "--prune"),
    (["--bed", "x", "--prune", "0.5", "--prune-window", "0"], "--prune-window must lie in 1 ... 4096 variants", "--prune"),
    (["--bed", "x", "--prune", "0.5", "--prune-window", "4097"], "--prune-window must lie in 1 ... 4096 variants", "--prune"),
])
def test_refused_setups(args, why, option, tmp_path):
    res = subprocess.run([BIN, "-a", "-k", "2"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, cwd=str(tmp_path))
    assert res.returncode == 11, (args, res.returncode, res.stderr[-500:])       # MC_EXIT_INVALID_USER_SETUP
    assert "ERROR [mc_main.c::parse_options]: " + why + " (argument '" + option + "')" in res.stderr


def test_projection_keeps_its_abbreviations(tmp_path):
    """--pr... is still --projection: only the two new options in full are taken for pruning"""
    res = subprocess.run([BIN, "--pr", "--pru", "--projection", "-f", "none.stru", "-k", "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=60, cwd=str(tmp_path))
    assert res.returncode == 5 and "prune" not in res.stderr       # the data file does not exist: the options were accepted
