"""-m gpu: mchip_bed_ld_band (multiclust_amd/csrc/mchip_bed.hip) against the definition restated in tests/ld_util.py, bit for bit, NaN
positions included.  Every sum of the definition is an integer, so there is no tolerance anywhere in this file.

What the cases are sized by: a workgroup owns TILE = 64 first variants and DCHUNK = 32 offsets, and stages 128 individuals (four
64-bit words of a bit plane) at a time; a record is read as 32-bit words from any byte offset, the bits behind the last individual
are masked.  So: I on either side of 32, 64 and 256 and of the record's byte and word ends, with ceil(I/4) of every residue mod 4,
and 1001 for several stages and several runs of individuals; L on either side of one and two tiles; windows on either side of the
tile and of L; records three bytes longer than they need be; garbage in every bit that carries no individual."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cli_util import ROOT
from device_util import ctx
import ld_util as lu
from multiclust_amd import hip
from synth import random_params

pytestmark = pytest.mark.gpu
IS = [1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1001]
LS = [1, 2, lu.TILE - 1, lu.TILE, lu.TILE + 1, 2 * lu.TILE - 1, 2 * lu.TILE, 2 * lu.TILE + 1]


def windows(L):
    return sorted({w for w in (1, 2, lu.TILE - 1, lu.TILE, lu.TILE + 1, L - 1, L + 5) if w >= 1})


def records(I, L, seed, missing, extra):
    bed, codes = lu.draw_records(I, L, seed=seed, missing=missing)
    where = lu.plant(codes, seed=seed)
    return lu.repack(codes, seed, extra), codes, where


def check_all_windows(ctx, I, bed):
    L = bed.shape[0]
    whole = lu.band(bed, I, max(windows(L)))
    for W in windows(L):
        got = ctx.bed_ld_band(I, bed, window=W)
        assert got.shape == (L, W)
        assert lu.same_bits(got, whole[:, :W]), (I, L, W)
    return whole


@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("I", IS)
def test_bits_at_every_individual_edge(ctx, I, extra):
    """missing rates 0 and 0.3 in turn; one variant all missing, one monomorphic, one all heterozygous, a pair of duplicates"""
    L = lu.TILE + 6
    missing = 0.3 if IS.index(I) % 2 else 0.0
    bed, codes, where = records(I, L, 100 + I, missing, extra)
    assert bed.shape[1] == (I + 3) // 4 + extra
    whole = check_all_windows(ctx, I, bed)
    for what in ("missing", "mono", "het"):
        assert np.isnan(whole[where[what]]).all() and np.isnan(whole[where[what] - 1, 0])
    if I >= 31 and not missing:
        assert whole[where["dup"], 0] == 1.0


@pytest.mark.parametrize("L", LS)
def test_bits_on_either_side_of_the_variant_tile(ctx, L):
    bed, codes, where = records(33, L, 200 + L, 0.3, 0)
    check_all_windows(ctx, 33, bed)


def test_band_is_not_all_nan_and_has_real_ld(ctx):
    """what the comparisons above compare: finite values in [0, 1] almost everywhere, neighbours in LD"""
    bed, codes, where = records(257, 200, 7, 0.1, 0)
    got = ctx.bed_ld_band(257, bed, window=10)
    fin = got[np.isfinite(got)]
    assert fin.size > 0.9 * (200 * 10 - 55) and (fin >= 0).all() and (fin <= 1).all()
    assert np.nanmean(got[:, 0]) > 3 * np.nanmean(got[:, 9]) > 0


@pytest.mark.parametrize("W", [5, lu.TILE + 9])
def test_every_slab_is_its_rows_of_the_whole(ctx, W):
    """every [l0, l0 + n) once: with them every split of [0, L) into two and into three slabs"""
    I, L = 33, lu.TILE + 3
    bed, codes, where = records(I, L, 300 + W, 0.3, 3)
    whole = ctx.bed_ld_band(I, bed, window=W)
    assert lu.same_bits(whole, lu.band(bed, I, W))
    for l0 in range(L + 1):
        for n in range(0, L - l0 + 1):
            got = ctx.bed_ld_band(I, bed, l0=l0, n_first=n, window=W)
            assert lu.same_bits(got, whole[l0:l0 + n]), (l0, n)


def test_slabs_of_several_runs_of_individuals(ctx):
    I, L, W = 1001, 150, 40
    bed, codes, where = records(I, L, 400, 0.3, 0)
    whole = ctx.bed_ld_band(I, bed, window=W)
    assert lu.same_bits(whole, lu.band(bed, I, W))
    for a, b in ((1, L - 1), (63, 64), (64, 65), (70, 149)):
        parts = [ctx.bed_ld_band(I, bed, l0=x, n_first=y - x, window=W) for x, y in ((0, a), (a, b), (b, L))]
        assert lu.same_bits(np.concatenate(parts), whole)


def test_bits_do_not_depend_on_the_launch_geometry(ctx):
    """the fixed case of ld_util in fresh processes under MCHIP_BLOCKS_PER_CU = 1 (the individuals in few runs) and 4096 (in as many
    as there are stages): integer sums, the same bits"""
    bed = lu.fixed_case()
    want = lu.digest(lu.band(bed, lu.FIXED["I"], lu.FIXED["window"]))
    assert lu.digest(ctx.bed_ld_band(lu.FIXED["I"], bed, window=lu.FIXED["window"])) == want
    for knob in ("1", "4096"):
        env = dict(os.environ, MCHIP_BLOCKS_PER_CU=knob)
        env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ld_util.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             text=True, timeout=120, env=env, cwd=ROOT)
        assert res.returncode == 0, res.stderr[-2000:]
        assert res.stdout.strip() == want, knob


def test_an_installed_fit_is_untouched():
    """a data set with a fitted model: get_p, get_q and mchip_loglik give the same bits before and after a band of other records"""
    I, L, K = 40, 90, 3
    bed, codes, where = records(I, L, 500, 0.1, 0)
    c = hip.Context(0)
    try:
        ua = c.set_genotypes_bed(I, bed)
        c.set_model(K)
        q0, p0 = random_params(I, ua, K, seed=5, lower_bound=1e-8)
        c.set_q(0, q0)
        c.set_p(0, p0)
        for _ in range(3):
            c.em_step(0, 0)
        before = (c.get_p(0).tobytes(), c.get_q(0).tobytes(), np.float64(c.loglik(0)).tobytes(), c.get_genotypes().tobytes())
        other, _, _ = records(70, 130, 501, 0.2, 3)
        got = c.bed_ld_band(70, other, window=33)
        assert lu.same_bits(got, lu.band(other, 70, 33))
        after = (c.get_p(0).tobytes(), c.get_q(0).tobytes(), np.float64(c.loglik(0)).tobytes(), c.get_genotypes().tobytes())
        assert before == after
        assert np.isfinite(c.em_step(0, 0))
    finally:
        c.close()


def test_no_data_set_is_needed():
    c = hip.Context(0)
    try:
        bed, codes, where = records(12, 20, 600, 0.0, 0)
        assert lu.same_bits(c.bed_ld_band(12, bed, window=4), lu.band(bed, 12, 4))
        assert c.I == 0 and c.T == 0
    finally:
        c.close()


def test_every_error_path_leaves_the_array_untouched(ctx):
    I, L, W = 10, 12, 4
    bed, codes, where = records(I, L, 700, 0.1, 0)
    rb = bed.shape[1]
    lib = ctx.lib
    good = dict(I=I, L=L, bed=bed.ctypes.data, rb=rb, l0=2, n=5, W=W)
    bad = [dict(I=0), dict(I=-1), dict(L=0), dict(rb=rb - 1), dict(rb=0), dict(l0=-1), dict(n=-1), dict(l0=L, n=1), dict(l0=8, n=5),
           dict(l0=2 ** 31 - 1, n=2 ** 31 - 1), dict(W=0), dict(W=-3), dict(W=lu.MAX_WINDOW + 1), dict(bed=None)]
    for change in bad:
        a = dict(good, **change)
        out = np.full((5, W), 12345.0)
        rc = lib.mchip_bed_ld_band(ctx.h, a["I"], a["L"], a["bed"], a["rb"], a["l0"], a["n"], a["W"], out.ctypes.data)
        assert hip.STATUS.get(rc, rc) == "INVALID", (change, rc)
        assert (out == 12345.0).all(), change
        assert b"bed_ld_band" in lib.mchip_last_error(ctx.h)
    assert lib.mchip_bed_ld_band(ctx.h, I, L, bed.ctypes.data, rb, 2, 5, W, None) == 1
    assert lib.mchip_bed_ld_band(None, I, L, bed.ctypes.data, rb, 2, 5, W, np.empty((5, W)).ctypes.data) == 1
    out = np.full((5, W), 12345.0)          # nothing to do is not an error, and writes nothing
    assert lib.mchip_bed_ld_band(ctx.h, I, L, bed.ctypes.data, rb, L, 0, W, out.ctypes.data) == 0 and (out == 12345.0).all()
    assert lu.same_bits(ctx.bed_ld_band(I, bed, l0=2, n_first=5, window=W), lu.band(bed, I, W, 2, 5))      # and the context still works
    assert lu.same_bits(ctx.bed_ld_band(I, bed, window=lu.MAX_WINDOW)[:, :L], lu.band(bed, I, L))
