"""-m gpu: mchip_bed_king (multiclust_amd/csrc/mchip_bed.hip) against the definition restated in tests/king_util.py: phi bit for bit,
NaN positions included, and the four counts.  Every count of the definition is an integer and phi is one division, so there is no
tolerance anywhere in this file.

What the cases are sized by: a workgroup of the pair kernel owns TILE = 64 row individuals x 64 column individuals and stages 256
variants (four 64-bit words of a bit plane) at a time; the transposing kernel takes 256 individuals x 64 variants per workgroup and
reads a record as 32-bit words from any byte offset, the bits behind the last individual masked.  So: I on either side of 64, 128
and 256, with ceil(I/4) of every residue mod 4; L on either side of one and two words and of a stage, and 1100 for several stages
and several runs of variants; slabs cut at, before and after a tile edge; records three bytes longer than they need be; garbage in
every bit that carries no individual."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bedfiles
from cli_util import ROOT
from device_util import ctx
import king_util as ku
from multiclust_amd import hip
from synth import random_params

pytestmark = pytest.mark.gpu
assert (ku.TILE, ku.STAGE_VARIANTS, ku.PLANE_INDIVIDUALS) == (64, 256, 256)      # the cases below are written for these
IS = [1, 2, 3, 5, ku.TILE - 1, ku.TILE, ku.TILE + 1, 2 * ku.TILE - 1, 2 * ku.TILE, 2 * ku.TILE + 2, ku.PLANE_INDIVIDUALS - 1,
      ku.PLANE_INDIVIDUALS, ku.PLANE_INDIVIDUALS + 1]
LS = [1, 63, 64, 65, 128, 129, ku.STAGE_VARIANTS - 1, ku.STAGE_VARIANTS, ku.STAGE_VARIANTS + 1, 2 * ku.STAGE_VARIANTS + 1]


def records(I, L, seed, missing, extra):
    codes = ku.draw_codes(I, L, seed, missing)
    where = ku.plant(codes, seed)
    return ku.repack(codes, seed, extra), codes, where


def check(ctx, I, bed, codes, **slab):
    phi, cnt = ctx.bed_king(I, bed, **slab)
    want_phi, want_cnt = ku.kinship(codes, slab.get("i0", 0), slab.get("n_rows"))
    assert phi.shape == want_phi.shape and cnt.shape == want_cnt.shape
    assert np.array_equal(cnt, want_cnt), (I, slab)
    assert ku.same_bits(phi, want_phi), (I, slab)
    return phi, cnt


@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("I", IS)
def test_bits_at_every_individual_edge(ctx, I, extra):
    """missing rates 0 and 0.1 in turn; one individual all missing (a NaN row and column), one without a heterozygous call, a pair
    of duplicates"""
    L = 70
    missing = 0.1 if IS.index(I) % 2 else 0.0
    bed, codes, where = records(I, L, 100 + I, missing, extra)
    assert bed.shape[1] == (I + 3) // 4 + extra
    phi, cnt = check(ctx, I, bed, codes)
    if where:
        m, z = where["missing"], where["nohet"]
        assert np.isnan(phi[m]).all() and np.isnan(phi[:, m]).all() and not cnt[m].any() and not cnt[:, m].any()
        assert np.isnan(phi[z, z]) and not cnt[z, :, 1].any() and not cnt[z, :, 3].any()
        others = [j for j in range(I) if j not in (m, z)]
        assert not np.isnan(phi[np.ix_(others, others)]).any()
        if not missing and where["dup_of"] not in (m, z) and where["dup"] not in (m, z):
            assert phi[where["dup"], where["dup_of"]] == 0.5
        assert (np.diag(phi)[others] == 0.5).all()      # the formula at j = i, no special case


@pytest.mark.parametrize("L", LS)
def test_bits_on_either_side_of_the_variant_words_and_stages(ctx, L):
    bed, codes, _ = records(67, L, 200 + L, 0.1, 0)
    check(ctx, 67, bed, codes)


def test_phi_is_symmetric_bit_for_bit_and_counts_transpose(ctx):
    bed, codes = ku.fixed_case()
    I = ku.FIXED["I"]
    phi, cnt = check(ctx, I, bed, codes)
    assert ku.same_bits(phi, phi.T)
    for s in range(3):
        assert np.array_equal(cnt[:, :, s], cnt[:, :, s].T)
    assert not np.array_equal(cnt[:, :, 3], cnt[:, :, 3].T)      # h_ij is the one that is not symmetric


def test_kinships_are_what_the_estimator_promises(ctx):
    """what the comparisons above compare: the planted pedigree's duplicate at 0.5, first-degree pairs near 0.25, the rest near or
    below 0"""
    codes, planted, pop = ku.pedigree(5, 4000)
    I = codes.shape[0]
    phi, _ = check(ctx, I, bedfiles.pack(codes, padding=1), codes)
    for i in range(I):
        for j in range(i + 1, I):
            if (i, j) in planted:
                assert 0.18 < phi[i, j] <= 0.5, (i, j, phi[i, j])
            else:
                assert phi[i, j] < 0.08, (i, j, phi[i, j])
    assert sum(phi[i, j] > 0.4 for i, j in planted) == 1


@pytest.mark.parametrize("cut", [ku.TILE - 1, ku.TILE, ku.TILE + 1])
def test_every_slab_is_its_rows_of_the_whole(ctx, cut):
    bed, codes = ku.fixed_case()
    I = ku.FIXED["I"]
    whole_phi, whole_cnt = ctx.bed_king(I, bed)
    parts = [ctx.bed_king(I, bed, i0=a, n_rows=b - a) for a, b in ((0, cut), (cut, cut), (cut, I - 1), (I - 1, I))]
    assert parts[1][0].shape == (0, I) and parts[1][1].shape == (0, I, 4)      # n_rows = 0
    assert ku.same_bits(np.concatenate([p for p, _ in parts]), whole_phi)
    assert np.array_equal(np.concatenate([c for _, c in parts]), whole_cnt)
    check(ctx, I, bed, codes, i0=cut - 3, n_rows=5)


def test_counts_may_be_null(ctx):
    bed, codes = ku.fixed_case()
    phi, cnt = ctx.bed_king(ku.FIXED["I"], bed, counts=False)
    assert cnt is None and ku.same_bits(phi, ku.kinship(codes)[0])


@pytest.fixture(scope="module")
def geometry_digests():
    """the restatement's digest of every case of king_util.GEOMETRY: computed once, never changed"""
    return {name: ku.digest(*ku.kinship(ku.geometry_case(name)[1])) for name in ku.GEOMETRY}


# case, MCHIP_BLOCKS_PER_CU, and the (n_split, stages_per_split) the launch must have had on 256 compute units: every way the pair
# kernel walks its 5 stages (the last of 2 words) -- one stage a workgroup; one workgroup through all five, the accumulators carried
# and the LDS tiles written over four times; runs of 2, 2 and 1 stages, the later runs beginning behind word 0
GEOMETRY_RUNS = [("fixed", "1", (5, 1)), ("fixed", "4096", (5, 1)), ("whole", "1", (1, 5)), ("runs", "1", (3, 2)), ("runs", "4096", (5, 1))]


@pytest.mark.parametrize("name,knob,split", GEOMETRY_RUNS)
def test_bits_do_not_depend_on_the_launch_geometry(ctx, geometry_digests, name, knob, split):
    """fresh processes under MCHIP_BLOCKS_PER_CU: the program says which geometry the launch had (king_util restates
    king_geometry_of; tests/test_king_cpu.py holds the restatement to the header), and the bits are the restatement's under each:
    integer counts"""
    assert ctx.device_info()[1] == 256      # GEOMETRY_RUNS is worked out for the MI355X
    g = ku.GEOMETRY[name]
    assert ku.king_geometry(g["I"], g["I"], g["L"], int(knob) * 256)[2:] == split
    env = dict(os.environ, MCHIP_BLOCKS_PER_CU=knob)
    env.pop("MCHIP_BLOCKS_PER_CU_IND", None)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "king_util.py"), name], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=120, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    digest, geometry = res.stdout.strip().split("\n")
    assert tuple(int(x) for x in geometry.split()) == split + (256,), (name, knob)
    assert digest == geometry_digests[name], (name, knob)


def test_default_geometry_on_the_larger_cases(ctx, geometry_digests):
    """in this process, under the knob it was started with (64 by default: one stage a workgroup)"""
    for name in ("fixed", "runs"):
        g = ku.GEOMETRY[name]
        assert ku.digest(*ctx.bed_king(g["I"], ku.geometry_case(name)[0])) == geometry_digests[name], name


def test_an_installed_fit_is_untouched():
    """a data set with a fitted model: get_p, get_q, mchip_loglik and the genotypes give the same bits before and after the
    kinships of other records"""
    I, L, K = 40, 90, 3
    bed, codes, _ = records(I, L, 500, 0.1, 0)
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
        other, other_codes, _ = records(70, 130, 501, 0.2, 3)
        check(c, 70, other, other_codes)
        after = (c.get_p(0).tobytes(), c.get_q(0).tobytes(), np.float64(c.loglik(0)).tobytes(), c.get_genotypes().tobytes())
        assert before == after
        assert np.isfinite(c.em_step(0, 0))
    finally:
        c.close()


def test_no_data_set_is_needed():
    c = hip.Context(0)
    try:
        bed, codes, _ = records(12, 20, 600, 0.0, 0)
        check(c, 12, bed, codes)
        assert c.I == 0 and c.T == 0
    finally:
        c.close()


def test_every_error_path_leaves_the_arrays_untouched(ctx):
    I, L = 10, 12
    bed, codes, _ = records(I, L, 700, 0.1, 0)
    rb = bed.shape[1]
    lib = ctx.lib
    good = dict(I=I, L=L, bed=bed.ctypes.data, rb=rb, i0=2, n=5)
    bad = [dict(I=0), dict(I=-1), dict(L=0), dict(L=-4), dict(rb=rb - 1), dict(rb=0), dict(i0=-1), dict(n=-1), dict(i0=I, n=1), dict(i0=8, n=3),
           dict(i0=2 ** 31 - 1, n=2 ** 31 - 1), dict(bed=None)]
    for change in bad:
        a = dict(good, **change)
        phi, cnt = np.full((5, I), 12345.0), np.full((5, I, 4), 777, dtype=np.uint32)
        rc = lib.mchip_bed_king(ctx.h, a["I"], a["L"], a["bed"], a["rb"], a["i0"], a["n"], phi.ctypes.data, cnt.ctypes.data)
        assert hip.STATUS.get(rc, rc) == "INVALID", (change, rc)
        assert (phi == 12345.0).all() and (cnt == 777).all(), change
        assert b"bed_king" in lib.mchip_last_error(ctx.h)
    cnt = np.full((5, I, 4), 777, dtype=np.uint32)
    assert lib.mchip_bed_king(ctx.h, I, L, bed.ctypes.data, rb, 2, 5, None, cnt.ctypes.data) == 1 and (cnt == 777).all()
    assert lib.mchip_bed_king(None, I, L, bed.ctypes.data, rb, 2, 5, np.empty((5, I)).ctypes.data, None) == 1
    phi = np.full((5, I), 12345.0)          # nothing to do is not an error, and writes nothing
    assert lib.mchip_bed_king(ctx.h, I, L, bed.ctypes.data, rb, I, 0, phi.ctypes.data, cnt.ctypes.data) == 0
    assert (phi == 12345.0).all() and (cnt == 777).all()
    check(ctx, I, bed, codes, i0=2, n_rows=5)      # and the context still works
