"""-m gpu: mchip_bed_qc (multiclust_amd/csrc/mchip_bed.hip) against the definition restated in tests/qc_util.py: the counts of both
axes and the Hardy-Weinberg p values bit for bit.  The counts are integers and the exact test is a fixed sequence of correctly
rounded double operations, subnormals included, so there is no tolerance anywhere in this file.

What the cases are sized by: the variant pass gives a wave to a variant, four to a workgroup, reads a record as 64-bit words of 32
individuals, 64 consecutive words a wave (2048 individuals a step), under a mask of 2 bits an individual with the padding cleared;
the individual pass takes 256 individuals x 64 variants per staged word and reads a record as 32-bit words from any byte offset.
So: I on either side of 4, 32, 64, 256 and of a step, with ceil(I/4) of every residue mod 4; L on either side of 4, 64 and 256;
records three bytes longer than they need be; garbage in every bit that carries no individual; keep masks that are absent, empty,
full, alternating, a single individual and drawn; an all-missing, a monomorphic and an all-heterozygous variant and a fully missing
individual in every case with room for them.  The runs of several steps and of several staged words a workgroup are the launch-
geometry test's, in fresh processes."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cli_util import ROOT
from device_util import ctx
import qc_util as qu
from multiclust_amd import hip
from synth import random_params

pytestmark = pytest.mark.gpu
assert (qu.QC_VARIANTS, qu.QC_STEP, qu.QC_ITILE) == (4, 64, 256)      # the cases below are written for these
IS = [1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257, qu.STEP_INDIVIDUALS - 1, qu.STEP_INDIVIDUALS + 1]
LS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257]


def same_p(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def check(ctx, I, bed, keep=None):
    ind, var, p = ctx.bed_qc(I, bed, ind_keep=keep)
    want_ind, want_var, want_p = qu.reference(bed, I, keep)
    assert np.array_equal(ind, want_ind), I
    assert np.array_equal(var, want_var), I
    assert same_p(p, want_p), (I, [(tuple(want_var[l]), p[l], want_p[l]) for l in np.flatnonzero(p.view(np.uint64) != want_p.view(np.uint64))[:5]])
    return ind, var, p


@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("I", IS)
def test_bits_at_every_individual_edge_under_every_keep_mask(ctx, I, extra):
    L = 70 if I < 1000 else 9
    bed, codes = qu.case(I, L, 100 + I, missing=0.1 if IS.index(I) % 2 else 0.0, extra=extra)
    assert bed.shape[1] == (I + 3) // 4 + extra
    for name, keep in qu.keep_masks(I, I).items():
        ind, var, p = check(ctx, I, bed, keep)
        n_keep = I if keep is None else int(np.count_nonzero(keep))
        assert (var.sum(axis=1) == n_keep).all() and (ind.sum(axis=1) == L).all(), name
        if name == "empty":
            assert (p == 1.0).all()


@pytest.mark.parametrize("L", LS)
def test_bits_on_either_side_of_the_variant_groups_and_words(ctx, L):
    bed, codes = qu.case(67, L, 200 + L, missing=0.1)
    ind, var, p = check(ctx, 67, bed, qu.keep_masks(67, L)["drawn"])
    check(ctx, 67, bed)


def test_the_planted_variants_and_individual(ctx):
    I, L = 90, 130
    bed, codes = qu.case(I, L, 5, missing=0.05, extra=1)
    ind, var, p = check(ctx, I, bed)
    assert (var[:, 1] == I).sum() >= 1 and ((var[:, 3] == I - 1) & (var[:, 1] == 1)).sum() >= 1       # all missing; monomorphic but for the missing individual
    allhet = np.flatnonzero(var[:, 2] == I - 1)
    assert len(allhet) >= 1 and (p[allhet] < 1e-20).all() and (ind[:, 1] == L).sum() == 1
    assert (p[var[:, 1] == I] == 1.0).all()                                                                 # N = 0


def test_every_subset_of_the_outputs(ctx):
    I, L = 45, 77
    bed, codes = qu.case(I, L, 6, missing=0.1, extra=2)
    keep = qu.keep_masks(I, 6)["drawn"]
    want = qu.reference(bed, I, keep)
    for mask in range(1, 8):
        got = ctx.bed_qc(I, bed, ind_keep=keep, ind=bool(mask & 1), var=bool(mask & 2), hwe=bool(mask & 4))
        for x, (g, w) in enumerate(zip(got, want)):
            if mask >> x & 1:
                assert g.tobytes() == w.tobytes(), (mask, x)
            else:
                assert g is None


def test_hwe_through_the_subnormals_and_at_the_walks_ends(ctx):
    """one variant per table: N about 2000 with weights that leave the normal range and reach zero, r = 0 and r = 1, n2 = mid"""
    for t in qu.HWE_TABLES:
        bed, I = qu.tables_from_codes(*t)
        ind, var, p = check(ctx, I, bed)
        assert tuple(var[0]) == (t[0], 0, t[1], t[2])
    bed, I = qu.tables_from_codes(1000, 0, 1000)
    assert ctx.bed_qc(I, bed)[2][0] == 0.0
    bed, I = qu.tables_from_codes(25, 50, 25)
    assert ctx.bed_qc(I, bed)[2][0] == 1.0


def test_the_fixture_of_the_command_line(ctx):
    codes, fids, iids, chrom = qu.cli_case()
    I = codes.shape[0]
    bed = qu.repack(codes, 3, 2)
    check(ctx, I, bed)
    check(ctx, I, bed, qu.decide(bed, I, mind=qu.CLI["mind"])["ind_keep"].astype(np.uint8))


@pytest.fixture(scope="module")
def geometry_digests():
    """the restatement's digest of every case of qc_util.GEOMETRY: computed once, never changed"""
    out = {}
    for name, g in qu.GEOMETRY.items():
        bed, keep = qu.geometry_case(name)
        out[name] = qu.digest(*qu.reference(bed, g["I"], keep))
    return out


# case, MCHIP_BLOCKS_PER_CU, and (v_split, steps_per_split, i_split, words_per_split) the launches must have had on 256 compute units
GEOMETRY_RUNS = [("steps", "1", (2, 2, 10, 1)), ("steps", "64", (4, 1, 10, 1)), ("whole", "1", (1, 4, 9, 2)), ("words", "1", (1, 1, 172, 3)),
                 ("words", "4096", (1, 1, 514, 1))]


@pytest.mark.parametrize("name,knob,split", GEOMETRY_RUNS)
def test_bits_do_not_depend_on_the_launch_geometry(ctx, geometry_digests, name, knob, split):
    """fresh processes under MCHIP_BLOCKS_PER_CU: the program says which geometry the launches had (qc_util restates qc_geometry_of;
    tests/test_qc_cpu.py holds the restatement to the header), and the bits are the restatement's under each"""
    assert ctx.device_info()[1] == 256      # GEOMETRY_RUNS is worked out for the MI355X
    g = qu.GEOMETRY[name]
    geo = qu.qc_geometry(g["I"], g["L"], int(knob) * 256)
    assert (geo[1], geo[2], geo[4], geo[5]) == split
    env = dict(os.environ, MCHIP_BLOCKS_PER_CU=knob)
    env.pop("MCHIP_BLOCKS_PER_CU_IND", None)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "qc_util.py"), name], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=120, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    digest, geometry = res.stdout.strip().split("\n")
    assert tuple(int(x) for x in geometry.split()) == split + (256,), (name, knob)
    assert digest == geometry_digests[name], (name, knob)


def test_default_geometry_on_the_larger_cases(ctx, geometry_digests):
    """in this process, under the knob it was started with"""
    for name, g in qu.GEOMETRY.items():
        bed, keep = qu.geometry_case(name)
        assert qu.digest(*ctx.bed_qc(g["I"], bed, ind_keep=keep)) == geometry_digests[name], name


def test_an_installed_fit_is_untouched():
    """a data set with a fitted model: get_p, get_q, mchip_loglik and the genotypes give the same bits before and after the counts
    of other records"""
    I, L, K = 40, 90, 3
    bed, codes = qu.case(I, L, 500, missing=0.1)
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
        other, _ = qu.case(70, 130, 501, missing=0.2, extra=3)
        check(c, 70, other, qu.keep_masks(70, 1)["alternating"])
        after = (c.get_p(0).tobytes(), c.get_q(0).tobytes(), np.float64(c.loglik(0)).tobytes(), c.get_genotypes().tobytes())
        assert before == after
        assert np.isfinite(c.em_step(0, 0))
    finally:
        c.close()


def test_no_data_set_is_needed():
    c = hip.Context(0)
    try:
        bed, _ = qu.case(12, 20, 600)
        check(c, 12, bed)
        assert c.I == 0 and c.T == 0
    finally:
        c.close()


def test_every_error_path_leaves_the_arrays_untouched(ctx):
    I, L = 10, 12
    bed, _ = qu.case(I, L, 700, missing=0.1)
    rb = bed.shape[1]
    lib = ctx.lib
    keep = np.ones(I, dtype=np.uint8)

    def call(h, ind, var, p, I=I, L=L, b=bed.ctypes.data, rb=rb):
        return lib.mchip_bed_qc(h, I, L, b, rb, keep.ctypes.data, None if ind is None else ind.ctypes.data, None if var is None else var.ctypes.data,
                                None if p is None else p.ctypes.data)

    for change, status in [(dict(I=0), "INVALID"), (dict(I=-1), "INVALID"), (dict(L=0), "INVALID"), (dict(L=-4), "INVALID"), (dict(rb=rb - 1), "INVALID"),
                           (dict(rb=0), "INVALID"), (dict(b=None), "INVALID"), (dict(I=2 ** 30, rb=2 ** 28), "UNSUPPORTED")]:
        ind, var, p = np.full((I, 4), 777, dtype=np.uint32), np.full((L, 4), 777, dtype=np.uint32), np.full(L, 12345.0)
        rc = call(ctx.h, ind, var, p, **change)
        assert hip.STATUS.get(rc, rc) == status, (change, rc)
        assert (ind == 777).all() and (var == 777).all() and (p == 12345.0).all(), change
        assert b"bed_qc" in lib.mchip_last_error(ctx.h)
    assert hip.STATUS.get(call(ctx.h, None, None, None)) == "INVALID"      # at least one output array
    assert call(None, np.empty((I, 4), dtype=np.uint32), None, None) == 1
    check(ctx, I, bed, keep)      # and the context still works
