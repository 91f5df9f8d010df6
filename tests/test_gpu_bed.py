"""-m gpu: PLINK .bed records unpacked on the device (mchip_set_genotypes_bed, multiclust_amd/csrc/mchip_bed.hip) against the
plain-C decoder (mc_bed_decode) uploaded the usual way (mchip_set_genotypes): the installed data set, the fits it gives, and
the command line's --bed against -f on the equivalent STRUCTURE file.  Every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

import bedfiles as bf
from bits import bits
from cli_util import BIN, CLOCK, result_files
import oracle_bind as ob
from multiclust_amd import hip, host
from procutil import run_program
from synth import random_params

pytestmark = pytest.mark.gpu

SHAPE_I = (1, 3, 4, 5, 8, 9, 63, 65, 257)
SHAPE_L = (1, 7, 8, 9, 63, 65, 300)


@pytest.fixture(scope="module")
def contexts():
    ctxs = [hip.Context(0) for _ in range(3)]
    yield ctxs
    for c in ctxs:
        c.close()


def empty_individuals(ctx):
    first = C.c_int(-2)
    n = ctx.lib.mchip_empty_individuals(ctx.h, C.byref(first))
    return n, first.value


def assert_same_install(ctxs, I, packed):
    """packed records through the device entry (ctxs[0]) and through decoder + mchip_set_genotypes (ctxs[1]); ctxs[2] takes a
    device copy of the former"""
    dev, ref, third = ctxs
    ua, geno = host.bed_decode(I, packed)
    ua_dev = dev.set_genotypes_bed(I, packed)
    ref.set_genotypes(ua, geno)
    assert ua_dev.dtype == np.int32 and np.array_equal(ua_dev, ua)
    got = dev.get_genotypes()
    assert np.array_equal(got, geno) and np.array_equal(ref.get_genotypes(), geno)
    assert dev.data_counts() == ref.data_counts()
    assert empty_individuals(dev) == empty_individuals(ref)
    third.copy_genotypes(dev)
    assert np.array_equal(third.get_genotypes(), geno)
    assert third.data_counts() == ref.data_counts() and empty_individuals(third) == empty_individuals(ref)
    return ua, geno


@pytest.mark.parametrize("L", SHAPE_L)
@pytest.mark.parametrize("I", SHAPE_I)
def test_device_unpacking_matches_decoder(I, L, contexts):
    for missing in (0.0, 0.03, 0.5):
        codes = bf.draw_codes(I, L, missing=missing, seed=1000 * I + L)
        assert_same_install(contexts, I, bf.pack(codes))
    # garbage in the padding bits of every record, and records further apart than ceil(I/4) bytes
    packed = bf.pack(bf.draw_codes(I, L, missing=0.03, seed=5 + I + L), padding=3)
    ua, geno = assert_same_install(contexts, I, packed)
    wide = np.full((L, packed.shape[1] + 3), 0xAA, dtype=np.uint8)
    wide[:, :packed.shape[1]] = packed
    ua_w = contexts[0].set_genotypes_bed(I, wide)
    assert np.array_equal(ua_w, ua) and np.array_equal(contexts[0].get_genotypes(), geno)


def test_empty_individuals_are_found_on_the_device(contexts):
    codes = bf.draw_codes(300, 130, missing=0.05, seed=9, plant=False)
    codes[[0, 17, 256, 299], :] = bf.MISS
    assert_same_install(contexts, 300, bf.pack(codes))
    assert empty_individuals(contexts[0]) == (4, 0)
    codes[0, 129] = bf.HET
    assert_same_install(contexts, 300, bf.pack(codes))
    assert empty_individuals(contexts[0]) == (3, 17)


def test_many_tiles(contexts):
    """2 000 x 20 000: 8 x 313 tiles, the last of either axis partial; 10 MB cross to the device instead of 80 MB"""
    codes = bf.draw_codes(2000, 20000, missing=0.03, seed=42)
    assert_same_install(contexts, 2000, bf.pack(codes))


def admixture_fit(ctx, K, window, steps=5):
    ctx.set_model(K, admixture=1)
    ctx.mstep_from_rand_partition(window, to=0)
    ll = [ctx.em_step(0, 0) for _ in range(steps)]
    return np.array(ll), ctx.get_q(0), ctx.get_p(0), ctx.expected_counts()


def mixture_fit(ctx, K, eta, p, steps=5):
    ctx.set_model(K, admixture=0)
    ctx.set_q(0, eta)
    ctx.set_p(0, p)
    ll = [ctx.em_step(0, 0) for _ in range(steps)]
    return np.array(ll), ctx.get_q(0), ctx.get_p(0), ctx.expected_counts()


FIT_CASES = {
    # missing calls, monomorphic loci, a locus without a call, an individual without a call: the general kernels
    "general": dict(I=300, L=1000, missing=0.03, plant=True),
    # every locus with exactly two alleles and no missing call: the scalar-operand (biallelic) kernels
    "biallelic": dict(I=300, L=1000, missing=0.0, plant=False),
}


@pytest.mark.parametrize("case", sorted(FIT_CASES))
def test_fits_are_bit_identical(case, contexts):
    spec = FIT_CASES[case]
    I = spec["I"]
    codes = bf.draw_codes(I, spec["L"], missing=spec["missing"], seed=11, plant=spec["plant"])
    packed = bf.pack(codes)
    dev, ref = contexts[0], contexts[1]
    ua, geno = host.bed_decode(I, packed)
    if case == "biallelic":
        assert (ua == 2).all() and not (geno == 0xFF).any()
    else:
        assert ua.min() == 0 and ua.max() == 3 and (geno == 0xFF).all(axis=(1, 2)).any()
    assert np.array_equal(dev.set_genotypes_bed(I, packed), ua)
    ref.set_genotypes(ua, geno)
    window, _ = ob.glibc_window(20260117)
    for K in (3, 8):
        a, b = admixture_fit(dev, K, window), admixture_fit(ref, K, window)
        assert np.isfinite(b[0]).all()
        for x, y in zip(a, b):
            assert x.shape == y.shape and bits(x) == bits(y)
    q0, p0 = random_params(I, ua, 2, seed=3)
    eta = q0.mean(axis=0)
    a, b = mixture_fit(dev, 2, eta, p0), mixture_fit(ref, 2, eta, p0)
    assert np.isfinite(b[0]).all()
    for x, y in zip(a, b):
        assert x.shape == y.shape and bits(x) == bits(y)


# n_models: the K values a run fits and writes its five result files for (-b fits H0: K - 1 beside HA: K)
@pytest.mark.parametrize("variant,args,n_models", [
    ("admixture", ["-a", "-k", "3", "-n", "2", "-T", "20", "-r", "5"], 1),
    ("streams", ["-a", "-k", "3", "-n", "2", "-T", "20", "-r", "5", "--streams", "2"], 1),
    ("mixture", ["-k", "3", "-n", "2", "-T", "20", "-r", "5"], 1),
    ("bootstrap", ["-a", "-k", "3", "-n", "2", "-T", "20", "-r", "5", "-b", "2"], 2),   # the observed haplotypes: lazy host decode
])
def test_command_line_bed_equals_structure(variant, args, n_models, tmp_path):
    codes = bf.draw_codes(60, 200, missing=0.03, seed=21, plant=False)
    codes[:, 7] = bf.HOM2
    codes[:, 100] = bf.MISS
    prefix, stru = str(tmp_path / "panel"), str(tmp_path / "equivalent.stru")
    bf.write_fileset(prefix, codes)
    bf.write_equivalent_stru(stru, codes)
    out = {}
    for name, data in (("A", ["--bed", prefix]), ("B", ["-f", stru])):
        d = tmp_path / name
        d.mkdir()
        # (with -o the stem is taken as it stands and -d goes unused, as in the reference: each run gets its own working directory)
        res = run_program([BIN] + data + args + ["-o", "stem", "-d", os.path.join(str(d), "")], cwd=str(d), timeout=300)
        assert res.returncode == 0, res.stderr
        out[name] = res.stdout
    a, b = result_files(str(tmp_path / "A")), result_files(str(tmp_path / "B"))
    assert len(a) == 5 * n_models and sorted(a) == sorted(b)
    for f in a:
        assert a[f] == b[f], f
    lines_a = CLOCK.sub("HH:MM:SS", out["A"].replace(prefix + ".bed", "DATA"))
    lines_b = CLOCK.sub("HH:MM:SS", out["B"].replace(stru, "DATA"))
    assert "DATA" in lines_a and lines_a == lines_b
