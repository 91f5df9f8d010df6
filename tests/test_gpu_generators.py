"""The device generators that consume the reference's rand() stream, on every form the dispatch reaches and on the inputs where an
inverse-CDF walk or a remainder is most likely to go wrong.  For these "close" does not count: one wrong draw is a different
replicate, a different fit and a different bootstrap p-value.

  * DISPATCH RULE: a Python statement of which kernel each case reaches (`sim_form`, `part_form`, each condition citing the C it
    restates); test_the_cases_reach_every_form (CPU) shows that the case lists reach every form;
  * test_device_bootstrap_on_every_form (-m gpu): mchip_simulate_genotypes -> get_genotypes byte for byte against the host
    generator (mc_bootstrap_genotypes, pinned to the reference's own parametric_bootstrap() on the same families by
    tests/test_generators_cpu.py) for every parameter family (negative entries, zeros, NaN rows, a NaN inside a p row, rows
    not summing to 1, exact ties with the draw and one ulp either side), per-individual and shared eta, and windows that put
    draws 0, 1, RAND_MAX - 1, RAND_MAX (or the tie draws) at the first and last copy, at individuals 255 | 256 (the workgroup
    edge of the tile form), at the first locus of the second tile and at the chunk boundary of k_simulate_admixture (copy
    1 984); and against the reference itself, live through `ref_time --bootstrap`, on a subset;
  * test_device_partition_on_every_form (-m gpu): for every K from 1 to 64, mchip_mstep_from_rand_partition bit for bit against
    mchip_mstep_from_partition of the assignment drawn in Python (rand() % K), with draws 0, K - 1, K and RAND_MAX placed at the
    workgroup edge and at the locus-chunk (tile form) or generator-chunk (k_draw_partition) edge.

Testing knobs are read when a context is created and at every set_genotypes / set_model, so each knob setting has a context of
its own and its environment in force around every call."""

import numpy as np
import pytest

import multiclust_amd as mc
import rand_window as rw
from synth import make_dataset
from test_generators_cpu import (FAMILIES, counts_of, family_params, host_bootstrap, needs_ref, placement_windows,
                                 reference_bootstrap)
from test_gpu_kernel_matrix import count_bits, geometry

RAND_MAX = rw.RAND_MAX

# ---------------------------------------------------------------------------------------------------------------- DISPATCH RULE
SIM_QW, SIM_PW = 8, 4        # mchip_generators.hip: widths of the FAST form's threshold rows
RNG_CHUNK = 4 * 31 * 32      # mchip_context.h: draws per thread of the chunked generators
SIM_COPIES = RNG_CHUNK // 2  # copies per thread of k_simulate_admixture


def sim_form(K, max_M, ploidy, knobs):
    """mchip_simulate_genotypes: fast = K <= SIM_QW && max_M <= SIM_PW; the tile form when fast && ploidy <= 8 && !sim_no_tile"""
    fast = K <= SIM_QW and max_M <= SIM_PW
    if fast and ploidy <= 8 and "MCHIP_SIM_NO_TILE" not in knobs:
        return "k_simulate_tile<%d>" % ploidy
    return "k_simulate_admixture<%s>" % ("true" if fast else "false")


def sim_tile(K, L):
    """mchip_simulate_genotypes: loci per tile of the tile form"""
    return min((16384 // (K * 12)) & ~7, 512, (L + 7) & ~7)


def part_form(K, ploidy, max_M, lchunk, knobs):
    """rand_partition_tiled (returns -1: k_draw_partition, or for K = 1 a memset of the assignment)"""
    KP = (K + 1) & ~1
    tile = max((16384 // (max_M * KP * 2)) & ~7, 8)
    tile = min(tile, lchunk)
    lds = (31 * 256 + (KP // 2) * 256 + tile * max_M * (KP // 2)) * 4
    if ploidy > 8 or lchunk * ploidy > 65535 or "MCHIP_PART_NO_TILE" in knobs or lds > 64 * 1024:
        return "k_draw_partition" if K > 1 else "memset"
    return "k_partition_tile<%d>" % ploidy


def part_lchunk(K, I, ua, ploidy, knobs):
    max_M = int(max(ua))
    return geometry(K, I, len(ua), int(sum(ua)), ploidy, max_M, 1, count_bits(ploidy, knobs), knobs)["lchunk"]


# ------------------------------------------------------------------------------------------------------------------ CASES
NO_SIM_TILE = {"MCHIP_SIM_NO_TILE": "1"}
NO_PART_TILE = {"MCHIP_PART_NO_TILE": "1"}


def sim_ua(L, lo, hi, seed):
    """allele counts in [lo, hi], both ends present"""
    ua = np.random.default_rng(seed).integers(lo, hi + 1, L).astype(np.int32)
    ua[0], ua[L // 2] = hi, lo
    return ua


def _tile_case(ploidy, K, I):
    L = sim_tile(K, 1 << 20) + 5            # a second tile of 5 loci; not a multiple of the tile or of 8
    return (I, L, ploidy, K, 2, 4, {})


# (I, L, ploidy, K, min alleles, max alleles, knobs): I = 256 n +- 1
SIM_CASES = [
    _tile_case(1, 2, 257), _tile_case(2, 8, 255), _tile_case(3, 5, 257), _tile_case(4, 8, 513),
    _tile_case(5, 6, 255), _tile_case(6, 8, 257), _tile_case(7, 4, 257), _tile_case(8, 8, 257),
    (257, 61, 9, 8, 2, 4, {}),                 # FAST, ploidy > 8
    (511, 203, 2, 6, 2, 4, NO_SIM_TILE),       # FAST under MCHIP_SIM_NO_TILE
    (255, 83, 2, 9, 2, 4, {}),                 # general: K > 8
    (255, 41, 3, 64, 2, 4, {}),                # general: K = 64
    (257, 45, 2, 4, 5, 254, {}),               # general: 5 .. 254 alleles
    (255, 70, 4, 3, 2, 5, {}),                 # general: one more allele than the FAST rows hold
]


def sim_case_id(c):
    I, L, ploidy, K, lo, hi, knobs = c
    return "%s-I%d-L%d-pl%d-K%d-M%d%s" % (sim_form(K, hi, ploidy, knobs), I, L, ploidy, K, hi, "-notile" if knobs else "")


def sim_positions(I, L, ploidy, K):
    """named draw positions (the first of 31 placed draws) for the edges of a data set of I x L x ploidy copies"""
    per_i = L * ploidy
    tile = sim_tile(K, L)
    return [("first copy", 0), ("last copy", 2 * I * per_i - 31), ("individuals 255|256", 2 * 256 * per_i - 16),
            ("second tile", 2 * (1 * per_i + tile * ploidy) - 16), ("chunk boundary", 2 * SIM_COPIES - 16)]


def part_cases():
    """every K from 1 to 64 in the tile form (ploidy 1 + (K - 1) % 8), and again through k_draw_partition: ploidy > 8,
    MCHIP_PART_NO_TILE, or the LDS budget (many clusters and 40 alleles); set_init_genotypes in force for the tile cases with
    K <= 8 and for every tenth of the others"""
    out = []
    for K in range(1, 65):
        out.append((257 if K % 2 else 255, 37 + K % 11, 1 + (K - 1) % 8, K, 4, {}, K <= 8))
        second = [(9, 4, {}), (2, 4, NO_PART_TILE), (2, 40, {}) if K >= 32 else (10, 4, {})][K % 3]
        out.append((255 if K % 2 else 257, 29 + K % 7, second[0], K, second[1], second[2], K % 10 == 7))
    return out


PART_CASES = part_cases()


def part_case_shape(c):
    I, L, ploidy, K, maxal, knobs, init = c
    ua, geno = make_dataset(I, L, max(K, 2), ploidy=ploidy, max_alleles=maxal, seed=K * 7 + ploidy, missing=0.02)
    return ua, geno


def part_case_id(c):
    I, L, ploidy, K, maxal, knobs, init = c
    ua, _ = part_case_shape(c)
    form = part_form(K, ploidy, int(ua.max()), part_lchunk(K, I, ua, ploidy, knobs), knobs)
    return "%s-K%d-pl%d-M%d%s%s" % (form, K, ploidy, maxal, "-notile" if knobs else "", "-init" if init else "")


def test_the_cases_reach_every_form():
    """CPU: the case lists reach the tile form for PL = 1..8, both k_simulate_admixture instances (FAST through ploidy > 8 and
    through MCHIP_SIM_NO_TILE; the general one through K > 8 and through more than 4 alleles), k_partition_tile<PL> for PL =
    1..8, and k_draw_partition through ploidy > 8, MCHIP_PART_NO_TILE and the LDS budget, each with set_init_genotypes once"""
    sim = {}
    for c in SIM_CASES:
        I, L, ploidy, K, lo, hi, knobs = c
        sim.setdefault(sim_form(K, hi, ploidy, knobs), []).append(c)
        assert I % 256 in (1, 255)
        if "tile" in sim_form(K, hi, ploidy, knobs):
            assert L > sim_tile(K, L) and L % sim_tile(K, L) and L % 8
    assert set(sim) == {"k_simulate_tile<%d>" % p for p in range(1, 9)} | {"k_simulate_admixture<true>", "k_simulate_admixture<false>"}
    assert {c[2] > 8 for c in sim["k_simulate_admixture<true>"]} == {True, False}
    assert any(c[3] > 8 for c in sim["k_simulate_admixture<false>"]) and any(c[5] > 4 for c in sim["k_simulate_admixture<false>"])
    assert any(c[5] == 254 for c in SIM_CASES)
    forms, ways, init = {}, set(), set()
    for c in PART_CASES:
        I, L, ploidy, K, maxal, knobs, with_init = c
        ua, _ = part_case_shape(c)
        lchunk = part_lchunk(K, I, ua, ploidy, knobs)
        f = part_form(K, ploidy, int(ua.max()), lchunk, knobs)
        forms.setdefault(f, set()).add(K)
        if with_init:
            init.add(f)
        if f == "k_draw_partition":
            ways.add("ploidy" if ploidy > 8 else ("knob" if knobs else ("lds" if lchunk * ploidy <= 65535 else "lchunk")))
    assert {"k_partition_tile<%d>" % p for p in range(1, 9)} <= set(forms) and "k_draw_partition" in forms
    assert {"ploidy", "knob", "lds"} <= ways
    assert set(range(2, 65)) <= forms["k_draw_partition"]
    assert set().union(*forms.values()) == set(range(1, 65))
    assert {"k_partition_tile<%d>" % p for p in range(1, 9)} | {"k_draw_partition"} <= init


# ------------------------------------------------------------------------------------------------------------------ GPU tests
@pytest.fixture(scope="module")
def contexts():
    ctxs = {}
    yield ctxs
    for c in ctxs.values():
        c.close()


def context_for(contexts, knobs, monkeypatch):
    """the module's context for this knob setting, with exactly those knobs in the environment"""
    for k in ("MCHIP_SIM_NO_TILE", "MCHIP_PART_NO_TILE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    key = tuple(sorted(knobs))
    if key not in contexts:
        contexts[key] = mc.Context(0)
    return contexts[key]


@pytest.mark.gpu
@pytest.mark.parametrize("case", SIM_CASES, ids=[sim_case_id(c) for c in SIM_CASES])
def test_device_bootstrap_on_every_form(contexts, monkeypatch, case):
    """every family x both eta forms x every window, against the host generator; the message lists every combination that differs"""
    I, L, ploidy, K, lo, hi, knobs = case
    ctx = context_for(contexts, knobs, monkeypatch)
    ua = sim_ua(L, lo, hi, seed=I + L + K)
    positions = sim_positions(I, L, ploidy, K)
    bad = []
    for family in FAMILIES:
        for eta in ("individual", "shared"):
            shared = eta == "shared"
            q, p = family_params(family, I, ua, K, shared=shared, seed=K + ploidy + len(family))
            for name, window in placement_windows(family, 2 * I * L * ploidy, positions, seed=I * L):
                want, _, _ = host_bootstrap(I, L, ploidy, ua, K, q, p, window, 1, int(shared))
                ctx.simulate_genotypes(I, L, ploidy, ua, window, K, q, p, eta_constrained=int(shared))
                got = ctx.get_genotypes()
                if not np.array_equal(got, want):
                    bad.append("%s/%s/%s: %d copies differ" % (family, eta, name, int(np.sum(got != want))))
    assert not bad, "; ".join(bad)


# a few dozen cases against the reference itself: every case, these (family, eta), draws placed at the first copy
REF_FAMILIES = (("negative", "individual"), ("nan_p", "shared"), ("tie-ulp", "individual"))


@pytest.mark.gpu
@needs_ref
@pytest.mark.parametrize("case", SIM_CASES, ids=[sim_case_id(c) for c in SIM_CASES])
def test_device_bootstrap_equals_the_reference(contexts, monkeypatch, tmp_path, case):
    I, L, ploidy, K, lo, hi, knobs = case
    ctx = context_for(contexts, knobs, monkeypatch)
    ua = sim_ua(L, lo, hi, seed=I + L + K)
    positions = sim_positions(I, L, ploidy, K)[:1]
    for family, eta in REF_FAMILIES:
        shared = eta == "shared"
        q, p = family_params(family, I, ua, K, shared=shared, seed=K + ploidy + len(family))
        name, window = placement_windows(family, 2 * I * L * ploidy, positions, seed=I * L)[1]
        ctx.simulate_genotypes(I, L, ploidy, ua, window, K, q, p, eta_constrained=int(shared))
        ref, _ = reference_bootstrap(str(tmp_path / family), I, L, ploidy, ua, K, q, p, window, 1, int(shared))
        assert np.array_equal(counts_of(ctx.get_genotypes(), ua), ref), (family, eta, name)


def part_positions(I, L, ploidy, K, form, lchunk):
    """(workgroup edge, chunk edge) draw positions for the first of the 31 placed draws"""
    per_i = L * ploidy
    edge_i = 256 * per_i if I > 256 else (I - 1) * per_i
    if form.startswith("k_partition_tile"):
        chunk = 1 * per_i + min(lchunk, L - 1) * ploidy          # individual 1, first locus of the second locus chunk
    else:
        chunk = RNG_CHUNK                                        # the second thread's first draw
    n = I * per_i
    return [min(max(edge_i - 16, 0), n - 31), min(max(chunk - 16, 0), n - 31)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", PART_CASES, ids=[part_case_id(c) for c in PART_CASES])
def test_device_partition_on_every_form(contexts, monkeypatch, case):
    I, L, ploidy, K, maxal, knobs, with_init = case
    ctx = context_for(contexts, knobs, monkeypatch)
    ua, geno = part_case_shape(case)
    lchunk = part_lchunk(K, I, ua, ploidy, knobs)
    form = part_form(K, ploidy, int(ua.max()), lchunk, knobs)
    n = I * L * ploidy
    other = np.ascontiguousarray(geno[::-1])      # the same loci, other haplotypes
    vals = [0, K - 1, K, RAND_MAX]
    for pos in part_positions(I, L, ploidy, K, form, lchunk):
        window = rw.window_placing([vals[t % 4] for t in range(31)], pos, fill_seed=K)
        assign = (rw.draws(window, n) % K).astype(np.uint8)
        assert assign[pos:pos + 4].tolist() == [0, (K - 1) % K, K % K, RAND_MAX % K]
        ctx.set_genotypes(ua, geno)
        ctx.set_model(K, lower_bound=1e-8)
        ctx.mstep_from_partition(assign, 0)
        q_want, p_want = ctx.get_q(0), ctx.get_p(0)
        if with_init:
            # a bootstrap fit: the data set held is another one, the partition counts read the installed haplotypes
            ctx.set_genotypes(ua, other)
            ctx.set_init_genotypes(geno)
            ctx.set_model(K, lower_bound=1e-8)
        ctx.mstep_from_rand_partition(window, 1)
        assert np.array_equal(ctx.get_q(1), q_want, equal_nan=True), (form, pos)
        assert np.array_equal(ctx.get_p(1), p_want, equal_nan=True), (form, pos)
