"""The mixture model's device generator (mchip_simulate_genotypes_mixture) on every form its dispatch reaches, byte for byte.

Stream geometry (bootstrap.c:132-175): individual i owns draws i * A .. (i + 1) * A - 1 with A = 1 + L * ploidy; the first chooses
its cluster by the walk over eta, draw 1 + l * ploidy + a chooses copy (l, a) by the walk over p[k][l][.].

  * DISPATCH RULE: `mix_form` / `mix_chunk` restate mchip_simulate_genotypes_mixture; tests/test_mixture_device_cpu.py shows that
    MIX_CASES reaches every form;
  * test_mixture_generator_on_every_form (-m gpu): against the host generator (mc_bootstrap_genotypes with admixture = 0, pinned
    to the reference's parametric_bootstrap() by tests/test_generators_cpu.py) for every parameter family of that file with eta
    shared, and windows that place draws 0, 1, RAND_MAX - 1, RAND_MAX (each of the four) on the cluster draw of individuals 0,
    255, 256 and I - 1, and runs of them over the first and the last copies, the first copies of the second tile (tile form)
    or of the second chunk of loci (general form).  For the tie families the placed draws put TIE_Q on the cluster draws and
    TIE_P on the allele draws: the draw equals a partial sum of the row, or the sum lies one ulp either side;
  * live against the reference (`ref_time --bootstrap` without -a) on a subset, and against the committed golden multi_mix_k3;
  * the generated data set is a working data set: the log likelihood of the same bytes uploaded."""
import numpy as np
import pytest

import multiclust_amd as mc
import oracle_bind as ob
import rand_window as rw
from golden_util import Golden
from test_bootstrap_cpu import golden_bootstrap
from test_generators_cpu import (EDGE_DRAWS, FAMILIES, TIE_P, TIE_Q, counts_of, family_params, host_bootstrap, needs_ref,
                                 reference_bootstrap)
from test_gpu_generators import NO_SIM_TILE, context_for, contexts, sim_ua  # noqa: F401 (contexts is a fixture)

# ---------------------------------------------------------------------------------------------------------------- DISPATCH RULE
SIM_PW = 4                   # mchip_generators.hip: width of the padded allele rows
MIX_GENERAL_CHUNK = 64       # mchip_generators.hip: loci per workgroup of the general form


def mix_form(max_M, ploidy, knobs):
    """mchip_simulate_genotypes_mixture: fast_p = max_M <= SIM_PW; the tile form when fast_p && ploidy <= 8 && !sim_no_tile, at
    every K; otherwise the general form, on padded allele rows when fast_p"""
    fast_p = max_M <= SIM_PW
    if fast_p and ploidy <= 8 and "MCHIP_SIM_NO_TILE" not in knobs:
        return "k_simulate_mixture_tile<%d>" % ploidy
    return "k_simulate_mixture_general<%s>" % ("padded" if fast_p else "rows")


def mix_chunk(K, L, max_M, ploidy, knobs):
    """loci per workgroup: the tile of the tile form, MIX_GENERAL_CHUNK in the general form"""
    if "tile" not in mix_form(max_M, ploidy, knobs):
        return MIX_GENERAL_CHUNK
    return min(max((16384 // (K * 12)) & ~7, 8), 512, (L + 7) & ~7)


# ------------------------------------------------------------------------------------------------------------------ CASES
def _tile_case(ploidy, K, I):
    L = mix_chunk(K, 1 << 20, 4, ploidy, {}) + 5       # a second tile of 5 loci; not a multiple of the tile or of 8
    return (I, L, ploidy, K, 2, 4, {})


# (I, L, ploidy, K, min alleles, max alleles, knobs): I = 256 n +- 1
MIX_CASES = [
    _tile_case(1, 2, 257), _tile_case(2, 9, 255), _tile_case(3, 5, 257), _tile_case(4, 3, 513),
    _tile_case(5, 64, 255), _tile_case(6, 8, 257), _tile_case(7, 1, 257), _tile_case(8, 27, 257),
    (257, 75, 9, 8, 2, 4, {}),                 # general on padded rows: ploidy > 8
    (511, 203, 2, 6, 2, 4, NO_SIM_TILE),       # general on padded rows: MCHIP_SIM_NO_TILE
    (255, 83, 3, 64, 2, 5, {}),                # general: K = 64, one more allele than the padded rows hold
    (257, 69, 2, 4, 5, 254, {}),               # general: 5 .. 254 alleles
    (255, 70, 12, 3, 2, 7, {}),                # general: ploidy > 8 and more than 4 alleles
]


def mix_case_id(c):
    I, L, ploidy, K, lo, hi, knobs = c
    return "%s-I%d-L%d-pl%d-K%d-M%d%s" % (mix_form(hi, ploidy, knobs), I, L, ploidy, K, hi, "-notile" if knobs else "")


def mix_draws(I, L, ploidy):
    return I + I * L * ploidy


def mix_placed_draws(family, pos, A, rotate=0):
    """the 31 draws placed at draw `pos` of the mixture stream.  Tie families: TIE_Q on cluster draws (j % A == 0), TIE_P on allele
    draws, both values of each in turn.  Others: the four edge draws in turn, `rotate` choosing which of them draw `pos` takes."""
    if family.startswith("tie"):
        return [TIE_Q[(j // A) % 2] if j % A == 0 else TIE_P[j % 2] for j in range(pos, pos + 31)]
    return [EDGE_DRAWS[(j - pos + rotate) % 4] for j in range(pos, pos + 31)]


def mix_windows(family, I, L, ploidy, chunk, seed):
    """(name, window): the stream of srand(seed); each edge draw on the cluster draw of individuals 0, 255, 256, I - 1; runs of
    placed draws over the first copies, the last copies, and the first copies of individual 1's second tile / chunk of loci"""
    A, n = 1 + L * ploidy, mix_draws(I, L, ploidy)
    out = [("seed", ob.glibc_window(seed)[0])]
    for i in sorted({0, 255, 256, I - 1}):
        if i >= I:
            continue
        for r in range(1 if family.startswith("tie") else 4):
            pos = i * A                    # A >= 31 in every case: the 31 placed draws end inside the individual's own span
            assert pos <= n - 31
            out.append(("cluster draw of %d, edge %d" % (i, r), rw.window_placing(mix_placed_draws(family, pos, A, r), pos, fill_seed=seed)))
    for name, pos in (("first copies", 1), ("last copies", n - 31), ("second chunk", A + 1 + chunk * ploidy - 16)):
        pos = min(max(pos, 0), n - 31)
        out.append((name, rw.window_placing(mix_placed_draws(family, pos, A), pos, fill_seed=seed)))
    return out


# ------------------------------------------------------------------------------------------------------------------ GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("case", MIX_CASES, ids=[mix_case_id(c) for c in MIX_CASES])
def test_mixture_generator_on_every_form(contexts, monkeypatch, case):
    """every family x every window, against the host generator; the message lists every combination that differs"""
    I, L, ploidy, K, lo, hi, knobs = case
    ctx = context_for(contexts, knobs, monkeypatch)
    ua = sim_ua(L, lo, hi, seed=I + L + K)
    chunk = mix_chunk(K, L, hi, ploidy, knobs)
    bad = []
    for family in FAMILIES:
        eta, p = family_params(family, I, ua, K, shared=True, seed=K + ploidy + len(family))
        for name, window in mix_windows(family, I, L, ploidy, chunk, seed=I * L):
            want, _, _ = host_bootstrap(I, L, ploidy, ua, K, eta, p, window, 0, 0)
            ctx.simulate_genotypes_mixture(I, L, ploidy, ua, window, K, eta, p)
            got = ctx.get_genotypes()
            if not np.array_equal(got, want):
                bad.append("%s/%s: %d copies differ" % (family, name, int(np.sum(got != want))))
    assert not bad, "; ".join(bad)


REF_FAMILIES = ("negative", "nan_p", "tie-ulp")


@pytest.mark.gpu
@needs_ref
@pytest.mark.parametrize("case", MIX_CASES, ids=[mix_case_id(c) for c in MIX_CASES])
def test_mixture_generator_equals_the_reference(contexts, monkeypatch, tmp_path, case):
    I, L, ploidy, K, lo, hi, knobs = case
    ctx = context_for(contexts, knobs, monkeypatch)
    ua = sim_ua(L, lo, hi, seed=I + L + K)
    chunk = mix_chunk(K, L, hi, ploidy, knobs)
    for family in REF_FAMILIES:
        eta, p = family_params(family, I, ua, K, shared=True, seed=K + ploidy + len(family))
        name, window = mix_windows(family, I, L, ploidy, chunk, seed=I * L)[1]      # an edge (or tie) draw on individual 0's cluster draw
        ctx.simulate_genotypes_mixture(I, L, ploidy, ua, window, K, eta, p)
        ref, _ = reference_bootstrap(str(tmp_path / family), I, L, ploidy, ua, K, eta, p, window, 0, 0)
        assert np.array_equal(counts_of(ctx.get_genotypes(), ua), ref), (family, name)


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", [{}, NO_SIM_TILE], ids=["tile", "general"])
def test_mixture_generator_equals_the_golden_replicate(contexts, monkeypatch, knobs):
    """the data set the reference's own parametric_bootstrap() drew for the mixture model (tests/golden/multi_mix_k3/bs_ilm.u8)"""
    g = Golden("multi_mix_k3")
    ctx = context_for(contexts, knobs, monkeypatch)
    window, _ = ob.glibc_window(g.m["bootstrap_seed"])
    ctx.simulate_genotypes_mixture(g.I, g.L, g.ploidy, g.ua, window, g.K, g.q("bs"), g.p("bs"))
    assert np.array_equal(counts_of(ctx.get_genotypes(), g.ua), golden_bootstrap(g))


@pytest.mark.gpu
@pytest.mark.parametrize("case", [MIX_CASES[3], MIX_CASES[10]], ids=["tile", "general"])
def test_generated_mixture_data_set_is_a_working_data_set(contexts, monkeypatch, case):
    """same log likelihood as the same bytes uploaded; a second replicate into the same context re-uses its buffers"""
    I, L, ploidy, K, lo, hi, knobs = case
    ctx = context_for(contexts, knobs, monkeypatch)
    ua = sim_ua(L, lo, hi, seed=I + L + K)
    eta, p = family_params("natural", I, ua, K, shared=True, seed=3)
    for seed in (11, 12):
        window, _ = ob.glibc_window(seed)
        ctx.simulate_genotypes_mixture(I, L, ploidy, ua, window, K, eta, p)
        sim = ctx.get_genotypes()
        ctx.set_model(K, admixture=0, lower_bound=1e-8)
        ctx.set_q(0, eta)
        ctx.set_p(0, p)
        ll_generated = ctx.loglik(0)
        other = mc.Context(0)
        other.set_genotypes(ua, sim)
        other.set_model(K, admixture=0, lower_bound=1e-8)
        other.set_q(0, eta)
        other.set_p(0, p)
        assert other.loglik(0) == ll_generated and np.isfinite(ll_generated)
        other.close()
