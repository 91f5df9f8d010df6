"""-m gpu: mchip_residual_products (multiclust_amd/csrc/mchip_residuals.hip) against the long-double reference of its definitions
(tests/resid_util.py, whose docstring derives the bounds).

What the kernels do with the bounds' assumptions: k_resid_tile forms t by the fma chain and r by one fma (the e of the bounds), s by an
fma chain over the locus's columns; k_resid_gram adds an element's products in column order, four to an FP64 matrix instruction, whose
internal order and rounding (fused or not) the bounds leave open: any order, at most two roundings per term.  The individuals are
padded to tiles of 64 (TILE), a workgroup's waves own 32 x 32 quarters of 16 x 16 tiles: I on either side of 16, 64 and 128.  The
loci are cut into chunks of whole loci with at most CHUNK columns (and CHUNK loci) each, a constant of the unit restated here: the
cases on either side of it fail when it moves; the operand panels are staged 16 rows at a time and consumed 4 rows an instruction:
column totals of every residue mod 4.  k_resid_tile stages the P rows of a block of 8 loci beside the q rows when they fit and reads
them from memory when they do not (K = 64 with a locus of 35 alleles); from K = 28 on fewer than 256 lanes fit a workgroup.

Each case prints error / bound of G and D."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from cli_util import ROOT
from device_util import ctx, snapshot, status_of
import resid_util as ru
from multiclust_amd import hip, host

pytestmark = pytest.mark.gpu
CHUNK, TILE = 512, 64
IS = [1, 2, 15, 16, 17, 63, 64, 65, 130]
TS = [CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 2, 2 * CHUNK + 5]
FORMS = [dict(admixture=1, eta_constrained=0), dict(admixture=1, eta_constrained=1)]


def n_chunks(ua):
    """the chunks the unit cuts: whole loci, greedily, at most CHUNK columns and CHUNK loci each"""
    n, cols, loci = 1, 0, 0
    for M in ua:
        if loci and (cols + M > CHUNK or loci >= CHUNK):
            n, cols, loci = n + 1, 0, 0
        cols, loci = cols + int(M), loci + 1
    return n


def install(ctx, ua, geno, K, Q, P, form=FORMS[0]):
    ctx.set_genotypes(ua, geno)
    ctx.set_model(K, **form)
    ctx.set_q(0, Q)
    ctx.set_p(0, P)
    assert np.array_equal(ctx.get_p(0), P)


def run_case(ctx, ua, geno, K, Q, P, form=FORMS[0], what=""):
    install(ctx, ua, geno, K, Q, P, form)
    G, D = ctx.residual_products(0)
    ref = ru.reference(ua, geno, Q, P)
    r = ru.check(G, D, ref)
    print("I=%d L=%d T=%d K=%d ploidy=%d %s: error / bound %s" % (geno.shape[0], len(ua), int(np.sum(ua)), K, geno.shape[2], what,
                                                                   " ".join("%s %.3f" % kv for kv in sorted(r.items()))))
    return G, D, ref


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("I", IS)
def test_individuals_and_columns_either_side_of_every_tile(I, T, ctx):
    """biallelic diploid loci at K = 3, 10 % of the copies missing: I around the MFMA tile, the wave's quarter and the workgroup's
    tile, in one, two and three tiles a side; T around one chunk and in three, with every residue mod 4"""
    ua, geno = ru.biallelic(I, T, seed=I + T, missing=0.1)
    assert int(ua.sum()) == T and n_chunks(ua) == {511: 1, 512: 1, 513: 2, 514: 2, 1029: 3}[T]
    assert sorted({t % 4 for t in TS}) == [0, 1, 2, 3]
    Q, P = ru.parameters(ua, I, 3, seed=I + T)
    run_case(ctx, ua, geno, 3, Q, P)


@pytest.mark.parametrize("K", [1, 2, 8, 27, 28, 64])
def test_every_k_of_the_list(K, ctx):
    I, L = 17, 65
    ua, geno = ru.biallelic(I, 2 * L, seed=K, missing=0.1)
    assert len(ua) == L
    Q, P = ru.parameters(ua, I, K, seed=K)
    run_case(ctx, ua, geno, K, Q, P)


def shaped_ua(L):
    """two columns mostly, a phantom third on some, and a monomorphic locus, one with 35 columns and two without a column"""
    ua = np.where(np.arange(L) % 3 == 1, 3, 2).astype(np.int32)
    ua[1], ua[2], ua[L // 2], ua[L - 1] = 1, 35, 0, 0
    return ua


@pytest.mark.parametrize("K", [3, 64])
@pytest.mark.parametrize("ploidy", [1, 2, 4])
def test_ploidies_and_allele_shapes(ploidy, K, ctx):
    """35 alleles at K = 64: the P rows of a block do not fit beside the q rows and are read from memory"""
    I, L = 17, 21
    ua = shaped_ua(L)
    geno = ru.genotypes(ua, I, ploidy, seed=ploidy, missing=0.1)
    Q, P = ru.parameters(ua, I, K, seed=ploidy + K)
    G, D, ref = run_case(ctx, ua, geno, K, Q, P)
    if ploidy > 1:
        assert ((ref["a"] > 0) & (ref["a"] < ploidy)).any()       # partially missing genotypes are in play


def test_missing_copies_and_an_individual_without_one(ctx):
    I = 17
    ua, geno = ru.biallelic(I, 131, seed=7, missing=0.2)
    geno[5] = ru.MISSING
    Q, P = ru.parameters(ua, I, 3, seed=7)
    G, D, ref = run_case(ctx, ua, geno, 3, Q, P, what="20 % missing")
    assert not G[5].any() and not G[:, 5].any() and not D[5].any()
    assert D[:, 5].tolist() == [0.0] * I                          # nobody's residuals lie at a locus where 5 has data
    assert not np.array_equal(D, D.T) and (D <= np.diag(G)[:, None] * (1 + 1e-12)).all()


def test_without_a_missing_copy_the_norms_are_the_diagonal(ctx):
    I = 65
    ua, geno = ru.biallelic(I, 514, seed=8)
    Q, P = ru.parameters(ua, I, 3, seed=8)
    G, D, ref = run_case(ctx, ua, geno, 3, Q, P, what="no missing")
    assert ref["no_missing"] and np.array_equal(D, np.repeat(np.diag(G)[:, None], I, axis=1))


def test_shared_proportions_and_rows_on_a_vertex(ctx):
    I, K = 17, 3
    ua, geno = ru.biallelic(I, 131, seed=9, missing=0.1)
    Q, P = ru.parameters(ua, I, K, seed=9)
    run_case(ctx, ua, geno, K, Q[0], P, FORMS[1], what="shared")
    V = np.zeros((I, K))
    V[np.arange(I), np.arange(I) % K] = 1.0
    run_case(ctx, ua, geno, K, V, P, what="vertex")


def test_host_gives_nan_rows_and_columns(ctx):
    """host.Fit.residual_correlation (mc_residual_correlation): cor from the device's sums, NaN on the diagonal and in the row and
    column of an individual without an observed copy, symmetric bit for bit; the model left as it was"""
    I, K = 17, 3
    ua, geno = ru.biallelic(I, 131, seed=10, missing=0.2)
    geno[2] = ru.MISSING
    Q, P = ru.parameters(ua, I, K, seed=10)
    fit = host.Fit(ua, geno, K, admixture=1)
    try:
        fit.set_params(Q, P)
        held_q = fit.get_q(0)
        out = fit.residual_correlation()
        assert np.array_equal(fit.get_q(0), held_q, equal_nan=True) and np.array_equal(fit.get_p(0), P)
    finally:
        fit.close()
    install(ctx, ua, geno, K, Q, P)
    G, D = ctx.residual_products(0)
    cor = out["cor"]
    assert np.array_equal(cor, ru.correlation(G, D), equal_nan=True) and np.array_equal(cor, cor.T, equal_nan=True)
    nan = np.isnan(cor)
    want = np.eye(I, dtype=bool)
    want[2, :] = want[:, 2] = True
    assert np.array_equal(nan, want)
    ref = ru.reference(ua, geno, Q, P)
    assert np.abs(cor[~nan] - ref["cor"][~nan].astype(np.float64)).max() <= 1e-12
    assert out["n_pairs"] == (I - 1) * (I - 2) // 2 and out["ind_partner"][2] == -1 and np.isnan(out["ind_mean"][2])
    assert out["max"] == np.nanmax(cor) and cor[out["max_pair"]] == out["max"]


def test_under_a_hold_out_the_hidden_copies_are_missing_copies():
    """bit for bit what the masked data set gives when it is uploaded afresh"""
    I, K = 17, 3
    ua, geno = ru.biallelic(I, 2 * CHUNK + 5, seed=11, missing=0.05)
    folds = np.random.default_rng(12).integers(0, 3, size=geno.shape[:2]).astype(np.uint8)
    Q, P = ru.parameters(ua, I, K, seed=11)
    a, b = hip.Context(0), hip.Context(0)
    try:
        a.set_genotypes(ua, geno)
        a.cv_set_folds(folds, 3)
        a.set_model(K)
        a.cv_hold_out(1)
        a.set_q(0, Q)
        a.set_p(0, P)
        masked = geno.copy()
        masked[folds == 1] = ru.MISSING
        assert np.array_equal(a.get_genotypes(), masked)
        install(b, ua, masked, K, Q, P)
        Ga, Da = a.residual_products(0)
        Gb, Db = b.residual_products(0)
        assert ru.hexbits(Ga, Da) == ru.hexbits(Gb, Db)
        ru.check(Ga, Da, ru.reference(ua, masked, Q, P))
        a.cv_hold_out(-1)
        Gf, Df = a.residual_products(0)
        ru.check(Gf, Df, ru.reference(ua, geno, Q, P))
        assert not np.array_equal(Gf, Ga)
    finally:
        a.close()
        b.close()


def test_same_state_same_bits_and_without_the_norms(ctx):
    G1, D1 = ru.fixed_case(ctx)
    G2, D2 = ctx.residual_products(0)
    assert ru.hexbits(G1, D1) == ru.hexbits(G2, D2) and np.array_equal(G1, G1.T)
    G3, D3 = ctx.residual_products(0, want_norms=False)
    assert D3 is None and np.array_equal(G3, G1)


def test_bits_do_not_depend_on_the_launch_geometry(ctx):
    """the same case in fresh processes under MCHIP_BLOCKS_PER_CU = 1, 8 and unset: the chunks are constants, not shares of the device"""
    here = ru.hexbits(*ru.fixed_case(ctx))
    seen = []
    for knob in (None, "1", "8"):
        env = {k: v for k, v in os.environ.items() if k != "MCHIP_BLOCKS_PER_CU"}
        if knob:
            env["MCHIP_BLOCKS_PER_CU"] = knob
        env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "resid_util.py")], stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, text=True, timeout=120, env=env, cwd=ROOT)
        assert res.returncode == 0, res.stderr[-2000:]
        seen.append(res.stdout.strip())
    assert seen == [here] * 3


def test_state_is_untouched():
    """slots, secants, expected counts and the data set before and after, bit for bit; and a context that asked for the products goes
    on exactly as one that did not (the held S-side sums included)"""
    I, K = 17, 3
    ua, geno = ru.biallelic(I, 131, seed=13, missing=0.1)
    Q, P = ru.parameters(ua, I, K, seed=13)
    seen = []
    ctxs = [hip.Context(0) for _ in range(2)]
    try:
        for n, c in enumerate(ctxs):
            install(c, ua, geno, K, Q, P)
            c.em_step(0, 1)
            c.em_step(1, 2)
            c.secant(0, 0, 1, 0)
            c.secant(1, 0, 2, 1)
            ll0 = c.loglik_prefetch(2)                           # the S-side sums of slot 2 are held
            before = snapshot(c, 1)
            if n == 0:
                for slot in (0, 1, 2):
                    G, D = c.residual_products(slot)
                    ru.check(G, D, ru.reference(ua, geno, c.get_q(slot), c.get_p(slot)))
                assert snapshot(c, 1) == before
            ll1 = c.em_step(2, 0)                                # uses the held sums
            seen.append((ll0, ll1, snapshot(c, 1)))
        assert seen[0] == seen[1]
    finally:
        for c in ctxs:
            c.close()


def test_refusals_leave_the_outputs_alone(ctx):
    lib = ctx.lib
    I, K = 5, 3
    ua, geno = ru.biallelic(I, 9, seed=1, missing=0.1)
    Q, P = ru.parameters(ua, I, K, seed=1)
    G, D = np.full((I, I), -3.0), np.full((I, I), -3.0)

    def call(c, slot, gram=True):
        return status_of(lib.mchip_residual_products(c.h, slot, G.ctypes.data if gram else None, D.ctypes.data))

    fresh = hip.Context(0)
    assert call(fresh, 0) == "STATE"                             # no data set
    fresh.set_genotypes(ua, geno)
    assert call(fresh, 0) == "STATE"                             # no model
    fresh.set_model(K, admixture=0)
    assert call(fresh, 0) == "UNSUPPORTED"                       # the mixture model
    # two I x I sums of doubles that no device holds (720 GB each): 300 000 individuals at one locus
    big = 300000
    fresh.set_genotypes(np.array([2], dtype=np.int32), np.zeros((big, 1, 2), dtype=np.uint8))
    fresh.set_model(1)
    assert status_of(lib.mchip_residual_products(fresh.h, 0, G.ctypes.data, None)) == "ALLOC"
    fresh.close()
    install(ctx, ua, geno, K, Q, P)
    for slot in (-1, 3):
        assert call(ctx, slot) == "INVALID"
    assert call(ctx, 0, gram=False) == "INVALID"
    assert (G == -3.0).all() and (D == -3.0).all()
    # norms may be left out, and the call still works afterwards
    assert lib.mchip_residual_products(ctx.h, 0, G.ctypes.data, None) == 0
    assert (D == -3.0).all()
    full = ctx.residual_products(0)
    assert np.array_equal(G, full[0])
    ru.check(full[0], full[1], ru.reference(ua, geno, Q, P))
