"""-m gpu: mchip_kinship_products (multiclust_amd/csrc/mchip_kinship.hip) against the long-double reference of its definitions
(tests/kin_util.py, whose docstring derives the bounds), on the shapes of tests/test_gpu_resid.py: the chunks, the product kernel and
the mirror are shared with mchip_residual_products (mchip_gram.h), the tile pass k_kin_tile is k_resid_tile's with w = a sqrt(t (1 - t))
beside r.  What the kernels do with the bounds' assumptions: t by the fma chain, 1 - t one subtraction, fmax, one product, a square root
(correctly rounded or not: two u are allowed for it) and the product with the copies; the sums as G's, any order, at most two roundings
per term.  `gram` is asserted equal, bit for bit, to mchip_residual_products' on the same state in every case.

Each case prints error / bound of G and V."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cli_util import ROOT
from device_util import ctx, snapshot, status_of
import kin_util as ku
import resid_util as ru
from multiclust_amd import hip
from test_gpu_resid import CHUNK, FORMS, IS, TS, install, n_chunks, shaped_ua

pytestmark = pytest.mark.gpu


def run_case(ctx, ua, geno, K, Q, P, form=FORMS[0], what=""):
    install(ctx, ua, geno, K, Q, P, form)
    G, V = ctx.kinship_products(0)
    ref = ku.reference(ua, geno, Q, P)
    r = ku.check(G, V, ref)
    print("I=%d L=%d T=%d K=%d ploidy=%d %s: error / bound %s" % (geno.shape[0], len(ua), int(np.sum(ua)), K, geno.shape[2], what,
                                                                   " ".join("%s %.3f" % kv for kv in sorted(r.items()))))
    Gr, _ = ctx.residual_products(0, want_norms=False)
    assert G.tobytes() == Gr.tobytes()                            # the same chunks, kernel and order: the same bits
    assert np.array_equal(V, V.T)
    return G, V, ref


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("I", IS)
def test_individuals_and_columns_either_side_of_every_tile(I, T, ctx):
    """biallelic diploid loci at K = 3, 10 % of the copies missing: I around the MFMA tile, the wave's quarter and the workgroup's
    tile, in one, two and three tiles a side; T around one chunk and in three, with every residue mod 4"""
    ua, geno = ru.biallelic(I, T, seed=I + T, missing=0.1)
    assert int(ua.sum()) == T and n_chunks(ua) == {511: 1, 512: 1, 513: 2, 514: 2, 1029: 3}[T]
    Q, P = ru.parameters(ua, I, 3, seed=I + T)
    run_case(ctx, ua, geno, 3, Q, P)


@pytest.mark.parametrize("K", [1, 2, 8, 27, 28, 64])
def test_every_k_of_the_list(K, ctx):
    I, L = 17, 65
    ua, geno = ru.biallelic(I, 2 * L, seed=K, missing=0.1)
    Q, P = ru.parameters(ua, I, K, seed=K)
    run_case(ctx, ua, geno, K, Q, P)


def test_multi_allelic_tetraploid_with_p_read_from_memory(ctx):
    """35 alleles at K = 64: the P rows of a block do not fit beside the q rows and are read from memory"""
    I, L, K = 17, 21, 64
    ua = shaped_ua(L)
    geno = ru.genotypes(ua, I, 4, seed=4, missing=0.1)
    Q, P = ru.parameters(ua, I, K, seed=4 + K)
    _, _, ref = run_case(ctx, ua, geno, K, Q, P, what="tetraploid")
    assert ((ref["a"] > 0) & (ref["a"] < 4)).any() and int(ua.max()) == 35


def test_shared_proportions(ctx):
    I, K = 17, 3
    ua, geno = ru.biallelic(I, 131, seed=9, missing=0.1)
    Q, P = ru.parameters(ua, I, K, seed=9)
    run_case(ctx, ua, geno, K, Q[0], P, FORMS[1], what="shared")


def test_without_a_missing_copy_the_diagonal_is_the_reference(ctx):
    """V_ii = sum_c a^2 t (1 - t): within its bound like every element, and with nothing missing the whole of V is positive"""
    I = 65
    ua, geno = ru.biallelic(I, 514, seed=8)
    Q, P = ru.parameters(ua, I, 3, seed=8)
    G, V, ref = run_case(ctx, ua, geno, 3, Q, P, what="no missing")
    d = np.abs(np.diag(V).astype(ku.LD) - np.diag(ref["V"]))
    assert ref["no_missing"] and (d <= np.diag(ref["v_bound"])).all() and (V > 0).all()
    phi = ku.kinship(G, V)
    assert np.isfinite(phi).all() and np.array_equal(phi, phi.T)


@pytest.mark.parametrize("p_hi", [1 - 1e-8, 1 - 1e-120])
def test_near_fixed_parameters_give_no_nan(p_hi, ctx):
    """one-hot q rows against columns at 1 - 1e-8 and at the 1e-120 bound (1 - 1e-120 is 1 in a double): t (1 - t) is tiny or 0,
    never negative under the root"""
    I, K = 17, 3
    ua, geno = ru.biallelic(I, 130, seed=14, missing=0.1)
    P = np.zeros((K, 130))
    P[:, 0::2], P[:, 1::2] = p_hi, max(1 - p_hi, 1e-120)
    P[1] = P[1].reshape(-1, 2)[:, ::-1].reshape(-1)               # cluster 1 fixed for the other allele
    Q = np.zeros((I, K))
    Q[np.arange(I), np.arange(I) % K] = 1.0
    G, V, _ = run_case(ctx, ua, geno, K, Q, P, what="near fixed")
    assert np.isfinite(V).all() and np.isfinite(G).all() and (V >= 0).all()


def test_an_individual_without_data_has_a_zero_row_and_column(ctx):
    I = 17
    ua, geno = ru.biallelic(I, 131, seed=7, missing=0.2)
    geno[5] = ru.MISSING
    Q, P = ru.parameters(ua, I, 3, seed=7)
    G, V, _ = run_case(ctx, ua, geno, 3, Q, P, what="20 % missing")
    assert not V[5].any() and not V[:, 5].any() and not G[5].any() and not G[:, 5].any()
    phi = ku.kinship(G, V)
    assert np.isnan(phi[5]).all() and np.isnan(phi[:, 5]).all() and np.isfinite(np.delete(np.delete(phi, 5, 0), 5, 1)).all()


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
        install(b, ua, masked, K, Q, P)
        Ga, Va = a.kinship_products(0)
        Gb, Vb = b.kinship_products(0)
        assert ku.hexbits(Ga, Va) == ku.hexbits(Gb, Vb)
        ku.check(Ga, Va, ku.reference(ua, masked, Q, P))
        a.cv_hold_out(-1)
        Gf, Vf = a.kinship_products(0)
        ku.check(Gf, Vf, ku.reference(ua, geno, Q, P))
        assert not np.array_equal(Vf, Va)
    finally:
        a.close()
        b.close()


def test_bits_do_not_depend_on_the_launch_geometry_or_the_form(ctx):
    """the same case in fresh processes, one per setting and each under its own time limit: MCHIP_BLOCKS_PER_CU = 1,
    MCHIP_BLOCKS_PER_CU_IND = 8, and the two products of a chunk as two launches instead of one"""
    here = ku.hexbits(*ku.fixed_case(ctx))
    knobs = ("MCHIP_BLOCKS_PER_CU", "MCHIP_BLOCKS_PER_CU_IND", "MCHIP_KIN_TWO_LAUNCHES")
    for name, value in (("MCHIP_BLOCKS_PER_CU", "1"), ("MCHIP_BLOCKS_PER_CU_IND", "8"), ("MCHIP_KIN_TWO_LAUNCHES", "1")):
        env = {k: v for k, v in os.environ.items() if k not in knobs}
        env[name] = value
        env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "kin_util.py")], stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, text=True, timeout=120, env=env, cwd=ROOT)
        assert res.returncode == 0, (name, res.stderr[-2000:])
        assert res.stdout.strip() == here, name


def test_state_is_untouched():
    """slots, secants, expected counts, the data set and the log likelihood before and after, bit for bit; and a context that asked for
    the sums goes on exactly as one that did not (the held S-side sums included)"""
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
                    G, V = c.kinship_products(slot)
                    ku.check(G, V, ku.reference(ua, geno, c.get_q(slot), c.get_p(slot)))
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
    G, V = np.full((I, I), -3.0), np.full((I, I), -3.0)

    def call(c, slot, gram=True, scale=True):
        return status_of(lib.mchip_kinship_products(c.h, slot, G.ctypes.data if gram else None, V.ctypes.data if scale else None))

    fresh = hip.Context(0)
    assert call(fresh, 0) == "STATE"                             # no data set
    fresh.set_genotypes(ua, geno)
    assert call(fresh, 0) == "STATE"                             # no model
    fresh.set_model(K, admixture=0)
    assert call(fresh, 0) == "UNSUPPORTED"                       # the mixture model
    # two I x I sums of doubles that no device holds (720 GB each): 300 000 individuals at one locus
    fresh.set_genotypes(np.array([2], dtype=np.int32), np.zeros((300000, 1, 2), dtype=np.uint8))
    fresh.set_model(1)
    assert call(fresh, 0) == "ALLOC"
    fresh.close()
    install(ctx, ua, geno, K, Q, P)
    for slot in (-1, 3):
        assert call(ctx, slot) == "INVALID"
    assert call(ctx, 0, gram=False) == "INVALID" and call(ctx, 0, scale=False) == "INVALID"
    assert (G == -3.0).all() and (V == -3.0).all()
    assert call(ctx, 0) == "OK"                                  # ... and the call still works afterwards
    ku.check(G, V, ku.reference(ua, geno, Q, P))
