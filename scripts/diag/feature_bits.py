"""Bit-level fingerprint (SHA-256) of every output of the data-set features and of the K-independent reductions, at the smallest
shapes at which each of their staging and summation helpers (multiclust_amd/csrc/mchip_device_util.h) can go wrong: run it under
two builds of the library (MCHIP_LIB_PATH), each in a fresh process, and diff the two outputs.  With them, the values that pass through the context's record of device scalars (mchip_scalars): EM steps, dot products,
a batched EM run and batched accelerated cycles under schemes 1 to 4, for both models.  Beside scripts/diag/bits.py, which
fingerprints the EM path at larger shapes."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import impute_util as iu
from multiclust_amd import hip
from synth import make_dataset, random_params

# three workgroup sizes of the lane-per-individual passes, P rows staged and not (tests/feature_geometry.py)
CASES = [(1, 2), (8, 4), (27, 2), (28, 2), (52, 2), (64, 6), (64, 7)]


def sha(*parts):
    h = hashlib.sha256()
    for x in parts:
        if x is None:
            h.update(b"none")
        elif isinstance(x, (int, np.integer)):
            h.update(np.int64(x).tobytes())
        elif isinstance(x, float):
            h.update(np.float64(x).tobytes())
        else:
            h.update(np.ascontiguousarray(x).tobytes())
    return h.hexdigest()


def divergence_parts(d):
    return [d[k] for k in ("het", "sqdiff", "locus_v", "locus_ht", "sum_v", "sum_ht", "n_loci")]


def slots(ctx):
    return [a for s in range(3) for a in (ctx.get_q(s), ctx.get_p(s))]


def accel_runs(ctx, label, q0, p0):
    """batched accelerated cycles (mchip_accel_run) under every scheme, each from two EM steps of (q0, p0): the run state the device
    decided (stop rule, step size, accept test) and the three slots"""
    for scheme in (1, 2, 3, 4):
        ctx.set_q(0, q0)
        ctx.set_p(0, p0)
        ctx.em_step(0, 1, sync=False)
        ctx.em_step(1, 0, sync=False)
        st = hip.RunState(logL=-np.inf, abs_error=1e-3, max_iter=25, n_iter=0)
        rc = ctx.lib.mchip_accel_run(ctx.h, 0, scheme, 3, C.byref(st))
        if rc:      # refused (no sparse layout for this data set): the same under either build
            print(label, "accel_run scheme %d status %d" % (scheme, rc), flush=True)
            continue
        run =(st.logL, st.bad_loglik, st.n_iter, st.stopped, st.converged, st.iter_stop, st.fatal)
        print(label, "accel_run scheme %d n_iter=%d stopped=%d fatal=%d" % (scheme, st.n_iter, st.stopped, st.fatal), sha(*run), sha(*slots(ctx)),
              flush=True)


def features(ctx, label, ua, n_real, geno, K, shared):
    I, L, pl = geno.shape
    q0, p0 = random_params(I, ua, K, seed=3 + K)
    ctx.set_genotypes(ua, geno)
    print(label, "data_counts", sha(*ctx.data_counts()), flush=True)
    ctx.set_model(K, admixture=1, eta_constrained=int(shared))
    ctx.set_q(0, q0.mean(axis=0) if shared else q0)
    ctx.set_p(0, p0)
    print(label, "impute", sha(*ctx.impute_missing(0, n_real)))
    print(label, "divergence", sha(*divergence_parts(ctx.divergence(0, np.arange(1, K + 1) / K))))
    print(label, "resid+norms", sha(*ctx.residual_products(0, True)))
    print(label, "resid", sha(*ctx.residual_products(0, False)))
    if not shared:
        rows = np.arange(0, I, 3, dtype=np.int32)
        print(label, "fit_q_rows", sha(*ctx.fit_q_rows(0, rows, 20, rel_error=1e-9)), sha(*ctx.fit_q_rows(0, rows, 5, from_slot=True)))
    folds = np.random.default_rng(I + L).integers(0, 5, size=(I, L)).astype(np.uint8)
    ctx.cv_set_folds(folds, 5)
    for f in (1, 4):
        ctx.cv_hold_out(f)
        print(label, "cv fold %d" % f, sha(*ctx.cv_heldout_loglik(0, 1.0 / (I * pl + 1))))
    ctx.cv_hold_out(-1)
    # two EM steps (shared mixing proportions: k_column_sums), the secants between them and their dot products
    ll = [ctx.em_step(0, 1), ctx.em_step(1, 2)]
    ctx.secant(0, 0, 1, 0)
    ctx.secant(1, 0, 2, 1)
    print(label, "em_step", sha(*(ll + slots(ctx))), "dots", sha(*(ctx.step_dots(0) + ctx.secant_dots(0, 0))))
    # a batched run that its own stop check ends: the absolute error, or the iteration limit
    st = hip.RunState(logL=-np.inf, abs_error=1e-3, max_iter=25, n_iter=0)
    rc = ctx.lib.mchip_em_run(ctx.h, 0, 40, C.byref(st))
    assert rc == 0 and st.stopped and not st.fatal, (label, rc, st.stopped, st.fatal)
    print(label, "em_run n_iter=%d converged=%d" % (st.n_iter, st.converged), sha(st.logL, *slots(ctx)), flush=True)
    accel_runs(ctx, label, q0.mean(axis=0) if shared else q0, p0)


def mixture_accel(ctx, label, ua, geno, K):
    q0, p0 = random_params(geno.shape[0], ua, K, seed=3 + K)
    ctx.set_genotypes(ua, geno)
    ctx.set_model(K, admixture=0)
    accel_runs(ctx, label, q0.mean(axis=0), p0)


def main():
    ctx = hip.Context(0)
    for K, alleles in CASES:
        for I in (63, 257):
            for L in (9, 130):
                for pl in (2, 4):
                    for missing in (0.0, 0.3):
                        ua, n_real, geno = iu.impute_dataset(I, L, pl, alleles, missing, seed=I + L + pl + K, specials=False)
                        for shared in (False, True):
                            label = "K%d a%d I%d L%d pl%d miss%g %s:" % (K, alleles, I, L, pl, missing, "shared" if shared else "indiv")
                            features(ctx, label, ua, n_real, geno, K, shared)
                        mixture_accel(ctx, "K%d a%d I%d L%d pl%d miss%g mixture:" % (K, alleles, I, L, pl, missing), ua, geno, K)
    # divergence with T on either side of the columns staged at a time (64) and of a workgroup's chunk (1024), both models
    for L in (31, 32, 33, 511, 512, 513):
        for K in (1, 8, 27, 64):
            ua, geno = make_dataset(63, L, 3, ploidy=2, max_alleles=2, seed=L)
            _, p0 = random_params(63, ua, K, seed=L + K)
            ctx.set_genotypes(ua, geno)
            for admixture in (1, 0):
                ctx.set_model(K, admixture=admixture)
                ctx.set_p(0, p0)
                d = ctx.divergence(0, np.ones(K))
                print("divergence T%d K%d admixture%d:" % (2 * L, K, admixture), sha(*divergence_parts(d)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
