"""The CPU oracle (oracle/mc_oracle.c in reference operation order) against the reference's own em() (oracle/_ref/ref_time), live,
on drawn shapes: ploidy 1-6, up to 12 alleles per locus, K 1-12, admixture / -c / mixture, plain EM and every acceleration
scheme.  Same iterate BIT FOR BIT -- log likelihood, mixing proportions, allele frequencies, iteration count -- which is what lets
the GPU tests use the oracle as the reference's stand-in on shapes no committed golden covers (tests/test_gpu_fuzz.py).
A quarter of the cases carry 3 % missing copies, a quarter 25 %, most of them with the extra allele slot the reference's reader
gives a locus with missing values.
Runs without a GPU; skipped where the binary is absent."""
import json
import os
import subprocess

import numpy as np
import pytest

from cli_util import ROOT
import oracle_bind as ob
from synth import make_dataset, random_params

REF_TIME = os.path.join(ROOT, "oracle", "_ref", "ref_time")
pytestmark = pytest.mark.skipif(not os.access(REF_TIME, os.X_OK), reason="oracle/_ref/ref_time not built")


def draw_cases(n, seed):
    rs = np.random.default_rng(seed)
    out = []
    for c in range(n):
        out.append((c, int(rs.integers(3, 70)), int(rs.integers(1, 90)), int(rs.choice([1, 2, 2, 2, 3, 4, 6])), int(rs.choice([2, 3, 4, 6, 12])),
                    int(rs.choice([1, 2, 3, 4, 5, 8, 12])), str(rs.choice(["admix", "admix", "admix_c", "mix"])),
                    int(rs.choice([0, 0, 1, 2, 3, 4, 5, 6])), int(rs.integers(2, 12)), int(rs.integers(1, 10 ** 6))))
    return out


@pytest.mark.parametrize("c,I,L,ploidy,maxal,K,model,scheme,iters,seed",
                         draw_cases(int(os.environ.get("MC_ORACLE_CASES", "60")), 99 + int(os.environ.get("MC_ORACLE_SEED", "0"))))
def test_oracle_against_the_reference_em_bit_for_bit(c, I, L, ploidy, maxal, K, model, scheme, iters, seed, tmp_path):
    I = max(I, K)
    missing = [0.0, 0.0, 0.03, 0.25][seed % 4]
    ua, geno = make_dataset(I, L, max(K, 2), ploidy=ploidy, max_alleles=maxal, seed=seed, missing=missing)
    if missing and seed % 8 < 6:
        # as the reference's reader shapes such data: a locus with missing copies counts one allele slot more, which nothing matches
        ua = (ua + (geno == 0xFF).any(axis=(0, 2)).astype(np.int32)).astype(np.int32)
    compare_with_reference(I, L, ploidy, K, model, scheme, iters, seed, ua, geno, tmp_path)


# The edge shapes of tests/test_gpu_kernel_matrix.py, outside the drawn range above: K on both sides of the lane splits (28, 37,
# 49) and K = 64; a locus with exactly the largest allele count the sparse pass takes at its K (the LDS edge) and one more; 33
# alleles; 65-120 alleles at one locus; ploidy 16 (no packed counts); projection off; lower bound 1e-40.
#   (I, L, ploidy, alleles per locus (low, high), K, model, scheme, iterations, missing, projection, bound, seed)
EDGE_SHAPES = [
    (70, 45, 2, (2, 4), 28, "admix", 0, 3, 0.0, 1, 1e-8, 1),
    (65, 37, 2, (2, 4), 37, "admix", 3, 4, 0.03, 1, 1e-8, 2),
    (63, 29, 4, (2, 4), 49, "admix", 0, 3, 0.0, 1, 1e-8, 3),
    (66, 21, 2, (2, 3), 64, "admix_c", 0, 3, 0.03, 1, 1e-8, 4),
    (65, 25, 2, (2, 6), 64, "mix", 0, 2, 0.0, 1, 1e-8, 5),
    (65, 30, 2, (2, 18), 27, "admix", 0, 3, 0.0, 1, 1e-8, 6),
    (65, 30, 2, (2, 19), 27, "admix", 0, 3, 0.0, 1, 1e-8, 7),
    (63, 27, 2, (2, 8), 56, "admix", 0, 2, 0.0, 1, 1e-8, 8),
    (63, 27, 4, (2, 9), 49, "admix", 0, 2, 0.03, 1, 1e-8, 9),
    (70, 25, 2, (2, 33), 5, "admix", 3, 4, 0.0, 1, 1e-8, 10),
    (80, 15, 2, (2, 120), 3, "admix", 0, 3, 0.0, 1, 1e-8, 11),
    (70, 12, 2, (2, 65), 37, "admix", 0, 2, 0.03, 1, 1e-8, 12),
    (70, 14, 3, (2, 90), 4, "mix", 0, 3, 0.0, 1, 1e-8, 13),
    (40, 30, 16, (2, 4), 6, "admix", 0, 3, 0.03, 1, 1e-8, 14),
    (40, 30, 16, (2, 4), 5, "mix", 0, 3, 0.0, 1, 1e-8, 15),
    (65, 40, 2, (2, 4), 8, "admix", 0, 3, 0.03, 0, 1e-8, 16),
    (65, 40, 4, (2, 4), 52, "admix", 0, 2, 0.0, 0, 1e-8, 17),
    (65, 40, 4, (2, 4), 52, "admix", 0, 2, 0.0, 1, 1e-40, 18),
    (65, 40, 2, (2, 3), 12, "admix", 3, 4, 0.03, 1, 1e-40, 19),
    (63, 33, 2, (2, 4), 28, "admix_c", 0, 3, 0.0, 0, 1e-8, 20),
]


@pytest.mark.parametrize("I,L,ploidy,spec,K,model,scheme,iters,missing,projection,bound,seed", EDGE_SHAPES)
def test_oracle_against_the_reference_em_bit_for_bit_on_the_matrix_edges(I, L, ploidy, spec, K, model, scheme, iters, missing,
                                                                         projection, bound, seed, tmp_path):
    rs = np.random.default_rng(seed)
    ua, geno = make_dataset(I, L, max(K, 2), ploidy=ploidy, max_alleles=min(spec[1], 12), seed=seed, missing=missing)
    ua = ua.copy()
    for l, M in ((0, spec[0]), (L // 2, spec[1])):          # exactly the smallest and the largest allele count asked for
        ua[l] = M
        geno[:, l, :] = np.where(geno[:, l, :] == 0xFF, 0xFF, rs.integers(0, M, size=(I, ploidy))).astype(np.uint8)
    compare_with_reference(I, L, ploidy, K, model, scheme, iters, seed, ua, geno, tmp_path, projection=projection, bound=bound)


def compare_with_reference(I, L, ploidy, K, model, scheme, iters, seed, ua, geno, tmp_path, projection=1, bound=1e-8):
    admixture, constrained = int(model != "mix"), int(model == "admix_c")
    if K == 1:
        scheme = 0                                         # em() leaves before any acceleration (em_alg.c:49-58)
    lb = min(bound, 0.5 / (I * ploidy))
    q0, p0 = random_params(I, ua, K, seed=seed + 1, lower_bound=lb)
    if constrained or not admixture:
        q0 = np.ascontiguousarray(q0.mean(axis=0) / q0.mean(axis=0).sum())
    d = str(tmp_path)
    np.ascontiguousarray(ua, dtype=np.int32).tofile(d + "/ua.i32")
    geno.tofile(d + "/geno.u8")
    q0.tofile(d + "/q0.f64")
    p0.tofile(d + "/p0.f64")
    flags = (["-a"] if admixture else []) + (["-c"] if constrained else []) + ["-k", str(K)] + (["-s", str(scheme)] if scheme else [])
    flags += (["--projection"] if not projection else []) + (["--bound", repr(bound)] if bound != 1e-8 else [])
    res = subprocess.run([REF_TIME, d, str(I), str(L), str(ploidy), str(K), str(iters - 1), "--", "-f", "x"] + flags,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    opt = ob.make_options(admixture=admixture, eta_constrained=constrained, lower_bound=lb, fused=0, accel_scheme=scheme,
                          abs_error=1e-300, max_iter=iters - 1, do_projection=projection)
    mod = ob.Model(ob.Data(I, L, ploidy, ua, geno), opt, K)
    mod.q(0)[...] = q0
    mod.p(0)[...] = p0
    mod.em()
    if res.returncode == 0 and not res.stdout.strip():
        # the reference left through exit(0): "nan", or a log likelihood one ulp lower at a fixed point reached to the last bit;
        # the oracle reports the same ending as a fatal state
        assert mod.fatal != 0, res.stderr[-300:]
        return
    assert res.returncode == 0, res.stderr[-1000:]
    ref = json.loads(res.stdout)
    assert mod.fatal == 0 and ref["n_iter"] == mod.n_iter
    assert ref["lower_bound"] == lb and ref["logL"] == mod.logL
    # (equal_nan: an individual whose every copy is missing -- a one-locus draw at 25 % -- has mixing proportions 0 / 0 in both)
    assert np.array_equal(np.fromfile(d + "/q_ref.f64").reshape(mod.q(mod.pindex).shape), mod.q(mod.pindex), equal_nan=True)
    assert np.array_equal(np.fromfile(d + "/p_ref.f64").reshape(K, -1), mod.p(mod.pindex), equal_nan=True)
