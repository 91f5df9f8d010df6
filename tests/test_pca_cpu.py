"""No GPU: the matrix of --pca (include/multiclust_hip.h, mchip_bed_pca) as tests/pca_util.py restates it, and the host algebra of
multiclust_amd/csrc/mchip_pca_algebra.h as a sanitized program of its own (tests/pca_algebra_driver.cpp).

  - the long-double reference against exact rationals: counts, mu, t_l and the sums of W on small tables;
  - the bounds of tests/test_gpu_pca.py: float64 restatements of Y in three orders of addition lie within HALF of them;
  - the algebra: MGS2, Jacobi against numpy.linalg.eigh, the zero-column rule, the sign rule, the residual formula, and the whole
    iteration on a dense G against eigh, within the bounds the GPU test holds the device to;
  - mutants of the definition and of the iteration, each caught by the check the GPU tests apply;
  - the constants and the start vectors of the restatement held to the headers."""
import os
from fractions import Fraction

import numpy as np
import pytest

import bedfiles
from cli_util import ROOT
import host_driver
import pca_util as pu
from multiclust_amd import hip

LD = pu.LD


def test_the_feature_is_there():
    assert "mchip_bed_pca" in hip.ABI_SYMBOLS and "mchip_bed_pca_apply" in hip.ABI_SYMBOLS
    for f in ("csrc/mchip_pca.hip", "csrc/mchip_pca_algebra.h", "host/mc_pca.c"):
        assert os.path.exists(os.path.join(ROOT, "multiclust_amd", f)), f


# ---- the reference against exact rationals ----
SMALL = [(5, 9, 1), (7, 12, 2), (12, 10, 3), (4, 6, 4)]


@pytest.mark.parametrize("I,L,seed", SMALL)
def test_reference_against_exact_rationals(I, L, seed):
    codes, _ = pu.draw_codes(I, L, seed, missing=0.15)
    codes[:, 0] = bedfiles.HOM2
    codes[0, 0] = bedfiles.HET                                   # s = 2 n - 1: the variant nearest fixation
    rng = np.random.default_rng(seed)
    x = rng.integers(-8, 9, size=(I, 3)).astype(np.float64)      # exactly representable, and so is every exact product below
    ref = pu.reference(codes, x)
    n_used = 0
    t_sum = Fraction(0)
    for l in range(L):
        col = [int(c) for c in codes[:, l]]
        n0, n2, n3 = col.count(0), col.count(2), col.count(3)
        assert [n0, col.count(1), n2, n3] == list(pu.counts(codes)[l])
        n, s = n0 + n2 + n3, n2 + 2 * n3
        used = 0 < s < 2 * n
        assert used == bool(ref["used"][l])
        if not used:
            assert ref["mu"][l] == 0 and ref["inv"][l] == 0 and ref["t"][l] == 0 and not ref["Z"][:, l].any() and not ref["W"][l].any()
            continue
        n_used += 1
        mu = Fraction(s, n)
        assert ref["mu"][l] == float(mu)                         # one correctly rounded division
        # inv against the exact 1 / sqrt(mu (1 - mu / 2)): its square against the rational.  mu's one rounding is amplified by
        # 0.5 mu / (1 - 0.5 mu) <= 2 n in the second factor; product, square root and reciprocal add three more
        exact_inv2 = 1 / (mu * (1 - mu / 2))
        got_inv2 = Fraction(float(ref["inv"][l])) ** 2
        assert abs(got_inv2 - exact_inv2) <= exact_inv2 * Fraction(2 * (2 * n + 4), 2 ** 53)
        t_exact = (n0 * mu ** 2 + n2 * (1 - mu) ** 2 + n3 * (2 - mu) ** 2) * exact_inv2
        assert abs(Fraction(float(ref["t"][l])) - t_exact) <= t_exact * Fraction(6 * n + 20, 2 ** 53)
        t_sum += Fraction(float(ref["t"][l]))
        # Z and the sums of W: exact in rationals from the float64 mu and inv of the definition; long double rounds each z twice and
        # each of the I products and I - 1 additions once
        mu_f, inv_f = Fraction(float(ref["mu"][l])), Fraction(float(ref["inv"][l]))
        z = [Fraction(0) if c == 1 else (Fraction(int(pu.DOSAGE[c])) - mu_f) * inv_f for c in col]
        for i in range(I):
            assert abs(Fraction(float(ref["Z"][i, l])) - z[i]) <= abs(z[i]) * Fraction(1, 2 ** 52)
        for c in range(x.shape[1]):
            w = sum(z[i] * Fraction(int(x[i, c])) for i in range(I))
            room = sum(abs(z[i] * int(x[i, c])) for i in range(I)) * Fraction(I + 3, 2 ** 63)
            got = ref["W"][l, c]
            hi = Fraction(float(got))                            # a long double as the sum of its float64 head and tail: exact
            assert abs(hi + Fraction(float(got - LD(float(got)))) - w) <= room, (l, c)
    assert ref["n_used"] == n_used and n_used >= 3
    assert abs(Fraction(float(ref["trace"])) - t_sum / n_used) <= t_sum / n_used * Fraction(1, 2 ** 50)


# ---- the bounds: float64 in three orders of addition stays within half of them ----
def y_float64(codes, x, order):
    used, mu, inv, _ = pu.scale_of(pu.counts(codes))
    Z = (pu.DOSAGE[codes].astype(np.float64) - mu[None, :]) * inv[None, :]
    Z[codes == bedfiles.MISS] = 0
    Z[:, ~used] = 0
    I, L = codes.shape
    if order == "blas":
        return (Z @ (Z.T @ x)) / float(used.sum())
    rows = range(I) if order == "forward" else range(I - 1, -1, -1)
    cols = range(L) if order == "forward" else range(L - 1, -1, -1)
    W = np.zeros((L, x.shape[1]))
    for i in rows:
        W += Z[i][:, None] * x[i][None, :]
    Y = np.zeros((I, x.shape[1]))
    for l in cols:
        Y += Z[:, l][:, None] * W[l][None, :]
    return Y / float(used.sum())


@pytest.mark.parametrize("I,L,n_vec,wide", [(5, 65, 1, False), (65, 257, 17, True), (130, 1000, 33, True), (257, 63, 16, False)])
def test_float64_in_three_orders_lies_within_half_of_the_bounds(I, L, n_vec, wide):
    codes, _ = pu.draw_codes(I, L, 30 + I)
    x = pu.draw_x(I, n_vec, I, wide)
    ref = pu.reference(codes, x)
    for order in ("forward", "reverse", "blas"):
        assert pu.apply_excess(y_float64(codes, x, order), ref, I, L) <= 0.5, order


# ---- the algebra as a sanitized program ----
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pca_algebra")
    exe = host_driver.build(tmp, "pca_algebra", ["tests/pca_algebra_driver.cpp"], cxx=True, werror=True)

    def run(*args, arrays=(), outputs=(), stdin=""):
        """arrays: the input files' contents in argument order; outputs: the shapes of the output files; returns (stdout, arrays)"""
        ins = []
        for k, a in enumerate(arrays):
            path = str(tmp / ("in%d" % k))
            np.ascontiguousarray(a, dtype=np.float64).tofile(path)
            ins.append(path)
        outs = [str(tmp / ("out%d" % k)) for k in range(len(outputs))]
        res = host_driver.run(exe, list(args) + ins + outs, stdin=stdin, timeout=300, quiet_stderr=True)
        return res.stdout, [np.fromfile(o, dtype=np.float64).reshape(shape) for o, shape in zip(outs, outputs)]
    return run


def test_constants_start_vectors_and_block_width_are_the_headers(driver):
    shapes = [(1, 1), (64, 4096), (65, 4097), (10000, 100000), (2 ** 31 - 66, 2 ** 31 - 1)]
    out, _ = driver("constants", stdin="".join("%d %d\n" % s for s in shapes))
    lines = [tuple(int(v) for v in ln.split()) for ln in out.splitlines()]
    assert lines[0] == (pu.LSLAB, pu.VARIANTS, pu.ITILE, pu.MAX_VECTORS)
    for (I, L), row in zip(shapes, lines[1:]):
        assert row == (-(-L // pu.VARIANTS), -(-I // pu.ITILE), -(-I // pu.ITILE) * pu.ITILE, -(-L // pu.LSLAB))
    src = open(os.path.join(ROOT, "include", "multiclust_hip.h")).read()
    assert "#define MCHIP_PCA_MAX_VECTORS %d\n" % pu.MAX_VECTORS in src
    _, (X0,) = driver("start", 70, 64, outputs=[(70, 64)])
    assert np.array_equal(X0, pu.start_block(70, 64)) and (X0 >= -1).all() and (X0 < 1).all() and abs(X0.mean()) < 0.05
    cases = [(I, n_pc, n_extra) for I in (1, 5, 16, 17, 40, 1000) for n_pc in (1, 3, 6, 7, 22, 23, 48) for n_extra in (0, 10, 16) if n_pc <= I]
    out, _ = driver("width", stdin="".join("%d %d %d\n" % c for c in cases))
    assert [int(v) for v in out.split()] == [pu.block_width(*c) for c in cases]
    assert pu.block_width(1000, 3, 10) == 16 and pu.block_width(1000, 7, 10) == 32 and pu.block_width(1000, 48, 10) == 64 and pu.block_width(5, 3, 10) == 5


def test_mgs2_orthonormality_and_the_zero_column_rule(driver):
    rng = np.random.default_rng(1)
    for I, b in ((17, 16), (130, 16), (200, 64), (64, 64)):
        X = rng.standard_normal((I, b))
        X[:, 1] = X[:, 0] + 1e-6 * X[:, 1]              # nearly dependent, keeps 1e-6 of its norm: the second pass is needed, the rule does not fire
        X *= np.exp(rng.uniform(-20, 20, size=b))       # columns of very different scale
        out, (Q,) = driver("mgs2", I, b, arrays=[X], outputs=[(I, b)])
        assert int(out) == 0
        assert np.abs(Q.T @ Q - np.eye(b)).max() <= 1e-14
        assert np.allclose(Q, pu.mgs2(X), rtol=0, atol=1e-9)
    # rank-deficient: a copy, a combination, a zero column and more columns than rows
    X = rng.standard_normal((8, 12))
    X[:, 3] = X[:, 1]
    X[:, 5] = 2 * X[:, 0] - X[:, 4]
    X[:, 7] = 0
    out, (Q,) = driver("mgs2", 8, 12, arrays=[X], outputs=[(8, 12)])
    zero = [c for c in range(12) if not Q[:, c].any()]
    assert not np.isnan(Q).any() and int(out) == len(zero) and zero == [3, 5, 7, 11]      # nine independent columns in eight rows: the last has nothing left
    kept = [c for c in range(12) if c not in zero]
    assert np.abs(Q[:, kept].T @ Q[:, kept] - np.eye(len(kept))).max() <= 1e-14
    assert np.array_equal(Q == 0, pu.mgs2(X) == 0)


def spectra(rng):
    """random symmetric matrices up to 64 x 64, among them repeated and zero eigenvalues and a diagonal one"""
    for b in (1, 2, 5, 16, 33, 64):
        A = rng.standard_normal((b, b))
        yield A + A.T
        Q, _ = np.linalg.qr(rng.standard_normal((b, b)))
        lam = rng.uniform(0.5, 9, size=b)
        lam[: b // 2] = 3.0                      # repeated
        lam[b // 2: b // 2 + b // 4] = 0.0       # zero
        H = (Q * lam) @ Q.T
        yield 0.5 * (H + H.T)
    yield np.diag([3.0, 1.0, 2.0, 2.0, 0.0])
    yield np.zeros((4, 4))


def test_jacobi_against_eigh(driver):
    """Every rotation perturbs H by a few roundings of its norm and a sweep has b (b - 1) / 2 of them, but the errors of rotations
    on disjoint index pairs do not add up linearly: the accepted bound for cyclic Jacobi is p(b) eps ||H|| with a low-degree p.  The
    test allows 32 b eps ||H||_F for the eigenvalues, the orthogonality of S and the decomposition H S = S diag(theta): eigh's own
    error is of order b eps ||H||."""
    for H in spectra(np.random.default_rng(2)):
        b = H.shape[0]
        out, (theta, S) = driver("jacobi", b, arrays=[H], outputs=[(b,), (b, b)])
        room = 32 * b * 2.0 ** -53 * max(np.sqrt(np.sum(H * H)), 1e-300)
        assert int(out) <= 12 and (np.diff(theta) <= 0).all()
        assert np.abs(theta - np.linalg.eigvalsh(H)[::-1]).max() <= room
        assert np.abs(S.T @ S - np.eye(b)).max() <= 32 * b * 2.0 ** -53
        assert np.abs(H @ S - S * theta).max() <= room
        t2, S2 = pu.jacobi(H)
        assert np.allclose(theta, t2, rtol=0, atol=room) and np.abs(np.abs(np.sum(S * S2, axis=0)) - 1).max() <= 1e-6 or b > 5 or not H.any()


def test_sign_rule_and_residual_formula(driver):
    for v, want in (([1.0, -3.0, 2.0], [-1.0, 3.0, -2.0]), ([2.0, -2.0], [2.0, -2.0]), ([-2.0, 2.0, 1.0], [2.0, -2.0, -1.0]), ([0.0, 0.0], [0.0, 0.0]),
                    ([0.5, 0.25], [0.5, 0.25])):
        _, (got,) = driver("sign", len(v), arrays=[v], outputs=[(len(v),)])
        assert np.array_equal(got, want) and np.array_equal(pu.fix_sign(np.array(v)), want)      # of equals the lowest index decides
    rng = np.random.default_rng(3)
    I, b, n_pc = 40, 16, 5
    A = rng.standard_normal((I, I))
    G = A @ A.T / I
    X = pu.mgs2(rng.standard_normal((I, b)))
    Y = G @ X
    H = X.T @ Y
    theta, S = pu.jacobi(0.5 * (H + H.T))
    _, (Umat, r) = driver("residuals", I, b, n_pc, arrays=[X, Y, S, theta], outputs=[(I, b), (n_pc,)])
    want = np.sqrt(np.sum((G @ (X @ S) - theta * (X @ S)) ** 2, axis=0))[:n_pc] / theta[0]      # G U, computed: the header takes it as Y S
    assert np.allclose(Umat, X @ S, rtol=0, atol=1e-14) and np.allclose(r, want, rtol=1e-10, atol=1e-15) and (r > 1e-3).all()


@pytest.mark.parametrize("k", range(len(pu.PLANTED)))
def test_whole_iteration_on_a_dense_matrix_against_eigh(driver, k):
    case = pu.planted_case(k)
    I, L, n_pc = case["I"], case["L"], case["n_pc"]
    G, _, trace = pu.gram(case["codes"])
    assert abs(float(np.trace(G) - trace)) <= 1e-12 * float(trace)      # the trace from the counts is the trace of the matrix
    out, (val, vec, res) = driver("iterate", I, n_pc, 10, case["cap"], repr(1e-9), arrays=[G.astype(np.float64)], outputs=[(n_pc,), (I, n_pc), (n_pc,)])
    r = dict(eigenvalues=val, eigenvectors=vec, residuals=res, n_iter=int(out))
    assert r["n_iter"] <= case["cap"] and res.max() <= 1e-9
    pu.check_pairs(r, G.astype(np.float64).astype(LD), I, L, 1e-9)
    mine = pu.iterate(lambda X: G.astype(np.float64) @ X, I, n_pc, 10, case["cap"], 1e-9)
    assert mine["n_iter"] == r["n_iter"] and np.allclose(mine["eigenvalues"], val, rtol=1e-12) and np.allclose(mine["eigenvectors"], vec, atol=1e-7)
    lam = np.linalg.eigvalsh(G.astype(np.float64))[::-1]
    assert lam[n_pc - 1] > 4.5 and lam[n_pc] < 1.7                    # planted structure above the bulk


def test_b_at_least_I_is_exact_after_two_iterations_and_one_iteration_is_no_error(driver):
    codes, _ = pu.draw_codes(17, 65, 5)
    G = pu.gram(codes)[0]
    G64 = G.astype(np.float64)
    out, (val, vec, res) = driver("iterate", 17, 3, 10, 50, repr(1e-9), arrays=[G64], outputs=[(3,), (17, 3), (3,)])
    assert int(out) == 2 and res.max() <= 1e-13
    pu.check_pairs(dict(eigenvalues=val, eigenvectors=vec, residuals=res), G64.astype(LD), 17, 65, 1e-9, planted_fixture=False)
    case = pu.planted_case(1)
    G64 = pu.gram(case["codes"])[0].astype(np.float64)
    out, (val, vec, res) = driver("iterate", case["I"], 3, 10, 1, repr(1e-9), arrays=[G64], outputs=[(3,), (case["I"], 3), (3,)])
    assert int(out) == 1 and (res > 1e-9).all() and not np.isnan(vec).any()


def test_rank_deficient_matrices_give_no_nan(driver):
    for I, L, n_pc in ((5, 40, 3), (17, 3, 2)):
        codes, _ = pu.draw_codes(I, L, 70 + I, plant=False)
        G64 = pu.gram(codes)[0].astype(np.float64)
        out, (val, vec, res) = driver("iterate", I, n_pc, 10, 50, repr(1e-9), arrays=[G64], outputs=[(n_pc,), (I, n_pc), (n_pc,)])
        assert (val >= -1e-14).all()
        pu.check_pairs(dict(eigenvalues=val, eigenvectors=vec, residuals=res), G64.astype(LD), I, L, 1e-9, planted_fixture=False)


# ---- mutants: each has to be told from the definition by the checks the GPU tests apply, on cases they use ----
def mutant_y(codes, x, kind):
    cnt = pu.counts(codes)
    c = codes.copy()
    if kind == "missing_is_dosage_0":
        Z, used, mu, inv, _ = pu.z_matrix(codes)
        Z = (pu.DOSAGE[codes].astype(LD) - mu.astype(LD)[None, :]) * inv.astype(LD)[None, :]      # the missing call keeps (0 - mu) inv
        Z[:, ~used] = 0
        return (Z @ (Z.T @ x.astype(LD))) / LD(used.sum())
    Z, used, mu, inv, _ = pu.z_matrix(c)
    if kind == "unused_counted":
        return (Z @ (Z.T @ x.astype(LD))) / LD(codes.shape[1])
    if kind == "not_divided":
        return Z @ (Z.T @ x.astype(LD))
    if kind == "inv_without_half":
        inv2 = np.zeros_like(inv)
        ok = used & (mu < 1)
        inv2[ok] = 1.0 / np.sqrt(mu[ok] * (1.0 - mu[ok]))
        Z = (pu.DOSAGE[codes].astype(LD) - mu.astype(LD)[None, :]) * inv2.astype(LD)[None, :]
        Z[codes == bedfiles.MISS] = 0
        Z[:, ~ok] = 0
        return (Z @ (Z.T @ x.astype(LD))) / LD(used.sum())
    assert kind == "none" and cnt is not None
    return (Z @ (Z.T @ x.astype(LD))) / LD(used.sum())


@pytest.mark.parametrize("kind", ["missing_is_dosage_0", "unused_counted", "not_divided", "inv_without_half"])
def test_mutants_of_the_matrix_are_caught(kind):
    for I, L in ((5, 65), (65, 63), (17, pu.LSLAB + 1)):
        codes, where = pu.draw_codes(I, L, 100 + I)
        assert {"all_missing", "monomorphic", "all_het", "missing_individual"} <= set(where)
        x = pu.draw_x(I, 3, I)
        ref = pu.reference(codes, x)
        assert pu.apply_excess(mutant_y(codes, x, "none"), ref, I, L) == 0
        assert pu.apply_excess(mutant_y(codes, x, kind), ref, I, L) > 1e6, (kind, I, L)


def test_mutants_of_the_iteration_are_caught():
    case = pu.planted_case(0)
    I, L, n_pc = case["I"], case["L"], case["n_pc"]
    G = pu.gram(case["codes"])[0]
    G64 = G.astype(np.float64)
    pu.check_pairs(pu.iterate(lambda X: G64 @ X, I, n_pc, 10, case["cap"], 1e-9), G, I, L, 1e-9)
    # the sign rule dropped: on some fixture a vector comes out with its largest component negative
    flipped = 0
    for k in range(len(pu.PLANTED)):
        c = pu.planted_case(k)
        Gk = pu.gram(c["codes"])[0].astype(np.float64)
        r = pu.iterate(lambda X: Gk @ X, c["I"], c["n_pc"], 10, c["cap"], 1e-9, sign_rule=False)
        flipped += sum(r["eigenvectors"][int(np.argmax(np.abs(r["eigenvectors"][:, j]))), j] < 0 for j in range(c["n_pc"]))
    assert flipped > 0
    r = pu.iterate(lambda X: G64 @ X, I, n_pc, 10, case["cap"], 1e-9, sign_rule=False)
    if any(r["eigenvectors"][int(np.argmax(np.abs(r["eigenvectors"][:, j]))), j] < 0 for j in range(n_pc)):
        with pytest.raises(AssertionError):
            pu.check_pairs(r, G, I, L, 1e-9)
    # the residual not divided by theta_1: it stops later than the cap of a planted fixture allows or reports a residual off by theta_1
    r = pu.iterate(lambda X: G64 @ X, I, n_pc, 10, case["cap"], 1e-9, divide_residual=False)
    with pytest.raises(AssertionError):
        pu.check_pairs(r, G, I, L, 1e-9)
    # a multiply that leaves out the division by L' scales every eigenvalue: |theta - lambda| is far beyond the residual
    n_used = pu.gram(case["codes"])[1]
    r = pu.iterate(lambda X: n_used * (G64 @ X), I, n_pc, 10, case["cap"], 1e-9)
    with pytest.raises(AssertionError):
        pu.check_pairs(r, G, I, L, 1e-9)
