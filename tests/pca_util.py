"""--pca for the tests (TEST INFRASTRUCTURE): the matrix of mchip_bed_pca (include/multiclust_hip.h) and the iteration of
multiclust_amd/csrc/mchip_pca_algebra.h restated, and the fixtures.

reference(): the counts are Python / numpy integers.  mu and inv are what the definition says they are -- `(double)s / (double)n` and
`1 / sqrt(mu * (1 - 0.5 * mu))`, float64 operations in that order -- because a variant near fixation (s = 2 n - 1) turns the one
rounding of mu into a relative error of about n roundings in 1 - 0.5 mu and in 2 - mu: a reference that took mu from exact
rationals would differ from every conforming implementation by more than the roundings the bounds count.  Everything from the table
on -- Z, W, Y, G, the trace -- is numpy.longdouble (64-bit mantissa here), and test_pca_cpu.py holds the counts, mu, t_l and the sums
to exact rationals.

The bounds (gamma_* below) count roundings, each at most 2^-53 relative, and hold for any order of addition:
  y: (I - 1) + (L - 1) additions, one rounding per product, at most eight in each of the two z factors, one division -> I + L + 20;
  w: (I - 1) additions, one per product, eight in the z factor -> I + 10."""
import hashlib

import numpy as np

import bedfiles

LD = np.longdouble
LSLAB, VARIANTS, ITILE, MAX_VECTORS = 4096, 64, 64, 64      # PCA_LSLAB, PCA_VARIANTS, PCA_ITILE, MCHIP_PCA_MAX_VECTORS (test_pca_cpu.py holds them to the headers)
ZERO_COLUMN, JACOBI_TOL, JACOBI_MAX_SWEEPS = 1e-10, 1e-15, 64
U = 2.0 ** -53
DOSAGE = np.array([0, 0, 1, 2])


def gamma_y(I, L):
    return (I + L + 20) * U


def gamma_w(I):
    return (I + 10) * U


def counts(codes):
    """[L][4] integers: individuals with code c at variant l"""
    return np.stack([(codes == c).sum(axis=0) for c in range(4)], axis=1).astype(np.int64)


def scale_of(cnt):
    """(used [L] bool, mu [L], inv [L], t [L]) as the definition states them in float64; 0 on an unused variant"""
    n0, n2, n3 = (cnt[:, c].astype(np.int64) for c in (0, 2, 3))
    n, s = n0 + n2 + n3, n2 + 2 * n3
    used = (s > 0) & (s < 2 * n)
    mu, inv, t = np.zeros(len(cnt)), np.zeros(len(cnt)), np.zeros(len(cnt))
    m = s[used].astype(np.float64) / n[used].astype(np.float64)
    v = 1.0 / np.sqrt(m * (1.0 - 0.5 * m))
    mu[used], inv[used] = m, v
    t[used] = (n0[used] * (m * m) + n2[used] * ((1.0 - m) * (1.0 - m)) + n3[used] * ((2.0 - m) * (2.0 - m))) * (v * v)
    return used, mu, inv, t


def z_matrix(codes):
    """(Z [I][L] long double, used, mu, inv, t): z = (x - mu) inv for a typed call, 0 for a missing one and on an unused variant"""
    used, mu, inv, t = scale_of(counts(codes))
    Z = (DOSAGE[codes].astype(LD) - mu.astype(LD)[None, :]) * inv.astype(LD)[None, :]
    Z[codes == bedfiles.MISS] = 0
    Z[:, ~used] = 0
    return Z, used, mu, inv, t


def reference(codes, x):
    """everything mchip_bed_pca_apply returns, in long double, and the sums of absolute values its bounds are stated in"""
    Z, used, mu, inv, t = z_matrix(codes)
    n_used = int(used.sum())
    X = np.asarray(x).astype(LD)
    W = Z.T @ X
    absW = np.abs(Z).T @ np.abs(X)
    out = dict(Z=Z, used=used, n_used=n_used, mu=mu, inv=inv, t=t, W=W, absW=absW)
    if n_used:
        out.update(Y=(Z @ W) / LD(n_used), absY=(np.abs(Z) @ absW) / LD(n_used), trace=t.astype(LD).sum() / LD(n_used))
    return out


def apply_excess(y, ref, I, L, w=None):
    """the largest |error| of y (and of w) over its bound, each in units of the bound: <= 1 passes.  Where the bound is 0 the value
    must be exactly the reference's (0 over 0 counts as 0)."""
    def ratio(got, want, room):
        err = np.abs(np.asarray(got).astype(LD) - want)
        out = np.zeros(err.shape, dtype=LD)
        pos = room > 0
        out[pos] = err[pos] / room[pos]
        out[~pos & (err > 0)] = np.inf
        return float(out.max()) if out.size else 0.0
    ry = ratio(y, ref["Y"], LD(gamma_y(I, L)) * ref["absY"])
    return ry if w is None else max(ry, ratio(w, ref["W"], LD(gamma_w(I)) * ref["absW"]))


def ulps(a, b):
    """|a - b| in units in the last place of b (float64 arrays of one sign pattern)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.spacing(np.abs(b))


def gram(codes):
    """(G = Z Z^T / L' [I][I] long double, L', trace)"""
    Z, used, _, _, t = z_matrix(codes)
    n_used = int(used.sum())
    return (Z @ Z.T) / LD(n_used), n_used, t.astype(LD).sum() / LD(n_used)


# ---- the iteration (multiclust_amd/csrc/mchip_pca_algebra.h) in float64 ----
M64 = (1 << 64) - 1


def start_value(i, c):
    z = (i * 64 + c) & M64
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return float(z >> 11) * 2.0 ** -52 - 1.0


def start_block(I, b):
    return np.array([[start_value(i, c) for c in range(b)] for i in range(I)])


def block_width(I, n_pc, n_extra):
    return min(I, min(64, -(-(n_pc + n_extra) // 16) * 16))


def mgs2(X):
    """modified Gram-Schmidt twice in column order; a column that keeps less than 1e-10 of its norm is zero"""
    X = np.array(X, dtype=np.float64)
    for c in range(X.shape[1]):
        before = np.sqrt(np.sum(X[:, c] * X[:, c]))
        for _ in range(2):
            for k in range(c):
                X[:, c] -= np.sum(X[:, k] * X[:, c]) * X[:, k]
        after = np.sqrt(np.sum(X[:, c] * X[:, c]))
        if not before > 0 or not after >= ZERO_COLUMN * before:
            X[:, c] = 0
        else:
            X[:, c] /= after
    return X


def jacobi(H):
    """cyclic Jacobi: (theta descending, S with the eigenvector of theta[c] in column c)"""
    H = np.array(H, dtype=np.float64)
    b = H.shape[0]
    S = np.eye(b)
    thr = JACOBI_TOL * np.sqrt(np.sum(H * H))
    for _ in range(JACOBI_MAX_SWEEPS):
        rotated = False
        for p in range(b - 1):
            for q in range(p + 1, b):
                hpq = H[p, q]
                if not abs(hpq) > thr:
                    continue
                rotated = True
                tau = (H[q, q] - H[p, p]) / (2.0 * hpq)
                t = (1.0 if tau >= 0 else -1.0) / (abs(tau) + np.sqrt(1.0 + tau * tau))
                cs = 1.0 / np.sqrt(1.0 + t * t)
                sn = t * cs
                hp, hq = H[:, p].copy(), H[:, q].copy()
                H[:, p], H[:, q] = cs * hp - sn * hq, sn * hp + cs * hq
                hp, hq = H[p, :].copy(), H[q, :].copy()
                H[p, :], H[q, :] = cs * hp - sn * hq, sn * hp + cs * hq
                H[p, q] = H[q, p] = 0.0
                sp, sq = S[:, p].copy(), S[:, q].copy()
                S[:, p], S[:, q] = cs * sp - sn * sq, sn * sp + cs * sq
        if not rotated:
            break
    order = np.argsort(-np.diag(H), kind="stable")
    return np.diag(H)[order].copy(), S[:, order].copy()


def fix_sign(v):
    at = int(np.argmax(np.abs(v)))      # the first of equals
    return -v if v[at] < 0 else v


def iterate(multiply, I, n_pc, n_extra, max_iter, tol, divide_residual=True, sign_rule=True):
    """the whole iteration: dict(eigenvalues, eigenvectors [I][n_pc], residuals, n_iter).  The two switches are the mutants of
    test_pca_cpu.py."""
    b = block_width(I, n_pc, n_extra)
    X = mgs2(start_block(I, b))
    it = 0
    while True:
        Y = multiply(X)
        it += 1
        H = X.T @ Y
        H = 0.5 * (H + H.T)
        theta, S = jacobi(H)
        Umat, GU = X @ S, Y @ S
        r = np.sqrt(np.sum((GU[:, :n_pc] - theta[:n_pc] * Umat[:, :n_pc]) ** 2, axis=0))
        if divide_residual and theta[0] > 0:
            r = r / theta[0]
        if r.max() <= tol or it >= max_iter:
            break
        X = mgs2(Y)
    vec = np.zeros((I, n_pc))
    for c in range(n_pc):
        norm = np.sqrt(np.sum(Umat[:, c] ** 2))
        v = Umat[:, c] / norm if norm > 0 else np.zeros(I)
        vec[:, c] = fix_sign(v) if sign_rule else v
    return dict(eigenvalues=theta[:n_pc].copy(), eigenvectors=vec, residuals=r, n_iter=it)


def check_pairs(r, G, I, L, tol, planted_fixture=True):
    """what the tests ask of eigenpairs r (the dict of iterate() / Context.bed_pca) of the long-double matrix G: for every component
    the test's own residual || G u - theta u || / theta_1 <= tol + 100 (I + L) 2^-53; unit norm to 1e-14; the sign rule; and on the
    planted fixtures, whose gaps make the c-th eigenvalue the one next to theta_c: |theta_c - lambda_c| <= residual theta_1 (a
    symmetric matrix has an eigenvalue that close to theta), sin of the angle to eigh's vector <= residual theta_1 / gap_c
    (Davis-Kahan), and the reported residual within a factor 2 of the test's own.  lambda_c is eigh's, refined by one Rayleigh
    quotient in long double.  Returns the test's own residuals."""
    theta, vec = np.asarray(r["eigenvalues"]), np.asarray(r["eigenvectors"])
    lam, V = np.linalg.eigh(G.astype(np.float64))
    lam, V = lam[::-1], V[:, ::-1].astype(LD)
    lam = np.array([(V[:, j] @ (G @ V[:, j])) / (V[:, j] @ V[:, j]) for j in range(len(lam))], dtype=LD)
    room = tol + 100 * (I + L) * U
    own = []
    assert not np.isnan(theta).any() and not np.isnan(vec).any() and not np.isnan(r["residuals"]).any()
    for c in range(len(theta)):
        u = vec[:, c].astype(LD)
        res = float(np.sqrt(np.sum((G @ u - LD(theta[c]) * u) ** 2)) / LD(theta[0]))
        own.append(res)
        assert res <= room, (c, res, room)
        norm = float(np.sqrt(u @ u))
        if planted_fixture or norm > 0:
            assert abs(norm - 1.0) <= 1e-14, (c, norm)
            assert vec[int(np.argmax(np.abs(vec[:, c]))), c] > 0, c
        if planted_fixture:
            assert abs(LD(theta[c]) - lam[c]) <= LD(res) * LD(theta[0]), (c, theta[c], lam[c], res)
            gap = float(np.min(np.abs(np.delete(lam, c) - LD(theta[c]))))
            v = V[:, c] / np.sqrt(V[:, c] @ V[:, c])
            sin = float(np.sqrt(np.sum((u - v * (v @ u)) ** 2)))
            assert sin <= res * theta[0] / gap, (c, sin, res, gap)
            assert 0.5 * res <= r["residuals"][c] <= 2 * res, (c, r["residuals"][c], res)
    return own


# ---- fixtures ----
def planted(I, L, n_pops, seed, fst=0.1, missing=0.05):
    """(codes [I][L], population of every individual): ancestral frequencies uniform in (0.1, 0.9), the populations' drawn from the
    Balding-Nichols beta at F_ST = fst, individuals assigned round-robin, `missing` of the calls missing"""
    rng = np.random.default_rng(seed)
    anc = rng.uniform(0.1, 0.9, size=L)
    freq = rng.beta(anc * (1 - fst) / fst, (1 - anc) * (1 - fst) / fst, size=(n_pops, L))
    pop = np.arange(I) % n_pops
    dosage = rng.binomial(2, freq[pop])
    codes = np.array([bedfiles.HOM1, bedfiles.HET, bedfiles.HOM2], dtype=np.uint8)[dosage]
    codes[rng.random((I, L)) < missing] = bedfiles.MISS
    return codes, pop


# I, L, populations, n_pc, and the iterations to residual 1e-9 with 16 vectors that the fixtures were made with; the tests allow three
# times as many
PLANTED = [(65, 4097, 3, 2, 14), (130, 1000, 4, 3, 14), (200, 8193, 5, 4, 12)]


def planted_case(k):
    I, L, n_pops, n_pc, iters = PLANTED[k]
    codes, pop = planted(I, L, n_pops, seed=1000 + k)
    return dict(I=I, L=L, n_pc=n_pc, cap=3 * iters, codes=codes, pop=pop)


def draw_codes(I, L, seed, missing=0.1, plant=True):
    """[I][L] codes with, where the shape has room, an all-missing variant, a monomorphic one, one at which everyone is heterozygous
    (mu = 1) and a fully missing individual"""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.05, 0.95, size=L)
    a = (rng.random((I, L)) < f) * 1 + (rng.random((I, L)) < f) * 1
    codes = np.array([bedfiles.HOM1, bedfiles.HET, bedfiles.HOM2], dtype=np.uint8)[a]
    codes[rng.random((I, L)) < missing] = bedfiles.MISS
    where = {}
    if plant and L >= 8:
        ls = rng.permutation(L)[:3]
        for l, c, name in zip(ls, (bedfiles.MISS, bedfiles.HOM2, bedfiles.HET), ("all_missing", "monomorphic", "all_het")):
            codes[:, l] = c
            where[name] = int(l)
    if plant and I >= 5:
        where["missing_individual"] = int(rng.integers(I))
        codes[where["missing_individual"], :] = bedfiles.MISS
        if "all_het" in where:
            codes[:, where["all_het"]] = bedfiles.HET      # (the missing individual included: mu is exactly 1 and every z is 0)
    return codes, where


def repack(codes, seed, extra):
    """packed records [L][ceil(I/4) + extra] with random bits wherever no individual is carried"""
    I, L = codes.shape
    rng = np.random.default_rng(seed + 12345)
    rb = (I + 3) // 4
    full = rng.integers(0, 4, size=(L, rb * 4), dtype=np.uint8)
    full[:, :I] = codes.T
    q = full.reshape(L, rb, 4)
    bed = (q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).astype(np.uint8)
    return np.ascontiguousarray(np.concatenate([bed, rng.integers(0, 256, size=(L, extra), dtype=np.uint8)], axis=1))


def draw_x(I, n_vec, seed, wide=False):
    """x [I][n_vec] of mixed sign; wide: magnitudes 1e-150 and 1e150 among them, a column each where there is room"""
    rng = np.random.default_rng(seed + 999)
    x = rng.standard_normal((I, n_vec))
    if wide:
        x[:, 0] *= 1e150
        if n_vec > 1:
            x[:, 1] *= 1e-150
        if n_vec > 2:
            x[:, 2] *= np.where(rng.random(I) < 0.5, 1e150, 1e-150)
    return x


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# the cases of the fresh-process tests: apply at several slabs and tiles with 33 vectors (48 columns on the device), and the whole
# iteration on the smallest planted fixture
FRESH = dict(I=130, L=2 * LSLAB + 1, n_vec=33, seed=4242)


def fresh_case():
    codes, _ = draw_codes(FRESH["I"], FRESH["L"], FRESH["seed"])
    return repack(codes, FRESH["seed"], 3), draw_x(FRESH["I"], FRESH["n_vec"], FRESH["seed"])


def fresh_digests(ctx):
    """(digest of mchip_bed_pca_apply's outputs on fresh_case(), digest of mchip_bed_pca's on planted_case(0))"""
    bed, x = fresh_case()
    y, w, sc, n_used, trace = ctx.bed_pca_apply(FRESH["I"], bed, x)
    case = planted_case(0)
    r = ctx.bed_pca(case["I"], bedfiles.pack(case["codes"]), case["n_pc"], n_extra=10, max_iter=case["cap"], tol=1e-9)
    return (digest(y, w, sc, np.int64(n_used), np.float64(trace)),
            digest(r["eigenvalues"], r["eigenvectors"], r["residuals"], np.float64(r["trace"]), np.int64(r["n_used"]), np.int64(r["n_iter"])))


if __name__ == "__main__":
    # pca_util.py: the two digests of the device's results in this process, under whatever knobs its environment sets
    from multiclust_amd import hip
    ctx = hip.Context(0)
    print("%s\n%s" % fresh_digests(ctx))
    ctx.close()
