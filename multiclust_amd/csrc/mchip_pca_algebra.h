/*
 * mchip_pca_algebra.h -- the host side of mchip_bed_pca (mchip_pca.hip): block subspace iteration with a Rayleigh-Ritz step every
 * iteration on a symmetric positive semi-definite matrix G that is known only through Y = G X.  Plain C++, no HIP types:
 * tests/pca_algebra_driver.cpp compiles it alone (as mchip_feature_geometry.h is compiled alone) and tests/pca_util.py restates it.
 *
 * Matrices are row-major: X, Y, U [I][b], H and S [b][b].
 *
 * Block width.  b = min(I, n_pc + n_extra rounded up to a multiple of 16, at most 64): the device pads the columns to a multiple
 * of 16 anyway, so the columns up to it are real start vectors that cost nothing there and speed convergence.
 * Start vectors.  X0[i][c] = pca_start_value(i, c), a function of (i, c) alone: with z = (uint64)i * 64 + c,
 *     z += 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^= z >> 31
 * (the output function of splitmix64, arithmetic modulo 2^64) and the value (double)(z >> 11) * 2^-52 - 1, in [-1, 1).  No seed
 * enters: the components do not change with the seed of a fit.
 * Orthonormalisation (pca_mgs2).  Modified Gram-Schmidt applied twice, in column order: column c has the columns before it
 * projected out one after the other, then once more, and is scaled to norm 1.  A column whose norm after the projections is below
 * 1e-10 of its norm before them (or was 0 before) is set to zero and stays zero: the rank-deficient case, b >= rank.  No division
 * by such a norm takes place, so no NaN arises.
 * Each iteration (pca_subspace_iteration).  Y = G X by the caller's multiply; H = X^T Y, symmetrised as (H + H^T) / 2; cyclic
 * Jacobi on H (pca_jacobi) gives theta in descending order and S; U = X S; the residual of component c < n_pc is
 * r_c = || Y S_c - theta_c U_c ||_2 / theta_1 (G U is never recomputed: it is Y S; theta_1 <= 0 leaves the norm undivided).  Stop
 * when max r_c <= tol or the iteration count reaches max_iter; else X = pca_mgs2(Y).
 * Output.  The first n_pc pairs (theta_c, U_c) and their residuals; each vector scaled to norm 1 (a zero vector stays zero) and
 * signed so that its component of largest magnitude is positive, the lowest index among equals (pca_fix_sign).  Not converging is
 * no error: the residuals say which components are still loose.
 * Convergence.  Component c converges at the rate lambda_{b+1} / lambda_c per iteration: components inside the noise bulk of the
 * spectrum converge slowly and mean nothing.  Block Krylov with thick restart is the known improvement and is not done here.
 */
#ifndef MCHIP_PCA_ALGEBRA_H
#define MCHIP_PCA_ALGEBRA_H

#include <math.h>
#include <stdint.h>
#include <vector>

constexpr int PCA_MAX_BLOCK = 64;		/* = MCHIP_PCA_MAX_VECTORS (include/multiclust_hip.h; mchip_pca.hip asserts it) */
constexpr double PCA_ZERO_COLUMN = 1e-10;	/* a column that keeps less than this of its norm through the projections is zero */
constexpr double PCA_JACOBI_TOL = 1e-15;	/* sweeps go on while an off-diagonal element exceeds this times ||H||_F */
constexpr int PCA_JACOBI_MAX_SWEEPS = 64;

static inline double pca_start_value(int i, int c)
{
	uint64_t z = (uint64_t)i * 64u + (uint64_t)c;
	z += 0x9E3779B97F4A7C15ull;
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	z ^= z >> 31;
	return (double)(z >> 11) * (1.0 / 4503599627370496.0) - 1.0;
}

static inline int pca_block_width(int I, int n_pc, int n_extra)
{
	int b = (n_pc + n_extra + 15) / 16 * 16;
	if (b > PCA_MAX_BLOCK) b = PCA_MAX_BLOCK;
	return b < I ? b : I;
}

/* the columns of X [I][b] orthonormalised in place; returns the number of columns set to zero.  The work is done on a transposed
 * copy, a column contiguous: the same operations in the same order, without a stride of b doubles in every inner loop. */
static inline int pca_mgs2(double *X, int I, int b)
{
	std::vector<double> T((size_t)I * b);
	for (int i = 0; i < I; i++)
		for (int c = 0; c < b; c++) T[(size_t)c * I + i] = X[(size_t)i * b + c];
	int n_zero = 0;
	for (int c = 0; c < b; c++) {
		double *v = T.data() + (size_t)c * I;
		double before = 0.0;
		for (int i = 0; i < I; i++) before += v[i] * v[i];
		before = sqrt(before);
		for (int pass = 0; pass < 2; pass++)
			for (int k = 0; k < c; k++) {
				const double *u = T.data() + (size_t)k * I;
				double dot = 0.0;
				for (int i = 0; i < I; i++) dot += u[i] * v[i];
				for (int i = 0; i < I; i++) v[i] -= dot * u[i];
			}
		double after = 0.0;
		for (int i = 0; i < I; i++) after += v[i] * v[i];
		after = sqrt(after);
		if (!(before > 0.0) || !(after >= PCA_ZERO_COLUMN * before)) {
			for (int i = 0; i < I; i++) v[i] = 0.0;
			n_zero++;
			continue;
		}
		for (int i = 0; i < I; i++) v[i] /= after;
	}
	for (int i = 0; i < I; i++)
		for (int c = 0; c < b; c++) X[(size_t)i * b + c] = T[(size_t)c * I + i];
	return n_zero;
}

/* cyclic Jacobi on the symmetric H [b][b] (destroyed): theta[b] descending, S [b][b] with the eigenvector of theta[c] in column c;
 * of equal eigenvalues the one found at the lower index comes first.  Returns the number of sweeps that rotated. */
static inline int pca_jacobi(double *H, int b, double *theta, double *S)
{
	for (int p = 0; p < b; p++)
		for (int q = 0; q < b; q++) S[(size_t)p * b + q] = p == q ? 1.0 : 0.0;
	double fro = 0.0;
	for (int x = 0; x < b * b; x++) fro += H[x] * H[x];
	const double thr = PCA_JACOBI_TOL * sqrt(fro);
	int sweeps = 0;
	for (; sweeps < PCA_JACOBI_MAX_SWEEPS; sweeps++) {
		int rotated = 0;
		for (int p = 0; p < b - 1; p++)
			for (int q = p + 1; q < b; q++) {
				const double hpq = H[(size_t)p * b + q];
				if (!(fabs(hpq) > thr)) continue;
				rotated = 1;
				const double tau = (H[(size_t)q * b + q] - H[(size_t)p * b + p]) / (2.0 * hpq);
				const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
				const double cs = 1.0 / sqrt(1.0 + t * t), sn = t * cs;
				for (int k = 0; k < b; k++) {	/* columns p and q */
					const double hkp = H[(size_t)k * b + p], hkq = H[(size_t)k * b + q];
					H[(size_t)k * b + p] = cs * hkp - sn * hkq;
					H[(size_t)k * b + q] = sn * hkp + cs * hkq;
				}
				for (int k = 0; k < b; k++) {	/* rows p and q */
					const double hpk = H[(size_t)p * b + k], hqk = H[(size_t)q * b + k];
					H[(size_t)p * b + k] = cs * hpk - sn * hqk;
					H[(size_t)q * b + k] = sn * hpk + cs * hqk;
				}
				H[(size_t)p * b + q] = H[(size_t)q * b + p] = 0.0;
				for (int k = 0; k < b; k++) {
					const double skp = S[(size_t)k * b + p], skq = S[(size_t)k * b + q];
					S[(size_t)k * b + p] = cs * skp - sn * skq;
					S[(size_t)k * b + q] = sn * skp + cs * skq;
				}
			}
		if (!rotated) break;
	}
	/* descending, stable: insertion sort of the column order */
	std::vector<int> order((size_t)b);
	for (int c = 0; c < b; c++) {
		int at = c;
		while (at > 0 && H[(size_t)order[at - 1] * b + order[at - 1]] < H[(size_t)c * b + c]) { order[at] = order[at - 1]; at--; }
		order[at] = c;
	}
	std::vector<double> sorted((size_t)b * b);
	for (int c = 0; c < b; c++) {
		theta[c] = H[(size_t)order[c] * b + order[c]];
		for (int k = 0; k < b; k++) sorted[(size_t)k * b + c] = S[(size_t)k * b + order[c]];
	}
	for (int x = 0; x < b * b; x++) S[x] = sorted[x];
	return sweeps;
}

/* v[0], v[stride], ... (n of them) negated when the component of largest magnitude, the lowest index among equals, is negative */
static inline void pca_fix_sign(double *v, int n, int stride)
{
	int at = 0;
	for (int i = 1; i < n; i++)
		if (fabs(v[(size_t)i * stride]) > fabs(v[(size_t)at * stride])) at = i;
	if (v[(size_t)at * stride] < 0.0)
		for (int i = 0; i < n; i++) v[(size_t)i * stride] = -v[(size_t)i * stride];
}

/* r[c] for c < n_pc of the Ritz pairs (theta, U = X S) given Y = G X: || Y S_c - theta_c U_c || / theta_1; U [I][b] is filled */
static inline void pca_ritz_residuals(const double *X, const double *Y, const double *S, const double *theta, int I, int b, int n_pc,
				      double *U, double *r)
{
	std::vector<double> sq((size_t)n_pc, 0.0), gu((size_t)b);
	for (int i = 0; i < I; i++) {
		const double *x = X + (size_t)i * b, *y = Y + (size_t)i * b;
		double *u = U + (size_t)i * b;
		for (int c = 0; c < b; c++) u[c] = gu[(size_t)c] = 0.0;
		for (int k = 0; k < b; k++)	/* (every sum over k ascending, the rows of S read along) */
			for (int c = 0; c < b; c++) { u[c] += x[k] * S[(size_t)k * b + c]; gu[(size_t)c] += y[k] * S[(size_t)k * b + c]; }
		for (int c = 0; c < n_pc; c++) { const double d = gu[(size_t)c] - theta[c] * u[c]; sq[(size_t)c] += d * d; }
	}
	for (int c = 0; c < n_pc; c++) r[c] = theta[0] > 0.0 ? sqrt(sq[(size_t)c]) / theta[0] : sqrt(sq[(size_t)c]);
}

/* The whole iteration.  multiply(X, Y) computes Y = G X for X, Y [I][b] and returns 0 or a status, which ends the iteration and is
 * returned.  eigenvalues [n_pc], eigenvectors [I][n_pc], residuals [n_pc] and *n_iter are written on success only. */
template <typename Multiply>
static inline int pca_subspace_iteration(int I, int b, int n_pc, int max_iter, double tol, Multiply &&multiply, double *eigenvalues,
					 double *eigenvectors, double *residuals, int *n_iter)
{
	const size_t n = (size_t)I * b;
	std::vector<double> X(n), Y(n), U(n), H((size_t)b * b), S((size_t)b * b), theta((size_t)b), r((size_t)n_pc);
	for (int i = 0; i < I; i++)
		for (int c = 0; c < b; c++) X[(size_t)i * b + c] = pca_start_value(i, c);
	pca_mgs2(X.data(), I, b);
	int it = 0;
	for (;;) {
		const int rc = multiply((const double *)X.data(), Y.data());
		if (rc) return rc;
		it++;
		for (size_t x = 0; x < (size_t)b * b; x++) H[x] = 0.0;
		for (int i = 0; i < I; i++)	/* (every element's sum over i ascending, the rows of X and Y read along) */
			for (int p = 0; p < b; p++)
				for (int q = 0; q < b; q++) H[(size_t)p * b + q] += X[(size_t)i * b + p] * Y[(size_t)i * b + q];
		for (int p = 0; p < b; p++)
			for (int q = p + 1; q < b; q++) H[(size_t)p * b + q] = H[(size_t)q * b + p] = 0.5 * (H[(size_t)p * b + q] + H[(size_t)q * b + p]);
		pca_jacobi(H.data(), b, theta.data(), S.data());
		pca_ritz_residuals(X.data(), Y.data(), S.data(), theta.data(), I, b, n_pc, U.data(), r.data());
		double worst = 0.0;
		for (int c = 0; c < n_pc; c++)
			if (!(r[(size_t)c] <= worst)) worst = r[(size_t)c];
		if (worst <= tol || it >= max_iter) break;
		X = Y;
		pca_mgs2(X.data(), I, b);
	}
	for (int c = 0; c < n_pc; c++) {
		double norm = 0.0;
		for (int i = 0; i < I; i++) norm += U[(size_t)i * b + c] * U[(size_t)i * b + c];
		norm = sqrt(norm);
		for (int i = 0; i < I; i++) eigenvectors[(size_t)i * n_pc + c] = norm > 0.0 ? U[(size_t)i * b + c] / norm : 0.0;
		pca_fix_sign(eigenvectors + c, I, n_pc);
		eigenvalues[c] = theta[(size_t)c];
		residuals[c] = r[(size_t)c];
	}
	*n_iter = it;
	return 0;
}

#endif
