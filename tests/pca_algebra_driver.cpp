/* multiclust_amd/csrc/mchip_pca_algebra.h and the PCA constants of mchip_feature_geometry.h as a program of their own, for
 * tests/test_pca_cpu.py.  Arrays travel as files of raw doubles, row-major.
 *   constants                                   -> "PCA_LSLAB PCA_VARIANTS PCA_ITILE PCA_MAX_BLOCK" and one line per "I L" on stdin:
 *                                                  n_vgroups n_itiles Ipad n_slabs
 *   start I b out                               -> X0 [I][b] before orthonormalisation
 *   width                                       -> one line per "I n_pc n_extra" on stdin: the block width
 *   mgs2 I b in out                             -> the columns of in [I][b] orthonormalised; stdout: the number of zero columns
 *   jacobi b in theta S                         -> theta [b], S [b][b] of the symmetric in [b][b]; stdout: the sweeps that rotated
 *   sign n in out                               -> the vector in [n] under the sign rule
 *   residuals I b n_pc X Y S theta U r          -> U [I][b] and r [n_pc] of pca_ritz_residuals
 *   iterate I n_pc n_extra max_iter tol G val vec res -> the whole iteration on the dense G [I][I]; stdout: n_iter */
#include "mchip_feature_geometry.h"
#include "mchip_pca_algebra.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static std::vector<double> load(const char *path, size_t n)
{
	std::vector<double> v(n);
	FILE *f = fopen(path, "rb");
	if (!f || fread(v.data(), sizeof(double), n, f) != n) { fprintf(stderr, "cannot read %zu doubles from %s\n", n, path); exit(2); }
	fclose(f);
	return v;
}

static void save(const char *path, const double *v, size_t n)
{
	FILE *f = fopen(path, "wb");
	if (!f || fwrite(v, sizeof(double), n, f) != n || fclose(f)) { fprintf(stderr, "cannot write %s\n", path); exit(2); }
}

int main(int argc, char **argv)
{
	if (argc < 2) return 2;
	const char *mode = argv[1];
	if (!strcmp(mode, "constants")) {
		int I, L;
		printf("%d %d %d %d\n", PCA_LSLAB, PCA_VARIANTS, PCA_ITILE, PCA_MAX_BLOCK);
		while (scanf("%d %d", &I, &L) == 2) {
			const pca_geometry g = pca_geometry_of(I, L);
			printf("%d %d %d %d\n", g.n_vgroups, g.n_itiles, g.Ipad, g.n_slabs);
		}
	} else if (!strcmp(mode, "width")) {
		int I, n_pc, n_extra;
		while (scanf("%d %d %d", &I, &n_pc, &n_extra) == 3) printf("%d\n", pca_block_width(I, n_pc, n_extra));
	} else if (!strcmp(mode, "start") && argc == 5) {
		const int I = atoi(argv[2]), b = atoi(argv[3]);
		std::vector<double> X((size_t)I * b);
		for (int i = 0; i < I; i++)
			for (int c = 0; c < b; c++) X[(size_t)i * b + c] = pca_start_value(i, c);
		save(argv[4], X.data(), X.size());
	} else if (!strcmp(mode, "mgs2") && argc == 6) {
		const int I = atoi(argv[2]), b = atoi(argv[3]);
		std::vector<double> X = load(argv[4], (size_t)I * b);
		printf("%d\n", pca_mgs2(X.data(), I, b));
		save(argv[5], X.data(), X.size());
	} else if (!strcmp(mode, "jacobi") && argc == 6) {
		const int b = atoi(argv[2]);
		std::vector<double> H = load(argv[3], (size_t)b * b), theta((size_t)b), S((size_t)b * b);
		printf("%d\n", pca_jacobi(H.data(), b, theta.data(), S.data()));
		save(argv[4], theta.data(), theta.size());
		save(argv[5], S.data(), S.size());
	} else if (!strcmp(mode, "sign") && argc == 5) {
		const int n = atoi(argv[2]);
		std::vector<double> v = load(argv[3], (size_t)n);
		pca_fix_sign(v.data(), n, 1);
		save(argv[4], v.data(), v.size());
	} else if (!strcmp(mode, "residuals") && argc == 11) {
		const int I = atoi(argv[2]), b = atoi(argv[3]), n_pc = atoi(argv[4]);
		std::vector<double> X = load(argv[5], (size_t)I * b), Y = load(argv[6], (size_t)I * b), S = load(argv[7], (size_t)b * b),
				    theta = load(argv[8], (size_t)b), U((size_t)I * b), r((size_t)n_pc);
		pca_ritz_residuals(X.data(), Y.data(), S.data(), theta.data(), I, b, n_pc, U.data(), r.data());
		save(argv[9], U.data(), U.size());
		save(argv[10], r.data(), r.size());
	} else if (!strcmp(mode, "iterate") && argc == 11) {
		const int I = atoi(argv[2]), n_pc = atoi(argv[3]), n_extra = atoi(argv[4]), max_iter = atoi(argv[5]);
		const double tol = atof(argv[6]);
		const std::vector<double> G = load(argv[7], (size_t)I * I);
		const int b = pca_block_width(I, n_pc, n_extra);
		std::vector<double> val((size_t)n_pc), vec((size_t)I * n_pc), res((size_t)n_pc);
		int n_iter = 0;
		const int rc = pca_subspace_iteration(I, b, n_pc, max_iter, tol, [&](const double *X, double *Y) {
			for (int i = 0; i < I; i++)
				for (int c = 0; c < b; c++) {
					double s = 0.0;
					for (int j = 0; j < I; j++) s += G[(size_t)i * I + j] * X[(size_t)j * b + c];
					Y[(size_t)i * b + c] = s;
				}
			return 0;
		}, val.data(), vec.data(), res.data(), &n_iter);
		if (rc) return 3;
		printf("%d\n", n_iter);
		save(argv[8], val.data(), val.size());
		save(argv[9], vec.data(), vec.size());
		save(argv[10], res.data(), res.size());
	} else {
		fprintf(stderr, "unknown mode or wrong number of arguments: %s\n", mode);
		return 2;
	}
	return 0;
}
