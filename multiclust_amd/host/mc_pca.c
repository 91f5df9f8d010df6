/*
 * mc_pca.c -- --pca <n> (an extension): the leading principal components of a PLINK fileset, the companion of every Q plot and the
 * usual cross-check on the choice of K.  It runs as the last stage of pre_fit() (mc_cli_stages.c), on the fileset quality control, --prune
 * and --king-cutoff left, and it is no filter: the data set is unchanged and every fit afterwards is the same, byte for byte.
 *
 * The matrix is defined in include/multiclust_hip.h (mchip_bed_pca): G = Z Z^T / L' with Z the genotypes standardised per variant by
 * the allele frequency of the typed individuals, a missing call imputed by the mean (z = 0), all-missing and monomorphic variants
 * left out -- the matrix of flashpca and of PLINK 2's --pca approx; NOT PLINK 1.9's pairwise-complete GRM and not smartpca's
 * normalisation.  The eigenpairs come from block subspace iteration on the device with n + MC_PCA_EXTRA start vectors (rounded up to
 * a multiple of 16), at most --pca-iter iterations, until every component's residual || G u - theta u || / theta_1 is at most
 * --pca-tol.  Component c converges at the rate lambda_{b+1} / lambda_c per iteration: components inside the noise bulk of the
 * spectrum converge slowly and mean nothing; the run says which ones are still loose and goes on.  All variants count: keeping to
 * the autosomes and thinning by LD first is the user's --prune / --extract.
 *
 * Everything in this file is libc, mc_files.h and mc_filter.h but the one function that calls the device (components_by_device:
 * mchip_bed_pca).
 */
#include "mc_cli.h"

#include <stdlib.h>
#include <string.h>

void mc_pca_result_free(mc_pca_result *r)
{
	if (!r) return;
	free(r->eigenvalues); free(r->eigenvectors); free(r->residuals);
	memset(r, 0, sizeof *r);
}

static int components_by_device(const mc_cli_options *opt, mc_device_band *dev, void *out)
{
	mc_pca_result *r = out;
	const mc_cli_data *d = dev->dat;
	return mchip_bed_pca(dev->ctx, d->I, d->L, d->bed, d->bed_record_bytes, r->n_pc, MC_PCA_EXTRA, opt->pca_iter, opt->pca_tol, r->eigenvalues,
			     r->eigenvectors, r->residuals, &r->trace, &r->n_used, &r->n_iter);
}

int mc_pca_data(const mc_cli_options *opt, const mc_cli_data *dat, mc_pca_result *r)
{
	const double t_start = mc_now_s();
	memset(r, 0, sizeof *r);
	if (!dat->bed) return MC_EXIT_INTERNAL_ERROR;	/* a fileset */
	if (opt->pca > dat->I - 1) {
		fprintf(stderr, "ERROR [mc_pca.c::mc_pca_data]: --pca %d asks for more components than the %d individuals of the data set allow (at most %d)\n",
			opt->pca, dat->I, dat->I - 1);
		return MC_EXIT_INVALID_USER_SETUP;
	}
	r->n_pc = opt->pca; r->I = dat->I; r->L = dat->L;
	r->eigenvalues = calloc((size_t)r->n_pc, sizeof(double));
	r->eigenvectors = calloc((size_t)r->n_pc * (size_t)r->I, sizeof(double));
	r->residuals = calloc((size_t)r->n_pc, sizeof(double));
	int rc = MC_EXIT_MEMORY_ALLOCATION;
	if (r->eigenvalues && r->eigenvectors && r->residuals)
		rc = mc_filter_on_device(opt, dat, "mc_pca.c::mc_pca_data", "--pca", "the principal components", components_by_device, r);
	if (rc) mc_pca_result_free(r);
	else mc_timing_line("mc_pca.c", "principal components", t_start);
	return rc;
}

static double largest_residual(const mc_pca_result *r)
{
	double m = 0.0;
	for (int c = 0; c < r->n_pc; c++)
		if (!(r->residuals[c] <= m)) m = r->residuals[c];
	return m;
}

void mc_pca_line(FILE *fp, const mc_pca_result *r)
{
	fprintf(fp, "PCA: %d components of %d individuals x %d of %d variants (%d iterations, largest residual %.6g): variance explained", r->n_pc, r->I,
		r->n_used, r->L, r->n_iter, largest_residual(r));
	for (int c = 0; c < r->n_pc; c++) fprintf(fp, " %.6g", r->eigenvalues[c] / r->trace);
	fprintf(fp, "\n");
}

int mc_pca_warn(FILE *fp, const mc_cli_options *opt, const mc_pca_result *r)
{
	int n = 0;
	for (int c = 0; c < r->n_pc; c++) n += !(r->residuals[c] <= opt->pca_tol);
	if (!n) return 0;
	fprintf(fp, "WARNING [mc_pca.c]: --pca: after %d iterations the residual still exceeds %g for", r->n_iter, opt->pca_tol);
	for (int c = 0; c < r->n_pc; c++)
		if (!(r->residuals[c] <= opt->pca_tol)) fprintf(fp, " PC%d", c + 1);
	fprintf(fp, " (largest %.6g): such components lie in the noise bulk of the spectrum or need more of --pca-iter\n", largest_residual(r));
	return n;
}

/* <stem>.eigenvec: PLINK 1.9's layout, no header: "FID IID PC1 ... PCn", one line per individual of the data set in its order, the
 * ids of its .fam line.  <stem>.eigenval: one eigenvalue per line.  <stem>.pca.txt: one header line, then one tab-separated line per
 * component: its number, eigenvalue, share of the trace, residual, and 1 when the residual is at most --pca-tol, else 0.  Doubles as
 * %.6g, as the quality-control tables print theirs. */
int mc_write_pca(const mc_cli_options *opt, const mc_cli_data *dat, const mc_pca_result *r)
{
	char path[4400];
	int rc;
	mc_result_path(opt, path, sizeof path, ".eigenvec");
	FILE *fp = mc_open_result("mc_pca.c", path, "w");
	if (!fp) return MC_EXIT_FILE_OPEN_ERROR;
	for (int i = 0; i < r->I; i++) {
		fprintf(fp, "%s %s", dat->pops[dat->locale[i]], dat->names[i]);
		for (int c = 0; c < r->n_pc; c++) fprintf(fp, " %.6g", r->eigenvectors[(size_t)i * (size_t)r->n_pc + (size_t)c]);
		fprintf(fp, "\n");
	}
	if ((rc = mc_close_result(fp))) return rc;
	mc_result_path(opt, path, sizeof path, ".eigenval");
	if (!(fp = mc_open_result("mc_pca.c", path, "w"))) return MC_EXIT_FILE_OPEN_ERROR;
	for (int c = 0; c < r->n_pc; c++) fprintf(fp, "%.6g\n", r->eigenvalues[c]);
	if ((rc = mc_close_result(fp))) return rc;
	mc_result_path(opt, path, sizeof path, ".pca.txt");
	if (!(fp = mc_open_result("mc_pca.c", path, "w"))) return MC_EXIT_FILE_OPEN_ERROR;
	fprintf(fp, "PC\tEIGENVALUE\tSHARE\tRESIDUAL\tCONVERGED\n");
	for (int c = 0; c < r->n_pc; c++)
		fprintf(fp, "%d\t%.6g\t%.6g\t%.6g\t%d\n", c + 1, r->eigenvalues[c], r->eigenvalues[c] / r->trace, r->residuals[c],
			r->residuals[c] <= opt->pca_tol ? 1 : 0);
	return mc_close_result(fp);
}
