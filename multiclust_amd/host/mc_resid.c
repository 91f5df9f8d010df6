/*
 * mc_resid.c -- residual correlation of the admixture fit between individuals (--resid; an extension: evalAdmix's check of a fit,
 * Garcia-Erill and Albrechtsen 2020, for multi-allelic data of any ploidy).  mc_residual_correlation asks the device for the sums
 * over the residuals "observed allele count minus the count the fit predicts" (mchip_residual_products, include/multiclust_hip.h
 * has the definitions) and forms cor_ij = G_ij / sqrt(D_ij D_ji) and its summary; the ratios, the summary and the writer are plain
 * functions of their arguments (libc only).  Under an adequate fit the correlations scatter around a slightly negative value -- P
 * was estimated with individual i in the data: of the order -1 / (size of i's cluster); evalAdmix's leave-one-out refit of the
 * frequencies, which removes that bias, is not done -- and relatives, duplicated samples, a K that is too small and unmodelled
 * substructure show as blocks of positive correlation.
 *
 * The files, with result files on (every number %.6f, a NaN as the word NaN, tab-separated):
 *   <stem>.admix.K=<K>.resid.txt      the I x I matrix, one line per individual: I^2 numbers
 *   <stem>.admix.K=<K>.resid.ind.txt  "i\tmean\tmax\tpartner", one line per individual: the mean of its finite correlations, the
 *                                     largest of them and the individual it has it with (NaN, NaN and -1 without a finite one)
 */
#include "mc_cli.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

/* cor [I][I] from G and D [I][I]: cor_ij = G_ij / sqrt(D_ij D_ji) for i != j, NaN where either D is 0 (or not a number) and on the
 * diagonal.  cor_ij and cor_ji come from the same three doubles (a product commutes): the matrix is symmetric bit for bit when G
 * is. */
void mc_residual_ratios(int I, const double *G, const double *D, double *cor)
{
	for (int i = 0; i < I; i++)
		for (int j = 0; j < I; j++) {
			const size_t ij = (size_t)i * I + j, ji = (size_t)j * I + i;
			const double a = D[ij], b = D[ji];
			cor[ij] = (i != j && a > 0.0 && b > 0.0) ? G[ij] / sqrt(a * b) : NAN;
		}
}

/* over the finite off-diagonal entries of cor: per individual the mean, the largest and its partner (the first, NaN / NaN / -1
 * without one); over the pairs i < j in (i, j) order their number, mean, mean absolute value and the largest with its pair (NaN and
 * -1 without one) */
void mc_residual_summary(int I, const double *cor, mc_resid_result *r)
{
	double sum = 0.0, asum = 0.0, hi = -INFINITY;
	long long n = 0;
	r->max_i = r->max_j = -1;
	for (int i = 0; i < I; i++) {
		double s = 0.0, m = -INFINITY;
		int cnt = 0, who = -1;
		for (int j = 0; j < I; j++) {
			const double c = cor[(size_t)i * I + j];
			if (j == i || !isfinite(c)) continue;
			s += c;
			cnt++;
			if (c > m) { m = c; who = j; }
			if (j > i) {
				sum += c;
				asum += fabs(c);
				n++;
				if (c > hi) { hi = c; r->max_i = i; r->max_j = j; }
			}
		}
		r->ind_mean[i] = cnt ? s / (double)cnt : NAN;
		r->ind_max[i] = cnt ? m : NAN;
		r->ind_partner[i] = who;
	}
	r->n_pairs = n;
	r->mean = n ? sum / (double)n : NAN;
	r->mean_abs = n ? asum / (double)n : NAN;
	r->max = n ? hi : NAN;
}

void mc_resid_result_free(mc_resid_result *r)
{
	free(r->cor); free(r->ind_mean); free(r->ind_max); free(r->ind_partner);
	memset(r, 0, sizeof *r);
}

int mc_residual_correlation(const mc_data *dat, mc_model *mod, mc_resid_result *out)
{
	const int I = dat->I;
	const size_t n2 = (size_t)I * I;
	double *G = malloc(sizeof(double) * n2), *D = malloc(sizeof(double) * n2);
	int rc = MCHIP_ERR_ALLOC;
	memset(out, 0, sizeof *out);
	out->K = mod->K;
	out->I = I;
	out->cor = malloc(sizeof(double) * n2);
	out->ind_mean = malloc(sizeof(double) * (size_t)I);
	out->ind_max = malloc(sizeof(double) * (size_t)I);
	out->ind_partner = malloc(sizeof(int32_t) * (size_t)I);
	if (!G || !D || !out->cor || !out->ind_mean || !out->ind_max || !out->ind_partner) goto DONE;
	rc = mchip_residual_products(mod->dev, mod->pindex, G, D);
	if (rc) {
		fprintf(stderr, "ERROR [mc_resid.c::mc_residual_correlation]: mchip_residual_products failed (%d): %s\n", rc, mchip_last_error(mod->dev));
		goto DONE;
	}
	mc_residual_ratios(I, G, D, out->cor);
	mc_residual_summary(I, out->cor, out);
DONE:
	free(G); free(D);
	if (rc) mc_resid_result_free(out);
	return rc;
}

/* the stdout line of --resid, without its line end */
void mc_resid_line(FILE *fp, const mc_resid_result *r)
{
	fprintf(fp, "Residual correlation (K=%d): ", r->K);
	if (r->n_pairs) fprintf(fp, "mean %.6f mean |r| %.6f max %.6f (%d, %d) over %lld pairs", r->mean, r->mean_abs, r->max, r->max_i, r->max_j, r->n_pairs);
	else fprintf(fp, "no pairs");
}

/* ---- the writer ---- */
static void put(FILE *fp, double v, char end)
{
	if (isnan(v)) fprintf(fp, "NaN%c", end);	/* (printf would say nan or -nan) */
	else fprintf(fp, "%.6f%c", v, end);
}

int mc_write_resid(const mc_cli_options *opt, const mc_resid_result *r)
{
	char path[4400];
	const int I = r->I;
	const size_t len = mc_result_path(opt, path, sizeof path, ".admix.K=%d.resid.txt", r->K);
	FILE *fp = mc_open_result("mc_resid.c", path, "w");
	if (!fp) return MC_EXIT_FILE_OPEN_ERROR;
	for (int i = 0; i < I; i++)
		for (int j = 0; j < I; j++) put(fp, r->cor[(size_t)i * I + j], j + 1 < I ? '\t' : '\n');
	if (mc_close_result(fp)) return MC_EXIT_FILE_OPEN_ERROR;
	snprintf(path + len, sizeof path - len, ".admix.K=%d.resid.ind.txt", r->K);
	if (!(fp = mc_open_result("mc_resid.c", path, "w"))) return MC_EXIT_FILE_OPEN_ERROR;
	fprintf(fp, "i\tmean\tmax\tpartner\n");
	for (int i = 0; i < I; i++) {
		fprintf(fp, "%d\t", i);
		put(fp, r->ind_mean[i], '\t');
		put(fp, r->ind_max[i], '\t');
		fprintf(fp, "%d\n", (int)r->ind_partner[i]);
	}
	return mc_close_result(fp);
}
