/*
 * mc_diverge.c -- divergence of the fitted clusters (--fst; an extension: the tables STRUCTURE ends a fit with -- net nucleotide
 * distance between the populations, expected heterozygosity within each -- and ADMIXTURE's F_ST between the estimated
 * populations).  mc_divergence asks the device for the sums over the allele-frequency table of the fit (mchip_divergence,
 * include/multiclust_hip.h has the definitions) with the weights the fit gives the clusters and derives H, D, F_ab, F_l and F from
 * them; the weights, the tables and the summary are plain functions of their arguments (libc only), and so is the writer.
 *
 * The files, with result files on (every number %.10f, a NaN as the word NaN, tab-separated):
 *   <stem>.<admix|mix>.K=<K>.fst.txt       "k\tweight\tH", one line "k\tw_k\tH_k" per cluster, an empty line, "D" and the K lines of
 *                                          the K x K net-distance matrix, an empty line, "Fst" and the K lines of the F_ST matrix
 *   <stem>.<admix|mix>.K=<K>.fst.loci.txt  "l\tcolumns\tHT\tFst", one line "l\tuniquealleles[l]\tHT_l\tF_l" per locus
 */
#include "mc_cli.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

/* the weights of the clusters: n_rows > 0: the column means of q [n_rows][K] over the rows without a NaN (individuals without an
 * observed copy and query individuals drop out), added in row order; 1 / K when no row is left.  n_rows = 0: q [K] itself. */
void mc_divergence_weights(int K, int n_rows, const double *q, double *w)
{
	int n = 0;
	if (!n_rows) {
		memcpy(w, q, sizeof(double) * (size_t)K);
		return;
	}
	for (int k = 0; k < K; k++) w[k] = 0.0;
	for (int i = 0; i < n_rows; i++) {
		const double *row = q + (size_t)i * K;
		int ok = 1;
		for (int k = 0; k < K; k++) if (isnan(row[k])) ok = 0;
		if (!ok) continue;
		for (int k = 0; k < K; k++) w[k] += row[k];
		n++;
	}
	for (int k = 0; k < K; k++) w[k] = n ? w[k] / (double)n : 1.0 / (double)K;
}

/* H_a = h_a / L1, D_ab = s_ab / (2 L1), F_ab = D_ab / (D_ab + (H_a + H_b) / 2), NaN when that denominator is 0 */
void mc_divergence_tables(int K, int n_loci, const double *het, const double *sqdiff, double *H, double *D, double *F)
{
	const double L1 = (double)n_loci;
	for (int a = 0; a < K; a++) H[a] = het[a] / L1;
	for (int a = 0; a < K; a++)
		for (int b = 0; b < K; b++) {
			const size_t x = (size_t)a * K + b;
			D[x] = sqdiff[x] / (2.0 * L1);
			const double den = D[x] + (H[a] + H[b]) / 2.0;
			F[x] = den != 0.0 ? D[x] / den : NAN;
		}
}

/* over the pairs a < b whose F_ab is a number, in (a, b) order: how many, and their mean, smallest and largest (NaN without one) */
void mc_divergence_summary(int K, const double *F, int *n_pairs, double *mean, double *min, double *max)
{
	double sum = 0.0, lo = INFINITY, hi = -INFINITY;
	int n = 0;
	for (int a = 0; a < K; a++)
		for (int b = a + 1; b < K; b++) {
			const double f = F[(size_t)a * K + b];
			if (isnan(f)) continue;
			sum += f;
			if (f < lo) lo = f;
			if (f > hi) hi = f;
			n++;
		}
	*n_pairs = n;
	*mean = n ? sum / (double)n : NAN;
	*min = n ? lo : NAN;
	*max = n ? hi : NAN;
}

void mc_divergence_result_free(mc_divergence_result *r)
{
	free(r->w); free(r->H); free(r->D); free(r->F); free(r->locus_ht); free(r->locus_f);
	memset(r, 0, sizeof *r);
}

int mc_divergence(const mc_options *opt, const mc_data *dat, mc_model *mod, mc_divergence_result *out)
{
	const int K = mod->K, L = dat->L, rows = (opt->admixture && !opt->eta_constrained) ? dat->I : 0;
	double *q = malloc(sizeof(double) * (size_t)(rows ? rows : 1) * K), *het = malloc(sizeof(double) * (size_t)K);
	double *sq = malloc(sizeof(double) * (size_t)K * K), *lv = malloc(sizeof(double) * (size_t)L);
	int32_t n1 = 0;
	int rc = MCHIP_ERR_ALLOC;
	memset(out, 0, sizeof *out);
	out->K = K;
	out->L = L;
	out->w = malloc(sizeof(double) * (size_t)K);
	out->H = malloc(sizeof(double) * (size_t)K);
	out->D = malloc(sizeof(double) * (size_t)K * K);
	out->F = malloc(sizeof(double) * (size_t)K * K);
	out->locus_ht = malloc(sizeof(double) * (size_t)L);
	out->locus_f = malloc(sizeof(double) * (size_t)L);
	if (!q || !het || !sq || !lv || !out->w || !out->H || !out->D || !out->F || !out->locus_ht || !out->locus_f) goto DONE;
	if ((rc = mc_model_get_q(mod, mod->pindex, q))) goto DONE;
	mc_divergence_weights(K, rows, q, out->w);
	rc = mchip_divergence(mod->dev, mod->pindex, out->w, het, sq, lv, out->locus_ht, &out->sum_v, &out->sum_ht, &n1);
	if (rc) {
		fprintf(stderr, "ERROR [mc_diverge.c::mc_divergence]: mchip_divergence failed (%d): %s\n", rc, mchip_last_error(mod->dev));
		goto DONE;
	}
	out->n_loci = (int)n1;
	mc_divergence_tables(K, out->n_loci, het, sq, out->H, out->D, out->F);
	mc_divergence_summary(K, out->F, &out->n_pairs, &out->f_mean, &out->f_min, &out->f_max);
	for (int l = 0; l < L; l++)
		out->locus_f[l] = (dat->uniquealleles[l] > 0 && out->locus_ht[l] != 0.0) ? lv[l] / out->locus_ht[l] : NAN;
	out->f_all = out->sum_ht != 0.0 ? out->sum_v / out->sum_ht : NAN;
DONE:
	free(q); free(het); free(sq); free(lv);
	if (rc) mc_divergence_result_free(out);
	return rc;
}

/* the stdout line of --fst, without its line end */
void mc_divergence_line(FILE *fp, const mc_divergence_result *r)
{
	fprintf(fp, "Divergence (K=%d): ", r->K);
	if (r->n_pairs) fprintf(fp, "pairwise Fst mean %.6f min %.6f max %.6f over %d pairs", r->f_mean, r->f_min, r->f_max, r->n_pairs);
	else fprintf(fp, "no pairs");
	fprintf(fp, "; among clusters %.6f [%d loci]", r->f_all, r->n_loci);
}

/* ---- the writer ---- */
static void put(FILE *fp, double v, char end)
{
	if (isnan(v)) fprintf(fp, "NaN%c", end);	/* (printf would say nan or -nan) */
	else fprintf(fp, "%.10f%c", v, end);
}

int mc_write_divergence(const mc_cli_options *opt, const mc_cli_data *dat, const mc_divergence_result *r)
{
	char path[4400];
	const int K = r->K;
	const size_t len = mc_result_path(opt, path, sizeof path, ".%s.K=%d.fst.txt", opt->em.admixture ? "admix" : "mix", K);
	FILE *fp = mc_open_result("mc_diverge.c", path, "w");
	if (!fp) return MC_EXIT_FILE_OPEN_ERROR;
	fprintf(fp, "k\tweight\tH\n");
	for (int k = 0; k < K; k++) {
		fprintf(fp, "%d\t", k);
		put(fp, r->w[k], '\t');
		put(fp, r->H[k], '\n');
	}
	for (int t = 0; t < 2; t++) {
		const double *m = t ? r->F : r->D;
		fprintf(fp, "\n%s\n", t ? "Fst" : "D");
		for (int a = 0; a < K; a++)
			for (int b = 0; b < K; b++) put(fp, m[(size_t)a * K + b], b + 1 < K ? '\t' : '\n');
	}
	if (mc_close_result(fp)) return MC_EXIT_FILE_OPEN_ERROR;
	snprintf(path + len, sizeof path - len, ".%s.K=%d.fst.loci.txt", opt->em.admixture ? "admix" : "mix", K);
	if (!(fp = mc_open_result("mc_diverge.c", path, "w"))) return MC_EXIT_FILE_OPEN_ERROR;
	fprintf(fp, "l\tcolumns\tHT\tFst\n");
	for (int l = 0; l < dat->L; l++) {
		fprintf(fp, "%d\t%d\t", l, (int)dat->uniquealleles[l]);
		put(fp, r->locus_ht[l], '\t');
		put(fp, r->locus_f[l], '\n');
	}
	return mc_close_result(fp);
}
