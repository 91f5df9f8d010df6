/*
 * mc_kinship.c -- kinship between individuals under the fitted admixture model (--kinship <t>; an extension: REAP's estimator,
 * Thornton et al. 2012, which PC-Relate shares, generalised to multi-allelic data of any ploidy).  mc_kinship asks the device for the
 * two sums (mchip_kinship_products, include/multiclust_hip.h has the definitions and the derivation) and forms phi_ij = G_ij / V_ij
 * and what is reported of it; the ratios, the rules and the writer are plain functions of their arguments (libc only).
 *
 * Unlike KING-robust (--king-cutoff, before the fit) the estimator uses allele frequencies, the individual-specific ones of the fit:
 * it holds for pairs of different or mixed ancestry.  Limits: P and Q were estimated with the pair in the data, so the estimates of
 * true relatives are biased slightly towards zero (no leave-one-out frequencies); a family large enough to have been fitted as a
 * cluster of its own is absorbed by the model and shows no kinship -- that is what --king-cutoff before the fit is for; columns whose
 * frequency lies at a bound contribute almost nothing to either sum.  Not done: k0 / k1 / k2, removal of individuals on this estimate.
 *
 * The degree of a pair by the usual cuts (powers of 2^-1/2 ... between the expected coefficients 1/2, 1/4, 1/8, 1/16): 0 = duplicate or
 * monozygotic twin, phi > 0.354; 1 = first degree, > 0.177; 2 = second, > 0.0884; 3 = third, > 0.0442; 4 = more distant.  A NaN
 * compares false everywhere: a pair without a number is reported nowhere.
 *
 * The files, with result files on (every real number %.6f, a NaN as the word NaN, tab-separated, indices from 0 as in .resid.ind.txt):
 *   <stem>.admix.K=<K>.kin0         "i\tj\tphi\tG\tV\tdegree", one line per pair i < j with phi > t, in (i, j) order
 *   <stem>.admix.K=<K>.kin.ind.txt  "i\tself\tinbreeding\tn_above\tmax\tpartner", one line per individual: phi_ii, 2 phi_ii - 1 (ploidy 2,
 *                                   otherwise NaN), how many others it has phi > t with, its largest finite phi with another and
 *                                   the first individual it has it with (NaN and -1 without one)
 * There is no I x I file.
 */
#include "mc_cli.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

int mc_kinship_degree(double phi)
{
	return phi > 0.354 ? 0 : phi > 0.177 ? 1 : phi > 0.0884 ? 2 : phi > 0.0442 ? 3 : 4;
}

static double ratio(double g, double v) { return v > 0.0 ? g / v : NAN; }

void mc_kinship_result_free(mc_kinship_result *r)
{
	free(r->pairs); free(r->self); free(r->inbreeding); free(r->ind_max); free(r->ind_count); free(r->ind_partner);
	memset(r, 0, sizeof *r);
}

/* everything mc_kinship reports, from the sums G and V [I][I] (the upper triangle is read for the pairs, the whole row for an
 * individual's largest: the sums are symmetric).  r->K is the caller's.  0, or MCHIP_ERR_ALLOC with nothing held. */
int mc_kinship_from_sums(int I, int ploidy, double t, const double *G, const double *V, mc_kinship_result *r)
{
	const int K = r->K;
	double sum = 0.0, hi = -INFINITY;
	size_t n_above = 0, at = 0;
	memset(r, 0, sizeof *r);
	r->K = K; r->I = I; r->ploidy = ploidy; r->t = t;
	r->max_i = r->max_j = -1;
	for (int i = 0; i < I; i++)
		for (int j = i + 1; j < I; j++) n_above += ratio(G[(size_t)i * I + j], V[(size_t)i * I + j]) > t;
	r->pairs = malloc(sizeof(mc_kin_pair) * (n_above ? n_above : 1));
	r->self = malloc(sizeof(double) * (size_t)I);
	r->inbreeding = malloc(sizeof(double) * (size_t)I);
	r->ind_max = malloc(sizeof(double) * (size_t)I);
	r->ind_count = calloc((size_t)I, sizeof(int32_t));
	r->ind_partner = malloc(sizeof(int32_t) * (size_t)I);
	if (!r->pairs || !r->self || !r->inbreeding || !r->ind_max || !r->ind_count || !r->ind_partner) {
		mc_kinship_result_free(r);
		return MCHIP_ERR_ALLOC;
	}
	for (int i = 0; i < I; i++) {
		double m = -INFINITY;
		int who = -1;
		for (int j = 0; j < I; j++) {
			const size_t ij = (size_t)i * I + j;
			const double phi = ratio(G[ij], V[ij]);
			if (j == i) {
				r->self[i] = phi;
				r->inbreeding[i] = ploidy == 2 ? 2.0 * phi - 1.0 : NAN;
				continue;
			}
			if (!isfinite(phi)) continue;
			if (phi > m) { m = phi; who = j; }
			if (phi > t) r->ind_count[i]++;
			if (j < i) continue;
			sum += phi;
			r->n_finite++;
			if (phi > hi) { hi = phi; r->max_i = i; r->max_j = j; }
			if (phi > t) {
				mc_kin_pair *p = &r->pairs[at++];
				p->i = i; p->j = j; p->phi = phi; p->G = G[ij]; p->V = V[ij];
				p->degree = mc_kinship_degree(phi);
				r->n_degree[p->degree]++;
			}
		}
		r->ind_max[i] = who >= 0 ? m : NAN;
		r->ind_partner[i] = who;
	}
	r->n_pairs = at;
	r->mean = r->n_finite ? sum / (double)r->n_finite : NAN;
	r->max = r->n_finite ? hi : NAN;
	return MCHIP_OK;
}

int mc_kinship(const mc_data *dat, mc_model *mod, double t, mc_kinship_result *out)
{
	const int I = dat->I;
	const size_t n2 = (size_t)I * I;
	double *G = malloc(sizeof(double) * n2), *V = malloc(sizeof(double) * n2);
	int rc = MCHIP_ERR_ALLOC;
	memset(out, 0, sizeof *out);
	if (!G || !V) goto DONE;
	rc = mchip_kinship_products(mod->dev, mod->pindex, G, V);
	if (rc) {
		fprintf(stderr, "ERROR [mc_kinship.c::mc_kinship]: mchip_kinship_products failed (%d): %s\n", rc, mchip_last_error(mod->dev));
		goto DONE;
	}
	out->K = mod->K;
	rc = mc_kinship_from_sums(I, dat->ploidy, t, G, V, out);
DONE:
	free(G); free(V);
	return rc;
}

/* the stdout line of --kinship, without its line end */
void mc_kinship_line(FILE *fp, const mc_kinship_result *r)
{
	fprintf(fp, "Kinship (K=%d): ", r->K);
	if (!r->n_finite) { fprintf(fp, "no pairs"); return; }
	fprintf(fp, "%zu pairs above %g (%lld duplicates, %lld first, %lld second, %lld third degree); largest %.6f (%d, %d); mean over %lld pairs %.6f",
		r->n_pairs, r->t, r->n_degree[0], r->n_degree[1], r->n_degree[2], r->n_degree[3], r->max, r->max_i, r->max_j, r->n_finite, r->mean);
}

/* ---- the writer ---- */
static void put(FILE *fp, double v, char end)
{
	if (isnan(v)) fprintf(fp, "NaN%c", end);	/* (printf would say nan or -nan) */
	else fprintf(fp, "%.6f%c", v, end);
}

int mc_write_kinship(const mc_cli_options *opt, const mc_kinship_result *r)
{
	char path[4400];
	const size_t len = mc_result_path(opt, path, sizeof path, ".admix.K=%d.kin0", r->K);
	FILE *fp = mc_open_result("mc_kinship.c", path, "w");
	if (!fp) return MC_EXIT_FILE_OPEN_ERROR;
	fprintf(fp, "i\tj\tphi\tG\tV\tdegree\n");
	for (size_t x = 0; x < r->n_pairs; x++) {
		const mc_kin_pair *p = &r->pairs[x];
		fprintf(fp, "%d\t%d\t", p->i, p->j);
		put(fp, p->phi, '\t');
		put(fp, p->G, '\t');
		put(fp, p->V, '\t');
		fprintf(fp, "%d\n", p->degree);
	}
	if (mc_close_result(fp)) return MC_EXIT_FILE_OPEN_ERROR;
	snprintf(path + len, sizeof path - len, ".admix.K=%d.kin.ind.txt", r->K);
	if (!(fp = mc_open_result("mc_kinship.c", path, "w"))) return MC_EXIT_FILE_OPEN_ERROR;
	fprintf(fp, "i\tself\tinbreeding\tn_above\tmax\tpartner\n");
	for (int i = 0; i < r->I; i++) {
		fprintf(fp, "%d\t", i);
		put(fp, r->self[i], '\t');
		put(fp, r->inbreeding[i], '\t');
		fprintf(fp, "%d\t", (int)r->ind_count[i]);
		put(fp, r->ind_max[i], '\t');
		fprintf(fp, "%d\n", (int)r->ind_partner[i]);
	}
	return mc_close_result(fp);
}
