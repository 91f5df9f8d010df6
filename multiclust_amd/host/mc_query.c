/*
 * mc_query.c -- query individuals: individuals of the data set that take no part in estimating the allele frequencies and whose
 * mixing proportions are fitted afterwards with P held fixed (an extension: in the reference every individual of the file shapes
 * P).  The query file marks them; mc_query_hide turns their genotypes into missing data on the device before a model is fitted
 * (the cross-validation hold-out, include/multiclust_hip.h: mchip_cv_set_folds, mchip_cv_hold_out), so every initialisation of
 * every K runs on the panel alone; mc_query_fit fits them against the best fit of a K (mchip_fit_q_rows, which reads the data set
 * saved by the hold-out).
 */
#include "mc_cli.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

int mc_query_read(const char *path, int I, uint8_t **mask_out)
{
	FILE *fp = fopen(path, "r");
	uint8_t *mask;
	char tok[16];
	int n[2] = { 0, 0 };
	*mask_out = NULL;
	if (!fp) {
		fprintf(stderr, "ERROR [mc_query.c::mc_query_read]: could not open file '%s'\n", path);
		return MC_EXIT_FILE_OPEN_ERROR;
	}
	if (!(mask = malloc((size_t)(I > 0 ? I : 1)))) { fclose(fp); return MC_EXIT_MEMORY_ALLOCATION; }
	for (int i = 0; i <= I; i++) {
		const int got = fscanf(fp, "%15s", tok);
		if (i == I) {	/* exactly I tokens */
			if (got == 1) {
				fprintf(stderr, "ERROR [mc_query.c::mc_query_read]: format of query file '%s': more than %d tokens\n", path, I);
				goto BAD;
			}
			break;
		}
		if (got != 1) {
			fprintf(stderr, "ERROR [mc_query.c::mc_query_read]: format of query file '%s': %d tokens wanted, %d found\n", path, I, i);
			goto BAD;
		}
		if ((tok[0] != '0' && tok[0] != '1') || tok[1]) {
			fprintf(stderr, "ERROR [mc_query.c::mc_query_read]: format of query file '%s': token %d is '%s', not 0 (panel) or 1 (query)\n", path, i + 1, tok);
			goto BAD;
		}
		mask[i] = (uint8_t)(tok[0] - '0');
		n[mask[i]]++;
	}
	if (!n[0] || !n[1]) {
		fprintf(stderr, "ERROR [mc_query.c::mc_query_read]: query file '%s': at least one panel (0) and one query (1) individual are needed\n", path);
		goto BAD;
	}
	fclose(fp);
	*mask_out = mask;
	return 0;
BAD:
	fclose(fp);
	free(mask);
	return MC_EXIT_FILE_FORMAT_ERROR;
}

static int query_fail(const mc_model *mod, int rc, const char *where, const char *what)
{
	if (rc) fprintf(stderr, "ERROR [mc_query.c::%s]: %s failed (%d): %s\n", where, what, rc, mchip_last_error(mod->dev));
	return rc;
}

int mc_query_hide(mc_model *mod, const mc_data *dat, const uint8_t *mask)
{
	/* two folds, fold(i, l) = mask[i]; fold 1 is held out */
	const size_t L = (size_t)dat->L;
	uint8_t *folds = malloc((size_t)dat->I * L);
	int rc;
	if (!folds) return MCHIP_ERR_ALLOC;
	for (int i = 0; i < dat->I; i++) memset(folds + (size_t)i * L, mask[i] ? 1 : 0, L);
	rc = query_fail(mod, mchip_cv_set_folds(mod->dev, folds, 2), "mc_query_hide", "mchip_cv_set_folds");
	free(folds);
	if (!rc) rc = query_fail(mod, mchip_cv_hold_out(mod->dev, 1), "mc_query_hide", "mchip_cv_hold_out");
	return rc;
}

void mc_query_result_free(mc_query_result *r)
{
	free(r->rows); free(r->q); free(r->logL); free(r->iter); free(r->converged);
	memset(r, 0, sizeof *r);
}

int mc_query_fit(const mc_options *opt, const mc_data *dat, mc_model *mod, const uint8_t *mask, mc_query_result *out)
{
	const int K = mod->K;
	int n = 0, rc;
	memset(out, 0, sizeof *out);
	if (!opt->admixture || opt->eta_constrained) return MCHIP_ERR_UNSUPPORTED;
	for (int i = 0; i < dat->I; i++) n += mask[i] ? 1 : 0;
	if (n < 1) return MCHIP_ERR_INVALID;
	out->n = n;
	out->K = K;
	out->rows = malloc(sizeof(int32_t) * (size_t)n);
	out->q = malloc(sizeof(double) * (size_t)n * K);
	out->logL = malloc(sizeof(double) * (size_t)n);
	out->iter = malloc(sizeof(int32_t) * (size_t)n);
	out->converged = malloc((size_t)n);
	if (!out->rows || !out->q || !out->logL || !out->iter || !out->converged) { mc_query_result_free(out); return MCHIP_ERR_ALLOC; }
	for (int i = 0, r = 0; i < dat->I; i++)
		if (mask[i]) out->rows[r++] = i;
	/* from 1 / K, with the run's tolerances and iteration cap; the context stays as it is, hold-out included */
	rc = query_fail(mod, mchip_fit_q_rows(mod->dev, mod->pindex, out->rows, n, 0, opt->max_iter > 0 ? opt->max_iter : MC_QUERY_MAX_ITER,
					      opt->abs_error, opt->rel_error, out->q, out->logL, out->iter, out->converged),
			"mc_query_fit", "mchip_fit_q_rows");
	if (rc) { mc_query_result_free(out); return rc; }
	for (int r = 0; r < n; r++) {
		if (out->converged[r]) out->n_converged++;
		if (out->iter[r] > out->max_iter) out->max_iter = out->iter[r];
		if (isfinite(out->logL[r])) out->sum_logL += out->logL[r];
		else out->n_failed++;
	}
	return 0;
}
