/*
 * mc_se.c -- standard errors of the mixing proportions by a non-parametric bootstrap over loci (an extension: the reference's
 * bootstrap is parametric and tests K - 1 against K; it gives no standard errors).  Loci, or blocks of neighbouring loci, are
 * drawn with replacement, the selection is installed on the device (include/multiclust_hip.h, mchip_resample_loci), the model is
 * refitted from the full-data estimate, and the spread of every q_ik over the replicates is reported.
 */
#include "mc_host.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

/* Welford's update of one entry, each operation rounded on its own (a fused multiply-add would change M2's bits from one build to
 * the next; equal values must give M2 = 0 exactly) */
#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))
#endif
static void welford(double x, double *mean, double *m2, int32_t *n)
{
	const double d = x - *mean;
	*n += 1;
	*mean += d / *n;
	*m2 += d * (x - *mean);
}

int mc_se_list_capacity(int L, int block)
{
	if (L < 1 || block < 1 || block > L) return 0;
	const long long nb = ((long long)L + block - 1) / block;
	return nb * block > 2147483647LL ? 0 : (int)(nb * block);
}

int mc_se_draw_lists(mc_rng *rng, int L, int block, int n_lists, int32_t *src, int32_t *len)
{
	const int cap = mc_se_list_capacity(L, block);
	if (!rng || !src || !len || !cap || n_lists < 0) return MCHIP_ERR_INVALID;
	const int nb = (L + block - 1) / block;
	for (int r = 0; r < n_lists; r++) {
		int32_t *list = src + (size_t)r * cap;
		int n = 0;
		for (int d = 0; d < nb; d++) {
			const int b = mc_rand(rng) % nb;
			const int end = (b + 1) * block < L ? (b + 1) * block : L;	/* (block <= L: no overflow of b * block past L + block) */
			for (int l = b * block; l < end; l++) list[n++] = l;
		}
		len[r] = n;
	}
	return 0;
}

static int set_model(const mc_options *opt, mc_model *mod)
{
	return mchip_set_model(mod->dev, mod->K, opt->admixture, opt->eta_constrained, opt->do_projection, opt->eta_lower_bound,
			       opt->p_lower_bound, opt->accel_scheme ? opt->q : 0);
}

int mc_locus_bootstrap(const mc_options *opt, const mc_data *dat, mc_model *mod, int n_replicates, int block, double *mean, double *se,
		       int32_t *count, mc_se_result *out)
{
	const int K = mod->K, L = dat->L;
	mc_refit est;
	int rc, rc2, skipped, T = 0;
	double *x = NULL, *m2 = NULL;
	int32_t *src = NULL, *ua2 = NULL, *toff = NULL;
	mc_rng rng;
	if (out) memset(out, 0, sizeof *out);
	if (!mean || !se || !count || !out) return MCHIP_ERR_INVALID;
	out->n_replicates = n_replicates;
	out->block = block;
	out->mean_se = out->max_se = NAN;
	if (n_replicates < 2 || n_replicates > MC_SE_MAX_REPLICATES || block < 1 || block > L) return MCHIP_ERR_INVALID;
	const int cap = mc_se_list_capacity(L, block);
	if (!cap) return MCHIP_ERR_INVALID;
	/* the full-data estimate waits on the host: the replicates have other shapes */
	if ((rc = mc_refit_begin(&est, mod, "mc_se.c::mc_locus_bootstrap"))) return rc;
	const int nq = est.nq;
	const double *p = est.p;
	x = malloc(sizeof(double) * (size_t)nq);
	m2 = calloc((size_t)nq, sizeof(double));
	src = malloc(sizeof(int32_t) * (size_t)cap);
	ua2 = malloc(sizeof(int32_t) * (size_t)cap);
	toff = malloc(sizeof(int32_t) * ((size_t)L + 1));
	if (!x || !m2 || !src || !ua2 || !toff) { rc = mc_refit_end(&est, MCHIP_ERR_ALLOC, MCHIP_ERR_ALLOC); goto DONE; }	/* (nothing installed yet) */
	for (int e = 0; e < nq; e++) { mean[e] = 0; se[e] = NAN; count[e] = 0; }
	for (int l = 0; l < L; l++) { toff[l] = T; T += dat->uniquealleles[l]; }
	toff[L] = T;
	/* the lists: a stream of their own from the run's seed, the same for every K; the run's main rand() stream stays where it is */
	mc_srand(&rng, opt->seed);
	for (int r = 0; r < n_replicates; r++) {
		int32_t L2 = 0;
		int T2 = 0;
		double *p2;
		mc_data rep = *dat;
		mc_se_draw_lists(&rng, L, block, 1, src, &L2);
		if ((rc = mc_refit_check(&est, mchip_resample_loci(mod->dev, src, L2), "mchip_resample_loci"))) break;
		if ((rc = mc_refit_check(&est, set_model(opt, mod), "mchip_set_model"))) break;
		for (int j = 0; j < L2; j++) T2 += (ua2[j] = dat->uniquealleles[src[j]]);
		if (!(p2 = malloc(sizeof(double) * (size_t)K * (size_t)T2))) { rc = MCHIP_ERR_ALLOC; break; }
		for (int k = 0; k < K; k++) {	/* the columns of the estimate follow their loci */
			double *to = p2 + (size_t)k * T2;
			for (int j = 0; j < L2; j++) {
				memcpy(to, p + (size_t)k * T + toff[src[j]], sizeof(double) * (size_t)ua2[j]);
				to += ua2[j];
			}
		}
		rc = mc_refit_warm_start(&est, p2);
		free(p2);
		if (rc) break;
		rep.L = L2;
		rep.uniquealleles = ua2;
		rep.geno = rep.init_geno = rep.bed = NULL;
		rep.bed_record_bytes = 0;
		rep.lazy = NULL;
		mc_em(opt, &rep, mod);
		if ((rc = mc_refit_fitted(&est, "replicate", r, "replicate skipped", &skipped))) break;
		out->n_iter += (uint64_t)mod->n_iter;
		if (skipped) {	/* the replicate does not count, the run goes on */
			out->n_failed++;
			continue;
		}
		if ((rc = mc_refit_check(&est, mc_model_get_q(mod, mod->pindex, x), "mchip_get_q"))) break;
		for (int e = 0; e < nq; e++) {	/* Welford; a NaN entry (an individual without an observed copy in this replicate) does not count */
			if (x[e] == x[e]) welford(x[e], &mean[e], &m2[e], &count[e]);
		}
	}
	/* the base and the estimate again, whatever happened */
	rc2 = mc_refit_check(&est, mchip_resample_loci(mod->dev, NULL, 0), "mchip_resample_loci");
	rc = mc_refit_end(&est, rc, rc2 ? rc2 : mc_refit_check(&est, set_model(opt, mod), "mchip_set_model"));
	if (!rc) {
		double sum = 0;
		int n = 0;
		for (int e = 0; e < nq; e++) {
			if (count[e] < 1) mean[e] = NAN;
			if (count[e] < 2) continue;
			se[e] = sqrt(m2[e] / (count[e] - 1));
			sum += se[e];
			if (!n || se[e] > out->max_se) out->max_se = se[e];
			n++;
		}
		if (n) out->mean_se = sum / n;
	}
DONE:
	free(x); free(m2); free(src); free(ua2); free(toff);
	return rc;
}
