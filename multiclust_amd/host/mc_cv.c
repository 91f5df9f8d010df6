/*
 * mc_cv.c -- K-fold cross-validation of one fitted admixture model (an extension: the reference chooses K by AIC / BIC and the
 * parametric bootstrap only).  The genotypes are split into folds on the device, each fold in turn is hidden from a fit that
 * starts from the full-data estimate, and the fit is scored on the copies it did not see (include/multiclust_hip.h, mchip_cv_*).
 */
#include "mc_host.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

static int cv_fail(mc_model *mod, int rc, const char *what)
{
	if (rc) fprintf(stderr, "ERROR [mc_cv.c::mc_cross_validate]: %s failed (%d): %s\n", what, rc, mchip_last_error(mod->dev));
	return rc;
}

double mc_cv_default_floor(const mc_data *dat) { return 1.0 / ((double)dat->I * dat->ploidy + 1.0); }

int mc_cross_validate(const mc_options *opt, const mc_data *dat, mc_model *mod, int n_folds, double floor, mc_cv_result *out)
{
	const int K = mod->K, mle = mod->pindex;
	const mc_model keep = *mod;	/* logL, n_iter, ring indices, ...: given back as they were */
	int nq = 0, np = 0, rc;
	double *q = NULL, *p = NULL;
	mc_rng rng;
	uint32_t window[31];
	memset(out, 0, sizeof *out);
	out->n_folds = n_folds;
	out->fatal_fold = -1;
	out->cv = NAN;
	if (n_folds < 2 || n_folds > MC_CV_MAX_FOLDS || !opt->admixture) return MCHIP_ERR_INVALID;
	if (!(floor > 0)) floor = mc_cv_default_floor(dat);
	out->floor = floor;
	if ((rc = cv_fail(mod, mchip_q_length(mod->dev, &nq), "mchip_q_length")) || (rc = cv_fail(mod, mchip_p_length(mod->dev, &np), "mchip_p_length")))
		return rc;
	q = malloc(sizeof(double) * (size_t)nq);
	p = malloc(sizeof(double) * (size_t)np);
	if (!q || !p) { free(q); free(p); return MCHIP_ERR_ALLOC; }
	/* the full-data estimate: an accelerated fit uses all three slots, so it waits on the host */
	if ((rc = cv_fail(mod, mchip_get_q(mod->dev, mle, q), "mchip_get_q")) || (rc = cv_fail(mod, mchip_get_p(mod->dev, mle, p), "mchip_get_p")))
		goto DONE;
	/* the folds: a stream of their own from the run's seed, the same for every K (the K are compared on one partition), and
	 * the run's main rand() stream stays where it is */
	mc_srand(&rng, opt->seed);
	for (int t = 0; t < 31; t++) window[t] = (uint32_t)rng.r[(rng.f + t) % 31];
	if ((rc = cv_fail(mod, mchip_cv_draw_folds(mod->dev, window, n_folds), "mchip_cv_draw_folds"))) goto DONE;
	for (int f = 0; f < n_folds; f++) {
		double s = 0;
		uint64_t n = 0, nf = 0;
		if ((rc = cv_fail(mod, mchip_cv_hold_out(mod->dev, f), "mchip_cv_hold_out"))) break;
		mc_reset_model_state(mod);	/* slot 0, iteration 0, logL = -inf: em() from the warm start */
		if ((rc = cv_fail(mod, mchip_set_q(mod->dev, 0, q), "mchip_set_q")) || (rc = cv_fail(mod, mchip_set_p(mod->dev, 0, p), "mchip_set_p")))
			break;
		mc_em(opt, dat, mod);
		if (mod->fatal == MC_FATAL_DEVICE) { rc = MCHIP_ERR_HIP; break; }
		out->fold_iter[f] = mod->n_iter;
		if (mod->fatal) {	/* NaN or a decrease of the log likelihood: this K has no CV error, the run goes on */
			fprintf(stderr, "WARNING [mc_cv.c::mc_cross_validate]: K = %d, fold %d: the fit stopped on %s; no cross-validation error for this K\n",
				K, f, mod->fatal == MC_FATAL_NAN ? "a NaN log likelihood" : "a decrease of the log likelihood");
			if (out->fatal_fold < 0) out->fatal_fold = f;
			out->fold_sum_log[f] = NAN;
			continue;
		}
		if ((rc = cv_fail(mod, mchip_cv_heldout_loglik(mod->dev, mod->pindex, floor, &s, &n, &nf), "mchip_cv_heldout_loglik"))) break;
		out->fold_sum_log[f] = s;
		out->fold_copies[f] = n;
		out->fold_floored[f] = nf;
		out->sum_log += s;
		out->n_copies += n;
		out->n_floored += nf;
	}
	{	/* the full data set and the estimate again, whatever happened */
		int rc2 = cv_fail(mod, mchip_cv_hold_out(mod->dev, -1), "mchip_cv_hold_out");
		if (!rc2) rc2 = cv_fail(mod, mchip_set_q(mod->dev, mle, q), "mchip_set_q");
		if (!rc2) rc2 = cv_fail(mod, mchip_set_p(mod->dev, mle, p), "mchip_set_p");
		if (!rc) rc = rc2;
	}
	{
		mchip_context *dev = mod->dev;
		void *cache = mod->init_cache;	/* (may have been built meanwhile: it belongs to the model) */
		*mod = keep;
		mod->dev = dev;
		mod->init_cache = cache;
	}
	if (!rc && out->fatal_fold < 0 && out->n_copies) out->cv = -out->sum_log / (double)out->n_copies;
	if (out->fatal_fold >= 0) out->sum_log = NAN;
DONE:
	free(q);
	free(p);
	return rc;
}
