/*
 * mc_cv.c -- K-fold cross-validation of one fitted admixture model (an extension: the reference chooses K by AIC / BIC and the
 * parametric bootstrap only).  The genotypes are split into folds on the device, each fold in turn is hidden from a fit that
 * starts from the full-data estimate, and the fit is scored on the copies it did not see (include/multiclust_hip.h, mchip_cv_*).
 */
#include "mc_host.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

double mc_cv_default_floor(const mc_data *dat) { return 1.0 / ((double)dat->I * dat->ploidy + 1.0); }

int mc_cross_validate(const mc_options *opt, const mc_data *dat, mc_model *mod, int n_folds, double floor, mc_cv_result *out)
{
	mc_refit est;
	int rc, skipped;
	mc_rng rng;
	uint32_t window[31];
	memset(out, 0, sizeof *out);
	out->n_folds = n_folds;
	out->fatal_fold = -1;
	out->cv = NAN;
	if (n_folds < 2 || n_folds > MC_CV_MAX_FOLDS || !opt->admixture) return MCHIP_ERR_INVALID;
	if (!(floor > 0)) floor = mc_cv_default_floor(dat);
	out->floor = floor;
	if ((rc = mc_refit_begin(&est, mod, "mc_cv.c::mc_cross_validate"))) return rc;
	/* the folds: a stream of their own from the run's seed, the same for every K (the K are compared on one partition), and
	 * the run's main rand() stream stays where it is */
	mc_srand(&rng, opt->seed);
	for (int t = 0; t < 31; t++) window[t] = (uint32_t)rng.r[(rng.f + t) % 31];
	if ((rc = mc_refit_check(&est, mchip_cv_draw_folds(mod->dev, window, n_folds), "mchip_cv_draw_folds")))
		return mc_refit_end(&est, rc, rc);	/* (nothing is held out yet, and the estimate is where it was) */
	for (int f = 0; f < n_folds; f++) {
		double s = 0;
		uint64_t n = 0, nf = 0;
		if ((rc = mc_refit_check(&est, mchip_cv_hold_out(mod->dev, f), "mchip_cv_hold_out")) || (rc = mc_refit_warm_start(&est, NULL))) break;
		mc_em(opt, dat, mod);
		if ((rc = mc_refit_fitted(&est, "fold", f, "no cross-validation error for this K", &skipped))) break;
		out->fold_iter[f] = mod->n_iter;
		if (skipped) {	/* this K has no CV error, the run goes on */
			if (out->fatal_fold < 0) out->fatal_fold = f;
			out->fold_sum_log[f] = NAN;
			continue;
		}
		if ((rc = mc_refit_check(&est, mchip_cv_heldout_loglik(mod->dev, mod->pindex, floor, &s, &n, &nf), "mchip_cv_heldout_loglik"))) break;
		out->fold_sum_log[f] = s;
		out->fold_copies[f] = n;
		out->fold_floored[f] = nf;
		out->sum_log += s;
		out->n_copies += n;
		out->n_floored += nf;
	}
	/* the full data set and the estimate again, whatever happened */
	rc = mc_refit_end(&est, rc, mc_refit_check(&est, mchip_cv_hold_out(mod->dev, -1), "mchip_cv_hold_out"));
	if (!rc && out->fatal_fold < 0 && out->n_copies) out->cv = -out->sum_log / (double)out->n_copies;
	if (out->fatal_fold >= 0) out->sum_log = NAN;
	return rc;
}
