/*
 * mc_refit.c -- refits of one fitted model to data sets derived from its own (the folds of mc_cv.c, the resampled loci of
 * mc_se.c), each from the estimate as a warm start: what such an analysis does around the part that is its own.
 */
#include "mc_host.h"

#include <stdlib.h>

int mc_refit_check(const mc_refit *h, int rc, const char *what)
{
	if (rc) fprintf(stderr, "ERROR [%s]: %s failed (%d): %s\n", h->where, what, rc, mchip_last_error(h->mod->dev));
	return rc;
}

int mc_refit_begin(mc_refit *h, mc_model *mod, const char *where)
{
	int rc;
	h->where = where;
	h->mod = mod;
	h->keep = *mod;
	h->q = h->p = NULL;
	if ((rc = mc_refit_check(h, mchip_q_length(mod->dev, &h->nq), "mchip_q_length")) ||
	    (rc = mc_refit_check(h, mchip_p_length(mod->dev, &h->np), "mchip_p_length"))) return rc;
	h->q = malloc(sizeof(double) * (size_t)h->nq);
	h->p = malloc(sizeof(double) * (size_t)h->np);
	if (!h->q || !h->p) rc = MCHIP_ERR_ALLOC;
	/* the estimate waits on the host: an accelerated fit uses all three slots, and a derived data set may have another shape */
	else if (!(rc = mc_refit_check(h, mchip_get_q(mod->dev, mod->pindex, h->q), "mchip_get_q")))
		rc = mc_refit_check(h, mchip_get_p(mod->dev, mod->pindex, h->p), "mchip_get_p");
	if (rc) { free(h->q); free(h->p); }
	return rc;
}

int mc_refit_warm_start(mc_refit *h, const double *p)
{
	int rc;
	mc_reset_model_state(h->mod);	/* slot 0, iteration 0, logL = -inf: em() from the warm start */
	if ((rc = mc_refit_check(h, mchip_set_q(h->mod->dev, 0, h->q), "mchip_set_q"))) return rc;
	return mc_refit_check(h, mchip_set_p(h->mod->dev, 0, p ? p : h->p), "mchip_set_p");
}

int mc_refit_fitted(const mc_refit *h, const char *unit, int index, const char *then, int *skipped)
{
	const int fatal = h->mod->fatal;
	*skipped = fatal != MC_FATAL_NONE;
	if (fatal == MC_FATAL_DEVICE) return MCHIP_ERR_HIP;
	if (fatal) fprintf(stderr, "WARNING [%s]: K = %d, %s %d: the fit stopped on %s; %s\n", h->where, h->mod->K, unit, index,
			   fatal == MC_FATAL_NAN ? "a NaN log likelihood" : "a decrease of the log likelihood", then);
	return 0;
}

int mc_refit_end(mc_refit *h, int rc, int rc_base)
{
	mc_model *mod = h->mod;
	mchip_context *dev = mod->dev;
	void *cache = mod->init_cache;	/* (may have been built meanwhile: it belongs to the model) */
	if (!rc_base) rc_base = mc_refit_check(h, mchip_set_q(dev, h->keep.pindex, h->q), "mchip_set_q");
	if (!rc_base) rc_base = mc_refit_check(h, mchip_set_p(dev, h->keep.pindex, h->p), "mchip_set_p");
	*mod = h->keep;			/* logL, n_iter, ring indices, ...: given back as they were */
	mod->dev = dev;
	mod->init_cache = cache;
	free(h->q);
	free(h->p);
	return rc ? rc : rc_base;
}
