/*
 * mc_cli_stages.c -- the two places of the `multiclust` binary where a feature plugs in: pre_fit(), what happens to the data set
 * between the reader and the first fit, and post_fit(), what is made of the best fit of every K.  Both are straight-line blocks that
 * run in the order they stand in.
 *
 * Where a filter of the fileset plugs in: pre_fit() runs them, quality control, then --prune, then --king-cutoff, each on what the one
 * before left; a new one (--keep, --extract, ...) is a unit like mc_ld.c on mc_filter.h and mc_files.h, one more block there, and its
 * option with its refusals in mc_cli_options.c.  --pca is the last block: it reads what the filters left and changes nothing.
 *
 * Where a post-fit analysis plugs in: the serial and the sharded route of mc_main.c differ in who fits which unit and share the rest.
 * Both keep the best fit of a K in a fit_record with its parameters whenever wants_post_fit() says so, and end in post_fit(), which puts
 * the record back into a model once and runs --fst, --resid, --kinship, --cv, --se, --query, --fill.  A new analysis is one more block there with
 * its line of text, its flag in wants_post_fit(), and its option with its refusals (refuse_post_fit) in mc_cli_options.c; one that
 * refits derived data sets builds on mc_refit_* (mc_refit.c).  Nothing in the scheduling of the fits changes for either.
 */
#include "mc_main.h"

#include <string.h>

/* ---- the pre-fit stage: the filters of a fileset, quality control (--mind, --geno, --maf, --hwe), then --prune, then --king-cutoff, each
 * on what the one before left, each with its stdout line -- "of <n>" is what the filter itself saw -- and, with result files on, its
 * lists.  The data set is the filtered one from here on; the lists say what of the fileset it holds.  --pca comes last and only
 * reads that data set: its line and, with result files on, its three files. ---- */
int pre_fit(const mc_cli_options *o, mc_cli_data *d)
{
	int rc;
	if (o->mind || o->geno || o->maf || o->hwe) {
		mchip_progress_note("mc_qc_data");
		if ((rc = mc_qc_data(o, d))) return rc;
		mc_qc_line(stdout, o, d);
		if (o->write_files && (rc = mc_write_qc_lists(o, d))) return rc;
	}
	if (o->prune) {
		const int L_seen = d->L;
		mchip_progress_note("mc_ld_prune_data");
		if ((rc = mc_ld_prune_data(o, d))) return rc;
		printf("LD pruning: kept %d of %d variants (r2 > %g within %d)\n", d->L, L_seen, o->prune_t, o->prune_window);
		if (o->write_files && (rc = mc_write_prune_lists(o, d))) return rc;
	}
	if (o->king) {
		const int I_seen = d->I;
		mchip_progress_note("mc_king_data");
		if ((rc = mc_king_data(o, d))) return rc;
		printf("Relatedness: kept %d of %d individuals (KING-robust kinship > %g: %zu pairs)\n", d->I, I_seen, o->king_t, d->n_king_pairs);
		if (o->write_files && (rc = mc_write_king_lists(o, d))) return rc;
	}
	if (o->pca) {	/* no filter: it reads what is left and changes nothing */
		mc_pca_result r;
		mchip_progress_note("mc_pca_data");
		if ((rc = mc_pca_data(o, d, &r))) return rc;
		mc_pca_line(stdout, &r);
		mc_pca_warn(stderr, o, &r);
		if (o->write_files) rc = mc_write_pca(o, d, &r);
		mc_pca_result_free(&r);
		if (rc) return rc;
	}
	return 0;
}

/* ---- the post-fit stage: --fst, --resid, --kinship, --cv, --se, --query and --fill, in that order, on the best fit of one K ----
 * fit: that fit, with its parameters.  mod: the model that fitted it (its slots are free again; --query needs this one: the
 * hold-out that hides the query individuals is in force on its context), or NULL: a model is created on `device` for the purpose
 * (the workers of a sharded fit are gone by the time the best unit is known).  The fit goes back into the model once: every
 * analysis leaves slot pindex and the host state of the model as it found them (mc_host.h).  Each analysis writes its file
 * (result files on) and adds its stdout line to st->post_lines. */
int wants_post_fit(const mc_cli_options *o, int bootstrap) { return (o->fst || o->resid || o->kinship || o->cv_folds || o->se_replicates || o->query_file || o->fill) && !bootstrap; }

int post_fit(const mc_cli_options *o, const mc_cli_data *d, const mc_data *md, run_state *st, const fit_record *fit, mc_model *mod, int device)
{
	const int K = fit->K;
	mc_model *own = NULL;
	size_t len = 0;
	int rc;
	if (!mod) {
		if ((rc = mc_model_create(&own, &o->em, md, K, device))) return rc;
		mod = own;
	}
	FILE *say = open_memstream(&st->post_lines, &len);
	if (!say) { mc_model_free(own); return MCHIP_ERR_ALLOC; }
	mc_reset_model_state(mod);
	if (!(rc = mc_model_set_q(mod, mod->pindex, fit->q))) rc = mc_model_set_p(mod, mod->pindex, fit->p);
	mod->logL = fit->logL; mod->n_iter = fit->n_iter; mod->converged = fit->converged;
	if (!rc && o->fst) {	/* first: it reads the slot and changes nothing.  With result files on: <stem>.<admix|mix>.K=<K>.fst.txt, .fst.loci.txt */
		mc_divergence_result res;
		mchip_progress_note("divergence of the clusters");
		if (!(rc = mc_divergence(&o->em, md, mod, &res))) {
			mc_divergence_line(say, &res);
			fputc('\n', say);
			if (o->write_files) rc = mc_write_divergence(o, d, &res);
			mc_divergence_result_free(&res);
		}
	}
	if (!rc && o->resid) {	/* next: it reads the slot and the installed data set, before anything installs another.  With result files on:
				 * <stem>.admix.K=<K>.resid.txt, .resid.ind.txt */
		mc_resid_result res;
		mchip_progress_note("residual correlation");
		if (!(rc = mc_residual_correlation(md, mod, &res))) {
			mc_resid_line(say, &res);
			fputc('\n', say);
			if (o->write_files) rc = mc_write_resid(o, &res);
			mc_resid_result_free(&res);
		}
	}
	if (!rc && o->kinship) {	/* like --resid: the slot and the installed data set, before anything installs another.  With result files
					 * on: <stem>.admix.K=<K>.kin0, .kin.ind.txt */
		mc_kinship_result res;
		mchip_progress_note("kinship");
		if (!(rc = mc_kinship(md, mod, o->kinship_t, &res))) {
			mc_kinship_line(say, &res);
			fputc('\n', say);
			if (o->write_files) rc = mc_write_kinship(o, &res);
			mc_kinship_result_free(&res);
		}
	}
	if (!rc && o->cv_folds) {
		mc_cv_result cv;
		mchip_progress_note("cross-validation");
		if (!(rc = mc_cross_validate(&o->em, md, mod, o->cv_folds, o->cv_floor, &cv)))
			fprintf(say, "CV error (K=%d, %d folds): %.10f  [%llu held-out copies, %llu floored]\n", K, o->cv_folds, cv.cv,
				(unsigned long long)cv.n_copies, (unsigned long long)cv.n_floored);
	}
	if (!rc && o->se_replicates) {	/* with result files on: <stem>.<admix|mix>.K=<K>.se.txt */
		const size_t nq = n_q(o, d, K);
		double *mean = malloc(sizeof(double) * nq), *se = malloc(sizeof(double) * nq);
		int32_t *count = malloc(sizeof(int32_t) * nq);
		mc_se_result res;
		mchip_progress_note("bootstrap over loci");
		rc = (mean && se && count) ? mc_locus_bootstrap(&o->em, md, mod, o->se_replicates, o->se_block, mean, se, count, &res) : MCHIP_ERR_ALLOC;
		if (!rc) fprintf(say, "Bootstrap SE (K=%d, %d replicates, block %d): mean %.10f  max %.10f  [%d failed]\n", K, res.n_replicates,
				 res.block, res.mean_se, res.max_se, res.n_failed);
		if (!rc && o->write_files) rc = mc_write_se(o, d, K, fit->q, mean, se, count);
		free(mean); free(se); free(count);
	}
	if (!rc && o->query_file) {	/* with result files on: <stem>.admix.K=<K>.query.txt */
		mc_query_result res;
		memset(&res, 0, sizeof res);
		mchip_progress_note("query fit");
		if (!(rc = mc_query_fit(&o->em, md, mod, st->query_mask, &res)))
			fprintf(say, "Query fit (K=%d): %d individuals, %d converged, %d failed, at most %d iterations, log likelihood %.6f\n", K,
				res.n, res.n_converged, res.n_failed, res.max_iter, res.sum_logL);
		if (!rc && o->write_files) rc = mc_write_query(o, K, res.n, res.rows, res.iter, res.converged, res.logL, res.q);
		mc_query_result_free(&res);
	}
	if (!rc && o->fill) {	/* last: --cv and --se have installed the data set again.  With result files on: <stem>.admix.K=<K>.filled.* */
		uint8_t *filled = malloc((size_t)d->I * d->L * d->ploidy);
		mc_impute_result res;
		mchip_progress_note("filling missing genotypes");
		rc = filled ? mc_impute(&o->em, md, mod, filled, &res) : MCHIP_ERR_ALLOC;
		if (!rc) fprintf(say, "Imputation (K=%d): %llu copies filled in %llu genotypes, %llu left missing, mean confidence %.6f\n", K,
				 (unsigned long long)res.n_filled, (unsigned long long)res.n_genotypes, (unsigned long long)res.n_left, res.mean_conf);
		if (!rc && o->write_files) rc = mc_write_filled(o, d, K, filled);
		free(filled);
	}
	fclose(say);
	mc_model_free(own);
	return rc;
}
