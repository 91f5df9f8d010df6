/*
 * mc_main.c -- the `multiclust` command line on top of the MI355X EM hot path: the fits and their bookkeeping.
 *
 * Keeps the reference's observable surface: the K loop of estimate_model (reference multiclust.c:365-452), the initialisation loop and
 * bookkeeping of maximize_likelihood (471-656), the per-initialisation stdout line (618-627), print_model_state (718-793),
 * run_bootstrap (675-708) and the -w repetition summary (201-347).  main() is the sequence of the run's stages; the options are
 * mc_cli_options.c's, what runs before the first fit and after the best fit of a K is mc_cli_stages.c's.
 *
 * The best fit of a K is kept in a fit_record; best_needs() says what of it, new_maximum() takes it when it improved on the K before
 * (H0 estimate, result files, -A), post_fit() runs the analyses on it.  maximize_likelihood() fits the initialisations of a K one after
 * the other on one model.  --gpus <n> and --streams <m> give a run n * m workers (host thread, context and stream each, mc_cli_workers.c):
 * maximize_likelihood_sharded() hands each the units u = x, x + n * m, ..., every one started from the serial program's rand() position
 * by jump-ahead, exchanges the per-unit result table once and replays the serial bookkeeping in unit order (admixture model, fixed
 * number of initialisations); run_bootstrap_sharded() hands out whole bootstrap replicates (-b) the same way, for both models.
 */
#include "mc_main.h"

#include <stdint.h>
#include <string.h>

static const char *accel_abbrev(const mc_cli_options *o, char *buf)
{
	static const char *ab[] = { "EM", "S1", "S2", "S3", "QN" };
	if (o->em.accel_scheme >= MC_QN) { sprintf(buf, "Q%d", o->em.q); return buf; }	/* multiclust.c:828 */
	return ab[o->em.accel_scheme];
}

/* fills the record from the model that just fitted initialisation `unit`; the parameters only when asked for (a record is used for
 * one K: its buffers are allocated on first need and written over afterwards) */
static int record_take(fit_record *r, const mc_cli_options *o, const mc_cli_data *d, mc_model *mod, int unit, int params, int sik)
{
	int rc;
	if (params && !r->q) { r->q = malloc(sizeof(double) * n_q(o, d, mod->K)); r->p = malloc(sizeof(double) * (size_t)mod->K * d->T); }
	if (sik && !r->sik) r->sik = malloc(sizeof(double) * (size_t)d->I * mod->K);
	if ((params && (!r->q || !r->p)) || (sik && !r->sik)) return MCHIP_ERR_ALLOC;
	if (params && ((rc = mc_model_get_q(mod, mod->pindex, r->q)) || (rc = mc_model_get_p(mod, mod->pindex, r->p)))) return rc;
	if (sik && (rc = mc_model_get_expected_counts(mod, r->sik))) return rc;
	r->K = mod->K; r->unit = unit; r->logL = mod->logL; r->n_iter = mod->n_iter; r->converged = mod->converged;
	return 0;
}

static void record_free(fit_record *r)
{
	free(r->q); free(r->p); free(r->sik);
	*r = (fit_record)FIT_RECORD_NONE;
}

static void print_model_state(const mc_cli_options *o, const mc_cli_data *d, const run_state *st, int K, int diff, int newline)
{
	char ab[16];
	(void)d;
	if (o->compact) {	/* multiclust.c:720-746 */
		fprintf(st->out, "%s %s %s %d %u %e %e %e %e %f %f %f ", o->filename, accel_abbrev(o, ab), o->em.admixture ? "admix" : "mix", K,
		       o->em.seed, o->em.eta_lower_bound, o->em.p_lower_bound, o->em.abs_error, o->em.rel_error,
		       st->sum.max_logL, st->sum.aic, st->sum.bic);
		if (o->afile) fprintf(st->out, "%f ", st->arand); else fprintf(st->out, "ND ");	/* multiclust.c:728-731 */
		fprintf(st->out, "%s %02d:%02d:%02d %d %d %d %d", st->sum.ever_converged ? "converged" : "not", diff / 3600, (diff % 3600) / 60,
		       diff % 60, st->sum.n_total_iter, st->sum.n_init, st->sum.n_maxll_init, st->sum.n_maxll_times);
		if (o->target_ll) fprintf(st->out, " %f %d %d", o->desired_ll, st->n_targetll_init, st->n_targetll_times);
		if (st->time_stop) fprintf(st->out, " time");
		if (newline) fprintf(st->out, "\n");
	} else {		/* multiclust.c:748-792 */
		fprintf(st->out, "Dataset: %s\nMethod/Model: %s, %s, K=%d\n", o->filename, accel_abbrev(o, ab), o->em.admixture ? "admix" : "mix", K);
		fprintf(st->out, "Convergence: ae=%e, re=%e\nBounds: e=%e, p=%e\n", o->em.abs_error, o->em.rel_error, o->em.eta_lower_bound, o->em.p_lower_bound);
		fprintf(st->out, "Total number of iterations: %d\nTotal time: %02d:%02d:%02d\n", st->sum.n_total_iter, diff / 3600, (diff % 3600) / 60, diff % 60);
		fprintf(st->out, "Iteration of max log likelihood: %d of %d\nNumber of times reach max log likelihood: %d\n", st->sum.n_maxll_init, st->sum.n_init, st->sum.n_maxll_times);
		fprintf(st->out, "Maximum log likelihood: %f\nAIC: %f\nBIC: %f\nConverged: %s\n", st->sum.max_logL, st->sum.aic, st->sum.bic, st->sum.ever_converged ? "yes" : "no");
		if (st->time_stop) fprintf(st->out, "WARNING: Fitting stopped because ran out of time\n");
	}
}

/* initialize_model (rnd_init.c:54-89).  With -P and -Q the admixture model starts from the parameters in those files instead
 * of a random partition (rnd_init.c:74-76): read_qfile (read_file.c:880-922: I*K numbers in i, k order, or K with -c) and
 * read_pfile (924-959: "assumes biallelic locus": L*K numbers p[k][l][0] in l, k order, p[k][l][1] = 1 - p[k][l][0], any further
 * allele of a locus keeps what the slot held).  No rand() is consumed, so every initialisation starts from the same point. */
static int cli_initialize(const mc_cli_options *o, const mc_cli_data *d, const mc_data *md, mc_model *mod, mc_rng *rng)
{
	if (!(o->em.admixture && o->pfile && o->qfile)) return mc_initialize_model(&o->em, md, mod, rng);
	const int K = mod->K, nq = o->em.eta_constrained ? K : d->I * K;
	double *q = malloc(sizeof(double) * (size_t)nq), *p = malloc(sizeof(double) * (size_t)K * d->T);
	FILE *fq = fopen(o->qfile, "r"), *fp = fopen(o->pfile, "r");
	int rc = 0;
	mod->n_iter = 0;
	mod->logL = -INFINITY;
	mod->converged = 0;
	if (o->em.accel_scheme) mod->pindex = mod->tindex = mod->findex = 0;
	if (!q || !p) rc = MCHIP_ERR_ALLOC;
	if (!rc && (!fq || !fp)) { fprintf(stderr, "ERROR [" MC_FRONT_END "::cli_initialize]: cannot open '%s'\n", fq ? o->pfile : o->qfile); rc = MC_EXIT_FILE_OPEN_ERROR; }
	for (int x = 0; !rc && x < nq; x++)
		if (fscanf(fq, "%lf", &q[x]) != 1) { fprintf(stderr, "ERROR [" MC_FRONT_END "::cli_initialize]: format of '%s'\n", o->qfile); rc = MC_EXIT_FILE_FORMAT_ERROR; }
	if (!rc) rc = mc_model_get_p(mod, mod->tindex, p);
	for (int l = 0; !rc && l < d->L; l++)
		for (int k = 0; !rc && k < K; k++) {
			double v;
			if (fscanf(fp, "%lf", &v) != 1) { fprintf(stderr, "ERROR [" MC_FRONT_END "::cli_initialize]: format of '%s'\n", o->pfile); rc = MC_EXIT_FILE_FORMAT_ERROR; break; }
			/* (the reference stores 1 - v in the locus's second allele slot whether or not there is one, read_file.c:950: a
			 * monomorphic locus makes it write past its allocation; refused here) */
			if (d->uniquealleles[l] < 2) { fprintf(stderr, "ERROR [" MC_FRONT_END "::cli_initialize]: -P needs two alleles at every locus\n"); rc = MC_EXIT_INVALID_USER_SETUP; break; }
			p[(size_t)k * d->T + d->toff[l]] = v;
			p[(size_t)k * d->T + d->toff[l] + 1] = 1 - v;
		}
	if (!rc) rc = mc_model_set_q(mod, mod->tindex, q);
	if (!rc) rc = mc_model_set_p(mod, mod->tindex, p);
	if (fq) fclose(fq);
	if (fp) fclose(fp);
	free(q); free(p);
	return rc;
}

/* the per-initialisation stdout line (multiclust.c:618-627) */
static void print_unit_line(const mc_cli_options *o, const run_state *st, int K, const mc_unit_result *r, int bootstrap)
{
	if (bootstrap || o->em.verbosity <= MC_QUIET || !o->write_files) return;
	fprintf(st->out, "K = %d, initialization = %d: %f (%s) in %3d iterations, %02d:%02d:%02d (%f; %d), seed: %u\n", K, r->unit, r->logL,
	       r->converged ? "converged" : "not converged", r->n_iter, (int)(r->seconds_run / 3600),
	       (int)((((int)r->seconds_run) % 3600) / 60), ((int)r->seconds_run) % 60, st->sum.max_logL, st->sum.n_maxll_times, o->em.seed);
}

/* what new_maximum() below reads of the fit: the parameters (and the expected counts, which only the partition needs) */
static int max_wants_partition(const mc_cli_options *o, int bootstrap) { return (!bootstrap && o->write_files) || (o->afile && !o->write_files); }
static int max_wants_h0(const mc_cli_options *o, const run_state *st, int K, int bootstrap) { return !bootstrap && o->n_bootstrap && K == st->null_K; }

/* what the record of a K's best fit must hold, for the serial loop and for the workers of a sharded fit: its parameters for the
 * post-fit stage, and for new_maximum() where the fit may be the maximum so far (the serial loop knows whether; a worker does
 * not, so it may be); the expected counts for new_maximum()'s partition alone.  The scalars are recorded in any case. */
typedef struct record_needs { int params, sik; } record_needs;
static record_needs best_needs(const mc_cli_options *o, const run_state *st, int K, int bootstrap, int may_be_max)
{
	const int sik = may_be_max && max_wants_partition(o, bootstrap);
	return (record_needs){ wants_post_fit(o, bootstrap) || sik || (may_be_max && max_wants_h0(o, st, K, bootstrap)), sik };
}

/* A fit improved on the maximum so far (st->sum holds it already): the serial loop comes here at every improvement, the sharded
 * path once per K for its best unit, the last improvement of the serial loop */
static int new_maximum(const mc_cli_options *o, const mc_cli_data *d, run_state *st, const fit_record *fit, int bootstrap)
{
	const int K = fit->K;
	int rc = 0;
	if (max_wants_h0(o, st, K, bootstrap)) {	/* multiclust.c:562-581 */
		const size_t nq = n_q(o, d, K), np = (size_t)K * d->T;
		record_free(&st->h0);
		st->h0 = *fit;			/* a copy of its own: the caller's record moves on */
		st->h0.sik = NULL;
		st->h0.q = malloc(sizeof(double) * nq);
		st->h0.p = malloc(sizeof(double) * np);
		if (!st->h0.q || !st->h0.p) return MCHIP_ERR_ALLOC;
		memcpy(st->h0.q, fit->q, sizeof(double) * nq);
		memcpy(st->h0.p, fit->p, sizeof(double) * np);
	}
	if (max_wants_partition(o, bootstrap)) {	/* multiclust.c:584-600; nothing is written with -w, but -A wants the partition */
		const mc_fit_view fv = { K, fit->converged, fit->logL, st->sum.aic, st->sum.bic, fit->q, fit->p, fit->sik };
		int *count_K = malloc(sizeof(int) * (size_t)K);
		if (!count_K) return MCHIP_ERR_ALLOC;
		mc_partition(d, &fv, st->I_K, count_K);
		if (o->write_files) rc = mc_write_results(o, d, &fv, count_K);
		free(count_K);
	}
	if (!rc && o->afile) {		/* multiclust.c:602-612 */
		/* (a bootstrap fit with result files on is not partitioned in the reference: dat->I_K is then the partition
		 * of an earlier fit, possibly with a cluster index this K does not have -- it indexes past its table there;
		 * the index is left as it was here) */
		int fits = 1;
		for (int x = 0; x < d->I; x++) if (st->I_K[x] >= K) fits = 0;
		if (fits) st->arand = mc_adjusted_rand(d->I, st->pK, K, st->partition_from_file, st->I_K);
	}
	return rc;
}

/* a K's fits begin.  estimate_model resets the maximum per call, not per K (multiclust.c:377), and nothing resets AIC / BIC: a K
 * whose fits do not beat the previous K's maximum reports that K's figures (and writes no files) */
static void summary_begin_K(run_state *st)
{
	const double max_logL_keep = st->sum.max_logL, aic_keep = st->sum.aic, bic_keep = st->sum.bic;
	mc_summary_reset(&st->sum);
	st->sum.max_logL = max_logL_keep;
	if (max_logL_keep > -INFINITY) { st->sum.aic = aic_keep; st->sum.bic = bic_keep; }
	st->time_stop = 0;
}

/* maximize_likelihood (multiclust.c:471-656) for one K */
static int maximize_likelihood(const mc_cli_options *o, const mc_cli_data *d, const mc_data *md, mc_model *mod, run_state *st, int bootstrap)
{
	const int K = mod->K, npar = mc_no_parameters(&o->em, md, K);
	/* the best fit of THIS K: what the post-fit stage sees.  The files follow the maximum over the K so far, and a fit that
	 * improves on that maximum is the best of this K too, so new_maximum() reads the same record */
	const int post = wants_post_fit(o, bootstrap);
	fit_record best = FIT_RECORD_NONE;
	int rc = 0;
	summary_begin_K(st);
	st->n_targetll_times = 0;
	mod->start = clock();
	const clock_t start = mod->start;
	for (int i = 0; o->target_revisit || o->target_ll || o->em.n_seconds || i < o->n_init; i++) {
		const int delta_keep = mod->delta_index;
		mc_unit_result r;
		mc_reset_model_state(mod);
		mod->delta_index = delta_keep;
		mod->start = start;			/* the time limit spans all initialisations (multiclust.c:488) */
		mchip_progress_note("maximize_likelihood: initialisation");
		if ((rc = cli_initialize(o, d, md, mod, &st->rng))) goto DONE;
		mchip_progress_note("maximize_likelihood: mc_em");
		mc_em(&o->em, md, mod);
		mchip_progress_note("maximize_likelihood: bookkeeping and result files");
		if (mod->fatal == MC_FATAL_DEVICE) { rc = MCHIP_ERR_HIP; goto DONE; }
		if (mod->fatal) exit(0);		/* the reference's reaction to NaN / decreasing logL (em_alg.c:106-120) */
		mc_unit_result_from_model(&r, i, mod);
		const int new_max = mod->logL > st->sum.max_logL;
		mc_summary_add(&o->em, &st->sum, &r, npar, d->I);
		if (mod->logL > best.logL) {
			const record_needs need = best_needs(o, st, K, bootstrap, new_max);
			if ((rc = record_take(&best, o, d, mod, i, need.params, need.sik))) goto DONE;
		}
		if (new_max && (rc = new_maximum(o, d, st, &best, bootstrap))) goto DONE;
		print_unit_line(o, st, K, &r, bootstrap);
		if (K == 1) break;
		if (mod->time_stop) { st->time_stop = 1; break; }
		if (o->target_revisit && st->sum.n_maxll_times >= o->target_revisit) break;
		if (o->target_ll) {		/* multiclust.c:643-652 */
			const int hit = mod->logL > o->desired_ll || (o->em.abs_error && fabs(o->desired_ll - mod->logL) <= o->em.abs_error);
			if (hit) {
				if (!st->n_targetll_times) st->n_targetll_init = st->sum.n_init;
				st->n_targetll_times++;
				if (!o->target_revisit || o->target_revisit <= st->n_targetll_times) break;
			}
		}
	}
	if (post && best.q) rc = post_fit(o, d, md, st, &best, mod, o->device);
DONE:
	record_free(&best);
	return rc;
}

/* ---- initialisations sharded over several GPUs of the node ---- */
typedef struct shard_worker {
	const mc_cli_options *o;
	const mc_cli_data *d;
	const mc_data *md;
	int K, index, n_dev, n_units;
	record_needs need;		/* what the record of this worker's best unit holds */
	const mc_simulation *sim;	/* bootstrap replicate generated on the device, or NULL */
	const mc_rng *starts;		/* [n_units + 1]: the serial stream's state at the start of every unit (and after the last) */
	mc_unit_result *res;		/* [n_units], shared: worker d writes rows u = d, d + n_dev, ... */
	fit_record best;		/* this worker's best unit */
} shard_worker;

static void *shard_main(void *arg)
{
	shard_worker *w = arg;
	mc_model *mod = NULL;
	int rc;
	w->best = (fit_record)FIT_RECORD_NONE;
	const int device = worker_device(w->o, w->index);
	if ((rc = w->sim ? mc_model_create_simulated(&mod, &w->o->em, w->md, w->K, device, w->sim)
			 : mc_model_create(&mod, &w->o->em, w->md, w->K, device))) return (void *)(intptr_t)rc;
	const clock_t start = clock();
	/* unit u starts where the serial stream stands after u initialisations (w->starts, walked once by the caller) */
	for (int u = w->index; u < w->n_units; u += w->n_dev) {
		mc_rng rng = w->starts[u];
		mc_reset_model_state(mod);
		mod->start = start;
		if ((rc = mc_initialize_model(&w->o->em, w->md, mod, &rng))) break;
		mc_em(&w->o->em, w->md, mod);
		if (mod->fatal == MC_FATAL_DEVICE) { rc = MCHIP_ERR_HIP; break; }
		mc_unit_result_from_model(&w->res[u], u, mod);
		if (mod->fatal) break;
		/* strict: the earliest of equal units wins, as in the serial loop */
		if (mod->logL > w->best.logL && (rc = record_take(&w->best, w->o, w->d, mod, u, w->need.params, w->need.sik))) break;
	}
	mc_model_free(mod);
	return (void *)(intptr_t)rc;
}

/* a unit's result as a row of the exchange table (the field behind these counts how often the unit was fitted) */
#define RES_FIELDS 9
static void pack_result(double *row, int u, const void *res)
{
	const mc_unit_result *r = (const mc_unit_result *)res + u;
	row[0] = r->logL; row[1] = r->converged; row[2] = r->n_iter; row[3] = r->time_stop;
	row[4] = r->iter_stop; row[5] = r->pindex; row[6] = r->fatal; row[7] = r->seconds_run;
}
static void unpack_result(const double *row, int unit, mc_unit_result *r)
{
	*r = (mc_unit_result){ unit, row[0], (int)row[1], (int)row[2], (int)row[3], (int)row[4], (int)row[5], (int)row[6], row[7] };
}

static int maximize_likelihood_sharded(const mc_cli_options *o, const mc_cli_data *d, const mc_data *md, int K, run_state *st, int bootstrap,
				       const mc_simulation *sim)
{
	const int n_dev = n_workers(o), n_units = (K == 1) ? 1 : o->n_init;
	const int npar = mc_no_parameters(&o->em, md, K), post = wants_post_fit(o, bootstrap);
	shard_worker *w = calloc((size_t)n_dev, sizeof *w);
	mc_unit_result *res = calloc((size_t)n_units, sizeof *res);
	double *tab = NULL;
	int rc = 0;
	mc_rng *starts = calloc((size_t)n_units + 1, sizeof *starts);
	if (!w || !res || !starts) { rc = MCHIP_ERR_ALLOC; goto DONE; }
	{	/* where each unit starts in the rand() stream: one walk (a jump per unit for the random allele partition, the host-side
		 * replay of the center draws for Rand-EM), instead of every worker replaying the units before its own */
		mc_model walker;
		memset(&walker, 0, sizeof walker);
		walker.K = K;
		rc = mc_unit_starts(&o->em, md, &walker, &st->rng, n_units, starts);
		mc_init_cache_free(&walker);
		if (rc) goto DONE;
	}
	for (int x = 0; x < n_dev; x++)
		w[x] = (shard_worker){ o, d, md, K, x, n_dev, n_units, best_needs(o, st, K, bootstrap, 1), sim, starts, res, FIT_RECORD_NONE };
	if ((rc = mc_run_workers(n_dev, shard_main, w, sizeof *w))) goto DONE;
	st->rng = starts[n_units];	/* where the serial stream stands after these initialisations */
	if ((rc = mc_exchange_rows(o, st, n_units, RES_FIELDS, pack_result, res, "per-initialisation results", "unit", &tab))) goto DONE;

	/* replay the serial bookkeeping in unit order (multiclust.c:534-560, 618-627) */
	summary_begin_K(st);
	int ub = 0;		/* the best unit of this K; where it improved on the maximum so far, st->sum.best_unit as well */
	for (int u = 0; u < n_units; u++) {
		mc_unit_result r;
		unpack_result(tab + (size_t)u * RES_FIELDS, u, &r);
		if (r.fatal) exit(0);		/* NaN / decreasing logL: the reference's reaction (em_alg.c:106-120) */
		mc_summary_add(&o->em, &st->sum, &r, npar, d->I);
		print_unit_line(o, st, K, &r, bootstrap);
		if (r.logL > res[ub].logL) ub = u;
	}
	/* the serial loop's last improvement on the maximum, if it had one in this K, is the best unit; its record came from the
	 * worker that fitted it */
	const fit_record *fit = &w[ub % n_dev].best;
	if ((st->sum.best_unit >= 0 || post) && fit->unit != ub) { fprintf(stderr, "ERROR [" MC_FRONT_END "]: owner of the best unit does not hold it\n"); rc = MCHIP_ERR_STATE; goto DONE; }
	if (st->sum.best_unit >= 0) rc = new_maximum(o, d, st, fit, bootstrap);
	if (!rc && post) rc = post_fit(o, d, md, st, fit, NULL, worker_device(o, ub % n_dev));
DONE:
	if (w) for (int x = 0; x < n_dev; x++) record_free(&w[x].best);
	free(w); free(res); free(tab); free(starts);
	return rc;
}

/* whole bootstrap replicates can be handed to workers: either model */
static int replicates_shardable(const mc_cli_options *o)
{
	/* MC_FORCE_SHARDED=1 sends even --gpus 1 through the sharded path (threads, jump-ahead, RCCL exchange, replay): the
	 * single-GPU rehearsal used by tests/test_gpu_cli.py */
	const int force = getenv("MC_FORCE_SHARDED") != NULL;
	return (o->n_gpus > 1 || o->n_streams > 1 || (force && o->n_gpus == 1)) && !o->target_revisit && !o->target_ll && !o->em.n_seconds &&
	       !(o->pfile && o->qfile) &&	/* initial parameters from files: every unit would be the same fit */
	       !o->query_file;		/* query individuals: one model, one hold-out */
}

/* the initialisations of one fit can be handed to workers: the admixture model only */
static int shardable(const mc_cli_options *o) { return replicates_shardable(o) && o->em.admixture; }

/* estimate_model (multiclust.c:365-452): K = min_K..max_K, or H0 / HA when bootstrapping */
/* sim != NULL: the models are fitted to the bootstrap data set it describes, generated on each device */
static int estimate_model(const mc_cli_options *o, const mc_cli_data *d, const mc_data *md, run_state *st, int bootstrap, int *total_iter,
			  const mc_simulation *sim)
{
	int K = o->n_bootstrap ? st->null_K : o->min_K, rc = 0;
	double min_aic = INFINITY, min_bic = INFINITY;
	const clock_t start = clock();
	st->sum.max_logL = -INFINITY;
	st->max_logL_H0 = -INFINITY;
	if (total_iter) *total_iter = 0;
	for (;;) {
		if (shardable(o)) {
			rc = maximize_likelihood_sharded(o, d, md, K, st, bootstrap, sim);
		} else {
			mc_model *mod = NULL;
			mc_model **slot = (sim && st->sim_models) ? &st->sim_models[K == st->alt_K ? 1 : 0] : NULL;
			if (slot && K == st->alt_K && st->alt_K != st->null_K && st->sim_models[0] && (!*slot || (*slot)->K == K)) {
				/* the alternative model takes the data set the null model of this replicate was just fitted to */
				if ((rc = mc_model_share_simulated(slot, &o->em, md, K, o->device, st->sim_models[0]))) return rc;
				mod = *slot;
			} else if (slot && *slot && (*slot)->K == K) {
				mod = *slot;
				if ((rc = mc_model_resimulate(mod, &o->em, md, sim))) return rc;
			} else {
				if ((rc = sim ? mc_model_create_simulated(&mod, &o->em, md, K, o->device, sim)
					      : mc_model_create(&mod, &o->em, md, K, o->device))) return rc;
				if (slot) { mc_model_free(*slot); *slot = mod; }
				/* --query: every initialisation of this K sees the panel alone */
				if (o->query_file && !sim && (rc = mc_query_hide(mod, md, st->query_mask))) { if (!slot) mc_model_free(mod); return rc; }
			}
			rc = maximize_likelihood(o, d, md, mod, st, bootstrap);
			if (!slot) mc_model_free(mod);
		}
		if (rc) return rc;
		if (o->n_repeat == 1 && o->em.verbosity)
			print_model_state(o, d, st, K, (int)(((double)clock() - start) / CLOCKS_PER_SEC), 1);
		if (st->post_lines) {	/* --fst, --resid, --cv, --se, --query, --fill (post_fit) */
			fputs(st->post_lines, st->out);
			free(st->post_lines);
			st->post_lines = NULL;
		}
		if (total_iter) *total_iter += st->sum.n_total_iter;
		if (o->n_bootstrap && K == st->null_K) st->max_logL_H0 = st->sum.max_logL;
		if (min_aic > st->sum.aic) { min_aic = st->sum.aic; st->aic_K = K; }
		if (min_bic > st->sum.bic) { min_bic = st->sum.bic; st->bic_K = K; }
		if (o->n_bootstrap && K == st->null_K) K = st->alt_K;
		else if (!o->n_bootstrap && K < o->max_K) K++;
		else break;
	}
	if (o->n_bootstrap) {
		const double diff = st->sum.max_logL - st->max_logL_H0;
		if (diff <= 0) {
			fprintf(stderr, "ERROR [" MC_FRONT_END "::estimate_model]: Null hypothesis likelihood exceeds alternative hypothesis likelihood.  "
				"Try increasing number of initializations (command-line option -n)\n");
			return MC_EXIT_INTERNAL_ERROR;		/* multiclust.c:437-443 */
		}
		if (!bootstrap) st->ts_obs = diff; else st->ts_bs = diff;
	}
	return 0;
}

/* ---- bootstrap replicates sharded over the GPUs of the node as whole units ----
 * Where replicate b = data set + H0 fits + HA fits begins in the rand() stream does not depend on any fit (mc_replicate_starts:
 * a jump per replicate for the admixture model, the replay of the center draws for the mixture model), so device x takes
 * replicates x, x + n_dev, ... each from where the serial program would be, generates the data
 * set on its own GPU and fits both models there; its stdout goes to a buffer.  One RCCL all-reduce completes the table
 * of test statistics on every device; the buffers are then printed in replicate order with the running p-value. */
typedef struct bs_worker {
	const mc_cli_options *o;
	const mc_cli_data *d;
	const mc_data *md;
	const run_state *st;		/* observed-data results: null_K, alt_K, H0 MLEs (read only), ts_obs */
	int index, n_dev;
	const mc_rng *starts;		/* [n_bootstrap + 1]: the serial stream's state at the start of every replicate */
	double *ts;			/* [n_bootstrap], shared: worker x writes entries b = x, x + n_dev, ... */
	char **text;			/* [n_bootstrap] captured stdout of each replicate */
} bs_worker;

static void *bs_main(void *arg)
{
	bs_worker *w = arg;
	mc_cli_options ow = *w->o;
	ow.device = worker_device(w->o, w->index);
	ow.n_gpus = 0;			/* the fits of a replicate stay on this device, on this worker's stream */
	ow.n_streams = 1;
	mc_model *kept[2] = { NULL, NULL };
	int *own_I_K = malloc(sizeof(int) * (size_t)(w->d->I > 0 ? w->d->I : 1));	/* -A: the partition record is per worker */
	int rc = 0;
	if (!own_I_K) return (void *)(intptr_t)MCHIP_ERR_ALLOC;
	memcpy(own_I_K, w->st->I_K, sizeof(int) * (size_t)w->d->I);
	for (int b = w->index; b < w->o->n_bootstrap; b += w->n_dev) {
		run_state ls = *w->st;
		ls.sim_models = kept;
		ls.I_K = own_I_K;
		mc_simulation gen;
		size_t len = 0;
		ls.rng = w->starts[b];
		if (!(ls.out = open_memstream(&w->text[b], &len))) { rc = MCHIP_ERR_ALLOC; break; }
		fprintf(ls.out, "Bootstrap dataset %d (of %d):", b + 1, w->o->n_bootstrap);
		mc_simulation_begin(&gen, &ow.em, w->md, ls.h0.K, ls.h0.q, ls.h0.p, &ls.rng);
		rc = estimate_model(&ow, w->d, w->md, &ls, 1, NULL, &gen);
		fclose(ls.out);
		if (rc) break;
		w->ts[b] = ls.ts_bs;
	}
	mc_model_free(kept[0]);
	mc_model_free(kept[1]);
	free(own_I_K);
	return (void *)(intptr_t)rc;
}

/* a replicate's row of the exchange table: its test statistic (and the count of how often it was fitted) */
static void pack_ts(double *row, int b, const void *ts) { row[0] = ((const double *)ts)[b]; }

static int run_bootstrap_sharded(const mc_cli_options *o, const mc_cli_data *d, const mc_data *md, run_state *st, int *ntime_out)
{
	const int n_dev = n_workers(o), B = o->n_bootstrap;
	mc_rng *starts = calloc((size_t)B + 1, sizeof *starts);
	bs_worker *w = calloc((size_t)n_dev, sizeof *w);
	double *ts = calloc((size_t)B, sizeof *ts), *tab = NULL;
	char **text = calloc((size_t)B, sizeof *text);
	int rc = 0, ntime = 0;
	if (!w || !ts || !text || !starts) { rc = MCHIP_ERR_ALLOC; goto DONE; }
	if ((rc = mc_replicate_starts(&o->em, md, &st->rng, B, st->null_K, st->alt_K, o->n_init, starts))) goto DONE;
	for (int x = 0; x < n_dev; x++) w[x] = (bs_worker){ o, d, md, st, x, n_dev, starts, ts, text };
	if ((rc = mc_run_workers(n_dev, bs_main, w, sizeof *w))) goto DONE;
	st->rng = starts[B];
	if ((rc = mc_exchange_rows(o, st, B, 2, pack_ts, ts, "bootstrap test statistics", "bootstrap replicate", &tab))) goto DONE;
	for (int b = 0; b < B; b++) {
		st->ts_bs = tab[2 * b];
		if (st->ts_bs >= st->ts_obs) ntime++;
		fputs(text[b] ? text[b] : "", stdout);
		printf(" test statistics bs=%f obs=%f (%f)\n", st->ts_bs, st->ts_obs, (double)ntime / (b + 1));
	}
	*ntime_out = ntime;
DONE:
	if (text) for (int b = 0; b < B; b++) free(text[b]);
	free(w); free(ts); free(tab); free(text); free(starts);
	return rc;
}

/* the bootstrap replicate is generated on the device(s) from the stream position (no host data set, no upload), for both models;
 * MC_HOST_BOOTSTRAP: drawn on the host and uploaded like any data set.  The host form of the mixture initialisation
 * (MC_HOST_INIT) and its Rand-EM read the replicate on the host, so they take the host route too. */
static int bootstrap_on_device(const mc_cli_options *o)
{
	return !getenv("MC_HOST_BOOTSTRAP") && (o->em.admixture || (!getenv("MC_HOST_INIT") && o->em.initialization_procedure != MC_RAND_EM));
}

/* whole replicates per worker when there is at least one for each; otherwise (or on one device) the replicates run in turn and
 * --gpus shards the initialisations inside each */
/* (Rand-EM draws a data-dependent number of values per initialisation: replicate b's place in the stream has no closed form) */
static int bootstrap_by_replicate(const mc_cli_options *o)
{
	return bootstrap_on_device(o) && replicates_shardable(o) && o->n_bootstrap >= n_workers(o) && o->em.initialization_procedure != MC_RAND_EM;
}

/* what --gpus / --streams do not apply to is said once, before anything is fitted */
static void warn_unsharded(const mc_cli_options *o)
{
	if ((o->n_gpus <= 1 && o->n_streams <= 1) || shardable(o)) return;
	if (!o->em.admixture && bootstrap_by_replicate(o))
		fprintf(stderr, "WARNING: --gpus / --streams split the bootstrap replicates of the mixture model; the two fits of the observed data run "
			"one initialisation at a time on one GPU\n");
	else
		fprintf(stderr, "WARNING: --gpus / --streams apply to the admixture model with a fixed number of initialisations; running one fit at a time on one GPU\n");
}

/* the sum and the sum of squares of the values added: what the -w summary takes its standard deviations from */
typedef struct moments { double s, s2; } moments;
static void moments_add(moments *m, double x) { m->s += x; m->s2 += x * x; }
static double moments_sd(const moments *m, double n) { return sqrt((m->s2 - m->s * m->s / n) / (n - 1)); }

/* timed_model_estimation (multiclust.c:201-347): same lines, same statistics */
static int timed_model_estimation(const mc_cli_options *o, const mc_cli_data *d, const mc_data *md, run_state *st)
{
	const clock_t start = clock();
	moments ll = { 0, 0 }, init = { 0, 0 }, iter = { 0, 0 }, aic_K = { 0, 0 }, bic_K = { 0, 0 };
	moments ar = { 0, 0 };		/* adjusted Rand index (-A); without it model::arand stays 0 */
	double esec = 0, max_ll = -INFINITY, min_aic = 0, min_bic = 0, first_ll = -INFINITY, max_ar = -1, max_ll_rand = 0;
	int n = 0, conv = 0, reached = 0, first_hit = 0, max_init = 0, max_iter = 0, enough = o->repeat_seconds ? 0 : 1, total, rc;
	char ab[16];
	while (n < o->n_repeat || !enough) {
		if ((rc = estimate_model(o, d, md, st, 0, &total, NULL))) return rc;
		if (st->sum.n_init > max_init) max_init = st->sum.n_init;
		if (st->sum.n_max_iter > max_iter) max_iter = st->sum.n_max_iter;
		if (st->sum.max_logL > max_ll) {
			mc_model probe;
			max_ll = st->sum.max_logL;
			min_aic = st->sum.aic;
			min_bic = st->sum.bic;
			max_ll_rand = st->arand;
			memset(&probe, 0, sizeof probe);
			probe.logL = st->sum.max_logL;	/* converged(opt, mod, first_ll) compares with the model's current logL */
			if (!mc_converged(&o->em, &probe, first_ll)) { first_ll = st->sum.max_logL; first_hit = n; }
		}
		if (st->arand > max_ar) max_ar = st->arand;	/* multiclust.c:252-253 */
		if (o->afile) moments_add(&ar, st->arand);
		moments_add(&init, st->sum.n_init);
		moments_add(&iter, st->sum.n_total_iter);
		moments_add(&aic_K, st->aic_K);
		moments_add(&bic_K, st->bic_K);
		moments_add(&ll, st->sum.max_logL);
		n++;
		if (st->sum.ever_converged) conv++;
		if (st->n_targetll_times) reached++;
		esec = ((double)clock() - start) / CLOCKS_PER_SEC;
		if (o->em.verbosity > MC_SILENT) {
			print_model_state(o, d, st, o->max_K, (int)esec, 0);
			printf(" %f %f %d %d %f", esec, esec / n, reached, conv, max_ll);
			if (o->target_ll) printf(" %f", o->desired_ll); else printf(" NA");
			printf(" %d %d %d %u\n", o->target_revisit, n, o->n_repeat, o->repeat_seconds);
		}
		if (!enough && esec > o->repeat_seconds) enough = 1;
		if (o->max_repeat_seconds && esec > o->max_repeat_seconds) break;
	}
	if (o->em.verbosity >= MC_SILENT) {
		printf("Data, Method, Model: %s, %s, %s\n", o->filename, accel_abbrev(o, ab),
		       o->em.admixture && o->em.eta_constrained ? "admix constrained" : o->em.admixture ? "admix" : "mix");
		printf("Run: %e %e %e %e n=%d i=%d u=(%f,%d) w=(%d,%u)\n", o->em.abs_error, o->em.rel_error, o->em.eta_lower_bound,
		       o->em.p_lower_bound, o->n_init, o->em.n_init_iter, o->desired_ll, o->target_revisit, o->n_repeat, o->repeat_seconds);
		printf("Number of repetitions: %d of %d requested, %d converged, %d reach target\n", n, o->n_repeat, conv, reached);
		printf("Average time: %fs (total: %fs; target: %u)\n", esec / n, esec, o->repeat_seconds);
		printf("Average log likelihood: %f (+/- %f)\n", ll.s / n, moments_sd(&ll, n));
		printf("Maximum log likelihood: %f first hit at run %d (AIC %f; BIC %f; RAND: %f)\n", max_ll, first_hit, min_aic, min_bic, max_ll_rand);
		printf("Adjusted RAND: avg = %f +/- %f; max = %f\n", ar.s / n, moments_sd(&ar, n), max_ar);
		if (o->max_K != o->min_K) {
			printf("Average K (AIC): %f (+/- %f)\n", aic_K.s / n, moments_sd(&aic_K, n));
			printf("Average K (BIC): %f (+/- %f)\n", bic_K.s / n, moments_sd(&bic_K, n));
		} else {
			printf("Total initializations, iterations: %d, %d\n", (int)init.s, (int)iter.s);
			printf("Average initializations: %f (+/- %f) [%e, %e]\n", init.s / n, moments_sd(&init, n), init.s2, init.s);
			/* (per initialisation, not per repetition: the reference's divisors) */
			printf("Average iterations: %f (+/- %f) [%e %e]\n", iter.s / init.s, moments_sd(&iter, init.s), iter.s2, iter.s);
			printf("Maximum initializations: %d\n", max_init);
			printf("Maximum iterations: %d\n", max_iter);
		}
	}
	return 0;
}

/* run_bootstrap (multiclust.c:675-708); d and md hold the replicate while it is fitted where it is drawn on the host */
static int run_bootstrap(const mc_cli_options *o, mc_cli_data *d, mc_data *md, run_state *st)
{
	const int on_device = bootstrap_on_device(o), by_replicate = bootstrap_by_replicate(o);
	uint8_t *orig = d->geno, *sim = on_device ? NULL : malloc((size_t)d->I * d->L * d->ploidy);
	/* the observed haplotypes the fits to an uploaded replicate initialise from (decoded here when the data set is held packed) */
	const uint8_t *observed = on_device ? NULL : mc_data_geno(md);
	mc_model *kept[2] = { NULL, NULL };
	int ntime = 0, rc = 0;
	if ((!on_device && (!sim || !observed)) || !st->h0.q) { free(sim); return MCHIP_ERR_ALLOC; }
	if (by_replicate && (rc = run_bootstrap_sharded(o, d, md, st, &ntime))) return rc;
	if (on_device && !shardable(o)) st->sim_models = kept;
	for (int b = 0; !rc && !by_replicate && b < o->n_bootstrap; b++) {
		printf("Bootstrap dataset %d (of %d):", b + 1, o->n_bootstrap);
		if (on_device) {
			mc_simulation gen;
			mc_simulation_begin(&gen, &o->em, md, st->h0.K, st->h0.q, st->h0.p, &st->rng);
			rc = estimate_model(o, d, md, st, 1, NULL, &gen);
		} else {
			mc_bootstrap_genotypes(&o->em, md, st->h0.K, st->h0.q, st->h0.p, &st->rng, sim);
			md->geno = d->geno = sim;
			md->init_geno = observed;
			rc = estimate_model(o, d, md, st, 1, NULL, NULL);
			md->geno = d->geno = orig;
			md->init_geno = NULL;
		}
		if (rc) break;
		if (st->ts_bs >= st->ts_obs) ntime++;
		printf(" test statistics bs=%f obs=%f (%f)\n", st->ts_bs, st->ts_obs, (double)ntime / (b + 1));
	}
	free(sim);
	st->sim_models = NULL;
	mc_model_free(kept[0]);
	mc_model_free(kept[1]);
	/* the reference divides two ints here (multiclust.c:703); kept */
	if (!rc) printf("p-value to reject H0: K=%d is %f\n", st->null_K, (double)(ntime / o->n_bootstrap));
	return rc;
}

/* the run, once the command line is read: the data set, what runs before the first fit, the fits, the bootstrap */
static int run(mc_cli_options *o)
{
	mc_cli_data d;
	run_state st;
	int rc;
	mchip_progress_note(o->bed_prefix ? "mc_read_bed" : "mc_read_structure");
	if ((rc = o->bed_prefix ? mc_read_bed(o, &d) : mc_read_structure(o, &d))) return rc;
	if ((rc = pre_fit(o, &d))) return rc;
	mchip_progress_note("estimate_model");
	if (o->em.verbosity >= MC_TALKATIVE)
		fprintf(stderr, "INFO: Finished reading data: %d %d-ploid individuals at %d loci.\n", d.I, d.ploidy, d.L);
	mc_data md = { d.I, d.L, d.ploidy, d.uniquealleles, d.geno, NULL, d.bed, d.bed_record_bytes, d.lazy };
	/* synchronize (multiclust.c:807-893) */
	if (mc_synchronize(&o->em, &md)) return MC_EXIT_INVALID_USER_SETUP;
	if ((rc = check_setup(o, &d))) return rc;
	memset(&st, 0, sizeof st);
	if (!(st.I_K = calloc((size_t)d.I, sizeof *st.I_K))) return MC_EXIT_MEMORY_ALLOCATION;
	if (o->afile && (rc = mc_read_afile(o->afile, d.I, &st.partition_from_file, &st.pK))) return rc;	/* synchronize's last step (multiclust.c:889-890) */
	if (o->query_file && (rc = mc_query_read(o->query_file, d.I, &st.query_mask))) return rc;
	st.out = stdout;
	mchip_comm *run_comm = NULL;
	st.comm = &run_comm;
	if (o->n_bootstrap) { st.null_K = o->max_K - 1; st.alt_K = o->max_K; }
	/* the reference seeds libc only when -r is given; otherwise rand() runs from glibc's default seed 1 although the
	 * banner prints 1234567 */
	mc_srand(&st.rng, o->seed_given ? o->em.seed : 1u);
	warn_unsharded(o);

	rc = (o->n_repeat > 1 || o->repeat_seconds) ? timed_model_estimation(o, &d, &md, &st) : estimate_model(o, &d, &md, &st, 0, NULL, NULL);
	if (!rc && o->parallel) printf("%f\n", st.sum.max_logL);	/* multiclust.c:143-145 */
	if (!rc && o->n_bootstrap) rc = run_bootstrap(o, &d, &md, &st);

	mchip_progress_note("end of main: freeing");
	if (run_comm) mchip_comm_destroy(run_comm);
	record_free(&st.h0);
	free(st.I_K); free(st.partition_from_file); free(st.query_mask); free(st.post_lines);
	mc_free_data(&d);
	return rc;
}

int main(int argc, const char **argv)
{
	mc_cli_options o;
	int rc;
	/* Every line leaves the process when it is complete, also into a pipe (same bytes as the reference's, earlier): a run that
	 * stops making progress has then said how far it got.  MC_WATCHDOG_S=<s>: leave with status 3 and a report of where every
	 * thread stands once nothing has happened for s seconds (mc_watchdog.c). */
	setvbuf(stdout, NULL, _IOLBF, 0);
	mc_watchdog_from_env();
	mchip_progress_note("parse_options");
	defaults(&o);
	if ((rc = parse_options(&o, argc, argv))) return rc;	/* -h included: the reference's -h leaves with status 1 */
	rc = run(&o);
	free_options(&o);
	mchip_progress_note("returning from main: the HIP runtime's own teardown follows");
	return rc;
}
