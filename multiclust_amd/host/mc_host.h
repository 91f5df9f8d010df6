/*
 * mc_host.h -- plain-C host side of the MI355X EM hot path.
 *
 * Mirrors the reference's EM-layer interface (reference multiclust.h:371-388: em, em_step, em_e_step,
 * em_2_steps, stop, converged, log_likelihood, accelerated_em_step, ...) with an mc_ prefix and the same
 * (options*, data*, model*) argument convention, the same ring-index / iteration-count / convergence
 * semantics and the same stderr lines; all array arithmetic goes through the C-ABI in
 * include/multiclust_hip.h (one mchip_context per model).  Differences that are deliberate:
 *   - fatal numerics (NaN logL, logL decrease) set model::fatal and stop instead of exit(0) inside the
 *     library (reference em_alg.c:106-120); the CLI turns fatal into the reference's exit(0).
 *   - parameters live on the device; mc_model_get_p/q fetch slot copies in the reference's flat order.
 */
#ifndef MC_HOST_H
#define MC_HOST_H

#include <stdint.h>
#include <stdio.h>
#include <time.h>
#include "multiclust_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The two device entry points of the mixture model's bootstrap and initialisation are weak references on the host side: the
 * host objects also link into CPU-only programs (sanitizer builds) that stand in for the device library with the entry points
 * they know and never reach these; against the real library they resolve as any other symbol. */
#if defined(__GNUC__) && !defined(__cplusplus)
extern __typeof__(mchip_simulate_genotypes_mixture) mchip_simulate_genotypes_mixture __attribute__((weak));
extern __typeof__(mchip_init_from_individual_centers) mchip_init_from_individual_centers __attribute__((weak));
/* the same for the packed upload: without it the host decodes the records and uploads the genotype as before */
extern __typeof__(mchip_set_genotypes_bed) mchip_set_genotypes_bed __attribute__((weak));
#endif

/* acceleration schemes (reference multiclust.h:125-131; 5, 6 = QN with q = 2, 3, multiclust.c:818-820) */
enum { MC_NONE = 0, MC_SQS1, MC_SQS2, MC_SQS3, MC_QN };
/* verbosity (reference message.h:45-53) */
enum { MC_ABSOLUTE_SILENCE = 0, MC_SILENT, MC_QUIET, MC_MINIMAL, MC_RESTRAINED, MC_TALKATIVE, MC_VERBOSE, MC_DEBUG };
/* initialisation procedures (reference multiclust.h:107-111) */
enum { MC_INIT_NOTHING = 0, MC_RAND_EM };
/* fatal conditions the reference answers with exit(0) */
enum { MC_FATAL_NONE = 0, MC_FATAL_NAN = 1, MC_FATAL_DECREASE = 2, MC_FATAL_DEVICE = 3 };

typedef struct mc_options {	/* subset of reference struct _options used by the EM layer (multiclust.h:155-215) */
	int admixture;
	int eta_constrained;
	int do_projection;
	int accel_scheme;
	int q;			/* number of secant conditions (QN) */
	int n_init_iter;
	int max_iter;
	unsigned int n_seconds;
	int adjust_step;
	int verbosity;
	double abs_error;
	double rel_error;
	double lower_bound;
	double eta_lower_bound;
	double p_lower_bound;
	unsigned int seed;
	int initialization_procedure;	/* MC_INIT_NOTHING (random initialisation) or MC_RAND_EM (multiclust.h:107-111) */
	int n_rand_em_init;		/* candidates per Rand-EM initialisation (-m, multiclust.c:936,1547) */
} mc_options;

typedef struct mc_data {	/* flat form of reference struct _data's genotype fields (multiclust.h:223-237) */
	int I, L, ploidy;
	const int32_t *uniquealleles;	/* [L] */
	const uint8_t *geno;		/* [I][L][ploidy] allele indices, MCHIP_MISSING = 0xFF */
	const uint8_t *init_geno;	/* NULL, or the observed data set while `geno` is a bootstrap replicate: the random
					 * partition of the admixture model keeps reading dat->IL (rnd_init.c:471) */
	/* a data set read from a PLINK .bed file (mc_bed.c) is held packed: geno is NULL, models upload `bed`
	 * (mchip_set_genotypes_bed), and what reads the genotype on the host asks mc_data_geno() for it */
	const uint8_t *bed;		/* NULL, or L records of bed_record_bytes bytes (the file behind its three header bytes) */
	size_t bed_record_bytes;
	struct mc_lazy_geno *lazy;	/* decodes `bed` on first need and keeps the result */
} mc_data;

typedef struct mc_lazy_geno {	/* (function pointers: the EM layer links without the .bed reader) */
	const uint8_t *(*get)(struct mc_lazy_geno *self, const mc_data *dat);	/* [I][L][2], NULL when out of memory; thread-safe */
	void (*release)(struct mc_lazy_geno *self);
} mc_lazy_geno;
/* dat->geno, or the decoded form of a packed data set */
const uint8_t *mc_data_geno(const mc_data *dat);

typedef struct mc_model {	/* EM-layer state of reference struct _model (multiclust.h:259-360) */
	int K;
	int pindex, findex, tindex;
	int delta_index;
	double logL;
	int n_iter, converged, stopped, accel_step, iter_stop, time_stop;
	int fatal;
	clock_t start;
	double seconds_run;
	double A[9], Ainv[9], cutu[3];
	double last_emll, last_step, last_ll;	/* diagnostics of the last accelerated cycle */
	int last_accepted;
	mchip_context *dev;
	int owns_dev;
	void *init_cache;		/* per-locus allele counts of the observed haplotypes (Rand-EM), built on first use */
} mc_model;

/* glibc-compatible rand() stream (TYPE_3 additive feedback): "same seed" means the same draws as the
 * reference's srand()/rand() (multiclust.c:1592-1596, rnd_init.c:467) on any libc. */
typedef struct mc_rng { int32_t r[31]; int f, b; } mc_rng;
void mc_srand(mc_rng *g, unsigned int seed);
int mc_rand(mc_rng *g);

/* advance the stream by n draws in O(31^2 log n): the generator is the linear recurrence
 * x_j = x_{j-31} + x_{j-3} (mod 2^32), so x^n mod (x^31 - x^28 - 1) gives the state n steps ahead.  This is
 * what lets unit u of a sharded run start exactly where the serial program would. */
void mc_rng_jump(mc_rng *g, uint64_t n);

void mc_make_options(mc_options *opt);				/* defaults of make_options, multiclust.c:902-978 */
int mc_synchronize(mc_options *opt, const mc_data *dat);	/* lower bounds + q, multiclust.c:812-820 */

/* allocate_model_for_k (multiclust.c:1181): creates the device context on `device`, uploads dat, sizes for K */
int mc_model_create(mc_model **mod, const mc_options *opt, const mc_data *dat, int K, int device);
void mc_model_free(mc_model *mod);

/* Parametric bootstrap (bootstrap.c:31-175).  mc_bootstrap_genotypes draws one data set on the host from the fitted
 * parameters q ([I][K] or [K]) and p ([K][T]) of a K-cluster model, consuming `rng` exactly as the reference consumes
 * rand(); mc_bootstrap_draws is the number of draws that takes.  The same data set can be generated on the device
 * instead of uploaded (both models; q is then eta[K] for the mixture model): fill an mc_simulation with mc_simulation_begin (which also moves rng
 * past the data set's draws) and create the replicate's models with mc_model_create_simulated. */
typedef struct mc_simulation { uint32_t window[31]; int K; const double *q, *p; } mc_simulation;
void mc_bootstrap_genotypes(const mc_options *opt, const mc_data *dat, int K, const double *q, const double *p,
			    mc_rng *rng, uint8_t *geno);
uint64_t mc_bootstrap_draws(const mc_options *opt, const mc_data *dat);
void mc_simulation_begin(mc_simulation *sim, const mc_options *opt, const mc_data *dat, int K, const double *q,
			 const double *p, mc_rng *rng);
int mc_model_create_simulated(mc_model **mod, const mc_options *opt, const mc_data *dat, int K, int device,
			      const mc_simulation *sim);
int mc_model_resimulate(mc_model *mod, const mc_options *opt, const mc_data *dat, const mc_simulation *sim);
int mc_model_share_simulated(mc_model **mod, const mc_options *opt, const mc_data *dat, int K, int device, const mc_model *like);
int mc_model_get_genotypes(mc_model *mod, uint8_t *geno);
const char *mc_model_error(const mc_model *mod);
int mc_model_set_p(mc_model *mod, int slot, const double *p);
int mc_model_get_p(mc_model *mod, int slot, double *p);
int mc_model_set_q(mc_model *mod, int slot, const double *q);
int mc_model_get_q(mc_model *mod, int slot, double *q);
int mc_model_get_expected_counts(mc_model *mod, double *sik);

/* initialize_model (rnd_init.c:54-89) for the admixture model, random allele partition (349-357,456-482) */
int mc_initialize_model(const mc_options *opt, const mc_data *dat, mc_model *mod, mc_rng *rng);
void mc_reset_model_state(mc_model *mod);	/* multiclust.c:518-524 + rnd_init.c:58-71 */
/* random_initialize_mixture (rnd_init.c:103-110): random_individual_center + initialize_parameters_mixture.  The host draws the
 * K centers; distances, counts and parameters are the device's (mchip_init_from_individual_centers), or, with MC_HOST_INIT set,
 * the host's from dat->geno */
int mc_initialize_mixture(const mc_data *dat, mc_model *mod, mc_rng *rng);
/* Rand-EM (rnd_init.c:123-160 mixture, 412-444 admixture): n_rand_em_init candidates -- random centers, parameters from the
 * partition, one EM iteration plus an E step (em_e_step) -- and the parameters of the candidate with the best log likelihood.
 * Admixture candidates are partitioned and counted on the device (mchip_init_from_allele_centers); the host only walks the
 * loci to draw the centers.  Consumes `rng` exactly as the reference consumes rand(). */
int mc_randem_initialize(const mc_options *opt, const mc_data *dat, mc_model *mod, mc_rng *rng);
/* Moves `rng` past n initialisations without performing them: where unit n of a sharded run starts in the serial stream.
 * A jump for the random allele partition; for Rand-EM and the mixture model the number of draws depends on the draws
 * themselves (center retries) and on the data (copies that match no center), so the host-side walk is replayed. */
int mc_skip_initializations(const mc_options *opt, const mc_data *dat, mc_model *mod, mc_rng *rng, int n);
/* starts[u], u = 0..n_units: the generator at the start of unit u of a sharded run (one walk over the units; `mod` supplies K and
 * holds the allele-count cache of the Rand-EM walk: a zeroed mc_model with K set will do, mc_init_cache_free() afterwards) */
int mc_unit_starts(const mc_options *opt, const mc_data *dat, mc_model *mod, const mc_rng *base, int n_units, mc_rng *starts);
void mc_init_cache_free(mc_model *mod);
/* starts[b], b = 0..n_replicates: the generator at the start of bootstrap replicate b (data set, then n_init initialisations of
 * the null_K and of the alt_K model, one when K = 1), `base` = where replicate 0 begins.  A jump per replicate for the admixture
 * model; for the mixture model the center draws of every earlier unit are replayed (their number depends on their values).
 * MCHIP_ERR_UNSUPPORTED with Rand-EM. */
int mc_replicate_starts(const mc_options *opt, const mc_data *dat, const mc_rng *base, int n_replicates, int null_K, int alt_K,
			int n_init, mc_rng *starts);
/* replicate b alone (no table: one jump, or the walk with the running state only) */
int mc_replicate_start(const mc_options *opt, const mc_data *dat, const mc_rng *base, int b, int null_K, int alt_K, int n_init,
		       mc_rng *start);

void mc_em(const mc_options *opt, const mc_data *dat, mc_model *mod);			/* em_alg.c:44 */
int mc_em_step(const mc_options *opt, const mc_data *dat, mc_model *mod);		/* em_alg.c:195 */
double mc_em_e_step(const mc_options *opt, const mc_data *dat, mc_model *mod);		/* em_alg.c:219 */
int mc_em_2_steps(mc_model *mod, const mc_data *dat, const mc_options *opt);		/* em_alg.c:1072 */
int mc_stop(const mc_options *opt, mc_model *mod, double loglik);			/* em_alg.c:101 */
int mc_converged(const mc_options *opt, mc_model *mod, double loglik);			/* em_alg.c:163 */
double mc_log_likelihood(const mc_options *opt, const mc_data *dat, mc_model *mod, int which);	/* log_likelihood.c:56 */
int mc_accelerated_em_step(const mc_options *opt, const mc_data *dat, mc_model *mod);	/* accel_em.c:35 */
double mc_step_size(const mc_options *opt, const mc_data *dat, mc_model *mod);		/* accel_em.c:130 */
double mc_accelerated_update(const mc_options *opt, const mc_data *dat, mc_model *mod, double s);	/* accel_em.c:422 */
double mc_qn_accelerated_update(const mc_options *opt, const mc_data *dat, mc_model *mod);	/* accel_em.c:262 */
double mc_aic(double max_logL, int no_parameters);			/* log_likelihood.c:70 */
double mc_bic(double max_logL, int no_parameters, int I);		/* log_likelihood.c:82 */
int mc_no_parameters(const mc_options *opt, const mc_data *dat, int K);	/* multiclust.c:1267-1276 */

/* ---- several initialisations: maximize_likelihood (multiclust.c:471-656) ---- */
typedef struct mc_unit_result {	/* what one initialisation + em() leaves behind */
	int unit;
	double logL;
	int converged, n_iter, time_stop, iter_stop, pindex, fatal;
	double seconds_run;	/* CPU seconds since the model's start stamp when the fit stopped (em_alg.c:147) */
} mc_unit_result;

typedef struct mc_summary {	/* state maintained across initialisations (multiclust.h:337-353) */
	int n_init, n_total_iter, n_max_iter, n_maxll_times, n_maxll_init, ever_converged, best_unit;
	double max_logL, first_max_logL, aic, bic;
} mc_summary;

void mc_summary_reset(mc_summary *s);						/* multiclust.c:477-486 */
/* multiclust.c:534-560; results must be fed in unit order to reproduce the serial program */
void mc_summary_add(const mc_options *opt, mc_summary *s, const mc_unit_result *r, int no_parameters, int I);
/* rand() draws one admixture initialisation consumes (rnd_init.c:460-467: one per allele copy, missing included) */
uint64_t mc_draws_per_init(const mc_options *opt, const mc_data *dat, int K);
/* what initialisation `unit` left behind in the model that just ran it */
void mc_unit_result_from_model(mc_unit_result *r, int unit, const mc_model *mod);
/* initialisation `unit` of a run seeded with `seed`: jump the stream to unit * draws_per_init, initialise, em() */
int mc_fit_unit(const mc_options *opt, const mc_data *dat, mc_model *mod, unsigned int seed, int unit, mc_unit_result *out);


/* ---- one bootstrap replicate: the other unit of sharding (run_bootstrap, multiclust.c:675-708) ---- */
typedef struct mc_replicate_result {
	int replicate;
	double logL_H0, logL_HA, ts;	/* best log likelihood of the null_K and alt_K fits, and their difference */
	int n_iter;			/* EM iterations of all fits of the replicate */
	int fatal;
} mc_replicate_result;
/* models[2] (may be NULL): the caller's null_K and alt_K models, created on first use and re-used for every later replicate
 * (free them with mc_model_free when the replicates are done); NULL: models are created and freed inside the call */
int mc_fit_replicate(const mc_options *opt, const mc_data *dat, int device, const mc_rng *base, int b, int null_K, int alt_K,
		     int n_init, int mle_K, const double *mle_q, const double *mle_p, mc_replicate_result *out, mc_model **models);

/* ---- refits of a fitted model to data sets derived from its own, from the estimate as a warm start (mc_refit.c): the part
 * mc_cross_validate and mc_locus_bootstrap below have in common.  `mod` holds the estimate in slot mod->pindex.
 * mc_refit_begin: the estimate and the host state of the model are kept in *h (on failure nothing is held); where = "file::function"
 * in front of every stderr line.  mc_refit_check: reports a failed device call `what` under that prefix and hands rc on.
 * mc_refit_warm_start, once the derived data set is installed: mc_reset_model_state, then q and p (NULL: the estimate's; else the
 * estimate rearranged for the data set) into slot 0; mc_em follows.  mc_refit_fitted, after mc_em: MCHIP_ERR_HIP on a device failure
 * (the call ends); *skipped on NaN or a decrease of the log likelihood ("WARNING ... K = <K>, <unit> <index>: the fit stopped on
 * ...; <then>" is printed and the run goes on).  mc_refit_end, whatever happened and after the
 * caller has installed the base data set again with status rc_base: the estimate back into its slot (unless rc_base), *mod as
 * it was but for dev and init_cache, the buffers freed; returns rc, or else what giving back failed with. */
typedef struct mc_refit { const char *where; mc_model *mod, keep; int nq, np; double *q, *p; } mc_refit;
int mc_refit_check(const mc_refit *h, int rc, const char *what);
int mc_refit_begin(mc_refit *h, mc_model *mod, const char *where);
int mc_refit_warm_start(mc_refit *h, const double *p);
int mc_refit_fitted(const mc_refit *h, const char *unit, int index, const char *then, int *skipped);
int mc_refit_end(mc_refit *h, int rc, int rc_base);

/* ---- K-fold cross-validation of a fitted admixture model (mc_cv.c; an extension, the reference has no counterpart) ----
 * `mod` holds the full-data estimate of its K in slot mod->pindex.  The folds are drawn on the device from a fresh stream seeded
 * with opt->seed -- a stream of their own, the same for every K, so the K are compared on one partition; the run's rand()
 * stream is not touched.  For each fold: hold it out (mchip_cv_hold_out), put the estimate into slot 0, run mc_em from that warm
 * start with the run's own options (acceleration, tolerances, iteration cap, projection, bounds), score the held-out copies
 * (mchip_cv_heldout_loglik).  Then the full data set is installed again and
 *     cv = - sum_f sum_log_f / sum_f n_copies_f,
 * the mean negative log predictive probability of a held-out allele copy.  floor: a prediction below it counts as the floor
 * (a copy whose allele is absent from the retained data otherwise scores log 0 after the first M step); <= 0 takes the default
 * 1 / (I ploidy + 1), below every non-zero sample frequency of an allele.
 * A fold whose fit stops on NaN or on a decrease of the log likelihood is reported on stderr and makes cv NaN (fatal_fold = the
 * first such fold); the call still returns 0.  On return the parameters of slot mod->pindex, mod->logL, mod->n_iter and the rest
 * of the host state are what they were (the other two slots, the secants and the expected counts are the last fold fit's).
 * Admixture models only (individual or shared mixing proportions), 2 <= n_folds <= MC_CV_MAX_FOLDS. */
#define MC_CV_MAX_FOLDS 64
typedef struct mc_cv_result {
	double cv, sum_log, floor;
	uint64_t n_copies, n_floored;
	int n_folds, fatal_fold;	/* fatal_fold: -1 = none */
	double fold_sum_log[MC_CV_MAX_FOLDS];
	uint64_t fold_copies[MC_CV_MAX_FOLDS], fold_floored[MC_CV_MAX_FOLDS];
	int fold_iter[MC_CV_MAX_FOLDS];	/* EM iterations of each fold's fit */
} mc_cv_result;
double mc_cv_default_floor(const mc_data *dat);
int mc_cross_validate(const mc_options *opt, const mc_data *dat, mc_model *mod, int n_folds, double floor, mc_cv_result *out);

/* ---- standard errors of the mixing proportions: non-parametric bootstrap over loci (mc_se.c; an extension -- the reference's
 * bootstrap is parametric, tests K - 1 against K and gives no standard errors) ----
 * `mod` holds the full-data estimate of its K in slot mod->pindex; both models (individual or shared mixing proportions, and the
 * mixture model's eta_k).  nq = mchip_q_length.
 * Stream convention: a fresh mc_rng seeded with opt->seed -- a stream of their own, so the run's rand() stream is not advanced,
 * and the lists do not depend on K.  The L loci form nb = ceil(L / block) blocks of consecutive loci (the last may be shorter).
 * Replicate r takes the next nb draws of the stream; each draw b = rand() % nb appends the loci b block ... min(L, (b + 1) block) - 1
 * to the replicate's list; L2 is what that adds up to.
 * For each replicate: the list is installed (mchip_resample_loci), the model set again (mchip_set_model with mc_model_create's
 * arguments), slot 0 takes the estimate -- q as it is (rows of empty individuals go up and come back as NaN), p with its columns
 * following their loci -- and mc_em runs from that warm start with the run's own options.  The warm start stands in for matching
 * cluster labels between replicates: a fit that starts at the estimate stays in its labelling unless the replicate moves it to a
 * permuted solution, which then inflates the standard errors of the entries concerned.  A fit that stops on NaN or on a decrease
 * of the log likelihood is reported on stderr, counted in n_failed and skipped; a device failure ends the call with its status.
 * Accumulation is on the host, from mc_model_get_q(pindex), in replicate order, per entry x by Welford's update
 *     n++; d = x - mean; mean += d / n; M2 += d (x - mean)
 * where a NaN entry (the row of an individual without an observed copy in this replicate) is skipped and does not count.
 * count[e] = the entry's n, se[e] = sqrt(M2 / (n - 1)) or NaN when n < 2, mean[e] NaN when n = 0; equal values give se = 0 exactly.
 * mean_se / max_se: over the entries with n >= 2 (NaN when there is none); n_iter: EM iterations of all the fits.
 * Afterwards, whatever happened, the base data set is installed again (mchip_resample_loci(NULL)), the model set, and the
 * parameters of slot mod->pindex, mod->logL, mod->n_iter and the rest of the host state are what they were; the other two slots,
 * the secants and the expected counts are unspecified.
 * 2 <= n_replicates <= MC_SE_MAX_REPLICATES and 1 <= block <= L, else MCHIP_ERR_INVALID. */
#define MC_SE_MAX_REPLICATES 10000
typedef struct mc_se_result { int n_replicates, block, n_failed; uint64_t n_iter; double mean_se, max_se; } mc_se_result;
int mc_locus_bootstrap(const mc_options *opt, const mc_data *dat, mc_model *mod, int n_replicates, int block,
		       double *mean /* [nq] */, double *se /* [nq] */, int32_t *count /* [nq] */, mc_se_result *out);
/* The next n_lists lists of the stream convention above, drawn from `rng` (mc_srand(rng, opt->seed) before the first): list r is
 * src[r * cap ... r * cap + len[r] - 1] with cap = mc_se_list_capacity(L, block) = nb * block (0 for a bad L or block). */
int mc_se_list_capacity(int L, int block);
int mc_se_draw_lists(mc_rng *rng, int L, int block, int n_lists, int32_t *src /* [n_lists][cap] */, int32_t *len /* [n_lists] */);

/* ---- query individuals: fitted against a panel's allele frequencies, not part of estimating them (mc_query.c; an extension) ----
 * mask[i] != 0 marks individual i of the data set as a query individual; the others are the panel.
 * mc_query_hide: call it right after mc_model_create.  It sets two folds on the device, fold(i, l) = mask[i], and holds fold 1
 * out (mchip_cv_set_folds, mchip_cv_hold_out): the query individuals become individuals without an observed copy -- they add
 * nothing to P, the log likelihood or the expected counts, their rows of Q are the NaN of mchip_empty_individuals, and the
 * result files show them as they show such individuals -- while the device keeps their genotypes in the saved full data set.
 * mc_query_fit: `mod` holds a fit of the panel in slot mod->pindex.  Every query individual's mixing proportions are fitted from
 * 1 / K with that slot's P held fixed (mchip_fit_q_rows) under the run's opt->abs_error / rel_error and an iteration cap of
 * opt->max_iter, or MC_QUERY_MAX_ITER when that is 0 (no limit): plain EM on K numbers takes tens of iterations, a row that
 * creeps along a boundary a few thousand, and the cap bounds a launch that cannot be interrupted.  The context is left as it was
 * found, the hold-out still in force.  out: one entry per query individual in data order -- rows[r] its index, q[r][K], logL[r],
 * iter[r], converged[r] -- with n_converged, n_failed (rows whose log likelihood is not finite: their q is NaN), max_iter = the
 * largest iter[r] and sum_logL over the finite rows; release it with mc_query_result_free.
 * Admixture model with individual mixing proportions only, else MCHIP_ERR_UNSUPPORTED. */
#define MC_QUERY_MAX_ITER 10000
typedef struct mc_query_result {
	int n, K, n_converged, n_failed, max_iter;
	double sum_logL;
	int32_t *rows, *iter;
	double *q, *logL;
	uint8_t *converged;
} mc_query_result;
int mc_query_hide(mc_model *mod, const mc_data *dat, const uint8_t *mask /* [I] */);
int mc_query_fit(const mc_options *opt, const mc_data *dat, mc_model *mod, const uint8_t *mask /* [I] */, mc_query_result *out);
void mc_query_result_free(mc_query_result *r);

/* ---- missing genotypes filled from a fitted admixture model (mc_impute.c; an extension) ----
 * `mod` holds a fit in slot mod->pindex.  Every missing copy of the data set installed on its context takes the most probable allele
 * given that slot's Q and P -- the r missing copies of a genotype together the mode of the multinomial(r; x), x_m proportional to
 * sum_k q_ik p_klm over the locus's real alleles (mchip_impute_missing, include/multiclust_hip.h) -- and geno_out [I][L][ploidy]
 * receives the data set with them filled in.  mc_impute_n_real: the candidates of every locus, uniquealleles[l] without the phantom
 * slot of a locus that has a missing copy, from the genotype or from the packed records of a PLINK fileset.  Counts are per copy
 * (n_filled, n_left: the locus has no observed allele, or no allele has a positive probability) and per filled genotype
 * (n_genotypes); sum_conf adds the probabilities of the filled genotypes, mean_conf = sum_conf / n_genotypes (0 without one).
 * A filled genotype is the most probable one, not a draw: filled data understate the variance of heterozygosity.
 * Nothing of the model or the context changes.  Admixture model only (individual or shared mixing proportions), else
 * MCHIP_ERR_UNSUPPORTED. */
typedef struct mc_impute_result { uint64_t n_filled, n_left, n_genotypes; double sum_conf, mean_conf; } mc_impute_result;
int mc_impute_n_real(const mc_data *dat, int32_t *n_real /* [L] */);
int mc_impute(const mc_options *opt, const mc_data *dat, mc_model *mod, uint8_t *geno_out /* [I][L][ploidy] */, mc_impute_result *out);

/* ---- divergence of the fitted clusters (mc_diverge.c; an extension) ----
 * `mod` holds a fit in slot mod->pindex; either model.  The weights of the clusters come from that slot's Q (mc_model_get_q): the
 * column means over the rows that are not NaN under the admixture model with individual mixing proportions -- individuals without
 * an observed copy and query individuals drop out; 1 / K when no row is left -- and eta itself under shared mixing proportions and
 * the mixture model (mc_divergence_weights: n_rows = I or 0).  mchip_divergence (include/multiclust_hip.h has every definition)
 * gives the sums over the slot's P; from them w [K], H [K] the expected heterozygosity of every cluster, D [K][K] the net distance
 * and F [K][K] Hudson's F_ST of every pair (mc_divergence_tables), locus_ht [L] and locus_f [L] = V_l / HT_l (NaN where HT_l = 0
 * or the locus has no column), sum_v, sum_ht and f_all = sum_v / sum_ht, and over the pairs a < b whose F_ab is a number their count
 * n_pairs, f_mean, f_min and f_max (mc_divergence_summary; NaN without such a pair).  n_loci: the loci with a column.
 * Nothing of the model or the context changes.  Release the arrays with mc_divergence_result_free; on failure nothing is held. */
typedef struct mc_divergence_result {
	int K, L, n_loci, n_pairs;
	double f_mean, f_min, f_max, sum_v, sum_ht, f_all;
	double *w, *H, *D, *F, *locus_ht, *locus_f;
} mc_divergence_result;
void mc_divergence_weights(int K, int n_rows, const double *q, double *w /* [K] */);
void mc_divergence_tables(int K, int n_loci, const double *het /* [K] */, const double *sqdiff /* [K][K] */, double *H, double *D, double *F);
void mc_divergence_summary(int K, const double *F /* [K][K] */, int *n_pairs, double *mean, double *min, double *max);
int mc_divergence(const mc_options *opt, const mc_data *dat, mc_model *mod, mc_divergence_result *out);
void mc_divergence_result_free(mc_divergence_result *r);
/* "Divergence (K=<K>): pairwise Fst mean <%.6f> min <%.6f> max <%.6f> over <n> pairs; among clusters <%.6f> [<L1> loci]", with
 * "no pairs" for the pairwise part when there is none (K = 1); no line end */
void mc_divergence_line(FILE *fp, const mc_divergence_result *r);

/* ---- residual correlation of the admixture fit between individuals (mc_resid.c; an extension: evalAdmix's check of a fit) ----
 * `mod` holds a fit of the admixture model (individual or shared mixing proportions) in slot mod->pindex; dat gives I.
 * mchip_residual_products (include/multiclust_hip.h has every definition) gives, over the data set installed on the context, G_ij =
 * sum_c r_ic r_jc of the residuals r = observed allele count - predicted count and the pairwise-complete D_ij = squared norm of i's
 * residuals over the loci at which j has data; from them cor [I][I], cor_ij = G_ij / sqrt(D_ij D_ji), NaN on the diagonal and
 * where either D is 0 -- an individual without an observed copy, a query individual -- symmetric bit for bit (mc_residual_ratios).
 * mc_residual_summary, over the finite off-diagonal entries: per individual ind_mean, ind_max and ind_partner (the first
 * individual it has its largest correlation with; NaN, NaN, -1 without a finite entry), and over the pairs i < j n_pairs, mean,
 * mean_abs = mean |cor|, max with its pair (max_i, max_j); NaN and -1 without a pair.
 * Limit: P was estimated with individual i in the data, so under a correct model the expected correlation is slightly negative, of
 * the order -1 / (size of i's cluster), not zero; evalAdmix's leave-one-out refit of the frequencies, which removes that, is not done.
 * Cost: quadratic in I -- I^2 T + 2 I^2 L multiply-adds on the device, three I x I arrays of doubles on the host.
 * Nothing of the model or the context changes.  Mixture model: MCHIP_ERR_UNSUPPORTED.  Release the arrays with
 * mc_resid_result_free; on failure nothing is held. */
typedef struct mc_resid_result {
	int K, I, max_i, max_j;
	long long n_pairs;
	double mean, mean_abs, max;
	double *cor, *ind_mean, *ind_max;
	int32_t *ind_partner;
} mc_resid_result;
void mc_residual_ratios(int I, const double *G /* [I][I] */, const double *D /* [I][I] */, double *cor /* [I][I] */);
void mc_residual_summary(int I, const double *cor /* [I][I] */, mc_resid_result *r /* its three [I] arrays allocated */);
int mc_residual_correlation(const mc_data *dat, mc_model *mod, mc_resid_result *out);
void mc_resid_result_free(mc_resid_result *r);
/* "Residual correlation (K=<K>): mean <%.6f> mean |r| <%.6f> max <%.6f> (<i>, <j>) over <n> pairs", with "no pairs" behind the colon
 * when no pair has a number; no line end */
void mc_resid_line(FILE *fp, const mc_resid_result *r);

/* ---- kinship between individuals under the fitted admixture model (mc_kinship.c; an extension: REAP's estimator) ----
 * `mod` holds a fit of the admixture model (individual or shared mixing proportions) in slot mod->pindex; dat gives I and the ploidy.
 * mchip_kinship_products (include/multiclust_hip.h has every definition and the derivation) gives, over the data set installed on
 * the context, G_ij = sum_c r_ic r_jc of the residuals and V_ij = sum_c w_ic w_jc of w = observed copies x sqrt(t (1 - t)), t the
 * individual-specific allele frequency; phi_ij = G_ij / V_ij, NaN where V_ij = 0 -- an individual without an observed copy, a query
 * individual, a pair without a shared locus.  mc_kinship_from_sums forms what is reported: `pairs`, the n_pairs pairs i < j with
 * phi > t in (i, j) order, each with its sums and its degree (mc_kinship_degree: 0 duplicate / MZ twin > 0.354, 1 first degree >
 * 0.177, 2 second > 0.0884, 3 third > 0.0442, 4 more distant), n_degree [5] how many of each; over the n_finite pairs i < j with a
 * number their mean and the largest with its pair (NaN and -1 without one); per individual self = phi_ii, inbreeding = 2 phi_ii - 1
 * (ploidy 2, otherwise NaN), ind_count = the others it has phi > t with, ind_max and ind_partner = its largest finite phi with
 * another and the first it has it with (NaN, -1 without one).  A NaN compares false: it is above no threshold.
 * Limits: P and Q were estimated with the pair in the data, so estimates of true relatives are biased slightly towards zero; a family
 * fitted as a cluster of its own shows no kinship (remove it before the fit: --king-cutoff); no k0 / k1 / k2.
 * Cost: quadratic in I -- 2 I^2 T multiply-adds on the device, half skipped by symmetry; two I x I arrays of doubles on the host.
 * Nothing of the model or the context changes.  Mixture model: MCHIP_ERR_UNSUPPORTED.  Release the arrays with
 * mc_kinship_result_free; on failure nothing is held. */
typedef struct mc_kin_pair { int i, j, degree; double phi, G, V; } mc_kin_pair;
typedef struct mc_kinship_result {
	int K, I, ploidy, max_i, max_j;
	double t, mean, max;
	long long n_finite, n_degree[5];
	size_t n_pairs;
	mc_kin_pair *pairs;
	double *self, *inbreeding, *ind_max;
	int32_t *ind_count, *ind_partner;
} mc_kinship_result;
int mc_kinship_degree(double phi);
int mc_kinship_from_sums(int I, int ploidy, double t, const double *G /* [I][I] */, const double *V /* [I][I] */, mc_kinship_result *r /* r->K set */);
int mc_kinship(const mc_data *dat, mc_model *mod, double t, mc_kinship_result *out);
void mc_kinship_result_free(mc_kinship_result *r);
/* "Kinship (K=<K>): <n> pairs above <t> (<d> duplicates, <f> first, <s> second, <h> third degree); largest <%.6f> (<i>, <j>); mean over
 * <m> pairs <%.6f>", with "no pairs" behind the colon when no pair has a number; no line end */
void mc_kinship_line(FILE *fp, const mc_kinship_result *r);

/* ---- opt-in watchdog (mc_watchdog.c): nothing in the reference corresponds -- it has nothing to wait for ----
 * mc_watchdog_start(s): a detached thread that polls the library's event count (mchip_progress_report) and, when it has stood
 * still for s seconds, prints where every thread stands (library record + /proc/self/task) on stderr and leaves with _exit(3).
 * mc_watchdog_from_env(): the same with s = $MC_WATCHDOG_S, nothing when the variable is unset.  mc_watchdog_report(): the
 * report alone (used by the tests). */
int mc_watchdog_start(double seconds);
int mc_watchdog_from_env(void);
void mc_watchdog_report(FILE *fp, double quiet_seconds);

#ifdef __cplusplus
}
#endif
#endif
