/*
 * mc_main.h -- what crosses the units of the `multiclust` binary: mc_main.c (the fits and their bookkeeping), mc_cli_options.c (the
 * command line), mc_cli_stages.c (what runs before the first fit and after the best fit of a K) and mc_cli_workers.c (the worker pool
 * and the exchange of a sharded run).  Not installed, and no unit of libmulticlust_host.so includes it.
 */
#ifndef MC_MAIN_H
#define MC_MAIN_H

#include "mc_cli.h"

#include <math.h>
#include <stdlib.h>

/* the name of the program's front end in the lines on stderr, "ERROR [mc_main.c::parse_options]: ..." and its like: tests and users'
 * scripts match on them, whichever unit the line comes from */
#define MC_FRONT_END "mc_main.c"

/* ---- one record of a fit: what the command line keeps of an initialisation once its model has moved on ---- */
typedef struct fit_record {
	int K, unit, n_iter, converged;	/* unit: the initialisation, -1 = nothing recorded yet */
	double logL;
	double *q, *p, *sik;		/* owned copies of slot pindex and of the expected counts (the layouts of mc_fit_view); NULL when not asked for */
} fit_record;
#define FIT_RECORD_NONE { 0, -1, 0, 0, -INFINITY, NULL, NULL, NULL }

/* ---- state across initialisations / models (reference struct _model, multiclust.h:337-360) ---- */
typedef struct run_state {
	mc_summary sum;
	double max_logL_H0, ts_obs, ts_bs;
	int n_targetll_times, n_targetll_init, time_stop;
	int aic_K, bic_K, null_K, alt_K;
	fit_record h0;			/* H0 MLEs for the bootstrap (multiclust.c:562-581): K, q, p */
	mc_rng rng;
	FILE *out;			/* stdout, or a replicate's buffer when bootstrap replicates run on several devices */
	mchip_comm **comm;		/* the run's RCCL communicator over devices device..device+n_gpus-1, created on first use */
	mc_model **sim_models;		/* [2] or NULL: this worker's H0 / HA models of the bootstrap data sets, kept from one replicate to
					 * the next (same shape, same K: the device re-uses every buffer, mc_model_resimulate) */
	/* -A (multiclust.c:602-612): the partition read from the file (labels - 1, pK of them), the MAP partition of the last fit that
	 * was partitioned (dat->I_K) and the adjusted Rand index of the two (model::arand: never reset, as in the reference) */
	int *partition_from_file, pK, *I_K;
	double arand;
	uint8_t *query_mask;		/* --query: which individuals are query individuals */
	char *post_lines;		/* what post_fit has to say about the K just fitted: estimate_model prints it behind the K's summary line */
} run_state;

static inline size_t n_q(const mc_cli_options *o, const mc_cli_data *d, int K) { return (o->em.admixture && !o->em.eta_constrained) ? (size_t)d->I * K : (size_t)K; }

/* sharded runs use n_gpus * n_streams workers (host thread + context + stream each); worker x sits on device
 * device + x % n_gpus, so consecutive units land on different GPUs first */
static inline int n_gpus(const mc_cli_options *o) { return o->n_gpus < 1 ? 1 : o->n_gpus; }
static inline int n_workers(const mc_cli_options *o) { return n_gpus(o) * (o->n_streams < 1 ? 1 : o->n_streams); }
static inline int worker_device(const mc_cli_options *o, int x) { return o->device + x % n_gpus(o); }

/* mc_cli_options.c.  parse_options: 0, or the status to leave with (-h included: 1); after 0, free_options gives back what it
 * allocated.  check_setup: what can only be checked against the data set that was read; it also settles the defaults that depend on
 * other options */
void defaults(mc_cli_options *o);
int parse_options(mc_cli_options *o, int argc, const char **argv);
void free_options(mc_cli_options *o);
int check_setup(mc_cli_options *o, const mc_cli_data *d);

/* mc_cli_stages.c */
int pre_fit(const mc_cli_options *o, mc_cli_data *d);
int wants_post_fit(const mc_cli_options *o, int bootstrap);
int post_fit(const mc_cli_options *o, const mc_cli_data *d, const mc_data *md, run_state *st, const fit_record *fit, mc_model *mod, int device);

/* mc_cli_workers.c.
 * mc_run_workers: fn(workers + x * stride) for x = 0 .. n - 1, each in a thread of its own (in this one when there is none to be had),
 * all joined; fn returns its status as a pointer, (void *)(intptr_t)rc.  Returns the last non-zero status in worker order, or 0.
 * mc_exchange_rows: a table of n_rows rows of n_fields doubles whose rows the workers of several devices hold: fill(row, r, arg) writes
 * the first n_fields - 1 fields of row r into the table of the device that owns it (row r is worker r % n_workers' row), the last
 * field counts how often the row was filled; one RCCL all-reduce (sum) completes every device's table when there is more than one
 * (or MC_FORCE_SHARDED asks for the rehearsal; MC_TRACE_EXCHANGE=1 reports it on stderr as "... (<what>) ..."); the tables must then
 * be equal and every count 1.0 ("<noun> %d was fitted %g times").  *out = device 0's table, the caller's to free.  Returns 0 or a status. */
typedef void (*mc_fill_row)(double *row, int r, const void *arg);
int mc_run_workers(int n, void *(*fn)(void *), void *workers, size_t stride);
int mc_exchange_rows(const mc_cli_options *o, run_state *st, int n_rows, int n_fields, mc_fill_row fill, const void *arg, const char *what,
		     const char *noun, double **out);

#endif
