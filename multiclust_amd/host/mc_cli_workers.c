/*
 * mc_cli_workers.c -- how a sharded run of the `multiclust` binary is scheduled, once for its two routes (the initialisations of one K,
 * whole bootstrap replicates; mc_main.c): the worker pool -- one host thread per worker -- and the one exchange of a route, an RCCL
 * all-reduce of the table of rows the workers filled, with its checks.  What a worker does and what a row holds is the
 * route's; nothing here knows an option of the command line beyond --device, --gpus and --streams.
 */
#include "mc_main.h"

#include <pthread.h>
#include <stdint.h>
#include <string.h>

int mc_run_workers(int n, void *(*fn)(void *), void *workers, size_t stride)
{
	pthread_t *th = calloc((size_t)n, sizeof *th);
	int *joinable = calloc((size_t)n, sizeof *joinable);	/* (a pthread_t has no "none" value) */
	void **ret = calloc((size_t)n, sizeof *ret);
	int rc = 0;
	if (!th || !joinable || !ret) { rc = MCHIP_ERR_ALLOC; goto DONE; }
	for (int x = 0; x < n; x++) {
		void *w = (char *)workers + (size_t)x * stride;
		if (pthread_create(&th[x], NULL, fn, w)) ret[x] = fn(w);	/* no thread to be had: in this one */
		else joinable[x] = 1;
	}
	for (int x = 0; x < n; x++) if (joinable[x]) pthread_join(th[x], &ret[x]);
	for (int x = 0; x < n; x++) if (ret[x]) rc = (int)(intptr_t)ret[x];
DONE:
	free(th); free(joinable); free(ret);
	return rc;
}

/* with one GPU its table is already complete (the workers are threads of this process); the rehearsal of the sharded
 * path on one GPU (MC_FORCE_SHARDED) still goes through RCCL */
static int exchange_needed(const mc_cli_options *o) { return o->n_gpus > 1 || getenv("MC_FORCE_SHARDED") != NULL; }

/* one communicator per run: creating it (ncclCommInitAll) costs seconds, an exchange microseconds */
static int get_comm(const mc_cli_options *o, run_state *st, mchip_comm **out)
{
	int rc = 0;
	if (!*st->comm) {
		const int n_dev = n_gpus(o);
		int *devs = malloc(sizeof(int) * (size_t)n_dev);
		if (!devs) return MCHIP_ERR_ALLOC;
		for (int x = 0; x < n_dev; x++) devs[x] = o->device + x;
		rc = mchip_comm_create(st->comm, n_dev, devs);
		free(devs);
		if (rc) fprintf(stderr, "ERROR [" MC_FRONT_END "]: cannot create the RCCL communicator (status %d)\n", rc);
	}
	*out = *st->comm;
	return rc;
}

/* the run's one exchange: RCCL all-reduce (sum) of the table; MC_TRACE_EXCHANGE=1 reports on stderr what
 * the communicator is and has done (tests/test_gpu_cli.py reads it: the one-GPU rehearsal has to go through RCCL, not past it) */
static int exchange_table(const mc_cli_options *o, run_state *st, double **tab, int count, const char *what)
{
	mchip_comm *comm = NULL;
	int rc = get_comm(o, st, &comm);
	if (rc) return rc;
	if ((rc = mchip_comm_all_reduce(comm, tab, count, 0))) { fprintf(stderr, "ERROR [" MC_FRONT_END "]: %s\n", mchip_comm_last_error(comm)); return rc; }
	if (getenv("MC_TRACE_EXCHANGE")) {
		int n = 0, ver = 0;
		unsigned long long done = 0;
		mchip_comm_info(comm, &n, &ver, &done);
		fprintf(stderr, "exchange: RCCL %d all-reduce #%llu, %d doubles (%s) over %d device(s)\n", ver, done, count, what, n);
	}
	return 0;
}

int mc_exchange_rows(const mc_cli_options *o, run_state *st, int n_rows, int n_fields, mc_fill_row fill, const void *arg, const char *what,
		     const char *noun, double **out)
{
	const int n_dev = n_workers(o), n_tab = n_gpus(o), count = n_rows * n_fields;
	double **tab = calloc((size_t)n_tab, sizeof *tab);
	int rc = 0;
	*out = NULL;
	if (!tab) return MCHIP_ERR_ALLOC;
	/* every device's table holds the rows its workers filled; the all-reduce (sum) completes them all */
	for (int g = 0; g < n_tab; g++)
		if (!(tab[g] = calloc((size_t)count, sizeof(double)))) { rc = MCHIP_ERR_ALLOC; goto DONE; }
	for (int r = 0; r < n_rows; r++) {
		double *row = tab[(r % n_dev) % n_tab] + (size_t)r * n_fields;
		fill(row, r, arg);
		row[n_fields - 1] = 1.0;
	}
	if (exchange_needed(o) && (rc = exchange_table(o, st, tab, count, what))) goto DONE;
	for (int g = 1; g < n_tab; g++)
		if (memcmp(tab[0], tab[g], sizeof(double) * (size_t)count)) { fprintf(stderr, "ERROR [" MC_FRONT_END "]: devices disagree after the all-reduce\n"); rc = MCHIP_ERR_STATE; goto DONE; }
	for (int r = 0; r < n_rows; r++) {
		const double times = tab[0][(size_t)r * n_fields + n_fields - 1];
		if (times != 1.0) { fprintf(stderr, "ERROR [" MC_FRONT_END "]: %s %d was fitted %g times\n", noun, r, times); rc = MCHIP_ERR_STATE; goto DONE; }
	}
	*out = tab[0];
	tab[0] = NULL;
DONE:
	for (int g = 0; g < n_tab; g++) free(tab[g]);
	free(tab);
	return rc;
}
