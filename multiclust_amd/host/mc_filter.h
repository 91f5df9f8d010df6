/*
 * mc_filter.h -- what the filters of a fileset that run before the fit (--prune, mc_ld.c; --king-cutoff, mc_king.c) have in common
 * (mc_cli.h, which includes this file at its end, says what each function does): the device opened around the part that asks it
 * for a band, the reader's summary made anew once the records have changed, and the per-individual fields made anew for the individuals kept.  A new filter writes its rule and its compaction,
 * calls these two, and is run by pre_fit() of mc_cli_stages.c.  static inline, as mc_files.h is and for the same reason; beside libc they
 * call mchip_create / mchip_destroy / mchip_last_error and mc_bed_summarize (mc_bed.c): the drivers under tests/ stub those.
 */
#ifndef MC_FILTER_H
#define MC_FILTER_H

static inline int mc_filter_on_device(const mc_cli_options *opt, const mc_cli_data *dat, const char *origin, const char *option, const char *noun,
			mc_filter_fn decide, void *out)
{
	mc_device_band dev = { NULL, dat };
	int rc = mchip_create(&dev.ctx, opt->device);
	if (rc) {
		fprintf(stderr, "ERROR [%s]: cannot open device %d for %s (status %d)\n", origin, opt->device, option, rc);
		return rc;
	}
	if ((rc = decide(opt, &dev, out))) fprintf(stderr, "ERROR [%s]: %s failed (status %d): %s\n", origin, noun, rc, mchip_last_error(dev.ctx));
	if (dev.ctx) mchip_destroy(dev.ctx);
	return rc;
}

static inline int mc_filter_resummarize(mc_cli_data *dat, int L_before, const char *origin, const char *what, double t_start)
{
	free(dat->uniquealleles); free(dat->toff);
	if (dat->L_alleles) for (int l = 0; l < L_before; l++) free(dat->L_alleles[l]);
	free(dat->L_alleles);
	dat->uniquealleles = dat->toff = NULL;
	dat->L_alleles = NULL;
	const int rc = mc_bed_summarize(dat);
	mc_timing_line(origin, what, t_start);
	return rc;
}

static inline void mc_qc_result_free(mc_qc_result *r)
{
	if (!r) return;
	free(r->ind_counts); free(r->var_counts); free(r->hwe_p); free(r->ind_keep); free(r->var_reason);
	free(r);
}

static inline int mc_filter_rebuild_individuals(mc_cli_data *dat, int n, const int *map)
{
	const int I = dat->I, first = !dat->fam_iid;
	char **fid = first ? calloc((size_t)I, sizeof *fid) : NULL, **names = calloc((size_t)n, sizeof *names), **pops = calloc((size_t)n, sizeof *pops);
	int *locale = calloc((size_t)n, sizeof *locale), *i_p = NULL, *new_of = malloc(sizeof(int) * (size_t)(dat->numpops ? dat->numpops : 1));
	int numpops = 0, ok = (fid || !first) && names && pops && locale && new_of;
	for (int i = 0; ok && first && i < I; i++) ok = (fid[i] = strdup(dat->pops[dat->locale[i]])) != NULL;
	for (int p = 0; ok && p < dat->numpops; p++) new_of[p] = -1;
	for (int x = 0; ok && x < n; x++) {
		const int old = dat->locale[map[x]];
		if (new_of[old] < 0) {
			if (!(pops[numpops] = strdup(dat->pops[old]))) { ok = 0; break; }
			new_of[old] = numpops++;
		}
		locale[x] = new_of[old];
		ok = (names[x] = strdup(dat->names[map[x]])) != NULL;
	}
	if (ok) ok = (i_p = calloc((size_t)(numpops ? numpops : 1), sizeof *i_p)) != NULL;
	free(new_of);
	if (!ok) {
		for (int i = 0; fid && i < I; i++) free(fid[i]);
		for (int x = 0; x < n; x++) { if (names) free(names[x]); if (pops) free(pops[x]); }
		free(fid); free(names); free(pops); free(locale);
		return MC_EXIT_MEMORY_ALLOCATION;
	}
	for (int x = 0; x < n; x++) i_p[locale[x]]++;
	for (int p = 0; p < dat->numpops; p++) free(dat->pops[p]);
	free(dat->pops); free(dat->locale); free(dat->i_p);
	if (first) {	/* the file's own ids move to fam_iid / fam_fid */
		dat->fam_iid = dat->names;
		dat->fam_fid = fid;
		dat->I_file = I;
	} else {
		for (int i = 0; i < I; i++) free(dat->names[i]);
		free(dat->names);
	}
	dat->names = names; dat->pops = pops; dat->locale = locale; dat->i_p = i_p;
	dat->numpops = numpops;
	dat->I = n;
	return 0;
}

#endif
