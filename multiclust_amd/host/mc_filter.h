/*
 * mc_filter.h -- what the filters of a fileset that run before the fit (--prune, mc_ld.c; --king-cutoff, mc_king.c) have in common
 * (mc_cli.h, which includes this file at its end, says what each function does): the device opened around the part that asks it
 * for a band, and the reader's summary made anew once the records have changed.  A new filter writes its rule and its compaction,
 * calls these two, and is run by pre_fit() of mc_main.c.  static inline, as mc_files.h is and for the same reason; beside libc they
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

#endif
