/*
 * mc_ld.c -- --prune (an extension): the variants of a PLINK fileset thinned by linkage disequilibrium before anything is fitted.
 * The admixture model assumes unlinked loci; every guide to such a fit asks for this step, and without it the user leaves for
 * another program and comes back with a second fileset.
 *
 * r2 of two variants is defined in include/multiclust_hip.h (mchip_bed_ld_band): the squared correlation of the dosages over the
 * individuals typed at both, from integer sums -- the same bits wherever it is computed.
 *
 * The rule is forward greedy, as SNPRelate's snpgdsLDpruning: walk the variants in file order; variant l is removed when some
 * variant l' already kept has l - W <= l' < l, the same chromosome (first field of the .bim line, compared as a string) and
 * r2(l', l) > t; otherwise it is kept.  NaN compares false: a monomorphic or all-missing variant is never removed.  This is NOT
 * PLINK's --indep-pairwise, which drops the rarer variant of a pair and slides its window by a step.
 * mc_ld_prune_greedy states it the other way round -- a kept variant removes its successors -- which is the same rule (when the walk
 * reaches a variant, every variant before it is decided) and needs one row of the band at a time: the band comes in slabs of at most
 * `slab` first variants, MC_LD_SLAB * W doubles at the most.
 *
 * Everything in this file is libc and mc_files.h but what mc_ld_prune_data calls: the band (mchip_bed_ld_band) and the filter stage
 * (mc_filter.h: the device opened and closed, the reader's summary of the records left).  tests/ld_host_driver.c stubs the device
 * and the reader and runs the rest as a program of its own.
 */
#include "mc_cli.h"

#include <stdlib.h>
#include <string.h>

int mc_ld_prune_greedy(int L, int W, double t, int slab, mc_ld_band_fn band, void *arg, const char *const *chrom, uint8_t *keep)
{
	if (L < 1 || W < 1 || slab < 1 || !band || !keep) return MCHIP_ERR_INVALID;
	const int ns = slab < L ? slab : L;
	double *r2 = malloc(sizeof(double) * (size_t)ns * (size_t)W);
	if (!r2) return MCHIP_ERR_ALLOC;
	int rc = 0;
	memset(keep, 1, (size_t)L);
	for (int l0 = 0; l0 < L && !rc; l0 += ns) {
		const int n = L - l0 < ns ? L - l0 : ns;
		if ((rc = band(arg, l0, n, W, r2))) break;
		for (int a = 0; a < n; a++) {
			const int l = l0 + a;
			if (!keep[l]) continue;		/* a removed variant removes nothing */
			const double *row = r2 + (size_t)a * (size_t)W;
			for (int d = 1; d <= W && d < L - l; d++) {
				if (!(row[d - 1] > t)) continue;
				if (chrom && chrom[l] != chrom[l + d] && strcmp(chrom[l], chrom[l + d])) continue;
				keep[l + d] = 0;
			}
		}
	}
	free(r2);
	return rc;
}

int mc_ld_compact(int L, size_t record_bytes, const uint8_t *keep, uint8_t *bed, int *variant_of)
{
	int n = 0;
	for (int l = 0; l < L; l++) {
		if (!keep[l]) continue;
		if (n != l) memmove(bed + (size_t)n * record_bytes, bed + (size_t)l * record_bytes, record_bytes);
		if (variant_of) variant_of[n] = l;
		n++;
	}
	return n;
}

static int band_on_device(void *arg, int l0, int n_first, int window, double *r2)
{
	const mc_device_band *b = arg;
	return mchip_bed_ld_band(b->ctx, b->dat->I, b->dat->L, b->dat->bed, b->dat->bed_record_bytes, l0, n_first, window, r2);
}

/* the chromosomes of the loci held: the fileset's, read through variant_of where quality control thinned the variants before */
static int keep_by_device(const mc_cli_options *opt, mc_device_band *dev, void *keep)
{
	const mc_cli_data *dat = dev->dat;
	const char **chrom = NULL;
	if (dat->chrom && dat->variant_of) {
		if (!(chrom = malloc(sizeof *chrom * (size_t)dat->L))) return MCHIP_ERR_ALLOC;
		for (int l = 0; l < dat->L; l++) chrom[l] = dat->chrom[dat->variant_of[l]];
	}
	const int rc = mc_ld_prune_greedy(dat->L, opt->prune_window, opt->prune_t, MC_LD_SLAB, band_on_device, dev,
					  chrom ? chrom : (const char *const *)dat->chrom, keep);
	free(chrom);
	return rc;
}

int mc_ld_prune_data(const mc_cli_options *opt, mc_cli_data *dat)
{
	const int L = dat->L;
	const size_t rb = dat->bed_record_bytes;
	uint8_t *keep = malloc((size_t)L);
	int *map = malloc(sizeof(int) * (size_t)L);
	int rc = MC_EXIT_MEMORY_ALLOCATION;
	const double t_start = mc_now_s();
	if (!keep || !map) goto DONE;
	if (!dat->bed || (dat->filters_run & MC_FILTER_PRUNE) || (dat->variant_of && !(dat->filters_run & MC_FILTER_QC))) {
		rc = MC_EXIT_INTERNAL_ERROR;	/* a fileset, and not thinned before but by quality control */
		goto DONE;
	}
	if ((rc = mc_filter_on_device(opt, dat, "mc_ld.c::mc_ld_prune_data", "--prune", "the LD band", keep_by_device, keep))) goto DONE;
	/* the data set is the kept variants' from here on: their records, and the reader's summary of those */
	dat->L = mc_ld_compact(L, rb, keep, dat->bed, map);
	memset(dat->bed + (size_t)dat->L * rb, 0, 8);	/* (the reader's spare bytes behind the last record) */
	if (dat->variant_of)	/* thinned before: the places in the fileset */
		for (int l = 0; l < dat->L; l++) map[l] = dat->variant_of[map[l]];
	free(dat->variant_of);
	dat->variant_of = map;
	map = NULL;
	dat->filters_run |= MC_FILTER_PRUNE;
	rc = mc_filter_resummarize(dat, L, "mc_ld.c", "LD pruning", t_start);
DONE:
	free(keep); free(map);
	return rc;
}

static void print_variant(FILE *fp, const void *dat, int v) { fprintf(fp, "%s\n", ((const mc_cli_data *)dat)->variant_id[v]); }

/* <stem>.prune.in: the ids (second field of the .bim line) of the variants kept, one per line in file order; <stem>.prune.out: of
 * those removed.  `plink --extract <stem>.prune.in` writes the fileset the run was made on. */
int mc_write_prune_lists(const mc_cli_options *opt, const mc_cli_data *dat)
{
	if (!dat->variant_of || !dat->variant_id) return MC_EXIT_INTERNAL_ERROR;
	return mc_write_kept_lists(opt, "mc_ld.c", ".prune", dat->L_file, dat->L, dat->variant_of, print_variant, dat);
}
