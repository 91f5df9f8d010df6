/* Stand-alone driver of the two --fill writers (multiclust_amd/host/mc_impute.c) for the sanitizer build of
 * tests/test_impute_cpu.py: reads a data set with the project's readers, fills every missing copy the way the device may
 * (the first, the last or alternating real alleles; nothing where the locus has none; every third genotype left missing) and
 * writes the filled file.  The device library is not linked: the entry points the three host sources name are stubs.
 *   impute_writers_driver stru <file> <ploidy> <missing> <R> <out>     |     impute_writers_driver bed <prefix> <out prefix> */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mc_cli.h"

int mchip_progress_note(const char *w) { (void)w; return 0; }
const char *mchip_last_error(const mchip_context *c) { (void)c; return "stub"; }
int mchip_impute_missing(mchip_context *c, int s, const int32_t *n, uint8_t *g, double *f, uint64_t *a, uint64_t *b, uint64_t *d, double *e)
{
	(void)c; (void)s; (void)n; (void)g; (void)f; (void)a; (void)b; (void)d; (void)e;
	return MCHIP_ERR_NO_DEVICE;
}

static int fill(const mc_cli_data *d, const uint8_t *geno, uint8_t *filled)
{
	const mc_data md = { d->I, d->L, d->ploidy, d->uniquealleles, d->geno, NULL, d->bed, d->bed_record_bytes, NULL };
	int32_t *n_real = malloc(sizeof(int32_t) * (size_t)d->L);
	size_t n = 0;
	if (!n_real || mc_impute_n_real(&md, n_real)) { free(n_real); return 1; }
	memcpy(filled, geno, (size_t)d->I * d->L * d->ploidy);
	for (int i = 0; i < d->I; i++)
		for (int l = 0; l < d->L; l++) {
			uint8_t *g = filled + ((size_t)i * d->L + l) * d->ploidy;
			if (!n_real[l] || (i + l) % 3 == 2) continue;
			for (int a = 0; a < d->ploidy; a++)
				if (g[a] == MCHIP_MISSING) g[a] = (uint8_t)((n++ % 2) ? n_real[l] - 1 : 0);
		}
	free(n_real);
	return 0;
}

int main(int argc, char **argv)
{
	mc_cli_options o;
	mc_cli_data d;
	int rc = 2;
	memset(&o, 0, sizeof o);
	if (argc == 7 && !strcmp(argv[1], "stru")) {
		o.filename = argv[2];
		o.ploidy = atoi(argv[3]);
		o.missing_value = atoi(argv[4]);
		o.R_format = atoi(argv[5]);
		if ((rc = mc_read_structure(&o, &d))) return rc;
		uint8_t *filled = malloc((size_t)d.I * d.L * d.ploidy);
		rc = filled && !fill(&d, d.geno, filled) ? mc_write_filled_structure(&o, &d, filled, argv[6]) : 3;
		free(filled);
	} else if (argc == 4 && !strcmp(argv[1], "bed")) {
		o.bed_prefix = argv[2];
		o.ploidy = 2;
		if ((rc = mc_read_bed(&o, &d))) return rc;
		uint8_t *geno = malloc((size_t)d.I * d.L * 2), *filled = malloc((size_t)d.I * d.L * 2);
		if (geno && filled) {
			mc_bed_decode(d.I, d.L, d.bed, d.bed_record_bytes, NULL, geno);
			rc = fill(&d, geno, filled) ? 3 : mc_write_filled_bed(&o, &d, filled, argv[3]);
		} else rc = 3;
		free(geno); free(filled);
	} else {
		fprintf(stderr, "usage: %s stru <file> <ploidy> <missing> <R> <out> | bed <prefix> <out prefix>\n", argv[0]);
		return 2;
	}
	mc_free_data(&d);
	printf("wrote %d\n", rc);
	return rc;
}
