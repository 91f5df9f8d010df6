/*
 * kinship_host_driver.c -- TEST INFRASTRUCTURE: mc_kinship.c as a program of its own, built with -fsanitize=address,undefined by
 * tests/test_kinship_cpu.py, which restates the sums made up here (driver_sums) and what mc_kinship.c has to make of them.  The one
 * device entry point mc_kinship.c calls is stubbed: individual 1 without an observed copy (its row and column of V are 0), pairs whose
 * phi lies exactly on each degree cut and just above it, the rest small.
 *
 *   kinship_host_driver <I> <ploidy> <t> <stem>    mc_kinship + mc_kinship_line + mc_write_kinship to <stem>.admix.K=2.kin0, .kin.ind.txt
 */
#include "mc_cli.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

static int n_ind;

int mchip_kinship_products(mchip_context *ctx, int slot, double *gram, double *scale)
{
	static const double ladder[4] = { 0.354, 0.177, 0.0884, 0.0442 };
	(void)ctx;
	if (slot != 1 || !gram || !scale) return MCHIP_ERR_INVALID;
	for (int i = 0; i < n_ind; i++)
		for (int j = 0; j < n_ind; j++) {
			const int lo = i < j ? i : j, hi = i < j ? j : i;
			double g = 0.0, v = 0.0;
			if (i != 1 && j != 1) {
				v = 8.0 + lo + 2 * hi;
				if (i == j) g = v * (0.5 + 0.03125 * (i % 3));
				else if (lo == 0 && hi >= 2 && hi < 6) { v = 16.0; g = 16.0 * ladder[hi - 2]; }
				else if (lo == 2 && hi >= 3 && hi < 7) g = v * (ladder[hi - 3] + 0.001);
				else g = v * 0.01 * (double)((lo * 3 + hi * 7) % 11 - 5) / 8.0;
			}
			gram[(size_t)i * n_ind + j] = g;
			scale[(size_t)i * n_ind + j] = v;
		}
	return MCHIP_OK;
}

const char *mchip_last_error(const mchip_context *ctx)
{
	(void)ctx;
	return "";
}

int main(int argc, char **argv)
{
	if (argc != 5) return 2;
	n_ind = atoi(argv[1]);
	mc_data dat;
	mc_model mod;
	mc_cli_options opt;
	mc_kinship_result res;
	memset(&dat, 0, sizeof dat);
	memset(&mod, 0, sizeof mod);
	memset(&opt, 0, sizeof opt);
	dat.I = n_ind;
	dat.ploidy = atoi(argv[2]);
	mod.K = 2;
	mod.pindex = 1;
	opt.outfile_name = argv[4];
	opt.em.admixture = 1;
	int rc = mc_kinship(&dat, &mod, strtod(argv[3], NULL), &res);
	if (rc) return 3;
	mc_kinship_line(stdout, &res);
	fputc('\n', stdout);
	rc = mc_write_kinship(&opt, &res);
	printf("wrote %d\n", rc);
	mc_kinship_result_free(&res);
	mod.pindex = 0;		/* the stub refuses: nothing is held afterwards */
	if (mc_kinship(&dat, &mod, 0.1, &res) != MCHIP_ERR_INVALID || res.pairs || res.self) return 4;
	if (mc_kinship_degree(NAN) != 4 || mc_kinship_degree(0.354) != 1 || mc_kinship_degree(0.3541) != 0) return 5;
	return rc;
}
