/*
 * resid_host_driver.c -- TEST INFRASTRUCTURE: mc_resid.c as a program of its own, built with -fsanitize=address,undefined by
 * tests/test_resid_cpu.py.  The one device entry point mc_resid.c calls is stubbed: it returns sums made up here -- individual 1
 * without an observed copy (its row of D is 0), the others with missing data (D not symmetric).
 *
 *   resid_host_driver <I> <stem>    mc_residual_correlation + mc_resid_line + mc_write_resid to <stem>.admix.K=2.resid.txt, .resid.ind.txt
 */
#include "mc_cli.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

static int n_ind;

int mchip_residual_products(mchip_context *ctx, int slot, double *gram, double *norms)
{
	(void)ctx;
	if (slot != 1 || !gram || !norms) return MCHIP_ERR_INVALID;
	for (int i = 0; i < n_ind; i++)
		for (int j = 0; j < n_ind; j++) {
			const int lo = i < j ? i : j, hi = i < j ? j : i;
			const int dead = i == 1 || j == 1;
			gram[(size_t)i * n_ind + j] = dead ? 0.0 : (i == j ? 10.0 + i : sin(1.0 + lo * 3 + hi * 7));
			norms[(size_t)i * n_ind + j] = i == 1 ? 0.0 : (j == 1 ? 0.0 : 10.0 + i - 0.25 * ((i + 2 * j) % 3));
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
	if (argc != 3) return 2;
	n_ind = atoi(argv[1]);
	mc_data dat;
	mc_model mod;
	mc_cli_options opt;
	mc_resid_result res;
	memset(&dat, 0, sizeof dat);
	memset(&mod, 0, sizeof mod);
	memset(&opt, 0, sizeof opt);
	dat.I = n_ind;
	mod.K = 2;
	mod.pindex = 1;
	opt.outfile_name = argv[2];
	opt.em.admixture = 1;
	int rc = mc_residual_correlation(&dat, &mod, &res);
	if (rc) return 3;
	mc_resid_line(stdout, &res);
	fputc('\n', stdout);
	rc = mc_write_resid(&opt, &res);
	printf("wrote %d\n", rc);
	mc_resid_result_free(&res);
	mod.pindex = 0;		/* the stub refuses: nothing is held afterwards */
	if (mc_residual_correlation(&dat, &mod, &res) != MCHIP_ERR_INVALID || res.cor) return 4;
	return rc;
}
