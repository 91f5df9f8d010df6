/*
 * mc_king.c -- --king-cutoff (an extension): close relatives removed from a PLINK fileset before anything is fitted.  The admixture
 * model takes a family in the panel for a cluster of its own (--resid shows it afterwards, as a block of positive residual
 * correlation); every guide to such a fit asks for this step beside LD pruning, and without it the user leaves for another program
 * and comes back with a second fileset.
 *
 * The kinship phi_ij of two individuals is defined in include/multiclust_hip.h (mchip_bed_king): KING-robust (Manichaikul et al.
 * 2010, eq. 11) from four integer counts per pair over the variants of the data set -- all of them: keeping to the autosomes is the
 * user's --extract -- the same bits wherever it is computed.  Two individuals are related when phi_ij > t; NaN compares false.
 *
 * The rule is greedy and this project's own: while some pair of remaining individuals is related, the remaining individual with
 * the most remaining related partners is removed; of several with as many, the one with the highest index, so that the individual
 * earlier in the .fam file stays.  It is in the spirit of PLINK 2's --king-cutoff and NOT its algorithm, and what it keeps is not a
 * maximum independent set of the relatedness graph: no two kept individuals are related, nothing more is claimed.
 *
 * The kinships come in slabs of at most `slab` rows against all individuals; the host keeps one slab (24 bytes a pair) and the
 * relatedness graph as an I x I bit matrix, I * I / 8 bytes: its only memory quadratic in I.
 *
 * Everything in this file is libc and mc_files.h but what mc_king_data calls: the kinships (mchip_bed_king), the filter stage
 * (mc_filter.h: the device opened and closed, the per-individual fields and the reader's summary made anew) and the reader's decoder (mc_bed_lazy_new, mc_bed.c).
 * tests/king_host_driver.c stubs the device and the reader and runs the rest as a program of its own.
 */
#include "mc_cli.h"

#include <stdlib.h>
#include <string.h>

static size_t row_words(int I) { return ((size_t)I + 63) / 64; }

int mc_king_edges(int I, double t, int slab, mc_king_band_fn band, void *arg, uint64_t **bits_out, mc_king_pair **pairs_out, size_t *n_pairs_out)
{
	if (I < 1 || slab < 1 || !band || !bits_out || !pairs_out || !n_pairs_out) return MCHIP_ERR_INVALID;
	const int ns = slab < I ? slab : I;
	const size_t rw = row_words(I);
	double *phi = malloc(sizeof(double) * (size_t)ns * (size_t)I);
	uint32_t *counts = malloc(sizeof(uint32_t) * 4 * (size_t)ns * (size_t)I);
	uint64_t *bits = calloc((size_t)I * rw, sizeof *bits);
	mc_king_pair *pairs = NULL;
	size_t n_pairs = 0, cap = 0;
	int rc = (phi && counts && bits) ? 0 : MCHIP_ERR_ALLOC;
	for (int i0 = 0; i0 < I && !rc; i0 += ns) {
		const int n = I - i0 < ns ? I - i0 : ns;
		if ((rc = band(arg, i0, n, phi, counts))) break;
		for (int a = 0; a < n && !rc; a++) {
			const int i = i0 + a;
			const double *row = phi + (size_t)a * (size_t)I;
			for (int j = 0; j < I; j++) {
				if (j == i || !(row[j] > t)) continue;
				bits[(size_t)i * rw + (size_t)j / 64] |= 1ull << (j % 64);
				if (j < i) continue;
				if (n_pairs == cap) {
					const size_t cap2 = cap ? 2 * cap : 64;
					mc_king_pair *p2 = realloc(pairs, sizeof *pairs * cap2);
					if (!p2) { rc = MCHIP_ERR_ALLOC; break; }
					pairs = p2;
					cap = cap2;
				}
				const uint32_t *c = counts + 4 * ((size_t)a * (size_t)I + (size_t)j);
				pairs[n_pairs++] = (mc_king_pair){ i, j, c[0], c[1], c[2], row[j] };
			}
		}
	}
	free(phi); free(counts);
	if (rc) { free(bits); free(pairs); return rc; }
	*bits_out = bits;
	*pairs_out = pairs;
	*n_pairs_out = n_pairs;
	return 0;
}

int mc_king_select(int I, const uint64_t *bits, uint8_t *keep)
{
	if (I < 1 || !bits || !keep) return MCHIP_ERR_INVALID;
	const size_t rw = row_words(I);
	int *deg = malloc(sizeof(int) * (size_t)I);
	if (!deg) return MCHIP_ERR_ALLOC;
	for (int i = 0; i < I; i++) {
		deg[i] = 0;
		for (size_t w = 0; w < rw; w++) deg[i] += __builtin_popcountll(bits[(size_t)i * rw + w]);
	}
	memset(keep, 1, (size_t)I);
	for (;;) {
		int worst = -1;
		for (int i = 0; i < I; i++)
			if (keep[i] && deg[i] > 0 && (worst < 0 || deg[i] >= deg[worst])) worst = i;	/* >=: of equals the highest index */
		if (worst < 0) break;
		keep[worst] = 0;
		for (size_t w = 0; w < rw; w++)
			for (uint64_t m = bits[(size_t)worst * rw + w]; m; m &= m - 1) {
				const int j = (int)(64 * w) + __builtin_ctzll(m);
				if (keep[j]) deg[j]--;
			}
	}
	free(deg);
	return 0;
}

int mc_king_compact(int I, int L, size_t record_bytes, const uint8_t *keep, uint8_t *bed, int *individual_of)
{
	int n = 0;
	for (int i = 0; i < I; i++)
		if (keep[i]) { if (individual_of) individual_of[n] = i; n++; }
	const size_t rb2 = ((size_t)n + 3) / 4;
	uint8_t *rec = calloc(rb2 ? rb2 : 1, 1);
	if (!rec) return -1;
	for (int l = 0; l < L; l++) {
		const uint8_t *src = bed + (size_t)l * record_bytes;
		memset(rec, 0, rb2);
		for (int i = 0, x = 0; i < I; i++) {
			if (!keep[i]) continue;
			rec[x / 4] |= (uint8_t)(((src[i / 4] >> (2 * (i % 4))) & 3) << (2 * (x % 4)));
			x++;
		}
		memcpy(bed + (size_t)l * rb2, rec, rb2);	/* (at or before the record just read: nothing unread is written over) */
	}
	memset(bed + (size_t)L * rb2, 0, 8);	/* the reader's spare bytes behind the last record */
	free(rec);
	return n;
}

static int band_on_device(void *arg, int i0, int n_rows, double *phi, uint32_t *counts)
{
	const mc_device_band *b = arg;
	return mchip_bed_king(b->ctx, b->dat->I, b->dat->L, b->dat->bed, b->dat->bed_record_bytes, i0, n_rows, phi, counts);
}

typedef struct king_graph {
	uint64_t *bits;
	mc_king_pair *pairs;
	size_t n_pairs;
} king_graph;

static int edges_by_device(const mc_cli_options *opt, mc_device_band *dev, void *out)
{
	king_graph *g = out;
	return mc_king_edges(dev->dat->I, opt->king_t, MC_KING_SLAB, band_on_device, dev, &g->bits, &g->pairs, &g->n_pairs);
}

int mc_king_data(const mc_cli_options *opt, mc_cli_data *dat)
{
	const int I = dat->I, L = dat->L;
	uint8_t *keep = malloc((size_t)I);
	int *map = malloc(sizeof(int) * (size_t)I);
	king_graph g = { NULL, NULL, 0 };
	int rc = MC_EXIT_MEMORY_ALLOCATION;
	const double t_start = mc_now_s();
	if (!keep || !map) goto DONE;
	if (!dat->bed || (dat->filters_run & MC_FILTER_KING) || (dat->individual_of && !(dat->filters_run & MC_FILTER_QC))) {
		rc = MC_EXIT_INTERNAL_ERROR;	/* a fileset, and not thinned before but by quality control */
		goto DONE;
	}
	if ((rc = mc_filter_on_device(opt, dat, "mc_king.c::mc_king_data", "--king-cutoff", "the kinship matrix", edges_by_device, &g))) goto DONE;
	if ((rc = mc_king_select(I, g.bits, keep))) goto DONE;
	/* the data set is the kept individuals' from here on: their codes in every record, their ids, and the reader's summary of those */
	const int n = mc_king_compact(I, L, dat->bed_record_bytes, keep, dat->bed, map);
	if (n < 1) { rc = MC_EXIT_MEMORY_ALLOCATION; goto DONE; }
	dat->bed_record_bytes = ((size_t)n + 3) / 4;
	if ((rc = mc_filter_rebuild_individuals(dat, n, map))) goto DONE;
	if (dat->individual_of) {	/* thinned before: the places in the fileset, of the kept ones and of the pairs */
		for (int x = 0; x < n; x++) map[x] = dat->individual_of[map[x]];
		for (size_t p = 0; p < g.n_pairs; p++) { g.pairs[p].i = dat->individual_of[g.pairs[p].i]; g.pairs[p].j = dat->individual_of[g.pairs[p].j]; }
		free(dat->individual_of);
	}
	dat->individual_of = map;
	map = NULL;
	dat->filters_run |= MC_FILTER_KING;
	dat->king_pairs = g.pairs;
	dat->n_king_pairs = g.n_pairs;
	g.pairs = NULL;
	if (dat->lazy) {	/* (nothing has been decoded yet; a decoded genotype would be the file's) */
		dat->lazy->release(dat->lazy);
		if (!(dat->lazy = mc_bed_lazy_new())) { rc = MC_EXIT_MEMORY_ALLOCATION; goto DONE; }
	}
	rc = mc_filter_resummarize(dat, L, "mc_king.c", "relatedness", t_start);
DONE:
	free(keep); free(map); free(g.bits); free(g.pairs);
	return rc;
}

static void print_individual(FILE *fp, const void *dat, int v)
{
	fprintf(fp, "%s\t%s\n", ((const mc_cli_data *)dat)->fam_fid[v], ((const mc_cli_data *)dat)->fam_iid[v]);
}

/* <stem>.king.cutoff.in: "FID\tIID" of the individuals kept, one per line in file order; <stem>.king.cutoff.out: of those removed
 * (`plink --keep <stem>.king.cutoff.in` writes the fileset the run was made on).  <stem>.king.kin0: one header line, then one line
 * per pair i < j with phi > t in (i, j) order: the two ids, N_SNP = n_ij, HETHET = hh_ij / n_ij, IBS0 = op_ij / n_ij and KINSHIP =
 * phi_ij, the three ratios as %.6f. */
int mc_write_king_lists(const mc_cli_options *opt, const mc_cli_data *dat)
{
	char path[4400];
	int rc;
	if (!dat->individual_of || !dat->fam_fid || !dat->fam_iid) return MC_EXIT_INTERNAL_ERROR;
	if ((rc = mc_write_kept_lists(opt, "mc_king.c", ".king.cutoff", dat->I_file, dat->I, dat->individual_of, print_individual, dat))) return rc;
	mc_result_path(opt, path, sizeof path, ".king.kin0");
	FILE *kin = mc_open_result("mc_king.c", path, "w");
	if (!kin) return MC_EXIT_FILE_OPEN_ERROR;
	fprintf(kin, "FID1\tIID1\tFID2\tIID2\tN_SNP\tHETHET\tIBS0\tKINSHIP\n");
	for (size_t p = 0; p < dat->n_king_pairs; p++) {
		const mc_king_pair *k = &dat->king_pairs[p];
		fprintf(kin, "%s\t%s\t%s\t%s\t%u\t%.6f\t%.6f\t%.6f\n", dat->fam_fid[k->i], dat->fam_iid[k->i], dat->fam_fid[k->j], dat->fam_iid[k->j],
			(unsigned)k->n, (double)k->hh / (double)k->n, (double)k->op / (double)k->n, k->phi);
	}
	return mc_close_result(kin);
}
