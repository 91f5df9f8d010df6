/*
 * king_host_driver.c -- TEST INFRASTRUCTURE: the libc functions of mc_king.c as a program of its own, built plain and with
 * -fsanitize=address,undefined by tests/test_king_cpu.py, and a plain-C restatement of the kinships and counts that mchip_bed_king
 * computes on the device (the definition in include/multiclust_hip.h, one pair and one variant at a time -- nothing of the kernel's
 * planes or population counts).  The device entry points mc_king.c names are stubbed -- the band is this restatement -- and so are
 * the reader's summary and its decoder.
 *
 *   king_host_driver band <I> <L> <rb> <i0> <n_rows> <bed> <phi> <counts>   phi: n_rows * I doubles; counts: n_rows * I * 4 uint32
 *   king_host_driver select <I> <rel> <out>                                   rel: I * I bytes '0' / '1'; out: I bytes '0' / '1' of
 *                                                                             mc_king_select
 *   king_host_driver compact <I> <L> <rb> <keep> <bed> <out> <map>            keep: I bytes '0' / '1'; bed: L * rb bytes; out: the
 *                                                                             records repacked and the 8 bytes behind them; map: one
 *                                                                             index per line.  Prints I'
 *   king_host_driver data <I> <L> <rb> <t> <slab> <bed> <fam> <stem> <out>    fam: I lines "FID IID"; mc_king_edges in slabs of
 *                                                                             `slab` rows against the rest of mc_king_data, then
 *                                                                             mc_king_data itself and mc_write_king_lists on <stem>;
 *                                                                             out: the data set's per-individual fields as text
 */
#include "mc_cli.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

static int code(const uint8_t *bed, size_t rb, int l, int i) { return (bed[(size_t)l * rb + (size_t)i / 4] >> (2 * (i % 4))) & 3; }

int mchip_bed_king(mchip_context *ctx, int I, int L, const uint8_t *bed, size_t record_bytes, int i0, int n_rows, double *phi, uint32_t *counts)
{
	(void)ctx;
	if (I < 1 || L < 1 || !bed || !phi || record_bytes < ((size_t)I + 3) / 4 || i0 < 0 || n_rows < 0 || (long long)i0 + n_rows > I) return MCHIP_ERR_INVALID;
	for (int a = 0; a < n_rows; a++)
		for (int j = 0; j < I; j++) {
			const int i = i0 + a;
			int64_t n = 0, hh = 0, op = 0, hij = 0, hji = 0;
			for (int l = 0; l < L; l++) {
				const int x = code(bed, record_bytes, l, i), y = code(bed, record_bytes, l, j);
				if (x == 1 || y == 1) continue;
				n++;
				hh += x == 2 && y == 2;
				op += (x == 0 && y == 3) || (x == 3 && y == 0);
				hij += x == 2;
				hji += y == 2;
			}
			const int64_t m = hij < hji ? hij : hji, num = 2 * hh - 4 * op - hij - hji + 2 * m;
			const size_t p = (size_t)a * (size_t)I + (size_t)j;
			phi[p] = m ? (double)num / (double)(4 * m) : NAN;
			if (counts) { counts[4 * p] = (uint32_t)n; counts[4 * p + 1] = (uint32_t)hh; counts[4 * p + 2] = (uint32_t)op; counts[4 * p + 3] = (uint32_t)hij; }
		}
	return MCHIP_OK;
}
int mchip_create(mchip_context **ctx, int device) { (void)device; *ctx = NULL; return MCHIP_OK; }
int mchip_destroy(mchip_context *ctx) { (void)ctx; return MCHIP_OK; }
const char *mchip_last_error(const mchip_context *ctx) { (void)ctx; return ""; }
/* (mc_bed.c: the reader is not part of this program) */
static int summarized;
int mc_bed_summarize(mc_cli_data *dat) { (void)dat; summarized++; return 0; }
static void lazy_release(mc_lazy_geno *self) { free(self); }
static int lazies;
mc_lazy_geno *mc_bed_lazy_new(void)
{
	mc_lazy_geno *z = calloc(1, sizeof *z);
	if (z) { z->release = lazy_release; lazies++; }
	return z;
}

static void *read_all(const char *path, size_t want, size_t spare)
{
	FILE *f = fopen(path, "rb");
	uint8_t *buf = calloc(want + spare + 1, 1);
	if (!f || !buf || fread(buf, 1, want, f) != want) { fprintf(stderr, "king_host_driver: cannot read %zu bytes of '%s'\n", want, path); exit(2); }
	fclose(f);
	return buf;
}

typedef struct cpu_band { int I, L; size_t rb; const uint8_t *bed; int calls, next, slab; } cpu_band;

static int band_in_order(void *arg, int i0, int n_rows, double *phi, uint32_t *counts)
{
	cpu_band *b = arg;
	if (i0 != b->next || n_rows < 1 || n_rows > b->slab || i0 + n_rows > b->I) return MCHIP_ERR_INVALID;	/* slabs in order, without gaps */
	b->next = i0 + n_rows;
	b->calls++;
	return mchip_bed_king(NULL, b->I, b->L, b->bed, b->rb, i0, n_rows, phi, counts);
}

int main(int argc, char **argv)
{
	if (argc == 10 && !strcmp(argv[1], "band")) {
		const int I = atoi(argv[2]), L = atoi(argv[3]), i0 = atoi(argv[5]), n_rows = atoi(argv[6]);
		const size_t rb = (size_t)atol(argv[4]), np = (size_t)(n_rows > 0 ? n_rows : 0) * (size_t)I;
		uint8_t *bed = read_all(argv[7], (size_t)L * rb, 0);
		double *phi = malloc(sizeof(double) * (np ? np : 1));
		uint32_t *counts = malloc(sizeof(uint32_t) * 4 * (np ? np : 1));
		if (mchip_bed_king(NULL, I, L, bed, rb, i0, n_rows, phi, counts)) return 3;
		FILE *pf = fopen(argv[8], "wb"), *cf = fopen(argv[9], "wb");
		if (!pf || !cf) return 2;
		fwrite(phi, sizeof(double), np, pf);
		fwrite(counts, sizeof(uint32_t), 4 * np, cf);
		fclose(pf); fclose(cf);
		free(bed); free(phi); free(counts);
		return 0;
	}
	if (argc == 5 && !strcmp(argv[1], "select")) {
		const int I = atoi(argv[2]);
		const size_t rw = ((size_t)I + 63) / 64;
		uint8_t *rel = read_all(argv[3], (size_t)I * (size_t)I, 0), *keep = malloc((size_t)I);
		uint64_t *bits = calloc((size_t)I * rw, sizeof *bits);
		for (int i = 0; i < I; i++)
			for (int j = 0; j < I; j++)
				if (rel[(size_t)i * I + j] == '1') bits[(size_t)i * rw + (size_t)j / 64] |= 1ull << (j % 64);
		if (mc_king_select(I, bits, keep)) return 3;
		if (mc_king_select(0, bits, keep) != MCHIP_ERR_INVALID || mc_king_select(I, NULL, keep) != MCHIP_ERR_INVALID ||
		    mc_king_select(I, bits, NULL) != MCHIP_ERR_INVALID) return 4;
		FILE *out = fopen(argv[4], "wb");
		if (!out) return 2;
		for (int i = 0; i < I; i++) fputc(keep[i] ? '1' : '0', out);
		fclose(out);
		free(rel); free(keep); free(bits);
		return 0;
	}
	if (argc == 9 && !strcmp(argv[1], "compact")) {
		const int I = atoi(argv[2]), L = atoi(argv[3]);
		const size_t rb = (size_t)atol(argv[4]);
		uint8_t *keep = read_all(argv[5], (size_t)I, 0), *bed = read_all(argv[6], (size_t)L * rb, 8);
		int *map = malloc(sizeof(int) * (size_t)I);
		memset(bed + (size_t)L * rb, 0xAB, 8);	/* (the spare bytes are the function's to clear, wherever they end up) */
		for (int i = 0; i < I; i++) keep[i] = keep[i] == '1';
		const int n = mc_king_compact(I, L, rb, keep, bed, map);
		if (n < 0) return 3;
		FILE *out = fopen(argv[7], "wb"), *mf = fopen(argv[8], "w");
		if (!out || !mf) return 2;
		fwrite(bed, 1, (size_t)L * (((size_t)n + 3) / 4) + 8, out);
		for (int x = 0; x < n; x++) fprintf(mf, "%d\n", map[x]);
		fclose(out); fclose(mf);
		printf("%d\n", n);
		free(keep); free(bed); free(map);
		return 0;
	}
	if (argc == 11 && !strcmp(argv[1], "data")) {
		const int I = atoi(argv[2]), L = atoi(argv[3]), slab = atoi(argv[6]);
		const size_t rb = (size_t)atol(argv[4]);
		const double t = atof(argv[5]);
		mc_cli_options opt;
		mc_cli_data dat;
		memset(&opt, 0, sizeof opt);
		memset(&dat, 0, sizeof dat);
		opt.king = 1; opt.king_t = t; opt.outfile_name = argv[9];
		dat.I = I; dat.L = dat.L_file = L; dat.ploidy = 2;
		dat.bed = read_all(argv[7], (size_t)L * rb, 8);
		dat.bed_record_bytes = rb;
		if (!(dat.lazy = mc_bed_lazy_new())) return 2;
		/* the ids as read_fam (mc_bed.c) holds them: locales numbered in order of first appearance */
		FILE *fam = fopen(argv[8], "r");
		if (!fam) return 2;
		dat.names = calloc((size_t)I, sizeof *dat.names);
		dat.locale = calloc((size_t)I, sizeof *dat.locale);
		dat.pops = calloc((size_t)I, sizeof *dat.pops);
		for (int i = 0; i < I; i++) {
			char fid[256], iid[256];
			if (fscanf(fam, "%255s %255s", fid, iid) != 2) return 2;
			int found = -1;
			for (int p = 0; p < dat.numpops; p++) if (!strcmp(dat.pops[p], fid)) found = p;
			if (found < 0) { dat.pops[dat.numpops] = strdup(fid); found = dat.numpops++; }
			dat.locale[i] = found;
			dat.names[i] = strdup(iid);
		}
		fclose(fam);
		dat.i_p = calloc((size_t)dat.numpops, sizeof *dat.i_p);
		for (int i = 0; i < I; i++) dat.i_p[dat.locale[i]]++;
		/* the edges in slabs of the size asked for: the same graph and pairs whatever the slab */
		cpu_band b = { I, L, rb, dat.bed, 0, 0, slab };
		uint64_t *bits = NULL;
		mc_king_pair *pairs = NULL;
		size_t n_pairs = 0;
		int rc = mc_king_edges(I, t, slab, band_in_order, &b, &bits, &pairs, &n_pairs);
		if (rc || b.next != I || b.calls != (I + slab - 1) / slab) { fprintf(stderr, "king_host_driver: edges %d, %d calls, next %d\n", rc, b.calls, b.next); return 3; }
		if (mc_king_edges(0, t, slab, band_in_order, &b, &bits, &pairs, &n_pairs) != MCHIP_ERR_INVALID ||
		    mc_king_edges(I, t, 0, band_in_order, &b, &bits, &pairs, &n_pairs) != MCHIP_ERR_INVALID ||
		    mc_king_edges(I, t, slab, NULL, &b, &bits, &pairs, &n_pairs) != MCHIP_ERR_INVALID) return 4;
		if ((rc = mc_king_data(&opt, &dat))) { fprintf(stderr, "king_host_driver: mc_king_data %d\n", rc); return 3; }
		if (summarized != 1 || lazies != 2) return 5;		/* the summary made once, the decoder made anew */
		if (dat.n_king_pairs != n_pairs) return 6;
		for (size_t p = 0; p < n_pairs; p++) {
			const mc_king_pair *x = &dat.king_pairs[p], *y = &pairs[p];
			if (x->i != y->i || x->j != y->j || x->n != y->n || x->hh != y->hh || x->op != y->op || memcmp(&x->phi, &y->phi, sizeof x->phi)) return 6;
		}
		const size_t rw = ((size_t)I + 63) / 64;
		for (size_t p = 0; p < n_pairs; p++) {		/* the pairs are the upper triangle of the graph, and the graph is symmetric */
			const int i = pairs[p].i, j = pairs[p].j;
			if (!(i < j) || !(bits[(size_t)i * rw + (size_t)j / 64] >> (j % 64) & 1) || !(bits[(size_t)j * rw + (size_t)i / 64] >> (i % 64) & 1)) return 7;
		}
		if (mc_king_data(&opt, &dat) != MC_EXIT_INTERNAL_ERROR) return 8;	/* not twice */
		if ((rc = mc_write_king_lists(&opt, &dat))) return 9;
		FILE *out = fopen(argv[10], "w");
		if (!out) return 2;
		fprintf(out, "I %d I_file %d record_bytes %zu numpops %d pairs %zu\n", dat.I, dat.I_file, dat.bed_record_bytes, dat.numpops, dat.n_king_pairs);
		for (int i = 0; i < dat.I; i++) fprintf(out, "%d %s %d %s\n", dat.individual_of[i], dat.names[i], dat.locale[i], dat.pops[dat.locale[i]]);
		for (int p = 0; p < dat.numpops; p++) fprintf(out, "pop %s %d\n", dat.pops[p], dat.i_p[p]);
		for (size_t x = 0; x < (size_t)L * dat.bed_record_bytes + 8; x++) fprintf(out, "%02x", dat.bed[x]);
		fprintf(out, "\n");
		fclose(out);
		for (int i = 0; i < dat.I; i++) free(dat.names[i]);
		for (int p = 0; p < dat.numpops; p++) free(dat.pops[p]);
		for (int i = 0; i < dat.I_file; i++) { free(dat.fam_fid[i]); free(dat.fam_iid[i]); }
		free(dat.names); free(dat.pops); free(dat.locale); free(dat.i_p); free(dat.fam_fid); free(dat.fam_iid);
		free(dat.individual_of); free(dat.king_pairs); free(dat.bed);
		dat.lazy->release(dat.lazy);
		free(bits); free(pairs);
		return 0;
	}
	fprintf(stderr, "usage: king_host_driver band | select | compact | data ... (see the head of tests/king_host_driver.c)\n");
	return 2;
}
