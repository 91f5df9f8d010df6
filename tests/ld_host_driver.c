/*
 * ld_host_driver.c -- TEST INFRASTRUCTURE: the libc functions of mc_ld.c as a program of its own, built plain and with
 * -fsanitize=address,undefined by tests/test_ld_cpu.py, and a plain-C restatement of the band of r2 that mchip_bed_ld_band
 * computes on the device (the definition in include/multiclust_hip.h, one pair and one individual at a time -- nothing of the
 * kernel's planes or population counts), which scripts/ld_bench.py times on one core.  The device entry points mc_ld.c names are
 * stubbed -- the band is this restatement -- and so is the reader's summary.
 *
 *   ld_host_driver greedy <L> <W> <t> <slab> <band> <chrom> <out>   band: L * W doubles; chrom: L lines, or "-" for one chromosome;
 *                                                                     out: L bytes '0' / '1' of mc_ld_prune_greedy
 *   ld_host_driver compact <L> <rb> <keep> <bed> <out> <map>         keep: L bytes '0' / '1'; bed: L * rb bytes; out: the kept
 *                                                                     records; map: one index per line.  Prints their number
 *   ld_host_driver band <I> <L> <rb> <W> <l0> <n_first> <bed> <out>  out: n_first * W doubles ("-": none); prints the seconds taken
 */
#include "mc_cli.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

static int dosage(const uint8_t *rec, int j)	/* -1 = missing */
{
	const int c = (rec[j / 4] >> (2 * (j % 4))) & 3;
	return c == 0 ? 0 : (c == 1 ? -1 : c - 1);
}

static double r2_of(int I, const uint8_t *a, const uint8_t *b)
{
	int64_t n = 0, Sx = 0, Sy = 0, Sxx = 0, Syy = 0, Sxy = 0;
	for (int j = 0; j < I; j++) {
		const int x = dosage(a, j), y = dosage(b, j);
		if (x < 0 || y < 0) continue;
		n++; Sx += x; Sy += y; Sxx += x * x; Syy += y * y; Sxy += x * y;
	}
	const int64_t C = n * Sxy - Sx * Sy, Vx = n * Sxx - Sx * Sx, Vy = n * Syy - Sy * Sy;
	if (!Vx || !Vy) return NAN;
	return ((double)C * (double)C) / ((double)Vx * (double)Vy);
}

int mchip_bed_ld_band(mchip_context *ctx, int I, int L, const uint8_t *bed, size_t record_bytes, int l0, int n_first, int window, double *r2)
{
	(void)ctx;
	if (I < 1 || L < 1 || !bed || !r2 || record_bytes < ((size_t)I + 3) / 4 || l0 < 0 || n_first < 0 || l0 + n_first > L || window < 1 ||
	    window > MCHIP_LD_MAX_WINDOW)
		return MCHIP_ERR_INVALID;
	for (int a = 0; a < n_first; a++)
		for (int d = 1; d <= window; d++) {
			const int l = l0 + a;
			r2[(size_t)a * window + d - 1] = l + d < L ? r2_of(I, bed + (size_t)l * record_bytes, bed + (size_t)(l + d) * record_bytes) : NAN;
		}
	return MCHIP_OK;
}
int mchip_create(mchip_context **ctx, int device) { (void)device; *ctx = NULL; return MCHIP_OK; }
int mchip_destroy(mchip_context *ctx) { (void)ctx; return MCHIP_OK; }
const char *mchip_last_error(const mchip_context *ctx) { (void)ctx; return ""; }
int mc_bed_summarize(mc_cli_data *dat) { (void)dat; return 0; }	/* (mc_bed.c: the reader is not part of this program) */

static void *read_all(const char *path, size_t want)
{
	FILE *f = fopen(path, "rb");
	void *buf = malloc(want ? want : 1);
	if (!f || !buf || fread(buf, 1, want, f) != want) { fprintf(stderr, "ld_host_driver: cannot read %zu bytes of '%s'\n", want, path); exit(2); }
	fclose(f);
	return buf;
}

typedef struct stored_band { const double *r2; int L, W, calls, next; } stored_band;

static int band_from_file(void *arg, int l0, int n_first, int window, double *r2)
{
	stored_band *b = arg;
	if (l0 != b->next || n_first < 1 || l0 + n_first > b->L || window != b->W) return MCHIP_ERR_INVALID;	/* slabs in order, without gaps */
	memcpy(r2, b->r2 + (size_t)l0 * window, sizeof(double) * (size_t)n_first * window);
	b->next = l0 + n_first;
	b->calls++;
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 9 && !strcmp(argv[1], "greedy")) {
		const int L = atoi(argv[2]), W = atoi(argv[3]), slab = atoi(argv[5]);
		const double t = atof(argv[4]);
		double *r2 = read_all(argv[6], sizeof(double) * (size_t)L * W);
		char **chrom = NULL, *text = NULL;
		if (strcmp(argv[7], "-")) {
			FILE *f = fopen(argv[7], "rb");
			if (!f) return 2;
			fseek(f, 0, SEEK_END);
			const long n = ftell(f);
			fseek(f, 0, SEEK_SET);
			text = read_all(argv[7], (size_t)n);
			fclose(f);
			chrom = calloc((size_t)L, sizeof *chrom);
			int l = 0;
			for (char *p = text, *eof = text + n; p < eof && l < L; l++) {
				char *q = memchr(p, '\n', (size_t)(eof - p));
				if (!q) return 2;
				*q = 0;
				chrom[l] = p;
				p = q + 1;
			}
			if (l != L) return 2;
		}
		uint8_t *keep = malloc((size_t)L);
		stored_band b = { r2, L, W, 0, 0 };
		const int rc = mc_ld_prune_greedy(L, W, t, slab, band_from_file, &b, (const char *const *)chrom, keep);
		if (rc || b.next != L || b.calls != (L + slab - 1) / slab) { fprintf(stderr, "ld_host_driver: greedy %d, %d calls, next %d\n", rc, b.calls, b.next); return 3; }
		FILE *out = fopen(argv[8], "wb");
		if (!out) return 2;
		for (int l = 0; l < L; l++) fputc(keep[l] ? '1' : '0', out);
		fclose(out);
		/* the checks of the arguments: nothing runs, nothing is written */
		if (mc_ld_prune_greedy(0, W, t, slab, band_from_file, &b, NULL, keep) != MCHIP_ERR_INVALID ||
		    mc_ld_prune_greedy(L, 0, t, slab, band_from_file, &b, NULL, keep) != MCHIP_ERR_INVALID ||
		    mc_ld_prune_greedy(L, W, t, 0, band_from_file, &b, NULL, keep) != MCHIP_ERR_INVALID ||
		    mc_ld_prune_greedy(L, W, t, slab, NULL, &b, NULL, keep) != MCHIP_ERR_INVALID) return 4;
		free(keep); free(chrom); free(text); free(r2);
		return 0;
	}
	if (argc == 8 && !strcmp(argv[1], "compact")) {
		const int L = atoi(argv[2]);
		const size_t rb = (size_t)atol(argv[3]);
		uint8_t *keep = read_all(argv[4], (size_t)L), *bed = read_all(argv[5], (size_t)L * rb);
		int *map = malloc(sizeof(int) * (size_t)L);
		for (int l = 0; l < L; l++) keep[l] = keep[l] == '1';
		const int n = mc_ld_compact(L, rb, keep, bed, map);
		FILE *out = fopen(argv[6], "wb"), *mf = fopen(argv[7], "w");
		if (!out || !mf) return 2;
		fwrite(bed, 1, (size_t)n * rb, out);
		for (int x = 0; x < n; x++) fprintf(mf, "%d\n", map[x]);
		fclose(out); fclose(mf);
		printf("%d\n", n);
		free(keep); free(bed); free(map);
		return 0;
	}
	if (argc == 10 && !strcmp(argv[1], "band")) {
		const int I = atoi(argv[2]), L = atoi(argv[3]), W = atoi(argv[5]), l0 = atoi(argv[6]), n_first = atoi(argv[7]);
		const size_t rb = (size_t)atol(argv[4]);
		uint8_t *bed = read_all(argv[8], (size_t)L * rb);
		double *r2 = malloc(sizeof(double) * (size_t)(n_first > 0 ? n_first : 1) * (size_t)(W > 0 ? W : 1));
		struct timespec t0, t1;
		clock_gettime(CLOCK_MONOTONIC, &t0);
		const int rc = mchip_bed_ld_band(NULL, I, L, bed, rb, l0, n_first, W, r2);
		clock_gettime(CLOCK_MONOTONIC, &t1);
		if (rc) return 3;
		if (strcmp(argv[9], "-")) {
			FILE *out = fopen(argv[9], "wb");
			if (!out) return 2;
			fwrite(r2, sizeof(double), (size_t)n_first * W, out);
			fclose(out);
		}
		printf("%.6f\n", (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec));
		free(bed); free(r2);
		return 0;
	}
	fprintf(stderr, "usage: ld_host_driver greedy | compact | band ... (see the head of tests/ld_host_driver.c)\n");
	return 2;
}
