/*
 * qc_host_driver.c -- TEST INFRASTRUCTURE: mc_qc.c, and mc_ld.c and mc_king.c on an axis that quality control thinned before, as a
 * program of its own, built plain and with -fsanitize=address,undefined by tests/test_qc_cpu.py.  The device entry points are stubbed
 * with plain-C restatements of the definitions in include/multiclust_hip.h, one individual and one variant at a time -- nothing of the
 * kernels' planes or population counts; tests/test_qc_cpu.py holds the stub of mchip_bed_qc to tests/qc_util.py first ("counts") --
 * and so are the reader's summary and its decoder.
 *
 *   qc_host_driver counts <I> <L> <rb> <bed> <keep | -> <ind> <var> <p>   keep: I bytes '0' / '1'; ind: I * 4 uint32; var: L * 4
 *                                                                           uint32; p: L doubles
 *   qc_host_driver chain <I> <L> <rb> <bed> <fam> <bim> <stem> <out> <mind> <geno> <maf> <hwe> <prune_t> <prune_w> <king_t>
 *                  fam: I lines "FID IID"; bim: L lines "chrom id"; thresholds, "-" = the option is not given.  mc_qc_data, its
 *                  line and lists, then mc_ld_prune_data and mc_king_data with theirs on <stem>; out: the line, what each filter
 *                  saw and left, and the data set's fields as text.  An emptied data set: prints "emptied" and the status
 */
#include "mc_cli.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

static int code(const uint8_t *bed, size_t rb, int l, int i) { return (bed[(size_t)l * rb + (size_t)i / 4] >> (2 * (i % 4))) & 3; }

static double hwe_p(int64_t n0, int64_t n2, int64_t n3)
{
	const int64_t N = n0 + n2 + n3;
	if (!N) return 1.0;
	const int64_t r = 2 * (n0 < n3 ? n0 : n3) + n2;
	int64_t mid = r * (2 * N - r) / (2 * N);
	if ((mid ^ r) & 1) mid++;
	double S = 0, T = 0, w_obs = 0;
	for (int pass = 0; pass < 2; pass++) {
		const double bound = w_obs * 1.0000001;
		int64_t h = mid, a = (r - mid) / 2, b = N - h - a;
		volatile double w = 1.0;	/* (volatile: every product and quotient is rounded to double where it stands) */
		if (!pass) { S += w; if (h == n2) w_obs = w; } else if (w <= bound) T += w;
		while (h >= 2) {
			w = w * (double)(h * (h - 1));
			w = w / (double)(4 * (a + 1) * (b + 1));
			h -= 2; a++; b++;
			if (!pass) { S += w; if (h == n2) w_obs = w; } else if (w <= bound) T += w;
		}
		h = mid; a = (r - mid) / 2; b = N - h - a; w = 1.0;
		while (h <= r - 2) {
			w = w * (double)(4 * a * b);
			w = w / (double)((h + 2) * (h + 1));
			h += 2; a--; b--;
			if (!pass) { S += w; if (h == n2) w_obs = w; } else if (w <= bound) T += w;
		}
	}
	const double p = T / S;
	return p > 1.0 ? 1.0 : p;
}

static int qc_calls, qc_calls_with_keep;
int mchip_bed_qc(mchip_context *ctx, int I, int L, const uint8_t *bed, size_t record_bytes, const uint8_t *ind_keep, uint32_t *ind_counts,
		 uint32_t *var_counts, double *hwe)
{
	(void)ctx;
	if (I < 1 || L < 1 || !bed || record_bytes < ((size_t)I + 3) / 4 || (!ind_counts && !var_counts && !hwe)) return MCHIP_ERR_INVALID;
	qc_calls++;
	qc_calls_with_keep += ind_keep != NULL;
	if (ind_counts) {
		memset(ind_counts, 0, sizeof(uint32_t) * 4 * (size_t)I);
		for (int l = 0; l < L; l++)
			for (int i = 0; i < I; i++) ind_counts[4 * (size_t)i + code(bed, record_bytes, l, i)]++;
	}
	for (int l = 0; l < L && (var_counts || hwe); l++) {
		uint32_t c[4] = { 0, 0, 0, 0 };
		for (int i = 0; i < I; i++)
			if (!ind_keep || ind_keep[i]) c[code(bed, record_bytes, l, i)]++;
		if (var_counts) memcpy(var_counts + 4 * (size_t)l, c, sizeof c);
		if (hwe) hwe[l] = hwe_p(c[0], c[2], c[3]);
	}
	return MCHIP_OK;
}

static int dosage(int c) { return c == 0 ? 0 : (c == 1 ? -1 : c - 1); }
int mchip_bed_ld_band(mchip_context *ctx, int I, int L, const uint8_t *bed, size_t record_bytes, int l0, int n_first, int window, double *r2)
{
	(void)ctx;
	if (I < 1 || L < 1 || !bed || !r2 || record_bytes < ((size_t)I + 3) / 4 || l0 < 0 || n_first < 0 || l0 + n_first > L || window < 1) return MCHIP_ERR_INVALID;
	for (int a = 0; a < n_first; a++)
		for (int d = 1; d <= window; d++) {
			const int l = l0 + a;
			double out = NAN;
			if (l + d < L) {
				int64_t n = 0, Sx = 0, Sy = 0, Sxx = 0, Syy = 0, Sxy = 0;
				for (int j = 0; j < I; j++) {
					const int x = dosage(code(bed, record_bytes, l, j)), y = dosage(code(bed, record_bytes, l + d, j));
					if (x < 0 || y < 0) continue;
					n++; Sx += x; Sy += y; Sxx += x * x; Syy += y * y; Sxy += x * y;
				}
				const int64_t C = n * Sxy - Sx * Sy, Vx = n * Sxx - Sx * Sx, Vy = n * Syy - Sy * Sy;
				if (Vx && Vy) out = ((double)C * (double)C) / ((double)Vx * (double)Vy);
			}
			r2[(size_t)a * window + d - 1] = out;
		}
	return MCHIP_OK;
}

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
mc_lazy_geno *mc_bed_lazy_new(void)
{
	mc_lazy_geno *z = calloc(1, sizeof *z);
	if (z) z->release = lazy_release;
	return z;
}

static void *read_all(const char *path, size_t want, size_t spare)
{
	FILE *f = fopen(path, "rb");
	uint8_t *buf = calloc(want + spare + 1, 1);
	if (!f || !buf || fread(buf, 1, want, f) != want) { fprintf(stderr, "qc_host_driver: cannot read %zu bytes of '%s'\n", want, path); exit(2); }
	fclose(f);
	return buf;
}

static int threshold(const char *arg, double *t)
{
	if (!strcmp(arg, "-")) return 0;
	*t = atof(arg);
	return 1;
}

static void release(mc_cli_data *d)
{
	for (int i = 0; i < d->I; i++) free(d->names[i]);
	for (int p = 0; p < d->numpops; p++) free(d->pops[p]);
	for (int i = 0; i < d->I_file; i++) { if (d->fam_fid) free(d->fam_fid[i]); if (d->fam_iid) free(d->fam_iid[i]); }
	for (int l = 0; l < d->L_file; l++) { free(d->chrom[l]); free(d->variant_id[l]); }
	free(d->names); free(d->pops); free(d->locale); free(d->i_p); free(d->fam_fid); free(d->fam_iid); free(d->chrom); free(d->variant_id);
	free(d->individual_of); free(d->variant_of); free(d->king_pairs); free(d->bed);
	mc_qc_result_free(d->qc);
	if (d->lazy) d->lazy->release(d->lazy);
}

int main(int argc, char **argv)
{
	if (argc == 10 && !strcmp(argv[1], "counts")) {
		const int I = atoi(argv[2]), L = atoi(argv[3]);
		const size_t rb = (size_t)atol(argv[4]);
		uint8_t *bed = read_all(argv[5], (size_t)L * rb, 0), *keep = strcmp(argv[6], "-") ? read_all(argv[6], (size_t)I, 0) : NULL;
		uint32_t *ind = malloc(sizeof(uint32_t) * 4 * (size_t)I), *var = malloc(sizeof(uint32_t) * 4 * (size_t)L);
		double *p = malloc(sizeof(double) * (size_t)L);
		for (int i = 0; keep && i < I; i++) keep[i] = keep[i] == '1';
		if (mchip_bed_qc(NULL, I, L, bed, rb, keep, ind, var, p)) return 3;
		FILE *fi = fopen(argv[7], "wb"), *fv = fopen(argv[8], "wb"), *fp = fopen(argv[9], "wb");
		if (!fi || !fv || !fp) return 2;
		fwrite(ind, sizeof(uint32_t), 4 * (size_t)I, fi);
		fwrite(var, sizeof(uint32_t), 4 * (size_t)L, fv);
		fwrite(p, sizeof(double), (size_t)L, fp);
		fclose(fi); fclose(fv); fclose(fp);
		free(bed); free(keep); free(ind); free(var); free(p);
		return 0;
	}
	if (argc == 17 && !strcmp(argv[1], "chain")) {
		const int I = atoi(argv[2]), L = atoi(argv[3]);
		const size_t rb = (size_t)atol(argv[4]);
		mc_cli_options opt;
		mc_cli_data dat;
		memset(&opt, 0, sizeof opt);
		memset(&dat, 0, sizeof dat);
		opt.outfile_name = argv[8];
		opt.mind = threshold(argv[10], &opt.mind_t);
		opt.geno = threshold(argv[11], &opt.geno_t);
		opt.maf = threshold(argv[12], &opt.maf_t);
		opt.hwe = threshold(argv[13], &opt.hwe_t);
		opt.prune = threshold(argv[14], &opt.prune_t);
		opt.prune_window = atoi(argv[15]);
		opt.king = threshold(argv[16], &opt.king_t);
		dat.I = I; dat.L = dat.L_file = L; dat.ploidy = 2;
		dat.bed = read_all(argv[5], (size_t)L * rb, 8);
		dat.bed_record_bytes = rb;
		if (!(dat.lazy = mc_bed_lazy_new())) return 2;
		/* the ids as read_fam (mc_bed.c) holds them: locales numbered in order of first appearance */
		FILE *fam = fopen(argv[6], "r"), *bim = fopen(argv[7], "r");
		if (!fam || !bim) return 2;
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
		dat.i_p = calloc((size_t)dat.numpops, sizeof *dat.i_p);
		for (int i = 0; i < I; i++) dat.i_p[dat.locale[i]]++;
		dat.chrom = calloc((size_t)L, sizeof *dat.chrom);
		dat.variant_id = calloc((size_t)L, sizeof *dat.variant_id);
		for (int l = 0; l < L; l++) {
			char c[256], id[256];
			if (fscanf(bim, "%255s %255s", c, id) != 2) return 2;
			dat.chrom[l] = strdup(c);
			dat.variant_id[l] = strdup(id);
		}
		fclose(fam); fclose(bim);
		FILE *out = fopen(argv[9], "w");
		if (!out) return 2;
		int rc = mc_qc_data(&opt, &dat);
		if (rc == MC_EXIT_INVALID_USER_SETUP) {
			fprintf(out, "emptied %d calls %d\n", rc, qc_calls);
			fclose(out);
			release(&dat);
			return 0;
		}
		if (rc) { fprintf(stderr, "qc_host_driver: mc_qc_data %d\n", rc); return 3; }
		if (qc_calls != (opt.mind ? 2 : 1) || qc_calls_with_keep != (opt.mind ? 1 : 0)) return 5;	/* one call for both axes, two with --mind */
		if (summarized != (dat.I < I || dat.L < L)) return 5;						/* the summary made once, when anything went */
		if (mc_qc_data(&opt, &dat) != MC_EXIT_INTERNAL_ERROR) return 8;				/* not twice */
		mc_qc_line(out, &opt, &dat);
		if ((rc = mc_write_qc_lists(&opt, &dat))) return 9;
		fprintf(out, "qc I %d L %d\n", dat.I, dat.L);
		if (opt.prune) {
			const int seen = dat.L;
			if ((rc = mc_ld_prune_data(&opt, &dat))) { fprintf(stderr, "qc_host_driver: mc_ld_prune_data %d\n", rc); return 3; }
			if (mc_ld_prune_data(&opt, &dat) != MC_EXIT_INTERNAL_ERROR) return 8;
			if ((rc = mc_write_prune_lists(&opt, &dat))) return 9;
			fprintf(out, "prune %d of %d\n", dat.L, seen);
		}
		if (opt.king) {
			const int seen = dat.I;
			if ((rc = mc_king_data(&opt, &dat))) { fprintf(stderr, "qc_host_driver: mc_king_data %d\n", rc); return 3; }
			if (mc_king_data(&opt, &dat) != MC_EXIT_INTERNAL_ERROR) return 8;
			if ((rc = mc_write_king_lists(&opt, &dat))) return 9;
			fprintf(out, "king %d of %d pairs %zu\n", dat.I, seen, dat.n_king_pairs);
		}
		fprintf(out, "I %d I_file %d L %d L_file %d record_bytes %zu numpops %d\n", dat.I, dat.individual_of ? dat.I_file : I, dat.L, dat.L_file,
			dat.bed_record_bytes, dat.numpops);
		fprintf(out, "variant_of");
		for (int l = 0; dat.variant_of && l < dat.L; l++) fprintf(out, " %d", dat.variant_of[l]);
		fprintf(out, "\nindividual_of");
		for (int i = 0; dat.individual_of && i < dat.I; i++) fprintf(out, " %d", dat.individual_of[i]);
		fprintf(out, "\n");
		for (int i = 0; i < dat.I; i++) fprintf(out, "%s %d %s\n", dat.names[i], dat.locale[i], dat.pops[dat.locale[i]]);
		for (int p = 0; p < dat.numpops; p++) fprintf(out, "pop %s %d\n", dat.pops[p], dat.i_p[p]);
		for (size_t x = 0; x < (size_t)dat.L * dat.bed_record_bytes + 8; x++) fprintf(out, "%02x", dat.bed[x]);
		fprintf(out, "\n");
		fclose(out);
		release(&dat);
		return 0;
	}
	fprintf(stderr, "usage: qc_host_driver counts | chain ... (see the head of tests/qc_host_driver.c)\n");
	return 2;
}
