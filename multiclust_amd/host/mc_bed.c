/*
 * mc_bed.c -- PLINK 1 binary filesets (.bed / .bim / .fam) as input: an extension, the reference knows PED only as an output
 * format.  The data set of a fileset is defined through the STRUCTURE reader (mc_cli.h, mc_read_bed): everything here yields
 * what mc_read_structure yields on the equivalent STRUCTURE file, without that file, without its 4-byte allele codes and
 * without the [I][L][2] genotype -- the 2-bit records stay as they are and go to the device as they are
 * (mchip_set_genotypes_bed).  mc_bed_decode is the plain-C form of the device's unpacking: the comparator of the kernels, and
 * what the few host-side consumers of the genotype get on first need (MC_HOST_INIT, MC_HOST_BOOTSTRAP, Rand-EM, the observed
 * haplotypes of an admixture bootstrap).
 */
#include "mc_cli.h"

#include <pthread.h>
#include <stdlib.h>
#include <string.h>

static int fail(const char *fn, int line, int status, const char *msg, const char *arg)
{
	fprintf(stderr, "ERROR [mc_bed.c::%s(%d)]: ", fn, line);
	fprintf(stderr, msg, arg ? arg : "");
	fprintf(stderr, "\n");
	return status;
}
#define FAIL(status, msg, arg) fail(__func__, __LINE__, status, msg, arg)

enum { BED_A1 = 1, BED_A2 = 2, BED_MISSING = 4 };

/* which of A1, A2 and "missing" occur among the I samples of one record: 32 samples per step, the last bytes through a mask
 * (padding bits read as 0 would otherwise count as homozygous A1) */
static int record_flags(const uint8_t *rec, int I)
{
	const uint64_t low = 0x5555555555555555ull;
	uint64_t a1 = 0, a2 = 0, ms = 0;
	int j = 0;
	for (; j + 32 <= I; j += 32) {
		uint64_t v;
		memcpy(&v, rec + j / 4, 8);
		const uint64_t lo = v & low, hi = (v >> 1) & low;
		a1 |= ~lo & low;	/* codes 0 and 2 carry A1 */
		a2 |= hi;		/* codes 2 and 3 carry A2 */
		ms |= lo & ~hi;		/* code 1 */
	}
	for (; j < I; j++) {
		const int c = (rec[j / 4] >> (2 * (j % 4))) & 3;
		if (c == 0 || c == 2) a1 = 1;
		if (c >= 2) a2 = 1;
		if (c == 1) ms = 1;
	}
	return (a1 ? BED_A1 : 0) | (a2 ? BED_A2 : 0) | (ms ? BED_MISSING : 0);
}

/* summarize_alleles' count for a locus with these flags (read_file.c:524-533): the phantom slot only beside an observed allele */
static int32_t flags_ua(int flags)
{
	const int nu = !!(flags & BED_A1) + !!(flags & BED_A2);
	return nu ? nu + !!(flags & BED_MISSING) : 0;
}

#define DECODE_BLOCK 64		/* loci per sweep over the individuals: 128 contiguous genotype bytes written per individual */
void mc_bed_decode(int I, int L, const uint8_t *bed, size_t record_bytes, int32_t *uniquealleles, uint8_t *geno)
{
	for (int b0 = 0; b0 < L; b0 += DECODE_BLOCK) {
		const int nb = L - b0 < DECODE_BLOCK ? L - b0 : DECODE_BLOCK;
		uint8_t pair[DECODE_BLOCK][4][2];	/* per locus of the block: the two allele indices of each code */
		for (int x = 0; x < nb; x++) {
			const int fl = record_flags(bed + (size_t)(b0 + x) * record_bytes, I);
			const uint8_t i2 = (fl & BED_A1) ? 1 : 0;	/* ascending allele list: A2 is index 1 beside an observed A1 */
			if (uniquealleles) uniquealleles[b0 + x] = flags_ua(fl);
			pair[x][0][0] = 0; pair[x][0][1] = 0;
			pair[x][1][0] = MCHIP_MISSING; pair[x][1][1] = MCHIP_MISSING;
			pair[x][2][0] = 0; pair[x][2][1] = 1;
			pair[x][3][0] = i2; pair[x][3][1] = i2;
		}
		if (!geno) continue;
		for (int i = 0; i < I; i++) {
			uint8_t *row = geno + ((size_t)i * L + b0) * 2;
			const uint8_t *col = bed + (size_t)b0 * record_bytes + i / 4;
			const int sh = 2 * (i % 4);
			for (int x = 0; x < nb; x++) {
				const int c = (col[(size_t)x * record_bytes] >> sh) & 3;
				row[2 * x] = pair[x][c][0];
				row[2 * x + 1] = pair[x][c][1];
			}
		}
	}
}

/* ---- the decoded genotype of a packed data set, built when something on the host first asks for it ---- */
typedef struct bed_lazy {
	mc_lazy_geno base;
	pthread_mutex_t lock;
	uint8_t *geno;
} bed_lazy;

static const uint8_t *lazy_get(mc_lazy_geno *self, const mc_data *dat)
{
	bed_lazy *z = (bed_lazy *)self;
	pthread_mutex_lock(&z->lock);
	if (!z->geno && (z->geno = malloc((size_t)dat->I * dat->L * 2))) {
		mchip_progress_note("mc_bed.c: decoding the packed records for a host-side reader");
		mc_bed_decode(dat->I, dat->L, dat->bed, dat->bed_record_bytes, NULL, z->geno);
	}
	pthread_mutex_unlock(&z->lock);
	return z->geno;
}

static void lazy_release(mc_lazy_geno *self)
{
	bed_lazy *z = (bed_lazy *)self;
	pthread_mutex_destroy(&z->lock);
	free(z->geno);
	free(z);
}

mc_lazy_geno *mc_bed_lazy_new(void)
{
	bed_lazy *z = calloc(1, sizeof *z);
	if (!z) return NULL;
	z->base.get = lazy_get;
	z->base.release = lazy_release;
	pthread_mutex_init(&z->lock, NULL);
	return &z->base;
}

/* ---- the three files ---- */
/* lines that hold anything but white space */
static size_t count_lines(char *buf, size_t n)
{
	size_t lines = 0;
	mc_lines it;
	for (mc_lines_start(&it, buf, n); mc_lines_next(&it);) lines++;
	return lines;
}

/* .fam: one line per individual, FID IID ...: the locale (numbered in order of first appearance, as the STRUCTURE reader numbers
 * its second column) and the name */
static int read_fam(const char *path, mc_cli_data *dat)
{
	char *buf;
	size_t n;
	int rc = mc_slurp("mc_bed.c", path, &buf, &n);
	if (rc) return rc;
	const size_t I = count_lines(buf, n);
	if (!I || I > 0x7FFFFFFF / 4) { free(buf); return FAIL(MC_EXIT_FILE_FORMAT_ERROR, "no individuals (or too many) in '%s'", path); }
	dat->I = (int)I;
	dat->names = calloc(I, sizeof *dat->names);
	dat->locale = calloc(I, sizeof *dat->locale);
	if (!dat->names || !dat->locale) { free(buf); return FAIL(MC_EXIT_MEMORY_ALLOCATION, "out of memory%s", NULL); }
	int i = 0;
	mc_lines it;
	for (mc_lines_start(&it, buf, n); mc_lines_next(&it); i++) {
		char *s = it.first, *q = it.end, *fid = s;
		while (s < q && !mc_is_blank(*s)) s++;
		const size_t flen = (size_t)(s - fid);
		while (s < q && mc_is_blank(*s)) s++;
		char *iid = s;
		while (s < q && !mc_is_blank(*s)) s++;
		const size_t ilen = (size_t)(s - iid);
		if (!ilen) { free(buf); return FAIL(MC_EXIT_FILE_FORMAT_ERROR, "line without family and individual ID in '%s'", path); }
		int found = -1;
		for (int x = 0; x < dat->numpops; x++)
			if (strlen(dat->pops[x]) == flen && !strncmp(dat->pops[x], fid, flen)) { found = x; break; }
		if (found < 0) {
			char **pops2 = realloc(dat->pops, sizeof *dat->pops * (size_t)(dat->numpops + 1));
			if (pops2) dat->pops = pops2;
			if (!pops2 || !(dat->pops[dat->numpops] = mc_dup_token(fid, flen))) { free(buf); return FAIL(MC_EXIT_MEMORY_ALLOCATION, "out of memory%s", NULL); }
			found = dat->numpops++;
		}
		dat->locale[i] = found;
		if (!(dat->names[i] = mc_dup_token(iid, ilen))) { free(buf); return FAIL(MC_EXIT_MEMORY_ALLOCATION, "out of memory%s", NULL); }
	}
	free(buf);
	if (!(dat->i_p = calloc((size_t)dat->numpops, sizeof *dat->i_p))) return FAIL(MC_EXIT_MEMORY_ALLOCATION, "out of memory%s", NULL);
	for (int x = 0; x < dat->I; x++) dat->i_p[dat->locale[x]]++;
	return 0;
}

/* summarize_alleles (read_file.c:443-600) from the flags of the L records held: uniquealleles, L_alleles, toff, T, M and
 * missing_data made anew (the caller has freed what was there) */
int mc_bed_summarize(mc_cli_data *dat)
{
	const int I = dat->I, L = dat->L;
	const size_t rb = dat->bed_record_bytes;
	dat->M = dat->T = dat->missing_data = 0;
	dat->uniquealleles = calloc((size_t)L, sizeof *dat->uniquealleles);
	dat->L_alleles = calloc((size_t)L, sizeof *dat->L_alleles);
	dat->toff = calloc((size_t)L + 1, sizeof *dat->toff);
	if (!dat->uniquealleles || !dat->L_alleles || !dat->toff) return FAIL(MC_EXIT_MEMORY_ALLOCATION, "out of memory%s", NULL);
	for (int l = 0; l < L; l++) {
		const int fl = record_flags(dat->bed + (size_t)l * rb, I);
		const int nu = !!(fl & BED_A1) + !!(fl & BED_A2);
		int *al = malloc(sizeof(int) * (size_t)(nu ? nu : 1));
		if (!al) return FAIL(MC_EXIT_MEMORY_ALLOCATION, "out of memory%s", NULL);
		int x = 0;
		if (fl & BED_A1) al[x++] = 1;	/* the allele codes of the equivalent STRUCTURE file */
		if (fl & BED_A2) al[x++] = 2;
		dat->L_alleles[l] = al;
		dat->uniquealleles[l] = flags_ua(fl);
		if ((fl & BED_MISSING) && nu) dat->missing_data = 1;
		if (dat->uniquealleles[l] > dat->M) dat->M = dat->uniquealleles[l];
		dat->toff[l + 1] = dat->toff[l] + dat->uniquealleles[l];
	}
	dat->T = dat->toff[L];
	return 0;
}

/* .bim: one line per variant, chromosome, variant id, ...: the two tokens are terminated in place (dat->bim_text, n bytes) and
 * pointed to by dat->chrom and dat->variant_id */
static int bim_fields(mc_cli_data *dat, size_t n, size_t nloci)
{
	dat->chrom = calloc(nloci, sizeof *dat->chrom);
	dat->variant_id = calloc(nloci, sizeof *dat->variant_id);
	if (!dat->chrom || !dat->variant_id) return MC_EXIT_MEMORY_ALLOCATION;
	size_t l = 0;
	mc_lines it;
	for (mc_lines_start(&it, dat->bim_text, n); mc_lines_next(&it); l++) {
		char *s = it.first, *q = it.end, *c = s;
		while (s < q && !mc_is_blank(*s)) s++;
		char *c_end = s;
		while (s < q && mc_is_blank(*s)) s++;
		char *id = s;
		while (s < q && !mc_is_blank(*s)) s++;
		*c_end = 0;
		*s = 0;		/* (the line's end, or the blank behind the id; the text has one more byte behind its last.  A line
				 * without a second field has the empty id) */
		dat->chrom[l] = c;
		dat->variant_id[l] = id;
	}
	return 0;
}

int mc_read_bed(const mc_cli_options *opt, mc_cli_data *dat)
{
	int rc = MC_EXIT_MEMORY_ALLOCATION;
	char *bedf = NULL, *bimf = NULL, *famf = NULL, *buf = NULL;
	FILE *f = NULL;
	size_t n;
	const double t_start = mc_now_s();
	memset(dat, 0, sizeof *dat);
	dat->ploidy = 2;
	if (!opt->bed_prefix) return FAIL(MC_EXIT_INVALID_USER_SETUP, "no fileset prefix%s", NULL);
	bedf = mc_path_of(opt->bed_prefix, ".bed"); bimf = mc_path_of(opt->bed_prefix, ".bim"); famf = mc_path_of(opt->bed_prefix, ".fam");
	if (!bedf || !bimf || !famf) { rc = FAIL(MC_EXIT_MEMORY_ALLOCATION, "out of memory%s", NULL); goto DONE; }
	mchip_progress_note("mc_read_bed: .fam and .bim");
	if ((rc = read_fam(famf, dat))) goto DONE;
	if ((rc = mc_slurp("mc_bed.c", bimf, &buf, &n))) goto DONE;
	const size_t nloci = count_lines(buf, n);
	if (!nloci || nloci > 0x7FFFFFFF / 4) { rc = FAIL(MC_EXIT_FILE_FORMAT_ERROR, "no variants (or too many) in '%s'", bimf); goto DONE; }
	dat->bim_text = buf;
	buf = NULL;
	if ((rc = bim_fields(dat, n, nloci))) { rc = FAIL(rc, "out of memory reading '%s'", bimf); goto DONE; }
	const int I = dat->I, L = dat->L = dat->L_file = (int)nloci;
	const size_t rb = ((size_t)I + 3) / 4;

	mchip_progress_note("mc_read_bed: .bed");
	if (!(f = fopen(bedf, "rb"))) { rc = FAIL(MC_EXIT_FILE_OPEN_ERROR, "could not open file '%s'", bedf); goto DONE; }
	uint8_t magic[3];
	if (fread(magic, 1, 3, f) != 3 || magic[0] != 0x6c || magic[1] != 0x1b) { rc = FAIL(MC_EXIT_FILE_FORMAT_ERROR, "'%s' is not a PLINK 1 .bed file (magic bytes)", bedf); goto DONE; }
	if (magic[2] != 0x01) { rc = FAIL(MC_EXIT_FILE_FORMAT_ERROR, "'%s' is not in variant-major mode (third byte must be 0x01)", bedf); goto DONE; }
	fseek(f, 0, SEEK_END);
	const long fsz = ftell(f);
	if (fsz < 0 || (size_t)fsz != 3 + (size_t)L * rb) { rc = FAIL(MC_EXIT_FILE_FORMAT_ERROR, "size of '%s' is not 3 + variants * ceil(individuals / 4) for its .bim and .fam", bedf); goto DONE; }
	fseek(f, 3, SEEK_SET);
	/* (8 spare bytes: record_flags reads 8 at a time, never past a record's last sample, but keep the block's end harmless) */
	if (!(dat->bed = malloc((size_t)L * rb + 8))) { rc = FAIL(MC_EXIT_MEMORY_ALLOCATION, "out of memory reading '%s'", bedf); goto DONE; }
	memset(dat->bed + (size_t)L * rb, 0, 8);
	if (fread(dat->bed, 1, (size_t)L * rb, f) != (size_t)L * rb) { rc = FAIL(MC_EXIT_FILE_FORMAT_ERROR, "short read on '%s'", bedf); goto DONE; }
	dat->bed_record_bytes = rb;

	mchip_progress_note("mc_read_bed: allele lists");
	if (!(dat->lazy = mc_bed_lazy_new())) { rc = FAIL(MC_EXIT_MEMORY_ALLOCATION, "out of memory%s", NULL); goto DONE; }
	if ((rc = mc_bed_summarize(dat))) goto DONE;
	mc_timing_line("mc_bed.c", "fileset read", t_start);	/* as mc_read_structure reports its phases */
	rc = 0;
DONE:
	if (f) fclose(f);
	free(buf); free(bedf); free(bimf); free(famf);
	if (rc) mc_free_data(dat);
	return rc;
}
