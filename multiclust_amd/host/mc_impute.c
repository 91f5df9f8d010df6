/*
 * mc_impute.c -- missing genotypes filled from the fitted admixture model (--fill; an extension: the reference's --impute
 * replaces every missing copy of a locus with one allele for all individuals before any fit, and its authors' TODO asks for
 * "a method to impute (and optionally write the data with imputed values to file)").  mc_impute asks the device for the most
 * probable alleles of every missing copy given Q and P of the fit (mchip_impute_missing, include/multiclust_hip.h has the rule);
 * the two writers put the filled copies back into the file the data set was read from, and change nothing else in it: libc only.
 */
#include "mc_cli.h"

#include <stdlib.h>
#include <string.h>

/* the candidates of every locus: the reader's L_alleles[l], i.e. uniquealleles[l] without the phantom trailing slot that a locus
 * with a missing copy (and an observed one) carries (read_file.c:527-533) */
int mc_impute_n_real(const mc_data *dat, int32_t *n_real)
{
	const int I = dat->I, L = dat->L, pl = dat->ploidy;
	uint8_t *miss = calloc((size_t)L, 1);
	if (!miss) return MCHIP_ERR_ALLOC;
	if (dat->geno) {
		for (int i = 0; i < I; i++) {
			const uint8_t *row = dat->geno + (size_t)i * L * pl;
			for (int l = 0; l < L; l++)
				for (int a = 0; a < pl; a++)
					if (row[(size_t)l * pl + a] == MCHIP_MISSING) miss[l] = 1;
		}
	} else if (dat->bed) {	/* code 1 (low bit set, high bit clear) among the I samples of the record */
		for (int l = 0; l < L; l++) {
			const uint8_t *rec = dat->bed + (size_t)l * dat->bed_record_bytes;
			for (int i = 0; i < I && !miss[l]; i += 4) {
				unsigned m = rec[i / 4] & ~(rec[i / 4] >> 1) & 0x55u;
				if (I - i < 4) m &= (1u << (2 * (I - i))) - 1u;		/* padding bits carry no sample */
				if (m) miss[l] = 1;
			}
		}
	} else {
		free(miss);
		return MCHIP_ERR_STATE;
	}
	for (int l = 0; l < L; l++) n_real[l] = dat->uniquealleles[l] - (miss[l] && dat->uniquealleles[l] > 0 ? 1 : 0);
	free(miss);
	return 0;
}

int mc_impute(const mc_options *opt, const mc_data *dat, mc_model *mod, uint8_t *geno_out, mc_impute_result *out)
{
	int32_t *n_real;
	int rc;
	memset(out, 0, sizeof *out);
	if (!opt->admixture) return MCHIP_ERR_UNSUPPORTED;
	if (!geno_out) return MCHIP_ERR_INVALID;
	if (!(n_real = malloc(sizeof(int32_t) * (size_t)dat->L))) return MCHIP_ERR_ALLOC;
	if (!(rc = mc_impute_n_real(dat, n_real))) {
		uint64_t nf = 0, nl = 0, ng = 0;
		rc = mchip_impute_missing(mod->dev, mod->pindex, n_real, geno_out, NULL, &nf, &nl, &ng, &out->sum_conf);
		if (rc) fprintf(stderr, "ERROR [mc_impute.c::mc_impute]: mchip_impute_missing failed (%d): %s\n", rc, mchip_last_error(mod->dev));
		out->n_filled = nf; out->n_left = nl; out->n_genotypes = ng;
		out->mean_conf = ng ? out->sum_conf / (double)ng : 0.0;
	}
	free(n_real);
	return rc;
}

/* ---- the writers ---- */
#define open_out(path) mc_open_result("mc_impute.c", path, "wb")

/* next token of [*cur, end): its first byte, *cur behind it; NULL when the line is exhausted */
static const char *next_token(const char **cur, const char *end)
{
	const char *p = *cur;
	while (p < end && mc_is_blank(*p)) p++;
	if (p >= end) { *cur = p; return NULL; }
	const char *s = p;
	while (p < end && !mc_is_blank(*p)) p++;
	*cur = p;
	return s;
}

/* The lines and tokens are found as mc_read_structure finds them: lines that hold anything but white space count; the first is
 * the header, a second one that starts with the token -1 is skipped, the next I (one line per individual, `ploidy` tokens per
 * locus) or I * ploidy (consecutive lines) are data lines of two label tokens and the allele tokens; whatever follows is copied. */
int mc_write_filled_structure(const mc_cli_options *opt, const mc_cli_data *dat, const uint8_t *filled, const char *out_path)
{
	const int I = dat->I, L = dat->L, pl = dat->ploidy, per_line = dat->interleaved ? pl : 1;
	const size_t ndata = dat->interleaved ? (size_t)I : (size_t)I * (size_t)pl;
	char *buf;
	size_t n;
	int rc = mc_slurp("mc_impute.c", opt->filename, &buf, &n);
	if (rc) return rc;
	if (!dat->geno) { free(buf); return MC_EXIT_INTERNAL_ERROR; }
	FILE *fp = open_out(out_path);
	if (!fp) { free(buf); return MC_EXIT_FILE_OPEN_ERROR; }
	const char *done = buf, *eof = buf + n;		/* [buf, done) is written */
	size_t line = 0, first = 1;
	rc = 0;
	mc_lines it;
	for (mc_lines_start(&it, buf, n); !rc && mc_lines_next(&it);) {
		const char *q = it.end, *c = it.first;
		const char *t = next_token(&c, q);
		const size_t idx = line++;
		if (idx == 1 && c - t == 2 && !strncmp(t, "-1", 2)) first = 2;
		if (idx < first || idx - first >= ndata) continue;
		const size_t ln = idx - first;
		if (!next_token(&c, q)) { rc = MC_EXIT_FILE_FORMAT_ERROR; break; }	/* (the first label was t) */
		for (int l = 0; l < L && !rc; l++)
			for (int x = 0; x < per_line; x++) {
				if (!(t = next_token(&c, q))) { rc = MC_EXIT_FILE_FORMAT_ERROR; break; }
				const size_t i = dat->interleaved ? ln : ln / (size_t)pl, a = dat->interleaved ? (size_t)x : ln % (size_t)pl;
				const size_t g = (i * (size_t)L + (size_t)l) * (size_t)pl + a;
				if (dat->geno[g] != MCHIP_MISSING || filled[g] == MCHIP_MISSING) continue;
				/* a missing copy at this locus: its list has uniquealleles[l] - 1 alleles (the phantom slot is not one) */
				if ((int)filled[g] >= dat->uniquealleles[l] - 1) { rc = MC_EXIT_INTERNAL_ERROR; break; }
				fwrite(done, 1, (size_t)(t - done), fp);
				fprintf(fp, "%d", dat->L_alleles[l][filled[g]]);
				done = c;
			}
	}
	if (!rc) fwrite(done, 1, (size_t)(eof - done), fp);
	if (ferror(fp)) rc = rc ? rc : MC_EXIT_FILE_OPEN_ERROR;
	fclose(fp);
	free(buf);
	if (rc) fprintf(stderr, "ERROR [mc_impute.c::mc_write_filled_structure]: could not write '%s' from '%s' (%d)\n", out_path, opt->filename, rc);
	return rc;
}

static int copy_file(const char *from, const char *to)
{
	char *buf;
	size_t n;
	int rc = mc_slurp("mc_impute.c", from, &buf, &n);
	if (rc) return rc;
	FILE *fp = open_out(to);
	if (!fp) { free(buf); return MC_EXIT_FILE_OPEN_ERROR; }
	if (fwrite(buf, 1, n, fp) != n) rc = MC_EXIT_FILE_OPEN_ERROR;
	fclose(fp);
	free(buf);
	return rc;
}

/* Index -> allele of a locus is the reader's: L_alleles[l][m] is 1 for A1 and 2 for A2 (mc_read_bed), so a filled pair is
 * homozygous A1 (code 0), heterozygous (2) or homozygous A2 (3).  The records are the file's: magic bytes (the reader accepts one
 * value of each) and padding bits stay as they are. */
int mc_write_filled_bed(const mc_cli_options *opt, const mc_cli_data *dat, const uint8_t *filled, const char *out_prefix)
{
	const int I = dat->I, L = dat->L;
	const size_t rb = dat->bed_record_bytes;
	static const uint8_t magic[3] = { 0x6c, 0x1b, 0x01 };
	char *src[2] = { mc_path_of(opt->bed_prefix, ".bim"), mc_path_of(opt->bed_prefix, ".fam") };
	char *dst[3] = { mc_path_of(out_prefix, ".bim"), mc_path_of(out_prefix, ".fam"), mc_path_of(out_prefix, ".bed") };
	uint8_t *rec = malloc(rb ? rb : 1);
	FILE *fp = NULL;
	int rc = MC_EXIT_MEMORY_ALLOCATION;
	if (!src[0] || !src[1] || !dst[0] || !dst[1] || !dst[2] || !rec) goto DONE;
	if (!dat->bed) { rc = MC_EXIT_INTERNAL_ERROR; goto DONE; }
	if (!(fp = open_out(dst[2]))) { rc = MC_EXIT_FILE_OPEN_ERROR; goto DONE; }
	rc = 0;
	fwrite(magic, 1, 3, fp);
	for (int l = 0; l < L && !rc; l++) {
		memcpy(rec, dat->bed + (size_t)l * rb, rb);
		for (int i = 0; i < I; i++) {
			const int sh = 2 * (i % 4);
			if (((rec[i / 4] >> sh) & 3) != 1) continue;
			const uint8_t *g = filled + ((size_t)i * L + (size_t)l) * 2;
			if (g[0] == MCHIP_MISSING || g[1] == MCHIP_MISSING) continue;	/* left missing */
			if ((int)g[0] >= dat->uniquealleles[l] - 1 || (int)g[1] >= dat->uniquealleles[l] - 1) { rc = MC_EXIT_INTERNAL_ERROR; break; }
			const int a = dat->L_alleles[l][g[0]], b = dat->L_alleles[l][g[1]];
			const unsigned code = (a == 1 && b == 1) ? 0u : ((a == 2 && b == 2) ? 3u : 2u);
			rec[i / 4] = (uint8_t)((rec[i / 4] & ~(3u << sh)) | (code << sh));
		}
		if (!rc && fwrite(rec, 1, rb, fp) != rb) rc = MC_EXIT_FILE_OPEN_ERROR;
	}
	if (fclose(fp)) rc = rc ? rc : MC_EXIT_FILE_OPEN_ERROR;
	fp = NULL;
	/* (the variants --prune removed have no record above and no line here; the individuals --king-cutoff removed none there) */
	for (int x = 0; x < 2 && !rc; x++)
		rc = (x == 0 && dat->variant_of) ? mc_copy_kept_lines("mc_impute.c", src[x], dst[x], dat->variant_of, L) :
		     (x == 1 && dat->individual_of) ? mc_copy_kept_lines("mc_impute.c", src[x], dst[x], dat->individual_of, I) : copy_file(src[x], dst[x]);
DONE:
	if (fp) fclose(fp);
	if (rc) fprintf(stderr, "ERROR [mc_impute.c::mc_write_filled_bed]: could not write the fileset '%s' (%d)\n", out_prefix, rc);
	free(src[0]); free(src[1]); free(dst[0]); free(dst[1]); free(dst[2]); free(rec);
	return rc;
}

int mc_write_filled(const mc_cli_options *opt, const mc_cli_data *dat, int K, const uint8_t *filled)
{
	char path[4400];
	mc_result_path(opt, path, sizeof path, ".admix.K=%d.filled%s", K, opt->bed_prefix ? "" : ".stru");
	return opt->bed_prefix ? mc_write_filled_bed(opt, dat, filled, path) : mc_write_filled_structure(opt, dat, filled, path);
}
