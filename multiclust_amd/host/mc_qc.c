/*
 * mc_qc.c -- --mind, --geno, --maf, --hwe (extensions): sample and variant quality control of a PLINK fileset before anything is
 * fitted -- the step every admixture guide runs before LD pruning and the removal of relatives (`plink --mind 0.1 --geno 0.05 --maf
 * 0.01`); without it a monomorphic or all-missing variant passes --prune (its r2 is NaN) and enters the fit as a locus without
 * information, a sample that is mostly missing goes into the kinships and into Q, and the user leaves for another program first.
 *
 * The four genotype counts of every individual and of every variant and the Hardy-Weinberg exact test are defined in
 * include/multiclust_hip.h (mchip_bed_qc): integers, and a fixed sequence of double operations -- the same bits wherever computed.
 *
 * The order is PLINK 1.9's.  --mind runs first, on the file as it is: individual i goes when miss_i / L > t over all L variants of the
 * file.  The three variant rules then run from one set of counts taken over the individuals --mind kept (I' of them): the missing
 * rate n1 / I' > --geno; the minor-allele frequency min(2 n0 + n2, 2 n3 + n2) / (2 N) < --maf, N = n0 + n2 + n3, 0 when N = 0; the
 * exact-test p < --hwe.  Each rate is one division of two integers converted to double; a rate exactly on its threshold stays; NaN
 * cannot arise.  A variant's reason for removal is the first rule it fails in the order geno, maf, hwe.  All variants and all
 * individuals count: sex chromosomes are for the user's --extract to remove.
 *
 * Everything in this file is libc, mc_files.h and mc_filter.h but the one function that calls the device (counts_by_device:
 * mchip_bed_qc) and the two compactions (mc_king_compact, mc_ld_compact).  tests/qc_host_driver.c stubs the device and the reader
 * and runs the rest as a program of its own.
 */
#include "mc_cli.h"

#include <stdlib.h>
#include <string.h>

double mc_qc_missing_rate(uint32_t num, uint32_t den) { return den ? (double)num / (double)den : 0.0; }

double mc_qc_maf(const uint32_t *c)
{
	const uint64_t a1 = 2 * (uint64_t)c[0] + c[2], a2 = 2 * (uint64_t)c[3] + c[2], N = (uint64_t)c[0] + c[2] + c[3];
	return N ? (double)(a1 < a2 ? a1 : a2) / (double)(2 * N) : 0.0;
}

int mc_qc_individuals(int I, int L, const uint32_t *ind_counts, double t, uint8_t *keep)
{
	int n = 0;
	for (int i = 0; i < I; i++) n += keep[i] = !(mc_qc_missing_rate(ind_counts[4 * (size_t)i + 1], (uint32_t)L) > t);
	return n;
}

void mc_qc_variants(const mc_cli_options *opt, int L, const uint32_t *var_counts, const double *hwe_p, uint8_t *reason, int *n_reason)
{
	memset(n_reason, 0, sizeof(int) * 4);
	for (int l = 0; l < L; l++) {
		const uint32_t *c = var_counts + 4 * (size_t)l;
		const uint32_t kept = c[0] + c[1] + c[2] + c[3];
		reason[l] = opt->geno && mc_qc_missing_rate(c[1], kept) > opt->geno_t ? MC_QC_GENO :
			    opt->maf && mc_qc_maf(c) < opt->maf_t ? MC_QC_MAF :
			    opt->hwe && hwe_p[l] < opt->hwe_t ? MC_QC_HWE : MC_QC_KEPT;
		n_reason[reason[l]]++;
	}
}

/* the counts of both axes and the keep bytes of --mind: one call of the device without --mind, two with it -- the second is given
 * the keep bytes, so nothing is compacted between them.  I_kept = 0 ends it before the second call. */
static int counts_by_device(const mc_cli_options *opt, mc_device_band *dev, void *out)
{
	mc_qc_result *r = out;
	const mc_cli_data *d = dev->dat;
	int rc;
	if (!opt->mind) {
		memset(r->ind_keep, 1, (size_t)r->I);
		r->I_kept = r->I;
		return mchip_bed_qc(dev->ctx, d->I, d->L, d->bed, d->bed_record_bytes, NULL, r->ind_counts, r->var_counts, r->hwe_p);
	}
	if ((rc = mchip_bed_qc(dev->ctx, d->I, d->L, d->bed, d->bed_record_bytes, NULL, r->ind_counts, NULL, NULL))) return rc;
	if (!(r->I_kept = mc_qc_individuals(r->I, r->L, r->ind_counts, opt->mind_t, r->ind_keep))) return 0;
	return mchip_bed_qc(dev->ctx, d->I, d->L, d->bed, d->bed_record_bytes, r->ind_keep, NULL, r->var_counts, r->hwe_p);
}

int mc_qc_data(const mc_cli_options *opt, mc_cli_data *dat)
{
	const int I = dat->I, L = dat->L;
	const double t_start = mc_now_s();
	mc_qc_result *r = calloc(1, sizeof *r);
	uint8_t *vkeep = NULL;
	int *imap = NULL, *vmap = NULL;
	int rc = MC_EXIT_MEMORY_ALLOCATION;
	if (!dat->bed || dat->filters_run || dat->variant_of || dat->individual_of || dat->qc) { rc = MC_EXIT_INTERNAL_ERROR; goto DONE; }	/* the first filter of a fileset */
	if (!r) goto DONE;
	r->I = I; r->L = L;
	r->ind_counts = calloc(4 * (size_t)I, sizeof *r->ind_counts);
	r->var_counts = calloc(4 * (size_t)L, sizeof *r->var_counts);
	r->hwe_p = calloc((size_t)L, sizeof *r->hwe_p);
	r->ind_keep = calloc((size_t)I, 1);
	r->var_reason = calloc((size_t)L, 1);
	vkeep = malloc((size_t)L);
	if (!r->ind_counts || !r->var_counts || !r->hwe_p || !r->ind_keep || !r->var_reason || !vkeep) goto DONE;
	if ((rc = mc_filter_on_device(opt, dat, "mc_qc.c::mc_qc_data", "--mind / --geno / --maf / --hwe", "the genotype counts", counts_by_device, r))) goto DONE;
	if (!r->I_kept) {
		fprintf(stderr, "ERROR [mc_qc.c::mc_qc_data]: --mind %g removes every one of the %d individuals: no data set is left\n", opt->mind_t, I);
		rc = MC_EXIT_INVALID_USER_SETUP;
		goto DONE;
	}
	mc_qc_variants(opt, L, r->var_counts, r->hwe_p, r->var_reason, r->n_reason);
	r->L_kept = r->n_reason[MC_QC_KEPT];
	if (!r->L_kept) {	/* the last rule that removed anything took what was left */
		const int last = r->n_reason[MC_QC_HWE] ? MC_QC_HWE : r->n_reason[MC_QC_MAF] ? MC_QC_MAF : MC_QC_GENO;
		fprintf(stderr, "ERROR [mc_qc.c::mc_qc_data]: %s %g removes the last of the %d variants (%d missing rate, %d MAF, %d HWE): no data set is left\n",
			last == MC_QC_HWE ? "--hwe" : last == MC_QC_MAF ? "--maf" : "--geno",
			last == MC_QC_HWE ? opt->hwe_t : last == MC_QC_MAF ? opt->maf_t : opt->geno_t, L, r->n_reason[MC_QC_GENO], r->n_reason[MC_QC_MAF],
			r->n_reason[MC_QC_HWE]);
		rc = MC_EXIT_INVALID_USER_SETUP;
		goto DONE;
	}
	/* the data set is the kept individuals' and variants' from here on; an axis that lost nothing stays as it was read */
	if (r->I_kept < I) {
		if (!(imap = malloc(sizeof(int) * (size_t)I))) { rc = MC_EXIT_MEMORY_ALLOCATION; goto DONE; }
		if (mc_king_compact(I, L, dat->bed_record_bytes, r->ind_keep, dat->bed, imap) != r->I_kept) { rc = MC_EXIT_MEMORY_ALLOCATION; goto DONE; }
		dat->bed_record_bytes = ((size_t)r->I_kept + 3) / 4;
		if ((rc = mc_filter_rebuild_individuals(dat, r->I_kept, imap))) goto DONE;
		dat->individual_of = imap;
		imap = NULL;
		if (dat->lazy) {	/* (nothing has been decoded yet; a decoded genotype would be the file's) */
			dat->lazy->release(dat->lazy);
			if (!(dat->lazy = mc_bed_lazy_new())) { rc = MC_EXIT_MEMORY_ALLOCATION; goto DONE; }
		}
	}
	if (r->L_kept < L) {
		if (!(vmap = malloc(sizeof(int) * (size_t)L))) { rc = MC_EXIT_MEMORY_ALLOCATION; goto DONE; }
		for (int l = 0; l < L; l++) vkeep[l] = r->var_reason[l] == MC_QC_KEPT;
		dat->L = mc_ld_compact(L, dat->bed_record_bytes, vkeep, dat->bed, vmap);
		memset(dat->bed + (size_t)dat->L * dat->bed_record_bytes, 0, 8);	/* (the reader's spare bytes behind the last record) */
		dat->variant_of = vmap;
		vmap = NULL;
	}
	dat->filters_run |= MC_FILTER_QC;
	dat->qc = r;
	r = NULL;
	rc = (dat->I < I || dat->L < L) ? mc_filter_resummarize(dat, L, "mc_qc.c", "quality control", t_start) : 0;
DONE:
	mc_qc_result_free(r);
	free(vkeep); free(imap); free(vmap);
	return rc;
}

void mc_qc_line(FILE *fp, const mc_cli_options *opt, const mc_cli_data *dat)
{
	const mc_qc_result *r = dat->qc;
	const char *sep = "";
	fprintf(fp, "Quality control:");
	if (opt->mind) fprintf(fp, " kept %d of %d individuals (missing rate > %g)", r->I_kept, r->I, opt->mind_t);
	if (opt->geno || opt->maf || opt->hwe) {
		fprintf(fp, "%s kept %d of %d variants (", opt->mind ? "," : "", r->L_kept, r->L);
		if (opt->geno) { fprintf(fp, "%d missing rate > %g", r->n_reason[MC_QC_GENO], opt->geno_t); sep = ", "; }
		if (opt->maf) { fprintf(fp, "%s%d MAF < %g", sep, r->n_reason[MC_QC_MAF], opt->maf_t); sep = ", "; }
		if (opt->hwe) fprintf(fp, "%s%d HWE p < %g", sep, r->n_reason[MC_QC_HWE], opt->hwe_t);
		fprintf(fp, ")");
	}
	fprintf(fp, "\n");
}

/* the ids of the .fam lines: the fileset's own once an axis was thinned, else the data set's */
static const char *fid_of(const mc_cli_data *d, int i) { return d->fam_fid ? d->fam_fid[i] : d->pops[d->locale[i]]; }
static const char *iid_of(const mc_cli_data *d, int i) { return d->fam_iid ? d->fam_iid[i] : d->names[i]; }
static void print_individual(FILE *fp, const void *dat, int v) { fprintf(fp, "%s\t%s\n", fid_of(dat, v), iid_of(dat, v)); }
static void print_variant(FILE *fp, const void *dat, int v) { fprintf(fp, "%s\n", ((const mc_cli_data *)dat)->variant_id[v]); }

/* <stem>.mind.in / .mind.out (with --mind): "FID\tIID" of the individuals kept and removed, one per line in file order.
 * <stem>.qc.in / .qc.out (with --geno, --maf or --hwe): the ids of the variants kept and removed (`plink --keep <stem>.mind.in
 * --extract <stem>.qc.in` writes the fileset the run was made on).
 * <stem>.qc.var.txt: one header line, then one tab-separated line per variant of the file: its id, the four counts n0 n1 n2 n3 over
 * the individuals kept, the missing rate, the MAF and the HWE p as %.6g, and kept / geno / maf / hwe.
 * <stem>.qc.ind.txt: one header line, then one line per individual of the file: FID, IID, the missing rate over all variants and the
 * heterozygosity n2 / (n0 + n2 + n3) (nan for an individual without a call) as %.6g, and kept / mind. */
int mc_write_qc_lists(const mc_cli_options *opt, const mc_cli_data *dat)
{
	static const char *const why[4] = { "kept", "geno", "maf", "hwe" };
	const mc_qc_result *r = dat->qc;
	char path[4400];
	int rc = 0;
	if (!r || !dat->variant_id) return MC_EXIT_INTERNAL_ERROR;
	int *kept = malloc(sizeof(int) * (size_t)(r->I > r->L ? r->I : r->L));
	if (!kept) return MC_EXIT_MEMORY_ALLOCATION;
	if (opt->mind) {
		int n = 0;
		for (int i = 0; i < r->I; i++) if (r->ind_keep[i]) kept[n++] = i;
		rc = mc_write_kept_lists(opt, "mc_qc.c", ".mind", r->I, n, kept, print_individual, dat);
	}
	if (!rc && (opt->geno || opt->maf || opt->hwe)) {
		int n = 0;
		for (int l = 0; l < r->L; l++) if (r->var_reason[l] == MC_QC_KEPT) kept[n++] = l;
		rc = mc_write_kept_lists(opt, "mc_qc.c", ".qc", r->L, n, kept, print_variant, dat);
	}
	free(kept);
	if (rc) return rc;
	mc_result_path(opt, path, sizeof path, ".qc.var.txt");
	FILE *fp = mc_open_result("mc_qc.c", path, "w");
	if (!fp) return MC_EXIT_FILE_OPEN_ERROR;
	fprintf(fp, "ID\tN_HOM1\tN_MISS\tN_HET\tN_HOM2\tF_MISS\tMAF\tHWE_P\tQC\n");
	for (int l = 0; l < r->L; l++) {
		const uint32_t *c = r->var_counts + 4 * (size_t)l;
		fprintf(fp, "%s\t%u\t%u\t%u\t%u\t%.6g\t%.6g\t%.6g\t%s\n", dat->variant_id[l], (unsigned)c[0], (unsigned)c[1], (unsigned)c[2], (unsigned)c[3],
			mc_qc_missing_rate(c[1], c[0] + c[1] + c[2] + c[3]), mc_qc_maf(c), r->hwe_p[l], why[r->var_reason[l]]);
	}
	if ((rc = mc_close_result(fp))) return rc;
	mc_result_path(opt, path, sizeof path, ".qc.ind.txt");
	if (!(fp = mc_open_result("mc_qc.c", path, "w"))) return MC_EXIT_FILE_OPEN_ERROR;
	fprintf(fp, "FID\tIID\tF_MISS\tHET\tQC\n");
	for (int i = 0; i < r->I; i++) {
		const uint32_t *c = r->ind_counts + 4 * (size_t)i;
		const uint32_t typed = c[0] + c[2] + c[3];
		fprintf(fp, "%s\t%s\t%.6g\t", fid_of(dat, i), iid_of(dat, i), mc_qc_missing_rate(c[1], (uint32_t)r->L));
		if (typed) fprintf(fp, "%.6g", (double)c[2] / (double)typed);
		else fprintf(fp, "nan");
		fprintf(fp, "\t%s\n", r->ind_keep[i] ? "kept" : "mind");
	}
	return mc_close_result(fp);
}
