/*
 * mc_cli.h -- the drop-in surface around the EM hot path: command line, STRUCTURE reader, result writers and the
 * model-selection driver of MULTICLUST, written from scratch as plain host C.  None of it touches the GPU
 * directly; all array arithmetic goes through mc_host.h -> include/multiclust_hip.h.
 * Each function cites the reference code whose observable behaviour (flags, file formats, stdout lines) it keeps.
 */
#ifndef MC_CLI_H
#define MC_CLI_H

#include <stdio.h>
#include "mc_host.h"

#define MC_MISSING (-9)		/* reference multiclust.h:140 */

/* exit status of the program: the reference returns its error enum from main() (message.h:21-41, multiclust.c:157-163), so a
 * script that tests $? sees these values */
enum { MC_EXIT_OK = 0, MC_EXIT_HELP = 1 /* -h: usage() is reached through the error path (multiclust.c:1500-1502) */, MC_EXIT_MEMORY_ALLOCATION = 3, MC_EXIT_FILE_OPEN_ERROR = 5, MC_EXIT_FILE_FORMAT_ERROR = 7,
       MC_EXIT_INVALID_CMDLINE = 8, MC_EXIT_INVALID_CMD_OPTION = 9, MC_EXIT_INVALID_CMD_ARGUMENT = 10, MC_EXIT_INVALID_USER_SETUP = 11, MC_EXIT_INTERNAL_ERROR = 13 };

typedef struct mc_cli_options {
	mc_options em;			/* the EM-layer options (mc_host.h) */
	const char *filename;		/* -f */
	const char *filename_file;	/* file part of filename (multiclust.c:1483-1492) */
	const char *path;		/* -d, default "./" */
	const char *outfile_name;	/* -o */
	int min_K, max_K;		/* -1 / -2 / -k, default 6 */
	int n_init;			/* -n, default 50 */
	int n_bootstrap;		/* -b */
	int n_rand_em_init;		/* -m (stored, never selects Rand-EM in the reference either) */
	int missing_value;		/* --missing */
	int R_format;			/* -R */
	int ploidy;			/* -p, default 2 */
	int seed_given;			/* -r seen: the reference only calls srand() then (multiclust.c:1592-1596) */
	int target_ll, target_revisit;	/* -u l / -u n */
	double desired_ll;
	int n_repeat;			/* -w n */
	unsigned int repeat_seconds, max_repeat_seconds;	/* -w t / -w m (minutes on the command line) */
	int write_files;
	int compact;
	int parallel;			/* -M */
	int device;			/* --device (extension): HIP device index */
	int n_gpus;			/* --gpus (extension): shard initialisations over devices device..device+n_gpus-1 */
	int n_streams;			/* --streams (extension): concurrent fits per device, each with its own context and
					 * stream; small data sets do not fill a GPU with one fit */
	const char *pfile, *qfile;	/* -P / -Q: initial parameters of the admixture model from files (read_file.c:880-959) */
	const char *afile;		/* -A: a partition of the individuals to compare the fitted one with (multiclust.c:1416-1418) */
	const char *bed_prefix;		/* --bed (extension): read <prefix>.bed / .bim / .fam instead of the STRUCTURE file of -f */
	int cv_folds;			/* --cv <F> (extension): F-fold cross-validation of the best fit of every K (admixture model); 0 = off */
	double cv_floor;		/* --cv-floor <x>: smallest prediction a held-out copy is scored with; 0 = the default of mc_cross_validate */
	int se_replicates;		/* --se <B> (extension): bootstrap standard errors of the mixing proportions of the best fit of every K
					 * from B resamples of the loci (mc_locus_bootstrap, either model); 0 = off */
	int se_block;			/* --se-block <n>: blocks of n neighbouring loci are resampled; default 1 */
	const char *query_file;		/* --query <file> (extension): I tokens 0 (panel) / 1 (query); the query individuals are hidden from every
					 * fit and fitted against the best fit of every K afterwards (mc_query.c) */
	int fill;			/* --fill (extension): the missing genotypes filled from the best fit of every K (mc_impute.c) */
	int fst;			/* --fst (extension): divergence of the clusters of the best fit of every K (mc_diverge.c) */
	int resid;			/* --resid (extension): residual correlation between the individuals under the best fit of every K (mc_resid.c) */
	int prune, prune_window_given;	/* --prune <t> / --prune-window <W> seen (extension, mc_ld.c; both need --bed) */
	double prune_t;			/* --prune <t>: a variant in r2 > t with a kept variant of its chromosome at most W before it is removed; 0 < t <= 1 */
	int prune_window;		/* --prune-window <W>: in variants, 1 ... MCHIP_LD_MAX_WINDOW; default 50 */
	int king;			/* --king-cutoff <t> seen (extension, mc_king.c; needs --bed) */
	double king_t;			/* --king-cutoff <t>: individuals are removed until no two kept ones have KING-robust kinship > t; 0 < t < 0.5 */
	int mind, geno, maf, hwe;	/* --mind / --geno / --maf / --hwe <t> seen (extensions, mc_qc.c; each needs --bed) */
	double mind_t;			/* --mind <t>: individuals whose missing rate over the variants of the file is > t are removed; 0 <= t < 1 */
	double geno_t;			/* --geno <t>: variants whose missing rate over the individuals kept is > t are removed; 0 <= t < 1 */
	double maf_t;			/* --maf <t>: variants whose minor-allele frequency over the individuals kept is < t are removed; 0 < t <= 0.5 */
	double hwe_t;			/* --hwe <t>: variants whose Hardy-Weinberg exact-test p over the individuals kept is < t are removed; 0 < t < 1 */
	int pca;			/* --pca <n> (extension, mc_pca.c; needs --bed): the n leading principal components of the fileset the filters left; 0 = off, 1 ... MC_PCA_MAX */
	int pca_iter;			/* --pca-iter <m>: iterations of the subspace iteration at most; default 200 */
	double pca_tol;			/* --pca-tol <t>: a component has converged when its residual is <= t; 0 < t < 1, default 1e-6 */
	int kinship;			/* --kinship <t> seen (extension, mc_kinship.c): kinship between the individuals under the best fit of every K */
	double kinship_t;		/* --kinship <t>: the pairs with phi > t are reported; 0 < t < 0.5 */
} mc_cli_options;

/* what --pca found (mc_pca.c): the n_pc leading eigenpairs of the matrix of mchip_bed_pca on the I individuals and L variants held, L' =
 * n_used of them polymorphic: eigenvalues [n_pc], eigenvectors [I][n_pc], residuals [n_pc], the trace of the matrix, the iterations run */
typedef struct mc_pca_result {
	int n_pc, I, L, n_used, n_iter;
	double trace;
	double *eigenvalues, *eigenvectors, *residuals;
} mc_pca_result;

/* what quality control (mc_qc.c) found in a fileset of I individuals and L variants: ind_counts [I][4] over all variants, ind_keep [I];
 * var_counts [L][4] and hwe_p [L] over the kept individuals (mchip_bed_qc), var_reason [L] = why a variant went */
enum { MC_QC_KEPT = 0, MC_QC_GENO = 1, MC_QC_MAF = 2, MC_QC_HWE = 3 };
typedef struct mc_qc_result {
	int I, L, I_kept, L_kept;
	int n_reason[4];		/* variants by var_reason */
	uint32_t *ind_counts, *var_counts;
	double *hwe_p;
	uint8_t *ind_keep, *var_reason;
} mc_qc_result;

/* one related pair of --king-cutoff: individuals i < j of the fileset, their counts n_ij, hh_ij, op_ij and kinship (mchip_bed_king) */
typedef struct mc_king_pair {
	int i, j;
	uint32_t n, hh, op;
	double phi;
} mc_king_pair;

typedef struct mc_cli_data {
	int I, L, ploidy, M;		/* M = max alleles at a locus */
	int missing_data;
	int interleaved;
	int *IL;			/* [I*ploidy][L] allele codes as read (reference dat->IL); released by the reader once geno exists */
	int32_t *uniquealleles;		/* [L] */
	int **L_alleles;		/* [L][..] ascending real alleles (phantom slot excluded) */
	uint8_t *geno;			/* [I][L][ploidy] allele indices, 0xFF missing */
	char **names;			/* [I] */
	int *locale;			/* [I] index into pops */
	char **pops;
	int numpops;
	int *i_p;			/* [numpops] individuals per locale */
	int T;
	int32_t *toff;			/* [L+1] */
	/* a PLINK fileset (mc_read_bed) stays packed: geno is NULL; see mc_data in mc_host.h */
	uint8_t *bed;			/* [L][bed_record_bytes]: the .bed file behind its three header bytes */
	size_t bed_record_bytes;	/* ceil(I/4) */
	struct mc_lazy_geno *lazy;
	/* the fileset's variants, L_file of them (mc_read_bed): chromosome and id of each, the first two fields of its .bim line (tokens of
	 * bim_text).  --prune leaves L of them: locus l is variant variant_of[l] of the fileset (ascending); NULL = every variant is a locus */
	int L_file;
	char *bim_text, **chrom, **variant_id;
	int *variant_of;
	/* the fileset's individuals, I_file of them.  --king-cutoff leaves I of them: individual i is individual individual_of[i] of the
	 * fileset (ascending), names, locale, pops, numpops and i_p are the kept ones', and fam_fid / fam_iid [I_file] hold every .fam line's
	 * two ids; king_pairs [n_king_pairs] are the related pairs found, in (i, j) order.  individual_of = NULL: every individual of the
	 * fileset is in the data set and none of these is set */
	int I_file;
	int *individual_of;
	char **fam_fid, **fam_iid;
	mc_king_pair *king_pairs;
	size_t n_king_pairs;
	/* the filters that have run (MC_FILTER_*): each runs once, quality control before the other two.  An axis that an earlier filter
	 * thinned is thinned further: variant_of / individual_of are composed and stay places in the fileset */
	int filters_run;
	mc_qc_result *qc;		/* what quality control found (mc_qc_data), NULL without it */
} mc_cli_data;
enum { MC_FILTER_QC = 1, MC_FILTER_PRUNE = 2, MC_FILTER_KING = 4 };

/* ---- file plumbing (mc_files.h, libc only, static inline): one copy of what the readers, the writers and the filters of a fileset share.  `origin`
 * is the caller's source file: the lines on stderr read "ERROR [<origin>::open_out]: ..." and "ERROR [<origin>::slurp]: ...".
 * mc_result_path: the stem of the result files -- opt->outfile_name (-o), else opt->path (-d), a '/' unless it is empty or ends in
 * '/' or '\', and the file part of the data file's name -- followed by the printf-style suffix, into out[n] (cut, never overrun).
 * Returns the length of the stem as it stands in out: snprintf(out + len, n - len, ...) puts another suffix behind the same stem.
 * mc_open_result: fopen, and the "could not open file" line on failure.  mc_close_result: fclose; MC_EXIT_FILE_OPEN_ERROR when the
 * stream had failed or the close does, else 0.
 * mc_path_of: prefix + ext, allocated.  mc_slurp: the whole file into memory, NUL-terminated, *size = its length; returns 0 or the
 * exit status of the failure, which it reports (cannot be opened 5, out of memory 3, short read 7).
 * mc_is_blank: the white space between the tokens of a line.  mc_dup_token: an allocated copy of len bytes, NUL-terminated.
 * mc_now_s: the monotonic clock in seconds.  mc_timing_line: under MC_READER_TIMING the line "INFO [<origin>]: <what> <seconds> s"
 * for the time since t_start; returns the clock, i.e. the start of the next phase.
 * mc_lines: the lines of text[n] that hold anything but white space, in order.  After mc_lines_next returned 1: line = the line's
 * first byte, first = its first byte that is not blank, end = its '\n' (or the text's end: a last line without one), stop = the
 * byte behind the line, its '\n' included; 0: no such line is left.
 * mc_copy_kept_lines: file `to` = of the lines of file `from` that hold anything but white space, the kept[0 .. n - 1]-th
 * (ascending), byte for byte with their ends.  mc_write_kept_lists: <stem><suffix>.in and <stem><suffix>.out -- of n_file entries
 * those that kept[0 .. n_kept - 1] (ascending) names and the others, each in file order, entry v as print(fp, arg, v) writes it. */
#include "mc_files.h"

/* read_file + summarize_alleles + sufficient_statistics (read_file.c:38-300,443-663), default (allele-code) mode */
int mc_read_structure(const mc_cli_options *opt, mc_cli_data *dat);
void mc_free_data(mc_cli_data *dat);

/* PLINK 1 binary fileset opt->bed_prefix + ".bed" / ".bim" / ".fam" (an extension: the reference reads STRUCTURE text only).
 * The data set is BY DEFINITION what mc_read_structure yields on the equivalent STRUCTURE file -- a header of L locus names,
 * then per individual of the .fam file, in its order, two lines "IID FID a_1 ... a_L" with homozygous A1 -> 1 / 1,
 * heterozygous -> 1 / 2, homozygous A2 -> 2 / 2, missing -> -9 / -9 -- so names are the IIDs, locales the FIDs in order of
 * first appearance, and uniquealleles, L_alleles, M, T, toff and missing_data are the reader's (a locus without an observed
 * call has no allele column and does not set missing_data).  ploidy = 2; geno stays NULL, the records are kept packed (bed,
 * bed_record_bytes) and models upload them as they are.  Returns 0 or the reference's exit status for the failure: a file that
 * cannot be opened 5; magic bytes, sample-major mode, file size against the line counts of .bim and .fam 7.
 * L_file = L; chrom and variant_id are the first two fields of every .bim line, variant_of stays NULL (mc_ld_prune_data sets it). */
int mc_read_bed(const mc_cli_options *opt, mc_cli_data *dat);
/* the part of mc_read_bed that follows the records: uniquealleles, L_alleles, M, T, toff and missing_data of the L records held in
 * dat->bed, allocated anew (the pointers are overwritten).  Returns 0 or MC_EXIT_MEMORY_ALLOCATION. */
int mc_bed_summarize(mc_cli_data *dat);
/* The CPU form of the device's unpacking: L records of record_bytes bytes (sample j of a record in byte j/4, bits 2(j%4) and
 * 2(j%4)+1: 0 homozygous A1, 1 missing, 2 heterozygous, 3 homozygous A2; padding bits ignored) -> uniquealleles[L] and
 * geno[I][L][2] of the equivalent STRUCTURE file.  Either output may be NULL. */
void mc_bed_decode(int I, int L, const uint8_t *bed, size_t record_bytes, int32_t *uniquealleles, uint8_t *geno);

/* what a finished initialisation hands to the writers */
typedef struct mc_fit_view {
	int K, converged;
	double logL, aic, bic;
	const double *q;	/* [I][K] or [K]: slot pindex */
	const double *p;	/* [K][T] */
	const double *sik;	/* [I][K]: sum_lm d_iklm of the last E step, or vik */
} mc_fit_view;

/* read_afile (read_file.c:970-999): I cluster labels 1, 2, ... (white space between them) -> labels[i] - 1 and their number
 * *pK = largest label; returns 0 or the reference's exit status for the failure (file cannot be opened 5, contents 7) */
int mc_read_afile(const char *path, int I, int **labels, int *pK);
/* adj_rand(..., ADJUSTED_RAND_INDEX) (multiclust.c:1903-1985): adjusted Rand index of two labelings of n observations with k1
 * and k2 classes, the reference's sums in the reference's order; NaN (0 / 0) where it has it */
double mc_adjusted_rand(int n, int k1, int k2, const int *cl1, const int *cl2);
/* partition_admixture / partition_mixture (write_file.c:350-382, 585-603): MAP cluster per individual, count_K */
void mc_partition(const mc_cli_data *dat, const mc_fit_view *fit, int *I_K, int *count_K);
/* write_file_detail + popq_* + indivq_* (write_file.c:203-348, 398-475, 492-569, 618-732) */
int mc_write_results(const mc_cli_options *opt, const mc_cli_data *dat, const mc_fit_view *fit, const int *count_K);
/* --se (an extension): <stem>.<admix|mix>.K=<K>.se.txt, lines "i k eta se mean n" (tab-separated, one header line; without i under
 * shared mixing proportions and the mixture model): the estimate q, and the standard error, mean and number of replicates of
 * mc_locus_bootstrap for every entry */
int mc_write_se(const mc_cli_options *opt, const mc_cli_data *dat, int K, const double *q, const double *mean, const double *se,
		const int32_t *count);

/* --query (an extension, mc_query.c): the query file -- exactly I tokens separated by white space, each 0 (panel) or 1 (query), in
 * the data set's individual order, at least one of each -> mask[I] (the caller frees it); returns 0 or the exit status mc_read_afile
 * gives the failure (file cannot be opened 5, contents 7) */
int mc_query_read(const char *path, int I, uint8_t **mask_out);
/* <stem>.admix.K=<K>.query.txt: one header line, then one tab-separated line per query individual in data order: i, iter, converged,
 * logL, and the K mixing proportions (%.10f, as .se.txt prints); arrays as mc_query_fit fills them */
int mc_write_query(const mc_cli_options *opt, int K, int n, const int32_t *rows, const int32_t *iter, const uint8_t *converged,
		   const double *logL, const double *q);


/* --fill (an extension, mc_impute.c): the data set with its missing copies filled (filled [I][L][ploidy], as mc_impute gives it),
 * written as a copy of the file it was read from.
 * mc_write_filled_structure: opt->filename byte for byte -- header, "-1" line, both layouts, label columns, white space, line ends --
 * except that each token the reader took for a missing allele copy and that was filled is the decimal label L_alleles[l][m].
 * mc_write_filled_bed: <out_prefix>.bed with each missing record that was filled replaced by homozygous A1 / heterozygous /
 * homozygous A2 (magic bytes and padding bits kept), .bim and .fam of opt->bed_prefix copied byte for byte (of a data set
 * pruned by --prune the .bim lines of the variants kept, of one thinned by --king-cutoff the .fam lines of the individuals kept).
 * mc_write_filled: the one the input calls for, to <stem>.admix.K=<K>.filled.stru or <stem>.admix.K=<K>.filled.bed / .bim / .fam.
 * Return 0 or an exit status of the enum above. */
int mc_write_filled_structure(const mc_cli_options *opt, const mc_cli_data *dat, const uint8_t *filled, const char *out_path);
int mc_write_filled_bed(const mc_cli_options *opt, const mc_cli_data *dat, const uint8_t *filled, const char *out_prefix);
int mc_write_filled(const mc_cli_options *opt, const mc_cli_data *dat, int K, const uint8_t *filled);

/* --fst (an extension, mc_diverge.c): <stem>.<admix|mix>.K=<K>.fst.txt -- per cluster its weight and expected heterozygosity, then
 * the K x K net-distance matrix and the K x K F_ST matrix -- and <stem>.<admix|mix>.K=<K>.fst.loci.txt -- per locus its index, its
 * number of columns, HT_l and F_l; the formats are in the header comment of mc_diverge.c.  Returns 0 or an exit status of the enum
 * above. */
int mc_write_divergence(const mc_cli_options *opt, const mc_cli_data *dat, const mc_divergence_result *r);

/* --resid (an extension, mc_resid.c): <stem>.admix.K=<K>.resid.txt -- the I x I matrix of residual correlations, I^2 numbers -- and
 * <stem>.admix.K=<K>.resid.ind.txt -- per individual its index, mean and largest correlation and the partner of that; the formats are
 * in the header comment of mc_resid.c.  Returns 0 or an exit status of the enum above. */
int mc_write_resid(const mc_cli_options *opt, const mc_resid_result *r);
/* --kinship (an extension, mc_kinship.c): <stem>.admix.K=<K>.kin0 -- the pairs above the threshold with phi, the two sums and the
 * degree -- and <stem>.admix.K=<K>.kin.ind.txt -- per individual its self-kinship, inbreeding coefficient, number of partners above the
 * threshold, largest phi and the partner of that; the formats are in the header comment of mc_kinship.c.  Returns 0 or an exit status
 * of the enum above. */
int mc_write_kinship(const mc_cli_options *opt, const mc_kinship_result *r);

/* ---- what the filters of a fileset that run before the fit share (mc_filter.h, included at the end of this file); pre_fit() of mc_cli_stages.c runs them.
 * mc_filter_on_device: opens device opt->device, calls decide(opt, &dev, out) -- dev is what a band callback on the device needs --
 * and closes it; the lines "ERROR [<origin>]: cannot open device .. for <option>" and "ERROR [<origin>]: <noun> failed (status ..):
 * <the device's last error>" are its.  Returns 0 or the status.
 * mc_filter_resummarize: the data set has changed -- uniquealleles, toff and L_alleles of the L_before loci it had are dropped and
 * made anew from the records held now (mc_bed_summarize), and under MC_READER_TIMING the seconds since t_start are reported as the
 * readers report theirs.  Returns mc_bed_summarize's status.
 * mc_filter_rebuild_individuals: everything of the data set that is per individual made anew for the n kept ones, map[x] = the x-th
 * kept one's place among the I held now (ascending): names, locale, pops, numpops, i_p as read_fam (mc_bed.c) yields them on the kept
 * lines, I = n.  The first time the ids of every .fam line move to fam_fid / fam_iid [I_file]; later they stay.  individual_of is the
 * caller's to compose.  Returns 0 or MC_EXIT_MEMORY_ALLOCATION, the data set then unchanged. */
typedef struct mc_device_band {
	mchip_context *ctx;
	const mc_cli_data *dat;
} mc_device_band;
typedef int (*mc_filter_fn)(const mc_cli_options *opt, mc_device_band *dev, void *out);

/* --prune (an extension, mc_ld.c; r2 is defined in include/multiclust_hip.h, the rule in the header comment of mc_ld.c).
 * mc_ld_band_fn: r2[n_first][window] of the variants l0 ... l0 + n_first - 1 with their successors, as mchip_bed_ld_band fills it;
 * returns 0 or a status.
 * mc_ld_prune_greedy: keep[l] = 1 / 0 for the L variants under the forward greedy rule with window W and threshold t (a pair counts
 * when its r2 > t: NaN never does); the band is asked for in slabs of at most `slab` first variants, in ascending order; chrom[l]
 * (NULL: one chromosome) are compared as strings, pairs on different chromosomes do not count.  Returns 0, MCHIP_ERR_INVALID,
 * MCHIP_ERR_ALLOC or the band's status.
 * mc_ld_compact: the kept records of bed [L][record_bytes] moved to its front in order; variant_of[n] (may be NULL) = the index the
 * n-th kept record had.  Returns their number.
 * mc_ld_prune_data: a data set as mc_read_bed yields it, pruned by opt->prune_t and opt->prune_window with the band of device
 * opt->device: the data set mc_read_bed yields on the fileset of the variants kept -- bed compacted, L their number, uniquealleles,
 * L_alleles, M, T, toff and missing_data theirs (mc_bed_summarize) -- with variant_of set; L_file, chrom and variant_id stay the
 * fileset's.  Of a data set whose variants quality control thinned before, variant_of is composed with the map held -- still places in
 * the fileset -- and the chromosomes are read through it.  Under MC_READER_TIMING it reports its seconds as the readers do.  Returns 0 or a
 * status; MC_EXIT_INTERNAL_ERROR when it ran before.
 * mc_write_prune_lists: <stem>.prune.in and <stem>.prune.out -- the ids of the variants kept and removed, one per line in file order. */
#define MC_LD_SLAB 65536
typedef int (*mc_ld_band_fn)(void *arg, int l0, int n_first, int window, double *r2);
int mc_ld_prune_greedy(int L, int W, double t, int slab, mc_ld_band_fn band, void *arg, const char *const *chrom, uint8_t *keep);
int mc_ld_compact(int L, size_t record_bytes, const uint8_t *keep, uint8_t *bed, int *variant_of);
int mc_ld_prune_data(const mc_cli_options *opt, mc_cli_data *dat);
int mc_write_prune_lists(const mc_cli_options *opt, const mc_cli_data *dat);

/* --king-cutoff (an extension, mc_king.c; the kinship is defined in include/multiclust_hip.h, the rule in the header comment of
 * mc_king.c).
 * mc_king_band_fn: phi[n_rows][I] and counts[n_rows][I][4] of the rows i0 ... i0 + n_rows - 1 against all individuals, as
 * mchip_bed_king fills them; returns 0 or a status.
 * mc_king_edges: the relatedness graph of I individuals at threshold t as an I x I bit matrix, ceil(I/64) words a row, bit j % 64
 * of word j / 64 of row i set where i != j and phi_ij > t (NaN never is), and the pairs i < j among them in (i, j) order; the
 * kinships are asked for in slabs of at most `slab` rows, in ascending order.  The caller frees both arrays.  Returns 0,
 * MCHIP_ERR_INVALID, MCHIP_ERR_ALLOC or the band's status.
 * mc_king_select: keep[i] = 1 / 0 under the greedy rule on such a matrix; at least one individual is kept.
 * mc_king_compact: every record of bed [L][record_bytes] repacked to the kept individuals' codes in order, ceil(I'/4) bytes a
 * record, padding bits 0, records back to back from the front, and the 8 bytes behind the last one 0 (bed has the reader's 8 spare
 * bytes behind its records); individual_of[n] (may be NULL) = the index the n-th kept individual had.  Returns I', or -1 when out of
 * memory.
 * mc_king_data: a data set as mc_read_bed (and mc_ld_prune_data) yields it, thinned at opt->king_t with the kinships of device
 * opt->device: the data set mc_read_bed yields on the fileset of the individuals kept -- I, names, locale, pops, numpops, i_p (locales
 * in order of first appearance among the kept), bed, bed_record_bytes, lazy, and uniquealleles, L_alleles, M, T, toff and missing_data
 * (mc_bed_summarize) theirs -- with I_file, individual_of, fam_fid, fam_iid and king_pairs set.  Of a data set whose individuals quality
 * control thinned before, individual_of is composed with the map held, I_file, fam_fid and fam_iid stay the fileset's, and king_pairs
 * name places in the fileset all the same.  Under MC_READER_TIMING it reports its seconds as the readers do.  Returns 0 or a status;
 * MC_EXIT_INTERNAL_ERROR when it ran before.
 * mc_write_king_lists: <stem>.king.cutoff.in and <stem>.king.cutoff.out -- "FID\tIID" of the individuals kept and removed, one per
 * line in file order -- and <stem>.king.kin0, the related pairs (the format is at the function). */
#define MC_KING_SLAB 1024
typedef int (*mc_king_band_fn)(void *arg, int i0, int n_rows, double *phi, uint32_t *counts);
int mc_king_edges(int I, double t, int slab, mc_king_band_fn band, void *arg, uint64_t **bits_out, mc_king_pair **pairs_out, size_t *n_pairs_out);
int mc_king_select(int I, const uint64_t *bits, uint8_t *keep);
int mc_king_compact(int I, int L, size_t record_bytes, const uint8_t *keep, uint8_t *bed, int *individual_of);
int mc_king_data(const mc_cli_options *opt, mc_cli_data *dat);
int mc_write_king_lists(const mc_cli_options *opt, const mc_cli_data *dat);
/* a new decoder of the packed records for dat->lazy (mc_bed.c): nothing decoded yet; NULL when out of memory */
struct mc_lazy_geno *mc_bed_lazy_new(void);

/* --mind, --geno, --maf, --hwe (extensions, mc_qc.c; the counts and the exact test are defined in include/multiclust_hip.h, the rules and
 * their order in the header comment of mc_qc.c).
 * mc_qc_missing_rate: num / den, one division of two integers converted to double; 0 when den = 0.
 * mc_qc_maf: min(2 n0 + n2, 2 n3 + n2) / (2 N) of c = {n0, n1, n2, n3} with N = n0 + n2 + n3, one division; 0 when N = 0.
 * mc_qc_individuals: keep[i] = 0 where individual i's missing rate ind_counts[i][1] / L is > t, else 1; returns the number kept.
 * mc_qc_variants: reason[l] = the first rule variant l fails in the order geno (missing rate var_counts[l][1] / (the four counts' sum)
 * > geno_t), maf (MAF < maf_t), hwe (hwe_p[l] < hwe_t), among the rules opt names, or MC_QC_KEPT; n_reason[4] counts them.
 * mc_qc_result_free (mc_filter.h, libc only: mc_free_data calls it): the arrays and the record.
 * mc_qc_data: a data set as mc_read_bed yields it, no filter having run, filtered by the rules opt names with the counts of device
 * opt->device -- one call of mchip_bed_qc without --mind, two with it, the second under the keep bytes: the data set mc_read_bed yields
 * on the fileset of the individuals and variants kept, individual_of / variant_of set on an axis that lost something, and dat->qc what
 * was found.  When no individual or no variant is left it says which option emptied the data set and returns
 * MC_EXIT_INVALID_USER_SETUP.  Returns 0 or a status.
 * mc_qc_line: the stdout line "Quality control: ..." of dat->qc, only the parts whose option was given.
 * mc_write_qc_lists: <stem>.mind.in / .out ("FID\tIID", with --mind), <stem>.qc.in / .out (variant ids, with --geno, --maf or --hwe),
 * <stem>.qc.var.txt and <stem>.qc.ind.txt (the formats are at the function). */
double mc_qc_missing_rate(uint32_t num, uint32_t den);
double mc_qc_maf(const uint32_t *c);
int mc_qc_individuals(int I, int L, const uint32_t *ind_counts, double t, uint8_t *keep);
void mc_qc_variants(const mc_cli_options *opt, int L, const uint32_t *var_counts, const double *hwe_p, uint8_t *reason, int *n_reason);
int mc_qc_data(const mc_cli_options *opt, mc_cli_data *dat);
void mc_qc_line(FILE *fp, const mc_cli_options *opt, const mc_cli_data *dat);
int mc_write_qc_lists(const mc_cli_options *opt, const mc_cli_data *dat);

/* --pca, --pca-iter, --pca-tol (extensions, mc_pca.c; the matrix is defined in include/multiclust_hip.h, the iteration in
 * csrc/mchip_pca_algebra.h).  MC_PCA_EXTRA start vectors run beside the n asked for.
 * mc_pca_data: the opt->pca leading components of the data set as the filters left it, with device opt->device; the data set is not
 * changed.  More components than I - 1 end the run: it says so, naming the option, and returns MC_EXIT_INVALID_USER_SETUP.  Not
 * converging is no error.  On success the caller owns the arrays (mc_pca_result_free).  Returns 0 or a status.
 * mc_pca_line: the stdout line "PCA: <n> components of <I> individuals x <L'> of <L> variants (<it> iterations, largest residual <r>):
 * variance explained <lambda_1 / trace> ...".
 * mc_pca_warn: when a residual exceeds opt->pca_tol, one line naming those components; returns their number.
 * mc_write_pca: <stem>.eigenvec, <stem>.eigenval and <stem>.pca.txt (the formats are at the function). */
#define MC_PCA_MAX 48
#define MC_PCA_EXTRA 10
int mc_pca_data(const mc_cli_options *opt, const mc_cli_data *dat, mc_pca_result *r);
void mc_pca_result_free(mc_pca_result *r);
void mc_pca_line(FILE *fp, const mc_pca_result *r);
int mc_pca_warn(FILE *fp, const mc_cli_options *opt, const mc_pca_result *r);
int mc_write_pca(const mc_cli_options *opt, const mc_cli_data *dat, const mc_pca_result *r);

#include "mc_filter.h"

#endif
