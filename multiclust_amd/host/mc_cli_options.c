/*
 * mc_cli_options.c -- the command line of the `multiclust` binary: usage(), the defaults, parse_options() with what the options
 * refuse of each other, and check_setup(), the checks that need the data set.
 *
 * Keeps the reference's observable surface: argv flags as its parse_options() reads them (reference multiclust.c:1396-1735; 2-3 letter
 * disambiguation of --bound/--format/--impute/--missing/--projection/--plus/--simulate, -I1) and the defaults of make_options
 * (902-978).  Deliberately absent (documented in DESIGN.md): -I/-I1 (allele-index mode gives different numbers from default mode in
 * the reference itself), --impute, --simulate, -x (not implemented in the reference either).  The extensions are spelled in full or
 * by a prefix no reference option has; usage() says what each does.
 *
 * A new option is a field of mc_cli_options (mc_cli.h), its lines in usage(), its case in the switch of parse_options() and its
 * refusals behind the switch: through refuse_post_fit() for a post-fit analysis, a row of qc_options[] for a threshold of quality
 * control.  The order of the refusals is the order in which a command line that breaks several rules hears of them.
 */
#include "mc_main.h"

#include <errno.h>
#include <stddef.h>
#include <string.h>

static void usage(FILE *fp, const char *prog)
{
	fprintf(fp,
		"Usage: %s -f <file> | --bed <prefix> [-a] [-k <K> | -1 <minK> -2 <maxK>] [options]\n"
		"  -a            admixture model (default: mixture)      -c  shared mixing proportions (with -a)\n"
		"  -k <n>        number of clusters K (default 6)        -1 <n>, -2 <n>  minimum / maximum K\n"
		"  -n <n>        random initialisations (default 50)     -r <seed>  random seed\n"
		"  -s <0..6>     acceleration: 0 EM, 1-3 SQUAREM, 4-6 quasi-Newton q=1..3\n"
		"  -E <d> -e <d> absolute (1e-4) / relative (0) log-likelihood convergence tolerance\n"
		"  -T <n> -t <m> iteration / time (minutes) limits        -i <n>  initial plain EM iterations\n"
		"  -g <n>        step-size back-tracking attempts         --bound <d>  parameter lower bound (1e-8)\n"
		"  --projection  disable the simplex projection           -p <n>  ploidy (default 2)\n"
		"  -b <n>        parametric bootstrap of H0: K-1 vs HA: K -u l <ll> | n <times>  target log likelihood / revisits\n"
		"  -w n <n> | t <min> | m <min>   repeat the fit for timing (no files written)\n"
		"  -d <dir> -o <stem>  output directory / file stem      -R  R-formatted STRUCTURE file\n"
		"  --missing <n> missing-data code (default -9)           -M  print only the maximum log likelihood\n"
		"  -v [level]    verbosity                                --device <n>  HIP device index\n"
		"  --gpus <n>    shard the initialisations (admixture) and the bootstrap replicates (both models) over n GPUs;\n"
		"                one RCCL all-reduce of each result table\n"
		"  --streams <n> n concurrent fits per GPU, each on its own stream (small data sets do not fill a GPU)\n"
		"  -P <file> -Q <file>  initial allele frequencies p[k][l][0] (L*K numbers, biallelic loci) and mixing proportions of the admixture model\n"
		"  --randem      Rand-EM initialisation: the best of -m <n> (50) candidates from random allele centers\n"
		"  -A <file>     a partition of the individuals (labels 1, 2, ...): the adjusted Rand index of the fitted one is reported\n"
		"  --bed <prefix>  read the PLINK 1 fileset <prefix>.bed/.bim/.fam instead of -f (diploid; not with -f, -R or -p other than 2;\n"
		"                --missing is ignored); the 2-bit records are uploaded as they are and unpacked on the GPU\n"
		"  --cv <F>      F-fold cross-validation (2..64) of the best fit of every K: one more line 'CV error (K=..)' per K; needs -a,\n"
		"                not with -b, -w, -M or --gpus above 1        --cv-floor <x>  smallest prediction scored, in (0, 1] (1/(I*ploidy+1))\n"
		"  --se <B>      standard errors of the mixing proportions of the best fit of every K from B (2..10000) bootstrap resamples of\n"
		"                the loci: one more line 'Bootstrap SE (K=..)' per K and a file <stem>.<admix|mix>.K=<K>.se.txt; either model; not with -b,\n"
		"                -w, -M or --gpus above 1    --se-block <n>  resample blocks of n neighbouring loci (1)\n"
		"  --query <file>  I tokens, 0 (panel) or 1 (query), in the order of the individuals: the query individuals are hidden from every\n"
		"                fit (the result files show them as individuals without data; AIC and BIC keep the data set's number of\n"
		"                individuals) and their mixing proportions are then fitted to the allele frequencies of the best fit of every K:\n"
		"                one more line 'Query fit (K=..)' per K and a file <stem>.admix.K=<K>.query.txt; needs -a, not with -c, -b, -w,\n"
		"                -M, -A, --cv, --se, --randem, or --gpus / --streams above 1\n"
		"  --fill        fill every missing allele copy with the most probable alleles under the best fit of every K: one more line\n"
		"                'Imputation (K=..)' per K and the data file with the copies filled in, <stem>.admix.K=<K>.filled.stru (or .filled.bed /\n"
		"                .bim / .fam with --bed); needs -a, not with -b, -w, -M, --query or --gpus above 1\n"
		"  --fst         divergence of the clusters of the best fit of every K: one more line 'Divergence (K=..)' per K -- mean, smallest and\n"
		"                largest pairwise Fst and the Fst among the clusters -- and the files <stem>.<admix|mix>.K=<K>.fst.txt (weight and expected\n"
		"                heterozygosity of every cluster, net distances, pairwise Fst) and .fst.loci.txt (Fst per locus); either model; not\n"
		"                with -b, -w, -M or --gpus above 1\n"
		"  --resid       residual correlation of the best fit of every K between every pair of individuals (near zero under an adequate fit;\n"
		"                relatives, duplicates and a K that is too small show as positive blocks): one more line 'Residual correlation\n"
		"                (K=..)' per K and the files <stem>.admix.K=<K>.resid.txt (the I x I matrix: I*I numbers) and .resid.ind.txt (mean,\n"
		"                largest and partner per individual); needs -a, not with -b, -w, -M or --gpus above 1\n"
		"  --kinship <t> kinship coefficients between the individuals under the best fit of every K, from the fit's individual-specific allele\n"
		"                frequencies (REAP, Thornton et al. 2012; PC-Relate's form; unlike --king-cutoff it holds for admixed pairs); the\n"
		"                pairs with phi > t (0 < t < 0.5) are reported: one more line 'Kinship (K=..)' per K with their number by degree\n"
		"                (duplicate > 0.354, first > 0.177, second > 0.0884, third > 0.0442) and the files <stem>.admix.K=<K>.kin0 (i, j, phi,\n"
		"                the two sums, degree) and .kin.ind.txt (self-kinship, inbreeding, partners above t, largest phi and partner per\n"
		"                individual); relatives fitted as a cluster of their own show none; needs -a, not with -b, -w, -M or --gpus above 1\n"
		"  --prune <t>   thin the variants of --bed by linkage disequilibrium before anything is fitted: in file order, a variant whose\n"
		"                squared dosage correlation with a variant already kept, on its chromosome and at most W variants before it,\n"
		"                exceeds t (0 < t <= 1) is removed (forward greedy, as SNPRelate's snpgdsLDpruning; not PLINK's --indep-pairwise);\n"
		"                one more line 'LD pruning: ...' and the ids kept and removed in <stem>.prune.in / .prune.out; the run is the run\n"
		"                on the fileset of the kept variants; needs --bed        --prune-window <W>  W in variants, 1..4096 (50)\n"
		"  --king-cutoff <t>  remove close relatives from --bed before anything is fitted (after --prune, on the variants kept): while two\n"
		"                remaining individuals have KING-robust kinship (Manichaikul et al. 2010; over all variants of the data set) above t\n"
		"                (0 < t < 0.5), the one with the most remaining relatives is removed, of equals the later in the .fam file (greedy, this\n"
		"                program's own rule; not PLINK 2's algorithm, not a maximum independent set); one more line 'Relatedness: ...', the ids\n"
		"                kept and removed in <stem>.king.cutoff.in / .king.cutoff.out and the related pairs in <stem>.king.kin0; the run is the\n"
		"                run on the fileset of the kept individuals: the files of -A and --query describe those, in their order; needs --bed\n"
		"  --mind <t>    remove the individuals of --bed whose missing rate over all variants of the file exceeds t (0 <= t < 1)\n"
		"  --geno <t>    remove the variants whose missing rate over the individuals kept exceeds t (0 <= t < 1)\n"
		"  --maf <t>     remove the variants whose minor-allele frequency over the individuals kept is below t (0 < t <= 0.5)\n"
		"  --hwe <t>     remove the variants whose Hardy-Weinberg exact-test p (Wigginton et al. 2005) over the individuals kept is below t\n"
		"                (0 < t < 1; population structure lowers p by itself: keep t lenient, 1e-6 or less).  Quality control runs before\n"
		"                anything is fitted and before --prune and --king-cutoff, in PLINK 1.9's order: --mind first, then the three variant\n"
		"                rules from one set of counts, a variant's reason being the first rule it fails (geno, maf, hwe); all variants and\n"
		"                individuals count (no chromosome is special); one more line 'Quality control: ...', the ids kept and removed in\n"
		"                <stem>.mind.in / .mind.out and <stem>.qc.in / .qc.out, and the counts, rates and p values of every variant and\n"
		"                individual of the file in <stem>.qc.var.txt / .qc.ind.txt; the run is the run on the fileset of those kept; need --bed\n"
		"  --pca <n>     the n leading principal components (1..48) of --bed as the filters above left it, on the device, before anything is\n"
		"                fitted; no filter: the data set and every fit stay as they are.  The matrix is Z Z'/L' of the genotypes standardised\n"
		"                per variant, missing calls imputed by the mean, monomorphic and all-missing variants left out (flashpca's and PLINK\n"
		"                2's --pca approx; NOT PLINK 1.9's pairwise-complete GRM, not smartpca's normalisation), by block subspace iteration\n"
		"                with n + 10 vectors; one more line 'PCA: ...', <stem>.eigenvec (FID IID PC1..PCn, no header), <stem>.eigenval and\n"
		"                <stem>.pca.txt (eigenvalue, share of the trace, residual, converged 0/1).  A component converges at the rate\n"
		"                lambda_{b+1}/lambda_c per iteration: components inside the noise bulk of the spectrum converge slowly and mean\n"
		"                nothing; those still loose are named in a warning on stderr, the exit status is unchanged; needs --bed\n"
		"                --pca-iter <m>  iterations at most (200)        --pca-tol <t>  residual a component has converged at, 0 < t < 1 (1e-6)\n", prog);
}

static int arg_int(int argc, const char **argv, int i, long *out)
{
	char *end;
	if (i >= argc) return 1;
	errno = 0;
	*out = strtol(argv[i], &end, 10);
	return errno || end == argv[i];
}
static int arg_dbl(int argc, const char **argv, int i, double *out)
{
	char *end;
	if (i >= argc) return 1;
	errno = 0;
	*out = strtod(argv[i], &end);
	return errno || end == argv[i];
}

void defaults(mc_cli_options *o)
{
	memset(o, 0, sizeof *o);
	mc_make_options(&o->em);
	o->path = "./";
	o->min_K = o->max_K = 6;
	o->n_init = 50;
	o->n_rand_em_init = 50;
	o->missing_value = MC_MISSING;
	o->ploidy = 2;
	o->n_repeat = 1;
	o->write_files = 1;
	o->compact = 1;
	o->n_gpus = 1;
	o->n_streams = 1;
	o->se_block = 1;
	o->prune_window = 50;
	o->pca_iter = 200;
	o->pca_tol = 1e-6;
}

#define BAD(msg) do { fprintf(stderr, "ERROR [" MC_FRONT_END "::parse_options]: %s (argument '%s'); try -h\n", msg, i < argc ? argv[i] : ""); return MC_EXIT_INVALID_CMD_ARGUMENT; } while (0)

/* "option X cannot be combined with ...": why = NULL when it can; the status is a bad argument's, or the one given */
static int refuse_as(const char *option, const char *why, int status)
{
	if (!why) return 0;
	fprintf(stderr, "ERROR [" MC_FRONT_END "::parse_options]: %s (argument '%s'); try -h\n", why, option);
	return status;
}
static int refuse(const char *option, const char *why) { return refuse_as(option, why, MC_EXIT_INVALID_CMD_ARGUMENT); }

/* what every post-fit option refuses, in this order: the mixture model where it needs -a, the bootstrap, --gpus above 1, a timed run;
 * then `extra`, the option's own rule (NULL: none, or not broken) */
static int refuse_post_fit(const mc_cli_options *o, const char *option, int needs_admixture, const char *extra)
{
	const char *common = needs_admixture && !o->em.admixture ? "%s needs the admixture model (-a)" :
			     o->n_bootstrap ? "%s cannot be combined with the bootstrap (-b)" :
			     o->n_gpus > 1 ? "%s cannot be combined with --gpus above 1" :
			     !o->write_files || o->parallel ? "%s cannot be combined with -w or -M" : NULL;
	char why[96];
	if (!common) return refuse(option, extra);
	snprintf(why, sizeof why, common, option);
	return refuse(option, why);
}

/* the thresholds of quality control, in the order they are refused in: the option, its "seen" flag and its threshold in
 * mc_cli_options, the interval the threshold must lie in (an end counts when its _in is set) and what is said when it does not */
typedef struct qc_option { const char *name; size_t flag, threshold; double lo, hi; int lo_in, hi_in; const char *range; } qc_option;
#define QC_FIELDS(f) offsetof(mc_cli_options, f), offsetof(mc_cli_options, f##_t)
static const qc_option qc_options[] = {
	{ "--mind", QC_FIELDS(mind), 0, 1, 1, 0, "the missing rate of --mind must lie in [0, 1)" },
	{ "--geno", QC_FIELDS(geno), 0, 1, 1, 0, "the missing rate of --geno must lie in [0, 1)" },
	{ "--maf", QC_FIELDS(maf), 0, 0.5, 0, 1, "the minor-allele frequency of --maf must lie in (0, 0.5]" },
	{ "--hwe", QC_FIELDS(hwe), 0, 1, 0, 0, "the p value of --hwe must lie in (0, 1)" },
};
#define N_QC_OPTIONS (sizeof qc_options / sizeof *qc_options)
static int *qc_flag(mc_cli_options *o, const qc_option *q) { return (int *)((char *)o + q->flag); }
static double *qc_threshold(mc_cli_options *o, const qc_option *q) { return (double *)((char *)o + q->threshold); }

int parse_options(mc_cli_options *o, int argc, const char **argv)
{
	long v;
	double d;
	for (int i = 1; i < argc; i++) {
		if (strlen(argv[i]) < 2) BAD("malformed option");
		/* (in full, ahead of the switch: -g... is the back-tracking, -h... the help, --mi... --missing, -m... the candidates) */
		const qc_option *qc = qc_options;
		while (qc < qc_options + N_QC_OPTIONS && strcmp(argv[i], qc->name)) qc++;
		if (qc < qc_options + N_QC_OPTIONS) {
			if (arg_dbl(argc, argv, ++i, &d)) BAD(qc->name);
			*qc_flag(o, qc) = 1;
			*qc_threshold(o, qc) = d;
			continue;
		}
		size_t j = 1;
		char a = argv[i][j];
		while (a == '-' && ++j < strlen(argv[i])) a = argv[i][j];
		const char *w = &argv[i][j];
		switch (a) {
		case 'a': o->em.admixture = 1; break;
		case 'b':
			if (!strncmp(w, "bed", 3)) { if (++i >= argc) BAD("--bed"); o->bed_prefix = argv[i]; }
			else if (!strncmp(w, "bou", 3)) { if (arg_dbl(argc, argv, ++i, &d) || d < 0) BAD("--bound"); o->em.lower_bound = d; }
			else { if (arg_int(argc, argv, ++i, &v) || v < 0) BAD("-b"); o->n_bootstrap = (int)v; }
			break;
		case 'c':
			if (!strncmp(w, "cv-f", 4)) { if (arg_dbl(argc, argv, ++i, &d) || !(d > 0 && d <= 1)) BAD("--cv-floor"); o->cv_floor = d; }
			else if (!strncmp(w, "cv", 2)) { if (arg_int(argc, argv, ++i, &v) || v < 2 || v > MC_CV_MAX_FOLDS) BAD("--cv"); o->cv_folds = (int)v; }
			else o->em.eta_constrained = 1;
			break;
		case 'd':
			if (!strncmp(w, "dev", 3)) { if (arg_int(argc, argv, ++i, &v) || v < 0) BAD("--device"); o->device = (int)v; }
			else { if (++i >= argc) BAD("-d"); o->path = argv[i]; }
			break;
		case 'e': if (arg_dbl(argc, argv, ++i, &d) || d < 0) BAD("-e"); o->em.rel_error = d; break;
		case 'E': if (arg_dbl(argc, argv, ++i, &d) || d < 0) BAD("-E"); o->em.abs_error = d; break;
		case 'f':
			if (!strcmp(argv[i], "--fill")) { o->fill = 1; break; }	/* (in full: -f... is the data file) */
			if (!strcmp(argv[i], "--fst")) { o->fst = 1; break; }	/* (in full as well) */
			if (!strncmp(w, "fo", 2)) { ++i; break; }	/* --format only matters to the data writer */
			if (++i >= argc) BAD("-f");
			o->filename = o->filename_file = argv[i];
			for (size_t x = strlen(o->filename); x-- > 1;)
				if (o->filename[x] == '/') { o->filename_file = &o->filename[x + 1]; break; }
			break;
		case 'g':
			if (!strncmp(w, "gp", 2)) { if (arg_int(argc, argv, ++i, &v) || v < 1 || v > 64) BAD("--gpus"); o->n_gpus = (int)v; }
			else { if (arg_int(argc, argv, ++i, &v) || v < 0) BAD("-g"); o->em.adjust_step = (int)v; }
			break;
		case 'h':
			usage(stdout, argv[0]);
			return 1;
		case 'i':
			if (!strncmp(w, "im", 2)) BAD("--impute is not supported by this build");
			if (arg_int(argc, argv, ++i, &v) || v < 0) BAD("-i");
			o->em.n_init_iter = (int)v;
			break;
		case 'I': BAD("-I / -I1 (alleles as indices) is not supported: the reference's own results differ in that mode");
		case '1': if (arg_int(argc, argv, ++i, &v) || v < 1) BAD("-1"); o->min_K = (int)v; break;
		case '2': if (arg_int(argc, argv, ++i, &v) || v < 1) BAD("-2"); o->max_K = (int)v; break;
		case 'k':
			if (!strcmp(argv[i], "--kinship")) { if (arg_dbl(argc, argv, ++i, &d)) BAD("--kinship"); o->kinship = 1; o->kinship_t = d; break; }	/* (in full as well) */
			if (!strcmp(argv[i], "--king-cutoff")) { if (arg_dbl(argc, argv, ++i, &d)) BAD("--king-cutoff"); o->king = 1; o->king_t = d; break; }	/* (in full: -k... is K) */
			if (arg_int(argc, argv, ++i, &v) || v < 1) BAD("-k");
			o->min_K = o->max_K = (int)v;
			break;
		case 'm':
			if (!strncmp(w, "mi", 2)) { if (arg_int(argc, argv, ++i, &v)) BAD("--missing"); o->missing_value = (int)v; }
			else { if (arg_int(argc, argv, ++i, &v) || v < 0) BAD("-m"); o->n_rand_em_init = o->em.n_rand_em_init = (int)v; }
			break;
		case 'M': o->parallel = 1; o->n_repeat = 1; o->em.verbosity = MC_SILENT; break;
		case 'n': if (arg_int(argc, argv, ++i, &v)) BAD("-n"); o->n_init = (int)v; if (!v) o->n_repeat = 0; break;
		case 'o': if (++i >= argc) BAD("-o"); o->outfile_name = argv[i]; break;
		case 'p':
			if (!strcmp(argv[i], "--pca")) { if (arg_int(argc, argv, ++i, &v)) BAD("--pca"); o->pca = (int)(v < 1 ? -1 : v > 1000000 ? 1000000 : v); break; }	/* (in full, like --prune) */
			if (!strcmp(argv[i], "--pca-iter")) { if (arg_int(argc, argv, ++i, &v) || v < 1 || v > 2147483647L) BAD("--pca-iter"); o->pca_iter = (int)v; break; }
			if (!strcmp(argv[i], "--pca-tol")) { if (arg_dbl(argc, argv, ++i, &d)) BAD("--pca-tol"); o->pca_tol = d; break; }
			if (!strcmp(argv[i], "--prune")) { if (arg_dbl(argc, argv, ++i, &d)) BAD("--prune"); o->prune = 1; o->prune_t = d; break; }	/* (in full: --pr... is --projection) */
			if (!strcmp(argv[i], "--prune-window")) { if (arg_int(argc, argv, ++i, &v)) BAD("--prune-window"); o->prune_window_given = 1; o->prune_window = (int)(v < -1 ? -1 : v > 1000000 ? 1000000 : v); break; }
			if (!strncmp(w, "pr", 2)) o->em.do_projection = 0;
			else if (!strncmp(w, "pl", 2)) ;	/* --plus: data-writer option */
			else { if (arg_int(argc, argv, ++i, &v) || v < 1) BAD("-p"); o->ploidy = (int)v; }
			break;
		case 'P': if (++i >= argc) BAD("-P"); o->pfile = argv[i]; break;
		case 'Q': if (++i >= argc) BAD("-Q"); o->qfile = argv[i]; break;
		case 'q':
			if (strncmp(w, "qu", 2)) {
				fprintf(stderr, "ERROR [" MC_FRONT_END "::parse_options]: unknown option (argument '%s'); try -h\n", argv[i]);
				return MC_EXIT_INVALID_CMD_OPTION;
			}
			if (++i >= argc) BAD("--query");
			o->query_file = argv[i];
			break;
		case 'A': if (++i >= argc) BAD("-A"); o->afile = argv[i]; break;	/* multiclust.c:1416-1418 */
		case 'R': o->R_format = 1; break;
		case 'r':
			if (!strcmp(argv[i], "--resid")) { o->resid = 1; break; }	/* (in full: -r... is the seed) */
			/* extension: --randem selects the Rand-EM initialisation the reference carries but cannot reach
			 * (initialization_procedure stays NOTHING, multiclust.c:935); -m <n> is its number of candidates */
			if (!strncmp(w, "ra", 2)) { o->em.initialization_procedure = MC_RAND_EM; break; }
			if (arg_int(argc, argv, ++i, &v) || v < 0) BAD("-r");
			o->em.seed = (unsigned)v;
			o->seed_given = 1;
			break;
		case 'x': BAD("-x (block relaxation) is not implemented, as in the reference");
		case 's':
			if (!strncmp(w, "si", 2)) BAD("--simulate is not supported by this build");
			if (!strncmp(w, "se-b", 4)) { if (arg_int(argc, argv, ++i, &v) || v < 1 || v > 2147483647L) BAD("--se-block"); o->se_block = (int)v; break; }
			if (!strncmp(w, "se", 2)) { if (arg_int(argc, argv, ++i, &v) || v < 2 || v > MC_SE_MAX_REPLICATES) BAD("--se"); o->se_replicates = (int)v; break; }
			if (!strncmp(w, "st", 2)) { if (arg_int(argc, argv, ++i, &v) || v < 1 || v > 16) BAD("--streams"); o->n_streams = (int)v; break; }
			if (arg_int(argc, argv, ++i, &v) || v < 0 || v > 6) BAD("-s");
			o->em.accel_scheme = (int)v;
			break;
		case 't': if (arg_int(argc, argv, ++i, &v) || v < 0) BAD("-t"); o->em.n_seconds = 60u * (unsigned)v; break;
		case 'T': if (arg_int(argc, argv, ++i, &v) || v < 0) BAD("-T"); o->em.max_iter = (int)v; break;
		case 'u':
			while (++i < argc && argv[i][0] != '-') {
				if (argv[i][0] == 'l') { if (arg_dbl(argc, argv, ++i, &d)) BAD("-u l"); o->target_ll = 1; o->desired_ll = d; }
				else if (argv[i][0] == 'n') { if (arg_int(argc, argv, ++i, &v) || v < 0) BAD("-u n"); o->target_revisit = (int)v; }
				else BAD("-u");
			}
			i--;
			break;
		case 'v':
			if (i + 1 == argc) o->em.verbosity = MC_VERBOSE;
			else if (arg_int(argc, argv, i + 1, &v)) o->em.verbosity = MC_VERBOSE;
			else { o->em.verbosity = (int)v; i++; }
			break;
		case 'w':
			while (++i < argc && argv[i][0] != '-') {
				if (arg_int(argc, argv, i + 1, &v)) BAD("-w");
				if (argv[i][0] == 't') o->repeat_seconds = 60u * (unsigned)v;
				else if (argv[i][0] == 'm') o->max_repeat_seconds = 60u * (unsigned)v;
				else if (argv[i][0] == 'n') { if (v <= 0) BAD("-w n"); o->n_repeat = (int)v; }
				else BAD("-w");
				i++;
			}
			i--;
			o->write_files = 0;
			break;
		default:
			fprintf(stderr, "ERROR [" MC_FRONT_END "::parse_options]: unknown option (argument '%s'); try -h\n", argv[i]);
			return MC_EXIT_INVALID_CMD_OPTION;
		}
	}
	/* extensions: what cross-validation, the bootstrap over loci (either model) and query individuals cannot be combined with is a
	 * usage error like a bad argument */
	const int timed = !o->write_files || o->parallel;
	int rc;
	if (o->cv_folds && (rc = refuse_post_fit(o, "--cv", 1, NULL))) return rc;
	if (o->se_replicates && (rc = refuse_post_fit(o, "--se", 0, NULL))) return rc;
	if (o->query_file && (rc = refuse("--query",
			!o->em.admixture ? "--query needs the admixture model (-a)" :
			o->em.eta_constrained ? "--query cannot be combined with shared mixing proportions (-c)" :
			o->n_bootstrap ? "--query cannot be combined with the bootstrap (-b)" :
			timed ? "--query cannot be combined with -w or -M" :
			o->afile ? "--query cannot be combined with a partition to compare with (-A)" :
			o->cv_folds || o->se_replicates ? "--query cannot be combined with --cv or --se (they share the fold state of the device)" :
			o->em.initialization_procedure == MC_RAND_EM ? "--query cannot be combined with --randem (its centers are drawn from the genotypes on the host)" :
			o->n_gpus > 1 || o->n_streams > 1 ? "--query cannot be combined with --gpus or --streams above 1" : NULL))) return rc;
	if (o->fill && (rc = refuse_post_fit(o, "--fill", 1,
			o->query_file ? "--fill cannot be combined with --query (the query individuals are hidden on the device)" : NULL))) return rc;
	if (o->fst && (rc = refuse_post_fit(o, "--fst", 0, NULL))) return rc;
	if (o->resid && (rc = refuse_post_fit(o, "--resid", 1, NULL))) return rc;
	if (o->kinship && (rc = refuse_post_fit(o, "--kinship", 1,
			!(o->kinship_t > 0 && o->kinship_t < 0.5) ? "the kinship threshold of --kinship must lie in (0, 0.5)" : NULL))) return rc;
	if ((o->prune || o->prune_window_given) && (rc = refuse_as(o->prune ? "--prune" : "--prune-window",
			!o->bed_prefix ? "--prune and --prune-window need a PLINK fileset (--bed)" :
			!o->prune ? "--prune-window needs --prune" :
			!(o->prune_t > 0 && o->prune_t <= 1) ? "the r2 threshold of --prune must lie in (0, 1]" :
			o->prune_window < 1 || o->prune_window > MCHIP_LD_MAX_WINDOW ? "--prune-window must lie in 1 ... 4096 variants" : NULL,
			MC_EXIT_INVALID_USER_SETUP))) return rc;
	if (o->king && (rc = refuse("--king-cutoff",
			!o->bed_prefix ? "--king-cutoff needs a PLINK fileset (--bed)" :
			!(o->king_t > 0 && o->king_t < 0.5) ? "the kinship threshold of --king-cutoff must lie in (0, 0.5)" : NULL))) return rc;
	for (const qc_option *q = qc_options; q < qc_options + N_QC_OPTIONS; q++) {
		const double t = *qc_threshold(o, q);
		char why[64];
		if (!*qc_flag(o, q)) continue;
		snprintf(why, sizeof why, "%s needs a PLINK fileset (--bed)", q->name);
		const int in_range = (t > q->lo || (q->lo_in && t == q->lo)) && (t < q->hi || (q->hi_in && t == q->hi));	/* (NaN is not) */
		if ((rc = refuse(q->name, !o->bed_prefix ? why : !in_range ? q->range : NULL))) return rc;
	}
	if (o->pca && (rc = refuse("--pca", !o->bed_prefix ? "--pca needs a PLINK fileset (--bed)" :
			o->pca < 1 || o->pca > MC_PCA_MAX ? "the number of components of --pca must lie in 1 ... 48" :
			!(o->pca_tol > 0 && o->pca_tol < 1) ? "the tolerance of --pca-tol must lie in (0, 1)" : NULL))) return rc;
	if (o->bed_prefix) {	/* extension: a PLINK fileset is the data file; its name in the output is <prefix>.bed */
		if (o->filename || o->R_format || o->ploidy != 2) {
			fprintf(stderr, "ERROR [" MC_FRONT_END "::parse_options]: --bed reads a diploid PLINK fileset: it cannot be combined with -f, -R or a ploidy (-p) other than 2.\n");
			return MC_EXIT_INVALID_USER_SETUP;
		}
		char *name = malloc(strlen(o->bed_prefix) + 5);		/* (lives as long as the options) */
		if (!name) return MC_EXIT_MEMORY_ALLOCATION;
		strcpy(name, o->bed_prefix);
		strcat(name, ".bed");
		o->filename = o->filename_file = name;
		for (size_t x = strlen(name); x-- > 1;)
			if (name[x] == '/') { o->filename_file = &name[x + 1]; break; }
	}
	if (!o->filename) {
		fprintf(stderr, "ERROR [" MC_FRONT_END "::parse_options]: You must specify the data file with command line option '-f'.  Try '-h' for help.\n");
		return MC_EXIT_INVALID_CMDLINE;
	}
	return 0;
}

/* what parse_options allocated, once it returned 0: the data file's name of a fileset */
void free_options(mc_cli_options *o)
{
	if (o->bed_prefix) free((char *)o->filename);
	o->filename = o->filename_file = NULL;
}

/* what synchronize (multiclust.c:807-893) checks once the data set is known, with the defaults that depend on other options */
int check_setup(mc_cli_options *o, const mc_cli_data *d)
{
	if (d->I < o->max_K) { fprintf(stderr, "ERROR: Maximum number of clusters (%d) (set with command-line argument -k) cannot exceed the number of individuals (%d)\n", o->max_K, d->I); return MC_EXIT_INVALID_USER_SETUP; }
	if (o->n_bootstrap && o->max_K <= 1) { fprintf(stderr, "ERROR: When bootstrapping, maximum K (%d) (set with command-line argument -k) must exceed 1.\n", o->max_K); return MC_EXIT_INVALID_USER_SETUP; }
	if (o->se_replicates && o->se_block > d->L) { fprintf(stderr, "ERROR: The block of --se-block (%d) cannot exceed the number of loci (%d).\n", o->se_block, d->L); return MC_EXIT_INVALID_USER_SETUP; }
	if (o->min_K > o->max_K) { fprintf(stderr, "ERROR: Minimum K (%d) must not exceed maximum K (%d).\n", o->min_K, o->max_K); return MC_EXIT_INVALID_USER_SETUP; }
	if (!o->target_ll && !o->target_revisit && !o->em.n_seconds && !o->n_init) o->n_init = 1;
	if (!o->em.n_rand_em_init) o->em.initialization_procedure = MC_INIT_NOTHING;	/* -m 0 (multiclust.c:1549-1550) */
	return 0;
}
