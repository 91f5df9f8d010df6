/*
 * multiclust_hip.h -- C-ABI of the MI355X-native EM hot path of MULTICLUST.
 *
 * Drop-in boundary.  The reference has no FFI: the seam is the set of C functions
 * its driver/init/writer layers call on the EM layer, all taking (options*, data*, model*)
 * (reference multiclust.h:371-388).  Each entry point below names the reference function(s) it replaces
 * (file:line under the reference checkout).  Conventions:
 *   - extern "C", plain pointers and sizes; no pointer into device memory crosses this boundary;
 *   - every function returns int, 0 = MCHIP_OK (reference: NO_ERROR, message.h:21); nothing here calls
 *     exit() -- the host keeps the reference's exit(0)-on-NaN/decrease semantics (em_alg.c:106-120);
 *   - an opaque context owns one HIP stream and all device buffers for (device, data set, K); contexts
 *     share nothing, so independent initialisations / bootstrap replicates can run one per stream;
 *   - parameters cross the boundary in the reference's own flat order:
 *       P[k][l][m]  -> double[K*T],  T = sum_l uniquealleles[l], index k*T + T_off[l] + m  (vpklm[slot][k][l][m])
 *       Q[i][k]     -> double[I*K]   (vetaik[slot][i][k]);  double[K] when eta is constrained / mixture (vetak[slot])
 *   - slots 0..2 are the reference's triple buffers vpklm[3]/vetaik[3] (multiclust.h:266-271).
 */
#ifndef MULTICLUST_HIP_H
#define MULTICLUST_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCHIP_ABI_VERSION 2	/* 2: mchip_profile_end fills MCHIP_PROF_KINDS = 4 entries (was 3); entry points added since 1 only */
#define MCHIP_MISSING 0xFF	/* genotype byte for a missing allele copy (reference MISSING = -9, multiclust.h:140) */
#define MCHIP_MAX_K 64		/* clusters supported by the K-specialised kernels (cost ~ 2K+6 per cell up to K ~ 20; above
				 * that the 2K-4K doubles a lane holds cost occupancy, above 32 they spill) */
#define MCHIP_MAX_SECANTS 3	/* options::q <= 3 without LAPACK (multiclust.c:847-851) */

enum mchip_status {
	MCHIP_OK = 0,
	MCHIP_ERR_INVALID = 1,		/* bad argument / shape */
	MCHIP_ERR_NO_DEVICE = 2,	/* no HIP device: the product path fails loudly, there is no CPU fallback */
	MCHIP_ERR_HIP = 3,		/* a HIP runtime call failed; see mchip_last_error() */
	MCHIP_ERR_ALLOC = 4,
	MCHIP_ERR_STATE = 5,		/* called out of order (no genotypes / no model yet) */
	MCHIP_ERR_UNSUPPORTED = 6
};

typedef struct mchip_context mchip_context;

int mchip_abi_version(void);
int mchip_device_count(int *count);
/* One context per (device, stream).  Replaces make_model/allocate_model_for_k ownership (multiclust.c:1087,1181). */
int mchip_create(mchip_context **ctx, int device);
int mchip_destroy(mchip_context *ctx);
const char *mchip_last_error(const mchip_context *ctx);
int mchip_synchronize(mchip_context *ctx);

/*
 * Upload one data set.  Replaces dat->IL / dat->L_alleles / dat->ILM as built by read_file.c:443-663:
 * geno[i][l][a] (I*L*ploidy bytes) is the index of allele copy a of individual i at locus l in that
 * locus's ascending allele list (the reference's own index form dat->ila, read_file.c:374-401), or
 * MCHIP_MISSING.  uniquealleles[l] = M_l includes the phantom trailing slot the reference creates for
 * loci with missing data (read_file.c:527-533); indices must be < M_l.  Called again per bootstrap
 * replicate (bootstrap.c:35-41 swaps dat->ILM).
 */
int mchip_set_genotypes(mchip_context *ctx, int I, int L, int ploidy,
			const int32_t *uniquealleles, const uint8_t *geno);
/*
 * Upload one diploid biallelic data set in PLINK 1 packed form and unpack it on the device (an extension: the reference reads
 * STRUCTURE text only).  bed points behind the three header bytes of a variant-major .bed file: L records, record l at
 * bed + l * record_bytes (record_bytes >= ceil(I/4)), sample j of a record in byte j/4, bits 2(j%4) and 2(j%4)+1; the two bits
 * (low bit first) mean 0 = homozygous A1, 1 = missing, 2 = heterozygous, 3 = homozygous A2.  Padding bits of a record's last
 * byte carry no sample, whatever they hold.
 * The data set installed is, by definition, the one the STRUCTURE reader yields on the equivalent STRUCTURE file -- per
 * individual two lines of L alleles: homozygous A1 -> 1 and 1, heterozygous -> 1 and 2, homozygous A2 -> 2 and 2, missing -> -9
 * and -9 -- so with the reader's semantics (read_file.c:443-600): uniquealleles[l] = observed alleles + the phantom slot when
 * the locus has a missing call, 0 when no call of the locus is observed; ascending allele indices (A1 -> 0 when observed,
 * A2 -> 0 or 1); missing copies MCHIP_MISSING.  Exactly what mchip_set_genotypes(ctx, I, L, 2, uniquealleles, geno) installs for
 * that data: mchip_get_genotypes, mchip_data_counts, mchip_empty_individuals, mchip_copy_genotypes and every fit behave the same
 * afterwards, and any model is dropped.  uniquealleles_out receives the L allele counts (may be NULL).  I*L/4 bytes cross to the
 * device instead of 2*I*L; the records are expanded straight into the kernels' two layouts, no [I][L][2] form exists on the way.
 */
int mchip_set_genotypes_bed(mchip_context *ctx, int I, int L, const uint8_t *bed, size_t record_bytes,
			    int32_t *uniquealleles_out);
/*
 * Linkage disequilibrium between neighbouring variants of packed records (an extension): the band of squared correlations that
 * --prune thins a fileset by.  bed, I, L and record_bytes as for mchip_set_genotypes_bed: the whole fileset behind its header.
 * Definition.  At a variant individual j carries code c_j in {0, 1, 2, 3} as above; its dosage is x_j = 0, none, 1, 2 for the codes
 * 0, 1 (missing), 2, 3.  For two variants a < b, over the individuals missing at neither (x at a, y at b; padding bits carry no
 * individual): n their number, Sx = sum x, Sy = sum y, Sxx = sum x^2, Syy = sum y^2, Sxy = sum x y.  In exact signed 64-bit
 * integers C = n Sxy - Sx Sy, Vx = n Sxx - Sx^2, Vy = n Syy - Sy^2, and then
 *     r2 = ((double)C * (double)C) / ((double)Vx * (double)Vy)
 * -- two products and one division, nothing that could be contracted -- or NaN exactly when Vx = 0 or Vy = 0 (a monomorphic
 * variant, an all-missing one, n < 2).  This is the Pearson r^2 of the dosages over pairwise-complete individuals, the quantity
 * PLINK's --indep-pairwise thresholds; it does not depend on which allele is counted.  Every sum is an integer: the result is the
 * same bits on every device, under every launch geometry and every knob of the environment.
 * Contract.  For l in [l0, l0 + n_first) and d in 1 ... window, r2[(l - l0) * window + d - 1] = r2(l, l + d), NaN where l + d >= L.
 * Only the records l0 ... min(L, l0 + n_first + window) - 1 cross to the device.  The context supplies the device, the stream and
 * mchip_last_error and nothing else: no data set need be installed, and nothing of an installed data set, model, slot, fold or
 * saved set changes.  Checked before anything runs: I, L >= 1, record_bytes >= ceil(I/4), 0 <= l0, 0 <= n_first, l0 + n_first <= L,
 * 1 <= window <= MCHIP_LD_MAX_WINDOW, non-null pointers; a failed check returns MCHIP_ERR_INVALID and leaves the array untouched.
 * MCHIP_ERR_ALLOC when the records, the six sums of every pair (24 bytes) and the band do not fit on the device.
 */
#define MCHIP_LD_MAX_WINDOW 4096
int mchip_bed_ld_band(mchip_context *ctx, int I, int L, const uint8_t *bed, size_t record_bytes, int l0, int n_first, int window,
		      double *r2);
/*
 * KING-robust kinship between the individuals of packed records (an extension): the matrix --king-cutoff removes relatives by.
 * bed, I, L and record_bytes as for mchip_set_genotypes_bed: the whole fileset behind its header.
 * Definition.  Codes as above: 0 = homozygous A1, 1 = missing, 2 = heterozygous, 3 = homozygous A2; padding bits carry no
 * individual.  For individuals i and j, over the L variants:
 *     n_ij  = variants typed (not missing) in both,
 *     hh_ij = variants at which both are heterozygous,
 *     op_ij = variants at which one is homozygous A1 and the other homozygous A2 (IBS0),
 *     h_ij  = variants at which i is heterozygous and j is typed (not symmetric: h_ji is the other one).
 * In exact signed 64-bit integers m = min(h_ij, h_ji) and num = 2 hh_ij - 4 op_ij - h_ij - h_ji + 2 m, and then
 *     phi_ij = (double)num / (double)(4 m)
 * -- one division -- or NaN exactly when m = 0.  This is eq. 11 of Manichaikul et al. (2010) brought to one fraction,
 * (hh - 2 op) / (2 m) + 1/2 - (h_ij + h_ji) / (4 m): the estimator of SNPRelate's snpgdsIBDKING(type = "KING-robust").  It needs no
 * allele frequencies and is robust to population structure.  Nothing is claimed about the bits of PLINK 2's --make-king.  The
 * diagonal is no special case: the formula at j = i gives 0.5, or NaN for an individual without a heterozygous call.  Every count
 * is an integer: the result is the same bits on every device, under every launch geometry and every knob of the environment,
 * whichever slab of rows a row is computed in, and phi_ij and phi_ji are the same bits.
 * Contract.  For i in [i0, i0 + n_rows) and every j in [0, I): phi[(i - i0) * I + j] = phi_ij and, when counts is not NULL,
 * counts[((i - i0) * I + j) * 4 + 0..3] = n_ij, hh_ij, op_ij, h_ij.  The context supplies the device, the stream and
 * mchip_last_error and nothing else: no data set need be installed, and nothing of an installed data set, model, slot, fold or
 * saved set changes.  Checked before anything runs: I, L >= 1, record_bytes >= ceil(I/4), 0 <= i0, 0 <= n_rows, i0 + n_rows <= I,
 * non-null bed and phi; a failed check returns MCHIP_ERR_INVALID and leaves the arrays untouched.  MCHIP_ERR_ALLOC when the
 * records, the three bit planes of every individual (3 L / 8 bytes each) and the slab's counts and kinships (28 bytes a pair) do
 * not fit on the device.  MCHIP_ERR_UNSUPPORTED, the arrays untouched as well, for a shape beyond one launch: more than 2^31 - 65
 * individuals, 2^31 or more tiles of 64 x 64 pairs in the slab (ask for fewer rows), or 2^31 or more blocks of 256 individuals x 64
 * variants in the fileset.
 */
int mchip_bed_king(mchip_context *ctx, int I, int L, const uint8_t *bed, size_t record_bytes, int i0, int n_rows, double *phi,
		   uint32_t *counts);
/*
 * Genotype counts along both axes of packed records and the Hardy-Weinberg exact test of every variant (an extension): what
 * --mind, --geno, --maf and --hwe filter a fileset by.  bed, I, L and record_bytes as for mchip_set_genotypes_bed.
 * Definition.  Codes as above: 0 = homozygous A1, 1 = missing, 2 = heterozygous, 3 = homozygous A2; padding bits of a record carry no
 * individual, whatever they hold.
 *     ind_counts[i][c] = the number of the L variants at which individual i has code c, for every i: ind_keep plays no part in it;
 *     var_counts[l][c] = the number of individuals i with ind_keep[i] != 0 (ind_keep = NULL: all of them) that have code c at
 *                        variant l;
 *     hwe_p[l]         = the exact test of Wigginton, Cutler & Abecasis (2005) on (n0, n2, n3) = var_counts[l][0, 2, 3], as the
 *                        following fixed sequence of IEEE double operations.
 * N = n0 + n2 + n3; N = 0 gives p = 1.0.  r = 2 min(n0, n3) + n2, the copies of the rarer allele.  mid = floor(r (2N - r) / (2N)) in
 * 64-bit integers, plus 1 when its parity differs from r's.  A walk visits every heterozygote count h of r's parity in [0, r] with
 * a weight w: start at h = mid with a = (r - mid) / 2, b = N - h - a and w = 1.0; downwards while h >= 2,
 *     w = (w * (double)(h (h - 1))) / (double)(4 (a + 1) (b + 1)),   then h -= 2, a += 1, b += 1;
 * restart at mid with w = 1.0; upwards while h <= r - 2,
 *     w = (w * (double)(4 a b)) / (double)((h + 2) (h + 1)),         then h += 2, a -= 1, b -= 1.
 * Each step is one multiply, then one divide; the integer products are exact in 64 bits (I < 2^30); nothing can be contracted;
 * subnormal weights are part of the definition and are not flushed.  The first walk gives S, the sum of w in visiting order (mid,
 * then down, then up), and w_obs, the w at h = n2.  The second walk makes the same weights again -- the same bits -- and gives T, the
 * sum in the same order of every w with w <= w_obs * 1.0000001 (SNPHWE2's device: weights equal in exact arithmetic are not split by
 * their roundings).  p = T / S, and 1.0 when that is larger.  No array of weights exists.  The counts are integers and the test is a
 * fixed sequence of correctly rounded operations: the same bits on every device and under every launch geometry.
 * Contract.  Any of the three arrays may be NULL, not all; hwe_p needs no var_counts from the caller.  The context supplies the
 * device, the stream and mchip_last_error and nothing else: no data set need be installed, and nothing of an installed data set,
 * model, slot, fold or saved set changes.  Checked before anything runs: I, L >= 1, record_bytes >= ceil(I/4), non-null bed, at least
 * one output array; a failed check returns MCHIP_ERR_INVALID and leaves the arrays untouched.  MCHIP_ERR_UNSUPPORTED, the arrays
 * untouched as well, for I >= 2^30.  MCHIP_ERR_ALLOC when the records, the mask and the outputs (16 bytes an individual, 24 a
 * variant) do not fit on the device.
 */
int mchip_bed_qc(mchip_context *ctx, int I, int L, const uint8_t *bed, size_t record_bytes, const uint8_t *ind_keep,
		 uint32_t *ind_counts, uint32_t *var_counts, double *hwe_p);
/*
 * Principal components of packed records (an extension): what --pca reports.  bed, I, L and record_bytes as for
 * mchip_set_genotypes_bed.
 * Definition.  Codes as above: 0 = homozygous A1, 1 = missing, 2 = heterozygous, 3 = homozygous A2, with the dosages x = 0, none, 1, 2;
 * padding bits carry no individual.  For variant l: n_l = the number of typed individuals and s_l = the sum of their dosages, both
 * integers from population counts.  The variant is USED iff 0 < s_l < 2 n_l: an all-missing and a monomorphic variant are not.  L' is
 * the number of used variants.  For a used variant
 *     mu = (double)s / (double)n,   inv = 1 / sqrt(mu (1 - 0.5 mu)),
 *     z_il = ((double)x_il - mu) inv for a typed individual, 0 for a missing one (mean imputation),
 * and z_il = 0 on an unused variant.  G = Z Z^T / L', an I x I matrix; its trace is (sum_l t_l) / L' with
 * t_l = (n0 mu^2 + n2 (1 - mu)^2 + n3 (2 - mu)^2) inv^2 from the counts, the sum in index order.
 * This is the mean-imputed standardised matrix of flashpca and of PLINK 2's --pca approx.  It is NOT PLINK 1.9's pairwise-complete
 * GRM (--make-rel / --pca), and not smartpca's normalisation.  The four values z takes at a variant involve a square root and a
 * reciprocal: no bit-for-bit claim is made about them.  What is fixed is the order of every sum: W = Z^T X adds over the individuals
 * in an order that depends on (I, padded column count) alone; Y adds over the variants within constant slabs of 4096 variants and
 * then over the slabs in index order; no floating-point atomics.  The same call gives the same bits on every device of a kind, under
 * every launch geometry and every knob of the environment.
 * mchip_bed_pca_apply: Y = Z (Z^T X) / L' for x [I][n_vec] -> y [I][n_vec], 1 <= n_vec <= MCHIP_PCA_MAX_VECTORS; w, when not NULL,
 * receives W = Z^T X [L][n_vec]; scale, when not NULL, [L][2] = mu, inv of every variant (0, 0 for an unused one); *n_used = L';
 * *trace (may be NULL) the trace of G.  The column count is padded to a multiple of 16 with zero columns inside the library; they
 * are never returned.
 * mchip_bed_pca: the first n_pc eigenpairs of G by block subspace iteration with a Rayleigh-Ritz step every iteration (the
 * iteration, its start vectors -- a fixed function of the indices, no seed -- and its stopping rule are stated in
 * multiclust_amd/csrc/mchip_pca_algebra.h): block width b = min(I, n_pc + n_extra rounded up to a multiple of 16, at most 64);
 * eigenvalues [n_pc] descending, eigenvectors [I][n_pc] of unit norm, the component of largest magnitude positive (the lowest index
 * among equals), residuals [n_pc] = || G u - theta u || / theta_1, *n_iter the iterations run.  The records, the per-variant
 * tables, X, W and Y stay on the device from the first launch to the last; the I x b blocks cross once each way an iteration, the
 * small dense algebra runs on the host.  Not converging within max_iter is NO error: MCHIP_OK, and the residuals say which
 * components are still loose.  Component c converges at the rate lambda_{b+1} / lambda_c per iteration: components inside the
 * noise bulk of the spectrum converge slowly and mean nothing.
 * Contract (both).  The context supplies the device, the stream and mchip_last_error and nothing else: no data set need be
 * installed, and nothing of an installed data set, model, slot, fold or saved set changes.  Checked before anything runs: I, L >= 1,
 * record_bytes >= ceil(I/4), non-null pointers (but w, scale and apply's trace), 1 <= n_vec <= 64; 1 <= n_pc <= I, 0 <= n_extra,
 * n_pc + n_extra <= 64, max_iter >= 1, 0 < tol < 1; a failed check returns MCHIP_ERR_INVALID and leaves the outputs untouched.  L' = 0
 * is MCHIP_ERR_INVALID as well ("no polymorphic variant"), the outputs untouched.  MCHIP_ERR_ALLOC when the records, the tables
 * (60 bytes a variant), X and Y, W (8 b bytes a variant) and the slabs' partial sums (ceil(L/4096) x I rounded up to 64 x b doubles)
 * do not fit on the device.  MCHIP_ERR_UNSUPPORTED for a shape beyond one launch: more than 2^31 - 65 individuals or more than 65535
 * slabs of variants.
 */
#define MCHIP_PCA_MAX_VECTORS 64
int mchip_bed_pca_apply(mchip_context *ctx, int I, int L, const uint8_t *bed, size_t record_bytes, int n_vec, const double *x, double *y,
			double *w, double *scale, int *n_used, double *trace);
int mchip_bed_pca(mchip_context *ctx, int I, int L, const uint8_t *bed, size_t record_bytes, int n_pc, int n_extra, int max_iter, double tol,
		  double *eigenvalues, double *eigenvectors, double *residuals, double *trace, int *n_used, int *n_iter);
/* Counted on the device when a data set is installed: cells (i, l, m) with ILM[i][l][m] > 0 -- the cells the reference's E step
 * visits (em_alg.c:338-342) and the unit the flop count of the path is stated in -- and non-missing allele copies. */
int mchip_data_counts(mchip_context *ctx, uint64_t *nonempty_cells, uint64_t *allele_copies);
/* Individuals of the data set held without a single observed allele copy (returns how many; *first = the first one's index or
 * -1).  Under the admixture model with individual mixing proportions the reference gives such a row 0 / 0 = NaN in its first M
 * step (em_alg.c:685-690) and, NaN then sitting in the secants, its step size is NaN and every accelerated cycle falls back to
 * its EM iterate (accel_em.c:58-62): mchip_get_q reports the row as NaN, the host side (mc_step_size) does the falling back. */
int mchip_empty_individuals(const mchip_context *ctx, int *first);
/* the data set currently held, back in the upload form [I][L][ploidy] */
int mchip_get_genotypes(mchip_context *ctx, uint8_t *geno);
/*
 * A parametric-bootstrap data set generated on the device instead of uploaded: parametric_bootstrap_admixture
 * (bootstrap.c:84-124).  Same shape arguments as mchip_set_genotypes; allele copy j (i, l, n order) uses draws 2j and
 * 2j+1 of the rand() stream described by `window` (see mchip_mstep_from_rand_partition): source cluster by the
 * inverse-CDF walk over q[i][.] (or q[.] when eta_constrained), then the allele by the walk over p[k][l][.], with
 * r = rand() / RAND_MAX and the reference's left-to-right partial sums.  q is [I][K] (or [K]), p is [K][T] (the H0
 * MLEs, multiclust.c:562-581).  Consumes 2*I*L*ploidy draws; every copy is simulated, as in the reference's default
 * build.  Like mchip_set_genotypes it drops any model: call mchip_set_model next.  When the context already holds a data set
 * of the same shape and allele lists (the previous replicate), every device buffer is re-used, the observed haplotypes
 * installed by mchip_set_init_genotypes stay in force (the reference's dat->IL stays in place across replicates,
 * bootstrap.c:35-41), and an mchip_set_model with unchanged arguments re-uses the model's buffers too.
 */
int mchip_simulate_genotypes(mchip_context *ctx, int I, int L, int ploidy, const int32_t *uniquealleles,
			     const uint32_t *window, int K, int eta_constrained, const double *q, const double *p);
/*
 * The mixture model's generator: parametric_bootstrap_mixture (bootstrap.c:132-175).  Individual i owns draws
 * i * (1 + L*ploidy) ... (i + 1) * (1 + L*ploidy) - 1 of the stream described by `window`: the first chooses its cluster k by the
 * walk over eta[0..K), draw 1 + l*ploidy + a chooses copy (l, a) by the walk over p[k][l][.].  Consumes I + I*L*ploidy draws;
 * every copy is simulated.  eta is [K], p is [K][T].  In everything else the contract of mchip_simulate_genotypes: drops the
 * model, re-uses the buffers of a same-shaped previous replicate, leaves mchip_set_init_genotypes in force, accepts every shape
 * mchip_set_genotypes accepts and parameters that are negative, do not sum to 1 or are NaN (the same integer thresholds).
 * Loci with at most 4 alleles and ploidy <= 8 are generated tile by tile straight into the device layouts at any K; other
 * shapes (and MCHIP_SIM_NO_TILE) take the general form through the upload order.
 * One limit of its own: K <= 256 (the cluster of an individual is kept as a byte), else MCHIP_ERR_INVALID; a model takes K <= 64.
 */
int mchip_simulate_genotypes_mixture(mchip_context *ctx, int I, int L, int ploidy, const int32_t *uniquealleles,
				     const uint32_t *window, int K, const double *eta /* [K] */, const double *p /* [K][T] */);
/*
 * The data set `src` holds, copied into `ctx` on the device (both contexts on one device).  run_bootstrap fits the null and the
 * alternative model to the SAME simulated data set (multiclust.c:675-708: one parametric_bootstrap(), then estimate_model()
 * over both K): the second model's context takes the first one's instead of generating it again.  Like
 * mchip_simulate_genotypes it keeps the init genotypes in force when the shape is unchanged and drops any model.
 */
int mchip_copy_genotypes(mchip_context *ctx, const mchip_context *src);
/*
 * The genotype the hard-partition M step reads, when it is not the data set itself.  While bootstrapping, the
 * reference's random_allele_partition still reads the observed haplotypes dat->IL (rnd_init.c:471;
 * parametric_bootstrap replaces only dat->ILM, bootstrap.c:35-41), so every fit to a simulated data set starts from
 * the observed alleles.  After this call mchip_mstep_from_partition / _from_rand_partition on this context do the
 * same; geno = NULL (and any new data set) goes back to the data set itself.  Same form as mchip_set_genotypes.
 */
int mchip_set_init_genotypes(mchip_context *ctx, const uint8_t *geno);

/*
 * Allocate parameter ring, secant buffers and workspaces for K.  Replaces allocate_model_for_k
 * (multiclust.c:1181-1265) and free_model_data (1288).  admixture/eta_constrained/do_projection are
 * options::admixture / eta_constrained / do_projection; the lower bounds are options::eta_lower_bound and
 * p_lower_bound after synchronize() (multiclust.c:812-815); n_secants is options::q.
 */
int mchip_set_model(mchip_context *ctx, int K, int admixture, int eta_constrained, int do_projection,
		    double eta_lower_bound, double p_lower_bound, int n_secants);

/* Parameter slots: mod->vpklm[slot], mod->vetaik[slot] / mod->vetak[slot].
 * Rows of individuals without a single observed copy (mchip_empty_individuals): the reference holds 0 / 0 = NaN for them from the
 * first M step on (em_alg.c:685-690); the device holds a finite 1 / K (nothing such a row is multiplied into carries a count) and
 * remembers PER SLOT whether the slot's rows stand for that NaN: set by whatever writes the slot from an M step (mchip_em_step's
 * `to`, mchip_em_run, every slot of mchip_accel_run, mchip_mstep_from_*partition), inherited by mchip_copy_slot,
 * mchip_accel_update and mchip_multisecant_update from the slot they start from, cleared by mchip_init_from_allele_centers
 * (counts start at 1 there: the row is 1 / K in the reference too).  mchip_get_q reports such rows as NaN; mchip_set_q accepts
 * them back -- a NaN row of such an individual is stored as 1 / K and the slot keeps reporting NaN (a get_q / set_q round trip
 * is safe), a finite row is stored and reported as given. */
int mchip_set_p(mchip_context *ctx, int slot, const double *p);
int mchip_get_p(mchip_context *ctx, int slot, double *p);
int mchip_set_q(mchip_context *ctx, int slot, const double *q);
int mchip_get_q(mchip_context *ctx, int slot, double *q);
int mchip_q_length(const mchip_context *ctx, int *n);	/* I*K or K */
int mchip_p_length(const mchip_context *ctx, int *n);	/* K*T */

/*
 * One EM iteration: E step on slot `from`, M step into slot `to` (may be equal: in place, as the
 * unaccelerated reference does).  Replaces e_step_admixture_orig + m_step_admixture_orig
 * (em_alg.c:291-486, 592-754) or e_step_mixture + m_step_mixture (763-1011) as sequenced by em_step
 * (195-207); d_iklm is never materialised.  *loglik = log likelihood of the `from` parameters (what the
 * reference's E step returns).  loglik may be NULL: the step is then only enqueued (no host sync);
 * fetch the value later with mchip_last_loglik().
 */
int mchip_em_step(mchip_context *ctx, int from, int to, double *loglik);
int mchip_last_loglik(mchip_context *ctx, double *loglik);
/*
 * A batch of in-place EM iterations with the stopping rule evaluated on the device: n_steps times
 * { em_step(slot -> slot); stop() } exactly as em() sequences them for the unaccelerated case (em_alg.c:78-88, 101-182),
 * enqueued without a host round trip per iteration; once the rule fires (convergence, iteration cap, NaN, decrease) the
 * remaining steps of the batch are no-ops, so parameters, n_iter and logL are those of the stopping iteration.
 * `state` is in/out: the host seeds it with model::logL / n_iter and reads back where the loop stands.
 * Available for every model (admixture with individual or shared mixing proportions, mixture).
 */
typedef struct mchip_run_state {
	double logL;		/* model::logL: log likelihood of the previous iteration (in), of the last executed one (out) */
	double bad_loglik;	/* the offending value when fatal != 0 */
	double abs_error, rel_error;	/* options::abs_error / rel_error */
	int n_iter;		/* model::n_iter */
	int max_iter;		/* options::max_iter (0 = unlimited) */
	int stopped, converged, iter_stop;
	int fatal;		/* 0, 1 = NaN log likelihood, 2 = log likelihood decrease (em_alg.c:106-120) */
} mchip_run_state;
int mchip_em_run(mchip_context *ctx, int slot, int n_steps, mchip_run_state *state);
/*
 * The same for the accelerated loop: n_cycles times accelerated_em_step (accel_em.c:35-114) as em() sequences it
 * (em_alg.c:84-88) for one secant pair and no back-tracking -- scheme 1, 2, 3 = SQUAREM S1-S3, 4 = QN with q = 1
 * (options::accel_scheme, multiclust.h:125-131) -- enqueued without a host round trip: em_2_steps with both stop() calls,
 * log_likelihood of the second EM iterate, step_size, accelerated_update with its log_likelihood, accept iff ll > emll,
 * all decided on the device.  `slot` holds the starting iterate (model::pindex) and, on return, the iterate the reference
 * would report (its pindex: the accepted extrapolation, else the second EM iterate, else -- when the stopping rule fired
 * inside em_2_steps -- the cycle's starting iterate, accel_em.c:44-45); the other two slots are scratch.  Same arithmetic as
 * driving the cycle call by call (mchip_em_step, mchip_secant, mchip_loglik, mchip_step_dots, mchip_accel_update,
 * mchip_loglik_prefetch).  Every model (admixture with individual or shared mixing proportions, mixture) with
 * n_secants >= 1; MCHIP_ERR_UNSUPPORTED without a secant pair, or for an admixture data set with more than 32 alleles at a
 * locus (the caller then drives the cycles call by call).
 */
int mchip_accel_run(mchip_context *ctx, int slot, int scheme, int n_cycles, mchip_run_state *state);

/* E step only (em_e_step's trailing E step, em_alg.c:226,230): refreshes the expected counts, returns logL. */
int mchip_e_step(mchip_context *ctx, int slot, double *loglik);
/* log_likelihood(): logL_admixture / logL_mixture (log_likelihood.c:96-147, 157-232).  Two departures from logL_mixture,
 * both where the reference gives no usable number: an individual without one ordinary log-sum (all NaN or -inf, or one
 * +inf) makes the result NaN where the reference's rescaling loop never ends; and where the reference's rescaled sum
 * overflows (exp(max) == 0, the halved maximum within ln S of log DBL_MAX, clusters of total weight S >= 1.32 relative to
 * the best) and its result is +inf, the individual's term is log sum_k exp(v_k - max) + max, e_step_mixture's form.
 * Every result that is finite in the reference's arithmetic keeps its bits. */
int mchip_loglik(mchip_context *ctx, int slot, double *loglik);
/* The same value, computed by the pass that also accumulates the E step's per-individual sums and keeps them: an
 * mchip_em_step from this slot that follows (no parameter write in between) skips that pass.  accelerated_update's
 * log_likelihood(tindex) (accel_em.c:544) is followed, whenever the extrapolated point is accepted, by exactly such
 * an E step at the head of the next cycle (em_alg.c:1089-1098). */
int mchip_loglik_prefetch(mchip_context *ctx, int slot, double *loglik);

/*
 * First M step from a hard allele partition: random_initialize_admixture (rnd_init.c:349-357) =
 * random_allele_partition (456-482) + m_step_admixture.  assign[i][l][a] in [0,K) is the cluster drawn for
 * allele copy a (the host draws it with the libc-compatible stream); d_iklm = 1 (not += 1) per matching copy.
 */
int mchip_mstep_from_partition(mchip_context *ctx, const uint8_t *assign, int to);
/*
 * The same with the partition drawn on the device: assign[j] = rand() % K for j = 0 .. I*L*ploidy-1 in the
 * reference's i, l, a order (rnd_init.c:456-467), where rand() is glibc's TYPE_3 generator
 * x_j = x_{j-31} + x_{j-3} (mod 2^32), rand() = x_j >> 1, and window[t] = x_{j0-31+t}, t = 0..30, are the 31 words
 * behind the first draw (oldest first; the host's generator state after srand() and any draws made so far).  The
 * caller advances its own copy of the stream by I*L*ploidy draws.  Bit-identical to drawing on the host and
 * calling mchip_mstep_from_partition; removes I*L*ploidy host rand() calls and the upload per initialisation.
 */
int mchip_mstep_from_rand_partition(mchip_context *ctx, const uint32_t *window, int to);

/*
 * One Rand-EM candidate: random_allele_center's partition + initialize_parameters_admixture (rnd_init.c:496-705) into slot
 * `to`.  The host walks the loci in order and draws each locus's center alleles from the rand() stream exactly as the
 * reference does (K draws plus uniqueness retries when the locus has at least K alleles, none otherwise), which also tells it
 * how many copies of the locus match no center and therefore where each locus's rand() % K draws lie in the stream:
 *   centers[l*K + k]  allele index of cluster k's center at locus l, 0xFF = none (the reference's -1);
 *   draw_offset[l]    position, counted from `window`, of the first draw that a non-matching copy of locus l consumes
 *                     (copies take them in i, a order; missing copies match no center);
 *   window, n_draws   the 31 words behind the candidate's first draw (as mchip_mstep_from_rand_partition) and the length
 *                     of the candidate's span of the stream.
 * The device assigns every copy (identity with a center, else its draw), counts -- eta_ik = (1 + copies of i in k) /
 * (ploidy L + K), missing copies included; p_klm = (1 + copies of allele m in k) / sum_m -- and normalises; nothing is
 * projected.  Reads the observed haplotypes when mchip_set_init_genotypes is in force (the reference reads dat->IL).
 */
int mchip_init_from_allele_centers(mchip_context *ctx, const uint8_t *centers, const uint64_t *draw_offset, const uint32_t *window,
				   uint64_t n_draws, int to);
/*
 * The mixture model's initialisation from K center individuals the host drew: random_individual_center +
 * initialize_parameters_mixture (rnd_init.c:192-339) into slot `to`.
 * centers[K]: distinct individuals in [0, I) (else MCHIP_ERR_INVALID).  A center k joins cluster k; every other individual joins
 * the first center of minimal L1 distance between the allele-count vectors (observed copies only); K = 1: cluster 0.  Then
 * eta[k] = (1 + n_k) / (I + K) and, per (k, l), p = e / sum_m e with e = 1 + (K - k) * (copies of allele m in cluster k) -- the
 * reference's quirk included.  Distances and counts are integers and the divisions are IEEE divisions of the operands the host
 * form divides: the parameters have the host form's bits.  Works on the data set the context holds (the simulated one while
 * bootstrapping: the mixture initialisation reads dat->ILM, not the observed haplotypes -- init genotypes are NOT used here).
 * assign_out: NULL, or I int32 receiving the assignment.  Needs a mixture model (admixture = 0), else MCHIP_ERR_STATE.
 */
int mchip_init_from_individual_centers(mchip_context *ctx, const int32_t *centers, int to, int32_t *assign_out);
/* parameters of slot `from` copied to slot `to`: Rand-EM keeps its best candidate (rnd_init.c:431-436 keeps the partition) */
int mchip_copy_slot(mchip_context *ctx, int to, int from);

/*
 * What the writers read from diklm / vik (write_file.c:359-381,446-459,531-542,593-598):
 * admixture: sik[i][k] = sum_{l,m} d_iklm of the last E step executed; mixture: vik[i][k].
 */
int mchip_get_expected_counts(mchip_context *ctx, double *sik);

/* ---- K-fold cross-validation of the admixture model (an extension: the reference offers AIC / BIC and the bootstrap only) ----
 * Fit with a share of the genotypes hidden, score how well the fit predicts them: every genotype (i, l) -- all `ploidy` copies of
 * it together -- belongs to one of n_folds folds, one byte per genotype kept on the device beside the data set.  The folds, the
 * saved full data set and the hold-out in force are state of the data set: every call that installs a new one
 * (mchip_set_genotypes, _bed, mchip_simulate_genotypes, _mixture, mchip_copy_genotypes) drops them.  Fold draw and hold-out work
 * with any model (or none); the score is the admixture model's. */
/*
 * fold[i*L + l] = rand() % n_folds, genotypes in i, l order, rand() the glibc stream described by `window` exactly as for
 * mchip_mstep_from_rand_partition (the same generator kernel with K := n_folds over I*L draws).  Consumes I*L draws: the caller
 * advances its own copy of the stream.  n_folds in [2, 64], else MCHIP_ERR_INVALID; MCHIP_ERR_STATE without a data set.  A
 * hold-out in force stays in force (it was built from the previous folds) until the next mchip_cv_hold_out.
 */
int mchip_cv_draw_folds(mchip_context *ctx, const uint32_t *window, int n_folds);
/* The same with folds the caller chose: folds[i*L + l] < n_folds, else MCHIP_ERR_INVALID (and the folds held stay as they were). */
int mchip_cv_set_folds(mchip_context *ctx, const uint8_t *folds /* [I][L], each < n_folds */, int n_folds);
/* the folds held, [I][L]; MCHIP_ERR_STATE without folds */
int mchip_cv_get_folds(mchip_context *ctx, uint8_t *folds /* [I][L] */);
/*
 * Install the data set with every copy of every genotype of fold `fold` turned into MCHIP_MISSING; fold = -1 installs the full
 * data set again, bit-identical (mchip_get_genotypes, mchip_data_counts, mchip_empty_individuals, every fit) to the one held
 * before the first hold-out.  The first call saves the full data set once, in upload form, on the device; each call masks it
 * into the stream buffer and takes the route of an uploaded genotype from there (layouts, packed counts, individuals left
 * without an observed copy).  Unlike mchip_set_genotypes it
 *   keeps   uniquealleles and T as they are -- a locus that gains missing copies only through the mask gets no phantom slot;
 *           the kernels accept a missing copy at such a locus;
 *           the model and every parameter slot, secants included, so a fit can start from the full-data estimate;
 *           the genotype and count buffers (written in place), the folds and the saved full data set;
 *   drops   what is derived from the data: the S-side sums held for a slot (mchip_loglik_prefetch), the counts of
 *           mchip_data_counts, and the per-slot "stands for NaN" marks of mchip_get_q, which are cleared as
 *           mchip_copy_genotypes clears them -- a slot written by an M step on the masked data is marked again.
 * MCHIP_ERR_STATE without a data set or without folds; MCHIP_ERR_INVALID for a fold outside [-1, n_folds).
 */
int mchip_cv_hold_out(mchip_context *ctx, int fold /* -1: the full data set again */);
/*
 * The held-out score of the parameters in `slot`: over every copy (i, l, a) of the saved full data set that is observed and whose
 * genotype lies in the fold held out, t = sum_k q_ik p_klm (m the copy's allele; q_k when eta is constrained), t' = max(t, floor):
 *   *sum_log = sum log t',  *n_copies = how many such copies,  *n_floored = how many of them had t < floor or t NaN.
 * Reads Q as the device stores it: an individual whose observed copies all fall into the fold holds the finite 1 / K there (see
 * the parameter slots above).  Partial sums are combined in a fixed order, no floating-point atomics: two calls on the same state
 * return the same bits.  Any of the three pointers may be NULL.
 * MCHIP_ERR_STATE without a data set, folds, a hold-out in force (fold >= 0) or a model; MCHIP_ERR_INVALID for a slot out of
 * range or floor outside (0, 1]; MCHIP_ERR_UNSUPPORTED for the mixture model (admixture = 0), where a held-out copy's prediction
 * needs the posterior of its individual's retained copies.
 */
int mchip_cv_heldout_loglik(mchip_context *ctx, int slot, double floor,
			    double *sum_log, uint64_t *n_copies, uint64_t *n_floored);

/* ---- mixing proportions of query individuals against fixed allele frequencies (an extension: the reference fits Q and P together
 * and has nothing for individuals kept out of the panel) ----
 * For every listed individual i = rows[r] (distinct, each in [0, I)) the admixture model's q_i. is fitted with P of `slot` held
 * fixed, each row to its own convergence:
 *   q(0)     1 / K, or row i of `slot` as the device stores it when from_slot != 0;
 *   n = 0, 1, ...   one pass over the individual's observed copies (i, l, a), m the copy's allele:
 *                   t = sum_k q_k p_klm,   l_n = sum log t,   S_k = q_k sum p_klm / t   (one term per copy);
 *            if n >= 1 and a test is made and every test made holds, stop converged -- the tests are mc_converged's
 *                   (em_alg.c:163-182): abs_error != 0: |l_n - l_(n-1)| <= abs_error; rel_error != 0: |l_n - l_(n-1)| / |l_(n-1)| <=
 *                   rel_error; a zero error is a test not made.  Where that rule is degenerate this one is not: the difference is
 *                   taken whichever test is made (there a relative test without an absolute one divides a zero), and with both
 *                   errors zero no row converges, the loop runs to max_iter (there such a fit stops at its first check);
 *            if n == max_iter, stop not converged;
 *            else q(n+1) = S / sum_k S_k, then the simplex projection with the model's lower bound when the model has
 *                   do_projection: the arithmetic of an EM step's Q side.
 *   on stopping:    q_rows[r][.] = q(n), loglik_rows[r] = l_n, iter_rows[r] = n, converged_rows[r] = 1 or 0.
 * An individual without an observed copy reports 1 / K, 0, n = 0, not converged.  A row whose l_n is not finite stops there and
 * reports NaN proportions, that l_n, n, not converged (a copy whose allele has frequency 0 in every cluster the row has weight in).
 * Reads the full data set: the saved one while a cross-validation hold-out is in force (as mchip_cv_heldout_loglik does), so
 * individuals hidden from the fit of P by a hold-out are fitted on their genotypes; otherwise the installed one.
 * Writes the four host arrays and nothing else: no parameter slot, secant, expected count, held S-side sum, data-set or hold-out
 * state changes.  Sums are combined in an order fixed by the shape, no floating-point atomics: two calls on the same state return
 * the same bits.  One workgroup per row, iterating inside one launch (mchip_query.hip).
 * MCHIP_ERR_STATE without a data set or model; MCHIP_ERR_UNSUPPORTED for the mixture model and for shared mixing proportions;
 * MCHIP_ERR_INVALID for a slot out of range, a null pointer, n_rows < 1, a row out of range or repeated, max_iter < 1 or an error
 * that is negative or NaN -- all checked before anything runs, the arrays stay untouched.
 */
int mchip_fit_q_rows(mchip_context *ctx, int slot, const int32_t *rows, int n_rows, int from_slot,
		     int max_iter, double abs_error, double rel_error,
		     double *q_rows /* [n_rows][K] */, double *loglik_rows, int32_t *iter_rows, uint8_t *converged_rows);

/* ---- missing allele copies filled from the fitted admixture model (an extension: the reference's --impute puts one allele per
 * locus into every missing copy before any fit) ----
 * For every genotype (i, l) of the INSTALLED data set with r >= 1 missing copies (under a cross-validation hold-out the hidden
 * copies are missing copies like any other), with the parameters of `slot`:
 *   candidates    the first n_real[l] allele slots of the locus (the reader's L_alleles[l]: uniquealleles[l] without the phantom
 *                 trailing slot);
 *   t_m           = sum_k q_ik p_klm, an fma chain in k order (q_k when the mixing proportions are shared); x_m = t_m / sum_cand t.
 *                 Q is read as the device stores it: an individual without an observed copy holds 1 / K (the slot section above);
 *   the r copies  together take the mode of the multinomial(r; x), found greedily: copy j = 1 .. r goes to argmax_m t_m / (c_m + 1),
 *                 c_m the earlier copies of this genotype given to m, ties to the lowest m.  r = 1: argmax t; a fully missing
 *                 diploid genotype becomes heterozygous when the larger x is below 2 / 3.  Observed copies of the genotype play no
 *                 part (copies are independent given q);
 *   written       the multiset, ascending by allele index, into the missing positions in copy order;
 *   confidence    c = r! / prod_m c_m! prod_m x_m^c_m, the probability of the filled multiset;
 *   left missing  all r copies when n_real[l] = 0 or no candidate has t > 0 (NaN is not > 0): they stay MCHIP_MISSING.
 * geno_out [I][L][ploidy] = mchip_get_genotypes byte for byte outside the filled copies.  conf_out: NULL, or [I][L] receiving c where
 * a genotype was filled and 0 elsewhere.  *n_filled / *n_left count copies, *n_genotypes the genotypes filled, *sum_conf is the sum
 * of their c; any of the four may be NULL.  The sum is combined in an order fixed by the shape, no floating-point atomics: two
 * calls on the same state return the same bits.
 * Writes its host arrays and nothing else: no parameter slot, secant, expected count, held S-side sum, data set, fold or saved set
 * changes.  The filled genotype is the most probable one given Q and P, not a draw: filled data understate the variance of
 * heterozygosity.
 * MCHIP_ERR_STATE without a data set or model; MCHIP_ERR_UNSUPPORTED for the mixture model (admixture = 0); MCHIP_ERR_INVALID for a
 * slot out of range, a null n_real or geno_out, or an n_real[l] outside [0, uniquealleles[l]] -- all checked before anything runs,
 * the arrays stay untouched.
 */
int mchip_impute_missing(mchip_context *ctx, int slot, const int32_t *n_real /* [L] */,
			 uint8_t *geno_out /* [I][L][ploidy] */, double *conf_out /* [I][L] or NULL */,
			 uint64_t *n_filled, uint64_t *n_left, uint64_t *n_genotypes, double *sum_conf);

/* ---- divergence of the fitted clusters (an extension: the tables STRUCTURE and ADMIXTURE end a fit with) ----
 * P is the table of `slot`: p_klm for cluster k, locus l and column m over ALL uniquealleles[l] columns of the locus, the phantom
 * slot included, whatever the M step left there; T columns in all.  L1 = the loci with at least one column; a locus with
 * uniquealleles[l] = 0 contributes nothing and is not counted.  Every quantity is a sum of non-negative terms: none is formed by
 * subtracting Gram-matrix entries, so two nearly equal clusters get their distance to full relative precision.
 * Per cluster and pair, over the T columns:
 *   het[a]          h_a = sum_c p_a (1 - p_a); the expected heterozygosity is H_a = h_a / L1;
 *   sqdiff[a*K+b]   s_ab = sum_c (p_a - p_b)^2, symmetric, 0 on the diagonal; the net distance (STRUCTURE's table) is
 *                   D_ab = s_ab / (2 L1), and Hudson's F_ST as a ratio of sums F_ab = D_ab / (D_ab + (H_a + H_b) / 2), NaN when the
 *                   denominator is 0.
 * Among the K clusters with weights[k] >= 0 (they are used as given: the caller makes them sum to 1), per locus:
 *   pbar_lm         = sum_k w_k p_klm as an fma chain in k order from 0 -- this double IS pbar in what follows;
 *   locus_ht[l]     HT_l = sum_m pbar_lm (1 - pbar_lm);
 *   locus_v[l]      V_l = sum_m sum_k w_k (p_klm - pbar_lm)^2, which is H_T - H_S in its non-negative form; both are 0 for a locus
 *                   without a column.  F_l = V_l / HT_l, NaN when HT_l = 0 or the locus has no column;
 *   *sum_v, *sum_ht sum_l V_l and sum_l HT_l: overall F = sum_v / sum_ht;   *n_loci = L1.
 * locus_v and locus_ht may be NULL; the other pointers are required.  Both models (the mixture model's P as well).  Every sum is
 * combined in an order fixed by T, L and K alone, without floating-point atomics: the same state gives the same bits on any device
 * and under any geometry knob of the environment.
 * Writes its host arrays and nothing else: no parameter slot, secant, expected count, held S-side sum, data set, fold or saved set
 * changes.
 * MCHIP_ERR_STATE without a data set or model; MCHIP_ERR_INVALID for a slot out of range, a null required pointer, a weight that is
 * negative, infinite or NaN, or weights that are all zero -- all checked before anything runs, the arrays stay untouched.
 */
int mchip_divergence(mchip_context *ctx, int slot, const double *weights /* [K] */, double *het /* [K] */,
		     double *sqdiff /* [K][K] */, double *locus_v /* [L] or NULL */, double *locus_ht /* [L] or NULL */,
		     double *sum_v, double *sum_ht, int32_t *n_loci);

/* ---- products of the fit's residuals between individuals (an extension: evalAdmix's check of an admixture fit, Garcia-Erill and
 * Albrechtsen 2020, for multi-allelic data of any ploidy) ----
 * The admixture model with individual or shared mixing proportions, the parameters of `slot`, the INSTALLED data set (under a
 * cross-validation hold-out the hidden copies are missing copies like any other).  For individual i, locus l and column c = (l, m)
 * over ALL uniquealleles[l] columns of the locus, the phantom slot included (T columns in all):
 *   a_il    the observed (not MCHIP_MISSING) copies of the genotype;   n_ic   how many of them carry allele m;
 *   t_ic    = sum_k q_ik p_kc, an fma chain in k order from 0 (q_k when the mixing proportions are shared).  Q is read as the
 *           device stores it: an individual without an observed copy holds 1 / K (the slot section above);
 *   r_ic    = fma(-a_il, t_ic, n_ic): the observed count minus the count the fit predicts -- this double IS the residual.  It is 0
 *           where a_il = 0;
 *   s_il    = sum_m r_ilm^2, by fma in m order from 0;   o_il = 1 if a_il > 0, else 0.
 * Returned are the sums; the caller forms cor_ij = G_ij / sqrt(D_ij D_ji):
 *   gram[i*I+j]    G_ij = sum_c r_ic r_jc over the T columns; symmetric bit for bit (the entries on and above the diagonal are
 *                  computed, the others are copies);
 *   norms[i*I+j]   D_ij = sum_l s_il o_jl: the squared norm of i's residuals over the loci at which j has data -- the
 *                  pairwise-complete denominators; NOT symmetric.  Where the data set has no missing copy D_ij is G_ii, bit for
 *                  bit.  norms = NULL: not computed.
 * An element's terms are added in the order of the columns (of the loci), four to an instruction of the FP64 matrix unit, the order
 * inside an instruction being the hardware's: at most two roundings per term.  The chunks the work is cut into depend on
 * uniquealleles alone; no floating-point atomics; no order of addition depends on the number of compute units: the same state gives
 * the same bits on any device and under every geometry knob of the environment.
 * Cost: I^2 T + 2 I^2 L multiply-adds and two I x I arrays of doubles on the device (one without norms) -- quadratic in I.
 * Writes its host arrays and nothing else: no parameter slot, secant, expected count, held S-side sum, data set, fold or saved set
 * changes.
 * MCHIP_ERR_STATE without a data set or model; MCHIP_ERR_UNSUPPORTED for the mixture model (admixture = 0); MCHIP_ERR_INVALID for a
 * slot out of range or a null gram -- all checked before anything runs, the arrays stay untouched; MCHIP_ERR_ALLOC when the I x I
 * sums or the chunk buffers do not fit on the device.
 */
int mchip_residual_products(mchip_context *ctx, int slot, double *gram /* [I][I] */, double *norms /* [I][I] or NULL */);

/* ---- kinship between individuals under the fitted admixture model (an extension: REAP's estimator, Thornton et al. 2012,
 * "Estimating kinship in recently admixed populations"; PC-Relate has the same form) ----
 * The admixture model with individual or shared mixing proportions, the parameters of `slot`, the INSTALLED data set (under a
 * cross-validation hold-out the hidden copies are missing copies like any other), ALL uniquealleles[l] columns of every locus, the
 * phantom slot included.  a_il, n_ic, t_ic and r_ic are those of mchip_residual_products above, double for double: t_ic the fma
 * chain in k order, r_ic = fma(-a_il, t_ic, n_ic), 0 where a_il = 0.  New here:
 *   v_ic    = t_ic * fmax(1 - t_ic, 0): the variance of one copy's indicator; a chain that rounds to 1 + ulp gives 0, never a NaN;
 *   w_ic    = a_il * sqrt(v_ic); 0 where a_il = 0.
 * Returned are the sums; the caller forms phi_ij = G_ij / V_ij, NaN where V_ij = 0 (an individual without an observed copy, a query
 * individual, a pair without a shared locus):
 *   gram[i*I+j]    G_ij = sum_c r_ic r_jc: the bits of mchip_residual_products' gram on the same state (the same chunks, kernel
 *                  and order of addition);
 *   scale[i*I+j]   V_ij = sum_c w_ic w_jc; symmetric bit for bit (the entries on and above the diagonal are computed, the others
 *                  are copies).
 * Both sums are pairwise-complete by construction: r and w are 0 where the individual has no observed copy at the locus.
 * Why the ratio is a kinship coefficient.  Given the individual-specific frequencies t_i. = sum_k q_ik p_k., the copies of i and j at
 * a column are indicators with means t_ic, t_jc, and a copy of i is identical by descent to a copy of j with probability phi_ij; to
 * first order Cov(n_ic, n_jc) = a_il a_jl phi_ij sqrt(t_ic (1 - t_ic) t_jc (1 - t_jc)), so E[r_ic r_jc] = phi_ij w_ic w_jc, and the
 * ratio of the sums is the moment estimator.  Diploid biallelic data without a missing copy: x = n_i1 is the dosage, mu = t_i1, a = 2,
 * the two columns of a locus carry the same products ((n_i0 - 2 t_i0) = -(x_i - 2 mu_i), t_i0 (1 - t_i0) = mu_i (1 - mu_i)), the
 * factor 2 cancels and phi_ij = sum (x_i - 2 mu_i)(x_j - 2 mu_j) / (4 sum sqrt(mu_i (1 - mu_i) mu_j (1 - mu_j))) over the SNPs typed in
 * both: REAP's formula.  For other ploidies, partially missing genotypes and multi-allelic loci it is the same moment estimator, a
 * generalisation of this project's own.  phi_ii is the self-kinship; for ploidy 2 the inbreeding coefficient is 2 phi_ii - 1.
 * Precision.  No bit-for-bit claim is made about w, which goes through a square root; the claim is the bound on V that
 * tests/kin_util.py derives: (T + 8) u on the sum of the terms plus the terms' own error from t's chain and the root.
 * An element's terms are added in the order of the columns, four to an instruction of the FP64 matrix unit, the order inside an
 * instruction being the hardware's: at most two roundings per term.  The chunks depend on uniquealleles alone; no floating-point
 * atomics; the same state gives the same bits on any device and under every geometry knob of the environment
 * (MCHIP_KIN_TWO_LAUNCHES, the two products of a chunk as two launches instead of one, included).
 * Cost: 2 I^2 T multiply-adds, the half below the diagonal skipped, and two I x I arrays of doubles on the device.
 * Writes its two host arrays and nothing else: no parameter slot, secant, expected count, held S-side sum, data set, fold or saved
 * set changes.
 * MCHIP_ERR_STATE without a data set or model; MCHIP_ERR_UNSUPPORTED for the mixture model (admixture = 0); MCHIP_ERR_INVALID for a
 * slot out of range or a null gram or scale -- all checked before anything runs, the arrays stay untouched; MCHIP_ERR_ALLOC when
 * the I x I sums or the chunk buffers do not fit on the device.
 */
int mchip_kinship_products(mchip_context *ctx, int slot, double *gram /* [I][I] */, double *scale /* [I][I] */);

/* ---- a selection of loci with repeats: the data sets of the non-parametric bootstrap over loci (an extension) ----
 * Let the base be the data set the context held when the first resample was asked for (I, L_base, ploidy, uniquealleles,
 * genotypes).  After the call the context holds exactly what
 *     mchip_set_genotypes(ctx, I, L2, ploidy, ua_base[src[.]], geno_base[:, src[.], :])
 * would install, bit for bit: mchip_get_genotypes, mchip_data_counts, mchip_empty_individuals, mchip_copy_genotypes and every fit of
 * every model.  The allele lists are the base's, gathered and not recounted: a locus keeps its phantom slot even when no missing
 * copy of it survives, a locus without one gets none.  Like every call that installs a data set it drops the model, the init
 * genotypes and the cross-validation state (folds, saved full data set).
 * The first call saves the base once, in upload form, on the device (read back from the kernels' layout, so a base installed by
 * mchip_set_genotypes_bed or generated on the device serves as well), with its allele lists and its individuals without an observed
 * copy; every later call gathers from the saved base, never from the replicate installed before it.  src = NULL (L2 is ignored)
 * installs the base again, bit-identical to the data set held before the first resample, and keeps it saved.  Any other call
 * that installs a data set (mchip_set_genotypes, _bed, mchip_simulate_genotypes, _mixture, mchip_copy_genotypes) drops the saved
 * base; mchip_cv_hold_out keeps it.
 * MCHIP_ERR_STATE without a data set, with a cross-validation hold-out in force (fold >= 0), or for src = NULL without a saved
 * base; MCHIP_ERR_INVALID for L2 < 1, for an index outside [0, L_base) or for a selection with more than 2 000 000 000 allele
 * columns -- all checked before anything is touched: the data set, the model and the saved base stay as they were.
 */
int mchip_resample_loci(mchip_context *ctx, const int32_t *src /* [L2], each in [0, L_base); NULL: the base again */, int L2);

/* ---- acceleration (accel_em.c, em_alg.c:1072-1211) ---- */
/* u (which=0) or v (which=1) secant j := x[to] - x[from], for p and eta (em_alg.c:1104-1161). */
int mchip_secant(mchip_context *ctx, int which, int j, int to, int from);
/* The secant buffers as model state: mod->u_pklm[j] / v_pklm[j] (which = 0 / 1) with u_etaik[j] / v_etaik[j] (or u_etak / v_etak),
 * multiclust.h:284-293, allocated by allocate_model_for_k (multiclust.c:1231-1258); p_part in the flat order of a P slot
 * (double[K*T]), q_part in that of a Q slot.  Together with the parameter slots and model::delta_index they are the whole state
 * of a quasi-Newton run with q > 1 between two cycles (em_alg.c:1171 rotates the slot the next pair goes to). */
int mchip_set_secant(mchip_context *ctx, int which, int j, const double *p_part, const double *q_part);
int mchip_get_secant(mchip_context *ctx, int which, int j, double *p_part, double *q_part);
/* utu, utvu, vutvu of secant pair j, eta terms then p terms (accel_em.c:143-184). out[3]. */
int mchip_step_dots(mchip_context *ctx, int j, double *out3);
/* u_{j1}.u_{j2} and u_{j1}.v_{j2} (quasi-Newton secant matrix, accel_em.c:291-310). out[2]. */
int mchip_secant_dots(mchip_context *ctx, int j1, int j2, double *out2);
/*
 * accelerated_update (accel_em.c:444-541): x[to] = x[base] - 2 s u_j + s^2 (v_j - u_j)  (qn_form = 0, SQUAREM)
 *                                       or x[base] + u_j + s v_j                         (qn_form = 1, QN q=1),
 * then simplex projection of every (k,l) block and every individual when do_projection.
 */
int mchip_accel_update(mchip_context *ctx, int to, int base, int j, double s, int qn_form);
/*
 * qn_accelerated_update (accel_em.c:364-415): x[to] = x[base] + u_{u_index}; then for t = 0..n_terms-1, in
 * order, x[to] += v_{v_index[t]} * coef_a[t] * coef_b[t]  (Ainv[j*q+n] and cutu[n]); then projection.
 */
int mchip_multisecant_update(mchip_context *ctx, int to, int base, int u_index, int n_terms,
			     const int *v_index, const double *coef_a, const double *coef_b);

/* ---- the path's one exchange step, for ONE process driving several GPUs ----
 * Independent fits (random initialisations multiclust.c:516-653, bootstrap replicates 681-701) run one per context on
 * different devices with no data-path collective; afterwards a single RCCL all-reduce over xGMI makes every device's
 * copy of the per-unit result table complete (rows are disjoint: op 0 = sum) or picks the best log likelihood
 * (op 1 = max).  host_bufs[d] is device d's table (count doubles), reduced in place.  RCCL is loaded lazily; without
 * it mchip_comm_create returns MCHIP_ERR_UNSUPPORTED.  (One process per GPU, as bench.py runs, exchanges through
 * torch.distributed instead.) */
typedef struct mchip_comm mchip_comm;
int mchip_comm_create(mchip_comm **comm, int n_devices, const int *devices);
int mchip_comm_all_reduce(mchip_comm *comm, double *const *host_bufs, int count, int op);
int mchip_comm_destroy(mchip_comm *comm);
const char *mchip_comm_last_error(const mchip_comm *comm);
/* what the communicator is and has done: devices it spans, the version of the RCCL it loaded (ncclGetVersion's code, 0 when the
 * library does not say) and the all-reduces completed on it -- the evidence a caller (or a test) has that the exchange went
 * through RCCL.  Any of the three pointers may be NULL. */
int mchip_comm_info(const mchip_comm *comm, int *n_devices, int *rccl_version, unsigned long long *n_reductions);

/* ---- measurement hooks (bench.py): HIP events on the context's own stream ---- */
int mchip_profile_begin(mchip_context *ctx);
/* total_ms: begin..end on the stream.  kernel_ms[MCHIP_PROF_KINDS] / launches[MCHIP_PROF_KINDS]: summed
 * durations and launch counts of the streaming passes over the genotype matrix, each launch bracketed
 * by its own event pair: [0] column pass of an EM step (N-side sums + logL), [1] individual pass
 * (S-side sums), [2] stand-alone log-likelihood pass, [3] dual individual pass of a batched accelerated cycle (the S-side
 * sums of the extrapolated point and the log likelihood of the second EM iterate in one pass; then [2] has no launches).
 * Launches that returned at once (batched runs: after the stopping
 * rule fired, or the S-side pass whose sums were already in place) took under 5 % of the kind's longest launch and are
 * left out of both figures.
 * Where an E step runs its column pass and its individual pass as ONE launch (the paired E step: diploid data on packed
 * counts, K <= 12; MCHIP_NO_PAIR=1 turns it off) no event pair can bracket either pass.  [0] and [1] then take, per launch,
 * the span from the first start to the last end of that pass's workgroups, read from the device's constant-rate clock, and
 * still count one launch each.  The two spans of a launch OVERLAP -- both run for nearly the whole launch -- so [0] + [1]
 * exceeds the time the E steps took; total_ms is unaffected.  A pass whose workgroups all returned at once (cached sums,
 * stopped run) has no span and is left out, as above. */
#define MCHIP_PROF_KINDS 4
int mchip_profile_end(mchip_context *ctx, double *total_ms, double *kernel_ms, int *launches);
/* device properties the bench reports (name, CU count, memory) */
int mchip_device_info(mchip_context *ctx, char *name, int name_len, int *compute_units, double *hbm_bytes);

/*
 * Which kernels a model on a data set of this shape would launch, and with what geometry: the library's own kernel selection
 * ("Kernel selection"), for tests and diagnosis.  Needs no context and no device.  The tuning knobs come from the
 * environment, as they do for a real model; n_cu is the compute-unit count of the device asked about (mchip_device_info).
 * buf receives one line per fact:
 *   - the kernel instances, spelled as in the source (k_column_counts<2,false,true>, k_finalize_qp, ...), that one mchip_em_step
 *     followed by mchip_loglik, mchip_e_step and mchip_loglik_prefetch would launch, or with accel_cycle != 0 one cycle of
 *     mchip_accel_run: the passes over the genotype matrix and the finalisers, each once, not the small fixed launches around them.
 *     An E step that runs as one paired launch is listed as k_estep_pair<...> and as the two instances whose bodies that launch runs;
 *   - key=value lines: n_ichunks, lchunk, n_lchunks, ind_waves, xcd_rows, sparse, col_slabs, ind_slabs, ll_parts, pair, dual,
 *     shared_eta, byte_flags.
 * MCHIP_ERR_INVALID for a bad query or a buffer too small (4 KiB always suffice); MCHIP_ERR_UNSUPPORTED for K > MCHIP_MAX_K and
 * for a cycle where mchip_accel_run itself is unsupported (loci with more alleles than the sparse pass takes).
 */
typedef struct mchip_plan_query {
	int K, I, L, T, ploidy;			/* T = sum of uniquealleles */
	int min_alleles, max_alleles;		/* smallest and largest uniquealleles[l] */
	int has_missing;			/* the data set has a missing allele copy */
	int admixture, eta_constrained, do_projection;	/* as for mchip_set_model */
	double p_lb;
	int n_cu;
	int accel_cycle;
} mchip_plan_query;
int mchip_describe_plan(const mchip_plan_query *q, char *buf, int buf_len);

/* ---- where the process stands: the record a watchdog reads when a run makes no progress ----
 * The reference is one thread of plain C that blocks on nothing but its own loops (em_alg.c:78-88, log_likelihood.c:212-221);
 * this library blocks on the HIP runtime (stream synchronisation behind every entry point that returns a value, copies,
 * allocation, graph capture, teardown).  Every entry point and every such runtime call records itself while it runs, and each of
 * those moments counts one event.  mchip_progress_report writes one line per host thread that has used the library -- the entry
 * point it is in, the runtime call it waits in (with source line), the last phase the host named, seconds since its last event
 * -- into buf (any length; truncated, NUL-terminated) and the process-wide event count into *events; either may be NULL / 0.
 * mchip_progress_note names a phase of the caller's own (a static string: the reader, the writers) and counts as an event.
 * multiclust's opt-in watchdog (MC_WATCHDOG_S=<seconds>, host/mc_fit.c) polls the count and, when it stands still for that long,
 * prints the report and leaves with _exit(3). */
int mchip_progress_report(char *buf, int buf_len, unsigned long long *events);
int mchip_progress_note(const char *what);

#ifdef __cplusplus
}
#endif
#endif
