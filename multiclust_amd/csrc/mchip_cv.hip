/*
 * mchip_cv.hip -- K-fold cross-validation of the admixture model: the mchip_cv_* entry points and the kernels behind
 * mchip_cv_hold_out and mchip_cv_heldout_loglik (include/multiclust_hip.h has the contract; mchip_context.h the per-context
 * state and the install path; the fold draw is draw_mod_stream with m := n_folds and lives in mchip_generators.hip with the generator).
 *
 *   k_cv_mask    a thread per genotype: copies its `ploidy` bytes of the saved full data set into the stream buffer, or 0xFF when
 *                the genotype's fold is the one held out; marks the individuals that keep an observed copy.
 *   k_cv_score   the held-out score, runtime K (it runs F times per K against hundreds of EM passes: one instance, not 64).
 *                Lane = individual, as the S-side pass.  The workgroup's q rows sit in LDS, K doubles per lane, lds_pitch(K)
 *                apart (mchip_device_util.h).  The P rows of the current block of 8 loci are staged per workgroup as they lie in
 *                the slot's [T][K] form (columns toff[l0] .. toff[l0 + 8]) when they fit beside the q rows; a data set with so
 *                many alleles per locus that they do not reads its rows from memory (lane_pass_geometry_of,
 *                mchip_feature_geometry.h).  A lane reads the eight fold bytes of its block at once and then only
 *                the genotype bytes of the loci that are in the fold; the K-FMA dot product and the logarithm run for the
 *                observed copies of those loci alone, about 1 / F of the cells.
 *                Measured at 10 000 x 100 000, K = 8, F = 5: 8.5 ms (profiles/cv_passes.txt).  Two other forms were tried and were
 *                slower: the workgroup staging tiles of fold and genotype rows in LDS with aligned word loads (12.0 ms), and the
 *                same with every lane walking the in-fold loci of its own row, so that the lanes of a wave are busy at different
 *                loci (12.3 ms; 10.5 ms with eight staging loads in flight per thread).  What binds is not established.
 *                Sums: a lane adds its terms in locus order; the workgroup's lanes by block_tree_sum; one partial per workgroup,
 *                k_reduce_sum (mchip_em.hip) adds the partials.  The two counts are integers: block_add_counts.
 */
#include "mchip_context.h"

constexpr int CV_PAD = 16;	/* bytes allocated behind the fold bytes [I][L]: they are read eight at a time from any byte offset */

/* out = full (the saved data set in upload form [I][L][ploidy]) with every copy of the genotypes of fold `fold_id` turned into
 * 0xFF; seen[i] (zeroed by the caller) = 1 for every individual that keeps an observed copy */

__global__ __launch_bounds__(256) void k_cv_mask(const uint8_t *__restrict__ full, const uint8_t *__restrict__ fold, int fold_id, int I,
						 int L, int pl, uint8_t *__restrict__ out, uint8_t *seen)
{
	const size_t n = (size_t)I * L, stride = (size_t)gridDim.x * 256;
	for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < n; g += stride) {
		const bool hide = (int)fold[g] == fold_id;
		bool any = false;
		for (int a = 0; a < pl; a++) {
			const uint8_t v = hide ? (uint8_t)MCHIP_MISSING : full[g * pl + a];
			any |= v != MCHIP_MISSING;
			out[g * pl + a] = v;
		}
		if (any) seen[g / L] = 1;	/* (every writer stores the same value) */
	}
}

/* eight bytes from any byte offset: two aligned loads (the second may reach 15 bytes behind `off`: CV_PAD) */
__device__ __forceinline__ uint64_t cv_load8(const uint8_t *__restrict__ base, size_t off)
{
	const uint64_t *w = reinterpret_cast<const uint64_t *>(base + (off & ~(size_t)7));
	const unsigned sh = 8u * (unsigned)(off & 7);
	const uint64_t lo = w[0];
	return sh ? (lo >> sh) | (w[1] << (64u - sh)) : lo;
}

constexpr int CV_LBLOCK = LANE_PASS_LBLOCK;	/* loci per staged block */
constexpr size_t CV_LDS_BUDGET = 64 * 1024 - 64;	/* dynamic LDS per workgroup (the kernel has 16 static bytes beside it: its counts) */
constexpr size_t CV_RED_BYTES = 256 * sizeof(double);	/* the tree's space */

/* sum of log max(t, floor) over the observed copies of the fold, one partial per workgroup in part[] (n_itiles * n_lchunks of
 * them); counts[0] += copies, counts[1] += floored copies (zeroed by the caller).  P is a slot's [T][K], Q its [I][K]
 * (qstride = K) or [K] (qstride = 0). */
__global__ __launch_bounds__(256) void k_cv_score(int I, int L, int pl, int K, int KS, int stage, int lchunk,
						  const uint8_t *__restrict__ full, const uint8_t *__restrict__ fold, int fold_id,
						  const int32_t *__restrict__ toff, const double *__restrict__ P, const double *__restrict__ Q,
						  int qstride, double floor_t, double *__restrict__ part, unsigned long long *counts)
{
	extern __shared__ __attribute__((aligned(16))) double cv_lds[];
	double *qs = cv_lds;						/* [blockDim.x][KS] */
	double *red = qs + (size_t)blockDim.x * KS;			/* [256] */
	double *ps = red + 256;						/* staged P rows of the block, KS apart */
	const int nthr = blockDim.x, tid = threadIdx.x;
	const int i0 = blockIdx.x * nthr, i = i0 + tid;
	const int lbeg = blockIdx.y * lchunk, lend = min(L, lbeg + lchunk);
	stage_q_rows(qs, KS, Q, qstride, i0, I, K, tid, nthr);
	const double *q = qs + (size_t)tid * KS;
	const bool live = i < I;
	const size_t row = (size_t)i * L;
	double sum = 0.0;
	unsigned long long n_in = 0, n_fl = 0;
	__syncthreads();
	for (int l0 = lbeg; l0 < lend; l0 += CV_LBLOCK) {
		const int c0 = toff[l0];	/* (toff is padded: offsets behind the last locus are T) */
		if (stage) {
			stage_rows(ps, KS, P + (size_t)c0 * K, toff[min(L, l0 + CV_LBLOCK)] - c0, K, tid, nthr);
			__syncthreads();
		}
		if (live) {
			const uint64_t f8 = cv_load8(fold, row + l0);
			const int nl = min(CV_LBLOCK, lend - l0);
			for (int j = 0; j < nl; j++) {
				if ((int)((f8 >> (8 * j)) & 0xFFu) != fold_id) continue;
				const int l = l0 + j;
				const int cl = toff[l];
				const uint8_t *gsrc = full + (row + l) * pl;
				for (int a = 0; a < pl; a++) {
					const unsigned m = gsrc[a];
					if (m == MCHIP_MISSING) continue;
					double t = 0.0;
					if (stage) {
						const double *p = ps + (size_t)(cl - c0 + (int)m) * KS;
						for (int k = 0; k < K; k++) t = fma(q[k], p[k], t);
					} else {
						const double *p = P + (size_t)(cl + (int)m) * K;
						for (int k = 0; k < K; k++) t = fma(q[k], p[k], t);
					}
					n_in++;
					if (!(t >= floor_t)) {	/* below the floor, or NaN */
						t = floor_t;
						n_fl++;
					}
					sum += log(t);
				}
			}
		}
		if (stage) __syncthreads();	/* the tile is overwritten by the next block */
	}
	block_tree_sum(red, sum);
	if (tid == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = red[0];
	const unsigned long long mine[2] = {n_in, n_fl};
	block_add_counts(mine, counts);
}

/* folds, the saved full data set and a hold-out in force belong to the data set that goes */
void drop_cv(mchip_context *ctx)
{
	dfree(ctx->d_cv_fold);
	drop_saved(ctx->cv_full);
	dfree(ctx->d_cv_part); dfree(ctx->d_cv_out);
	ctx->cv_n_folds = 0;
	ctx->cv_fold = -1;
	ctx->cv_part_cap = 0;
}

static int cv_check_data(mchip_context *ctx, int need_folds)
{
	if (!ctx->T) return fail(ctx, MCHIP_ERR_STATE, "no genotypes set%s", nullptr);
	if (need_folds && !ctx->d_cv_fold) return fail(ctx, MCHIP_ERR_STATE, "no folds: mchip_cv_draw_folds or mchip_cv_set_folds first%s", nullptr);
	return MCHIP_OK;
}

/* one byte per genotype, whole generator chunks (draw_mod_stream writes whole chunks) and the padding the score's reads want */
static int cv_fold_buffer(mchip_context *ctx)
{
	if (ctx->d_cv_fold) return MCHIP_OK;
	const size_t n = (size_t)ctx->I * ctx->L, bytes = ((n + RNG_CHUNK - 1) / RNG_CHUNK) * RNG_CHUNK + CV_PAD;
	HIPCHK(hipMalloc((void **)&ctx->d_cv_fold, bytes));
	HIPCHK(hipMemsetAsync(ctx->d_cv_fold, 0, bytes, ctx->stream));
	return MCHIP_OK;
}

extern "C" {

int mchip_cv_draw_folds(mchip_context *ctx, const uint32_t *window, int n_folds)
{
	MCHIP_ENTRY();
	if (!ctx) return MCHIP_ERR_INVALID;
	int rc = cv_check_data(ctx, 0);
	if (rc) return rc;
	if (!window) return fail(ctx, MCHIP_ERR_INVALID, "null pointer%s", nullptr);
	if (n_folds < 2 || n_folds > 64) return fail(ctx, MCHIP_ERR_INVALID, "cv: n_folds must be in [2, 64]%s", nullptr);
	HIPCHK(hipSetDevice(ctx->device));
	if ((rc = cv_fold_buffer(ctx))) return rc;
	if ((rc = draw_mod_stream(ctx, window, (size_t)ctx->I * ctx->L, n_folds, ctx->d_cv_fold))) return rc;
	HIPCHK(hipStreamSynchronize(ctx->stream));
	ctx->cv_n_folds = n_folds;
	return MCHIP_OK;
}

int mchip_cv_set_folds(mchip_context *ctx, const uint8_t *folds, int n_folds)
{
	MCHIP_ENTRY();
	if (!ctx) return MCHIP_ERR_INVALID;
	int rc = cv_check_data(ctx, 0);
	if (rc) return rc;
	if (!folds) return fail(ctx, MCHIP_ERR_INVALID, "null pointer%s", nullptr);
	if (n_folds < 2 || n_folds > 64) return fail(ctx, MCHIP_ERR_INVALID, "cv: n_folds must be in [2, 64]%s", nullptr);
	const size_t n = (size_t)ctx->I * ctx->L;
	for (size_t x = 0; x < n; x++)
		if (folds[x] >= n_folds) return fail(ctx, MCHIP_ERR_INVALID, "cv: fold byte >= n_folds%s", nullptr);
	HIPCHK(hipSetDevice(ctx->device));
	if ((rc = cv_fold_buffer(ctx))) return rc;
	HIPCHK(hipMemcpyAsync(ctx->d_cv_fold, folds, n, hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	ctx->cv_n_folds = n_folds;
	return MCHIP_OK;
}

int mchip_cv_get_folds(mchip_context *ctx, uint8_t *folds)
{
	MCHIP_ENTRY();
	if (!ctx) return MCHIP_ERR_INVALID;
	int rc = cv_check_data(ctx, 1);
	if (rc) return rc;
	if (!folds) return fail(ctx, MCHIP_ERR_INVALID, "null pointer%s", nullptr);
	HIPCHK(hipSetDevice(ctx->device));
	HIPCHK(hipMemcpyAsync(folds, ctx->d_cv_fold, (size_t)ctx->I * ctx->L, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	return MCHIP_OK;
}

int mchip_cv_hold_out(mchip_context *ctx, int fold)
{
	MCHIP_ENTRY();
	if (!ctx) return MCHIP_ERR_INVALID;
	int rc = cv_check_data(ctx, 1);
	if (rc) return rc;
	if (fold < -1 || fold >= ctx->cv_n_folds) return fail(ctx, MCHIP_ERR_INVALID, "cv: fold outside [-1, n_folds)%s", nullptr);
	HIPCHK(hipSetDevice(ctx->device));
	/* the data set installed now is the full one: keep it */
	if (!ctx->cv_full.d_raw && (rc = save_installed(ctx, ctx->cv_full))) return rc;
	if (!ctx->d_cv_out) HIPCHK(hipMalloc((void **)&ctx->d_cv_out, 4 * sizeof(unsigned long long)));
	if (fold < 0)
		rc = install_saved(ctx, ctx->cv_full);
	else
		rc = install_derived(ctx, [&](uint8_t *d_out, uint8_t *d_seen) {
			hipLaunchKernelGGL(k_cv_mask, dim3(nblk_capped((size_t)ctx->I * ctx->L, 256, (size_t)1 << 20)), dim3(256), 0, ctx->stream,
					   ctx->cv_full.d_raw, ctx->d_cv_fold, fold, ctx->I, ctx->L, ctx->ploidy, d_out, d_seen);
		});
	if (rc) return rc;
	ctx->s_cache_slot = -1;
	ctx->cv_fold = fold;
	return MCHIP_OK;
}

int mchip_cv_heldout_loglik(mchip_context *ctx, int slot, double floor, double *sum_log, uint64_t *n_copies, uint64_t *n_floored)
{
	MCHIP_ENTRY();
	if (!ctx) return MCHIP_ERR_INVALID;
	int rc = cv_check_data(ctx, 1);
	if (rc || (rc = require_fit(ctx, slot, "cv: the held-out score is the admixture model's"))) return rc;
	if (ctx->cv_fold < 0 || !ctx->cv_full.d_raw) return fail(ctx, MCHIP_ERR_STATE, "cv: no fold is held out%s", nullptr);
	if (!(floor > 0.0 && floor <= 1.0)) return fail(ctx, MCHIP_ERR_INVALID, "cv: floor must be in (0, 1]%s", nullptr);
	HIPCHK(hipSetDevice(ctx->device));
	const lane_pass_geometry g = lane_pass_geometry_of(ctx->I, ctx->L, ctx->K, ctx->max_M, ctx->n_cu, CV_RED_BYTES, 64, CV_LDS_BUDGET);
	if ((rc = check_lds(ctx, k_cv_score, g.lds, "cv: the kernel's static LDS has outgrown CV_LDS_BUDGET"))) return rc;
	const size_t parts = (size_t)g.n_itiles * g.n_lchunks;
	if (ctx->cv_part_cap < parts) {
		dfree(ctx->d_cv_part);
		ctx->cv_part_cap = 0;
		HIPCHK(hipMalloc((void **)&ctx->d_cv_part, parts * sizeof(double)));
		ctx->cv_part_cap = parts;
	}
	HIPCHK(hipMemsetAsync(ctx->d_cv_out, 0, 4 * sizeof(unsigned long long), ctx->stream));
	hipLaunchKernelGGL(k_cv_score, dim3((unsigned)g.n_itiles, (unsigned)g.n_lchunks), dim3((unsigned)g.threads), g.lds, ctx->stream, ctx->I,
			   ctx->L, ctx->ploidy, ctx->K, lds_pitch(ctx->K), g.stage, g.lchunk, ctx->cv_full.d_raw, ctx->d_cv_fold, ctx->cv_fold, ctx->d_toff,
			   ctx->d_p[slot], ctx->d_q[slot], ctx->qstride, floor, ctx->d_cv_part, ctx->d_cv_out + 1);
	HIPCHK(hipGetLastError());
	launch_reduce_sum(ctx, ctx->d_cv_part, (int)parts, reinterpret_cast<double *>(ctx->d_cv_out));
	HIPCHK(hipGetLastError());
	unsigned long long h[3];
	HIPCHK(hipMemcpyAsync(h, ctx->d_cv_out, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	if (sum_log) memcpy(sum_log, &h[0], sizeof(double));
	if (n_copies) *n_copies = h[1];
	if (n_floored) *n_floored = h[2];
	return MCHIP_OK;
}

}
