/*
 * mchip_cv.hip -- K-fold cross-validation of the admixture model: the kernels behind mchip_cv_hold_out and
 * mchip_cv_heldout_loglik (include/multiclust_hip.h has the contract; mchip.hip has the entry points and the per-context state;
 * the fold draw is k_draw_partition with K := n_folds and lives there with the generator).
 *
 *   k_cv_mask    a thread per genotype: copies its `ploidy` bytes of the saved full data set into the stream buffer, or 0xFF when
 *                the genotype's fold is the one held out; marks the individuals that keep an observed copy.
 *   k_cv_score   the held-out score, runtime K (it runs F times per K against hundreds of EM passes: one instance, not 64).
 *                Lane = individual, as the S-side pass.  The workgroup's q rows sit in LDS, K doubles per lane, the rows an odd
 *                number of doubles apart: lane i reads dwords 2 (KS i + k) and the next one, and with KS odd the 32 lanes of a
 *                ds_read_b64 lane group fall on 32 different bank pairs of the 64.  The P rows of the current block of 8 loci are
 *                staged per workgroup as they lie in the slot's [T][K] form (columns toff[l0] .. toff[l0 + 8], K contiguous
 *                doubles each, rows KS apart), when they fit beside the q rows; a data set with so many alleles per locus that
 *                they do not reads its rows from memory.  A lane reads the eight fold bytes of its block at once and then only
 *                the genotype bytes of the loci that are in the fold; the K-FMA dot product and the logarithm run for the
 *                observed copies of those loci alone, about 1 / F of the cells.
 *                Measured at 10 000 x 100 000, K = 8, F = 5: 8.5 ms (profiles/cv_passes.txt).  Two other forms were tried and were
 *                slower: the workgroup staging tiles of fold and genotype rows in LDS with aligned word loads (12.0 ms), and the
 *                same with every lane walking the in-fold loci of its own row, so that the lanes of a wave are busy at different
 *                loci (12.3 ms; 10.5 ms with eight staging loads in flight per thread).  What binds is not established.
 *                Sums: a lane adds its terms in locus order; the workgroup's lanes are added by a fixed tree in LDS; one partial
 *                per workgroup, k_reduce_sum (mchip.hip) adds the partials.  No floating-point atomics: the same state gives the
 *                same bits.  The two counts are integers and go through atomics.
 */
#include "mchip_internal.h"

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

void mchip_cv_mask(hipStream_t s, const uint8_t *full, const uint8_t *fold, int fold_id, int I, int L, int ploidy, uint8_t *out,
		   uint8_t *seen)
{
	const size_t n = (size_t)I * L, blocks = (n + 255) / 256, cap = (size_t)1 << 20;
	hipLaunchKernelGGL(k_cv_mask, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(256), 0, s, full, fold, fold_id, I, L, ploidy, out, seen);
}

/* eight bytes from any byte offset: two aligned loads (the second may reach 15 bytes behind `off`: MCHIP_CV_PAD) */
__device__ __forceinline__ uint64_t cv_load8(const uint8_t *__restrict__ base, size_t off)
{
	const uint64_t *w = reinterpret_cast<const uint64_t *>(base + (off & ~(size_t)7));
	const unsigned sh = 8u * (unsigned)(off & 7);
	const uint64_t lo = w[0];
	return sh ? (lo >> sh) | (w[1] << (64u - sh)) : lo;
}

constexpr int CV_LBLOCK = 8;			/* loci per staged block */
constexpr size_t CV_LDS_BUDGET = 64 * 1024 - 64;	/* dynamic LDS per workgroup (the kernel has 16 static bytes beside it) */

/* geometry of the score pass: lanes per workgroup, whether the P rows of a block are staged, locus chunks */
struct cv_geometry {
	int threads, stage, lchunk, n_lchunks, n_itiles;
	size_t lds;
};
static inline int cv_ks(int K) { return K | 1; }
static cv_geometry cv_score_geometry(int I, int L, int K, int max_M, int n_cu)
{
	cv_geometry g;
	const size_t ks = (size_t)cv_ks(K), red = 256 * sizeof(double);
	const size_t ptile = (size_t)CV_LBLOCK * (size_t)max_M * ks * sizeof(double);
	/* the most lanes whose q rows leave room for the P tile; when no workgroup size does, the most lanes that fit alone */
	g.threads = 0;
	for (int t = 256; t >= 64 && !g.threads; t >>= 1)
		if ((size_t)t * ks * sizeof(double) + red + ptile <= CV_LDS_BUDGET) g.threads = t;
	g.stage = g.threads ? 1 : 0;
	for (int t = 256; t >= 64 && !g.threads; t >>= 1)
		if ((size_t)t * ks * sizeof(double) + red <= CV_LDS_BUDGET) g.threads = t;	/* (64 lanes at K = 64: 35 KB) */
	g.lds = (size_t)g.threads * ks * sizeof(double) + red + (g.stage ? ptile : 0);
	g.n_itiles = (I + g.threads - 1) / g.threads;
	/* enough workgroups to fill the device a few times over; chunks are whole blocks of 8 loci */
	const int lblocks = (L + CV_LBLOCK - 1) / CV_LBLOCK;
	int want = (16 * (n_cu > 0 ? n_cu : 256) + g.n_itiles - 1) / g.n_itiles;
	if (want > lblocks) want = lblocks;
	if (want > 65535) want = 65535;
	if (want < 1) want = 1;
	g.lchunk = ((lblocks + want - 1) / want) * CV_LBLOCK;
	g.n_lchunks = (L + g.lchunk - 1) / g.lchunk;
	return g;
}

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
	/* q rows of the workgroup's individuals: consecutive threads read consecutive doubles of Q */
	if (qstride) {
		const int rows = min(nthr, I - i0);
		for (int x = tid; x < rows * K; x += nthr) qs[(x / K) * KS + x % K] = Q[(size_t)i0 * K + x];
	} else {
		for (int x = tid; x < nthr * K; x += nthr) qs[(x / K) * KS + x % K] = Q[x % K];
	}
	const double *q = qs + (size_t)tid * KS;
	const bool live = i < I;
	const size_t row = (size_t)i * L;
	double sum = 0.0;
	unsigned long long n_in = 0, n_fl = 0;
	__syncthreads();
	for (int l0 = lbeg; l0 < lend; l0 += CV_LBLOCK) {
		const int c0 = toff[l0];	/* (toff is padded: offsets behind the last locus are T) */
		if (stage) {
			const int ncols = toff[min(L, l0 + CV_LBLOCK)] - c0;
			for (int x = tid; x < ncols * K; x += nthr) ps[(x / K) * KS + x % K] = P[(size_t)c0 * K + x];
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
	/* the workgroup's lanes in a fixed tree (lanes of a wave first, then the waves) */
	red[tid] = sum;
	__syncthreads();
	for (int w = nthr >> 1; w > 0; w >>= 1) {
		if (tid < w) red[tid] += red[tid + w];
		__syncthreads();
	}
	if (tid == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = red[0];
	/* counts: integers, order does not matter */
	__shared__ unsigned long long cnt[2];
	if (tid == 0) cnt[0] = cnt[1] = 0;
	__syncthreads();
	if (n_in) atomicAdd(&cnt[0], n_in);
	if (n_fl) atomicAdd(&cnt[1], n_fl);
	__syncthreads();
	if (tid == 0) {
		if (cnt[0]) atomicAdd(&counts[0], cnt[0]);
		if (cnt[1]) atomicAdd(&counts[1], cnt[1]);
	}
}

int mchip_cv_score_parts(int I, int L, int K, int max_M, int n_cu)
{
	const cv_geometry g = cv_score_geometry(I, L, K, max_M, n_cu);
	return g.n_itiles * g.n_lchunks;
}

int mchip_cv_score(hipStream_t s, int I, int L, int ploidy, int K, int max_M, int n_cu, const uint8_t *full, const uint8_t *fold,
		   int fold_id, const int32_t *toff, const double *P, const double *Q, int qstride, double floor, double *part,
		   unsigned long long *counts)
{
	const cv_geometry g = cv_score_geometry(I, L, K, max_M, n_cu);
	hipLaunchKernelGGL(k_cv_score, dim3((unsigned)g.n_itiles, (unsigned)g.n_lchunks), dim3((unsigned)g.threads), g.lds, s, I, L, ploidy, K,
			   cv_ks(K), g.stage, g.lchunk, full, fold, fold_id, toff, P, Q, qstride, floor, part, counts);
	return g.n_itiles * g.n_lchunks;
}
