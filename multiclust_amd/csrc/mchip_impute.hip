/*
 * mchip_impute.hip -- missing allele copies filled from the fitted admixture model: mchip_impute_missing and its kernel
 * (include/multiclust_hip.h has the contract and the rule; mchip_context.h the per-context state).
 *
 *   k_impute   runtime K, one instance (it runs once per K of a run).  Lane = individual, as the S-side pass and k_cv_score.  A
 *              lane's 8 loci of a block are the 8 * ploidy contiguous bytes of its gtS group, read as `ploidy` aligned 64-bit
 *              words; consecutive lanes read consecutive groups.  A word without a 0xFF byte costs one compare, and a block in
 *              which no lane of the workgroup has a missing copy is left after one vote (it stages nothing).  The q rows sit in
 *              LDS, K | 1 doubles apart (k_cv_score's reasoning: 32 lanes, 32 bank pairs); the P rows of the block of 8 loci are
 *              staged per workgroup as they lie in the slot's [T][K] form when they fit beside the q rows, and read from memory
 *              when a data set has so many alleles per locus that they do not.
 *              A genotype with r missing copies: t_m = sum_k q_k p_klm by an fma chain in k order over the first n_real[l]
 *              slots; copy j = 1 .. r goes to the first m with the largest t_m / (c_m + 1), c_m the copies given to m so far
 *              (the t_m are computed again for every copy: nothing is kept per candidate, so any number of alleles runs in the
 *              same registers).  The picks are kept in ascending order in a per-lane array of `ploidy` bytes of private
 *              memory and stored into the missing positions of the upload-form scratch in copy order; the observed bytes of the
 *              scratch are never written.  c = prod_j j t_mj / ((c_mj + 1) sum_m t_m).
 *              sum_conf: a lane adds its c in locus order; the workgroup's lanes are added by a fixed tree in LDS; one partial per
 *              workgroup, k_reduce_sum (mchip.hip) adds the partials.  No floating-point atomics: the same state gives the same
 *              bits.  The three counts are integers and go through atomics.
 *              Not yet timed on a device and not tuned (profiles/impute.txt, scripts/impute_bench.py).
 */
#include "mchip_context.h"

constexpr int IMP_LBLOCK = 8;				/* loci per gtS group and per staged block */
constexpr size_t IMP_LDS_BUDGET = 64 * 1024 - 512;	/* dynamic LDS per workgroup (the kernel has 288 static bytes beside it: its
							 * counts and the scratch of the workgroup vote; checked at the launch) */
constexpr int IMP_MAX_PL = 64;				/* set_shape's limit on the ploidy */

/* geometry of the pass: lanes per workgroup, whether the P rows of a block are staged, locus chunks (whole blocks of 8) */
struct imp_geometry {
	int threads, stage, lchunk, n_lchunks, n_itiles;
	size_t lds;
};
static inline int imp_ks(int K) { return K | 1; }
static imp_geometry impute_geometry(int I, int L, int K, int max_M, int n_cu)
{
	imp_geometry g;
	const size_t ks = (size_t)imp_ks(K), red = 256 * sizeof(double);
	const size_t ptile = (size_t)IMP_LBLOCK * (size_t)max_M * ks * sizeof(double);
	/* the most lanes whose q rows leave room for the P tile; when no workgroup size does, the most lanes that fit alone */
	g.threads = 0;
	for (int t = 256; t >= 64 && !g.threads; t >>= 1)
		if ((size_t)t * ks * sizeof(double) + red + ptile <= IMP_LDS_BUDGET) g.threads = t;
	g.stage = g.threads ? 1 : 0;
	for (int t = 256; t >= 64 && !g.threads; t >>= 1)
		if ((size_t)t * ks * sizeof(double) + red <= IMP_LDS_BUDGET) g.threads = t;	/* (64 lanes at K = 64: 35 KB) */
	g.lds = (size_t)g.threads * ks * sizeof(double) + red + (g.stage ? ptile : 0);
	g.n_itiles = (I + g.threads - 1) / g.threads;
	const int lblocks = (L + IMP_LBLOCK - 1) / IMP_LBLOCK;
	int want = (16 * (n_cu > 0 ? n_cu : 256) + g.n_itiles - 1) / g.n_itiles;
	if (want > lblocks) want = lblocks;
	if (want > 65535) want = 65535;
	if (want < 1) want = 1;
	g.lchunk = ((lblocks + want - 1) / want) * IMP_LBLOCK;
	g.n_lchunks = (L + g.lchunk - 1) / g.lchunk;
	return g;
}

/* non-zero iff a byte of v is 0xFF */
__device__ __forceinline__ uint64_t imp_has_missing(uint64_t v)
{
	const uint64_t x = ~v;	/* a zero byte of x */
	return (x - 0x0101010101010101ull) & ~x & 0x8080808080808080ull;
}

/* t_m of candidate column `col` (a staged row, or the slot's row in memory) */
__device__ __forceinline__ double imp_dot(const double *__restrict__ q, const double *__restrict__ p, int K)
{
	double t = 0.0;
	for (int k = 0; k < K; k++) t = fma(q[k], p[k], t);
	return t;
}

/* raw: the installed data set in upload form [I][L][pl]; its missing copies are filled in place.  conf: NULL or [I][L], zeroed by
 * the caller.  part[]: one partial sum of c per workgroup (n_itiles * n_lchunks of them).  counts[0] += copies filled, [1] += copies
 * left missing, [2] += genotypes filled (zeroed by the caller).  P is a slot's [T][K], Q its [I][K] (qstride = K) or [K] (0). */
__global__ __launch_bounds__(256) void k_impute(int I, int L, int pl, int K, int KS, int stage, int lchunk,
						const uint8_t *__restrict__ gtS, const int32_t *__restrict__ toff,
						const int32_t *__restrict__ n_real, const double *__restrict__ P,
						const double *__restrict__ Q, int qstride, uint8_t *__restrict__ raw, double *__restrict__ conf,
						double *__restrict__ part, unsigned long long *counts)
{
	extern __shared__ __attribute__((aligned(16))) double imp_lds[];
	double *qs = imp_lds;						/* [blockDim.x][KS] */
	double *red = qs + (size_t)blockDim.x * KS;			/* [256] */
	double *ps = red + 256;						/* staged P rows of the block, KS apart */
	const int nthr = blockDim.x, tid = threadIdx.x;
	const int i0 = blockIdx.x * nthr, i = i0 + tid;
	const int lbeg = blockIdx.y * lchunk, lend = min(L, lbeg + lchunk);
	if (qstride) {
		const int rows = min(nthr, I - i0);
		for (int x = tid; x < rows * K; x += nthr) qs[(x / K) * KS + x % K] = Q[(size_t)i0 * K + x];
	} else {
		for (int x = tid; x < nthr * K; x += nthr) qs[(x / K) * KS + x % K] = Q[x % K];
	}
	const double *q = qs + (size_t)tid * KS;
	const bool live = i < I;
	const size_t grp = (size_t)IMP_LBLOCK * pl;
	double sum = 0.0;
	unsigned long long n_fill = 0, n_left = 0, n_geno = 0;
	uint8_t picks[IMP_MAX_PL];	/* the copies given so far, ascending */
	__syncthreads();
	for (int l0 = lbeg; l0 < lend; l0 += IMP_LBLOCK) {
		const uint8_t *g = gtS + ((size_t)(l0 / IMP_LBLOCK) * I + (live ? i : 0)) * grp;
		uint64_t any = 0;
		if (live) {
			const uint64_t *gw = reinterpret_cast<const uint64_t *>(g);
			for (int w = 0; w < pl; w++) any |= imp_has_missing(gw[w]);
		}
		/* (loci behind L are padded with 0xFF in gtS: the last block always votes yes and masks them below) */
		if (!__syncthreads_or(any != 0)) continue;	/* also: everybody is done with the tile of the block before */
		const int c0 = toff[l0];	/* (toff is padded: offsets behind the last locus are T) */
		if (stage) {
			const int ncols = toff[min(L, l0 + IMP_LBLOCK)] - c0;
			for (int x = tid; x < ncols * K; x += nthr) ps[(x / K) * KS + x % K] = P[(size_t)c0 * K + x];
			__syncthreads();
		}
		if (!any) continue;
		const int nl = min(IMP_LBLOCK, lend - l0);
		for (int j = 0; j < nl; j++) {
			const uint8_t *gj = g + (size_t)j * pl;
			int r = 0;
			for (int a = 0; a < pl; a++) r += gj[a] == MCHIP_MISSING;
			if (!r) continue;
			const int l = l0 + j, cl = toff[l], M = n_real[l];
			const double *prow = stage ? ps + (size_t)(cl - c0) * KS : P + (size_t)cl * K;
			const int pstep = stage ? KS : K;
			/* the first copy: argmax t and the normalising sum, in m order */
			double best = 0.0, tsum = 0.0;
			int bm = -1;
			for (int m = 0; m < M; m++) {
				const double t = imp_dot(q, prow + (size_t)m * pstep, K);
				tsum += t;
				if (t > best) {	/* NaN is not > */
					best = t;
					bm = m;
				}
			}
			if (bm < 0) {	/* no candidate, or none with t > 0 */
				n_left += (unsigned)r;
				continue;
			}
			picks[0] = (uint8_t)bm;
			double c = best / tsum;
			for (int n = 1; n < r; n++) {	/* copy n + 1: the first m with the largest t_m / (c_m + 1) */
				best = 0.0;
				bm = -1;
				for (int m = 0; m < M; m++) {
					int cm = 0;
					for (int x = 0; x < n; x++) cm += picks[x] == m;
					const double t = imp_dot(q, prow + (size_t)m * pstep, K);
					const double v = cm ? t / (double)(cm + 1) : t;
					if (v > best) {
						best = v;
						bm = m;
					}
				}
				if (bm < 0) break;	/* (cannot happen: the first copy found a t > 0) */
				c *= (best * (double)(n + 1)) / tsum;
				int x = n;	/* keep the picks ascending */
				while (x > 0 && picks[x - 1] > bm) {
					picks[x] = picks[x - 1];
					x--;
				}
				picks[x] = (uint8_t)bm;
			}
			uint8_t *dst = raw + ((size_t)i * L + l) * pl;
			for (int a = 0, x = 0; a < pl; a++)
				if (gj[a] == MCHIP_MISSING) dst[a] = picks[x++];
			if (conf) conf[(size_t)i * L + l] = c;
			sum += c;
			n_fill += (unsigned)r;
			n_geno++;
		}
	}
	/* the workgroup's lanes in a fixed tree */
	red[tid] = sum;
	__syncthreads();
	for (int w = nthr >> 1; w > 0; w >>= 1) {
		if (tid < w) red[tid] += red[tid + w];
		__syncthreads();
	}
	if (tid == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = red[0];
	/* counts: integers, order does not matter */
	__shared__ unsigned long long cnt[3];
	if (tid == 0) cnt[0] = cnt[1] = cnt[2] = 0;
	__syncthreads();
	if (n_fill) atomicAdd(&cnt[0], n_fill);
	if (n_left) atomicAdd(&cnt[1], n_left);
	if (n_geno) atomicAdd(&cnt[2], n_geno);
	__syncthreads();
	if (tid == 0)
		for (int x = 0; x < 3; x++)
			if (cnt[x]) atomicAdd(&counts[x], cnt[x]);
}

extern "C" int mchip_impute_missing(mchip_context *ctx, int slot, const int32_t *n_real, uint8_t *geno_out, double *conf_out,
				    uint64_t *n_filled, uint64_t *n_left, uint64_t *n_genotypes, double *sum_conf)
{
	MCHIP_ENTRY();
	if (!ctx) return MCHIP_ERR_INVALID;
	if (!ctx->T) return fail(ctx, MCHIP_ERR_STATE, "no genotypes set%s", nullptr);
	int rc = check_slot(ctx, slot);
	if (rc) return rc;
	if (!ctx->admixture) return fail(ctx, MCHIP_ERR_UNSUPPORTED, "impute: the predictive distribution used is the admixture model's%s", nullptr);
	if (!n_real || !geno_out) return fail(ctx, MCHIP_ERR_INVALID, "null pointer%s", nullptr);
	const int I = ctx->I, L = ctx->L, pl = ctx->ploidy, K = ctx->K;
	for (int l = 0; l < L; l++)
		if (n_real[l] < 0 || n_real[l] > ctx->h_ua[(size_t)l])
			return fail(ctx, MCHIP_ERR_INVALID, "impute: n_real[l] outside [0, uniquealleles[l]]%s", nullptr);
	HIPCHK(hipSetDevice(ctx->device));
	const imp_geometry g = impute_geometry(I, L, K, ctx->max_M, ctx->n_cu);
	const size_t parts = (size_t)g.n_itiles * g.n_lchunks, n_geno = (size_t)I * L;
	hipFuncAttributes attr;
	HIPCHK(hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(k_impute)));
	if (attr.sharedSizeBytes + g.lds > 64 * 1024) return fail(ctx, MCHIP_ERR_STATE, "impute: the kernel's static LDS has outgrown IMP_LDS_BUDGET%s", nullptr);
	/* the installed data set in upload form: the kernel stores the filled bytes into it */
	saved_set scratch;
	if ((rc = save_installed(ctx, scratch))) return rc;
	struct drop_on_exit {
		saved_set &s;
		~drop_on_exit() { drop_saved(s); }
	} drop{scratch};
	scoped_dev<int32_t> d_nreal;
	scoped_dev<double> d_conf, d_part;
	scoped_dev<unsigned long long> d_out;	/* [0] the sum of c (a double), [1..3] the counts */
	HIPCHK(d_nreal.alloc((size_t)L));
	HIPCHK(d_part.alloc(parts));
	HIPCHK(d_out.alloc(4));
	if (conf_out) {
		HIPCHK(d_conf.alloc(n_geno));
		HIPCHK(hipMemsetAsync(d_conf.p, 0, n_geno * sizeof(double), ctx->stream));
	}
	HIPCHK(hipMemcpyAsync(d_nreal.p, n_real, (size_t)L * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(hipMemsetAsync(d_out.p, 0, 4 * sizeof(unsigned long long), ctx->stream));
	hipLaunchKernelGGL(k_impute, dim3((unsigned)g.n_itiles, (unsigned)g.n_lchunks), dim3((unsigned)g.threads), g.lds, ctx->stream, I, L, pl, K,
			   imp_ks(K), g.stage, g.lchunk, ctx->d_gtS, ctx->d_toff, d_nreal.p, ctx->d_p[slot], ctx->d_q[slot], ctx->qstride,
			   scratch.d_raw, d_conf.p, d_part.p, d_out.p + 1);
	HIPCHK(hipGetLastError());
	launch_reduce_sum(ctx, d_part.p, (int)parts, reinterpret_cast<double *>(d_out.p));
	HIPCHK(hipGetLastError());
	unsigned long long h[4];
	HIPCHK(hipMemcpyAsync(h, d_out.p, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));	/* (n_real crossed in pageable memory: done when the stream is) */
	/* the caller's arrays are written once everything on the device has succeeded */
	HIPCHK(hipMemcpyAsync(geno_out, scratch.d_raw, n_geno * pl, hipMemcpyDeviceToHost, ctx->stream));
	if (conf_out) HIPCHK(hipMemcpyAsync(conf_out, d_conf.p, n_geno * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	if (sum_conf) memcpy(sum_conf, &h[0], sizeof(double));
	if (n_filled) *n_filled = h[1];
	if (n_left) *n_left = h[2];
	if (n_genotypes) *n_genotypes = h[3];
	return MCHIP_OK;
}
