/*
 * mchip_impute.hip -- missing allele copies filled from the fitted admixture model: mchip_impute_missing and its kernel
 * (include/multiclust_hip.h has the contract and the rule; mchip_context.h the per-context state).
 *
 *   k_impute   runtime K, one instance (it runs once per K of a run).  Lane = individual, as the S-side pass and k_cv_score.  A
 *              lane's 8 loci of a block are the 8 * ploidy contiguous bytes of its gtS group, read as `ploidy` aligned 64-bit
 *              words; consecutive lanes read consecutive groups.  A word without a 0xFF byte costs one compare, and a block in
 *              which no lane of the workgroup has a missing copy is left after one vote (it stages nothing).  The q rows sit in
 *              LDS, lds_pitch(K) apart (mchip_device_util.h); the P rows of the block of 8 loci are staged per workgroup when they
 *              fit beside the q rows and read from memory when they do not (lane_pass_geometry_of, mchip_feature_geometry.h).
 *              A genotype with r missing copies: t_m = sum_k q_k p_klm by an fma chain in k order over the first n_real[l]
 *              slots; copy j = 1 .. r goes to the first m with the largest t_m / (c_m + 1), c_m the copies given to m so far
 *              (the t_m are computed again for every copy: nothing is kept per candidate, so any number of alleles runs in the
 *              same registers).  The picks are kept in ascending order in a per-lane array of `ploidy` bytes of private
 *              memory and stored into the missing positions of the upload-form scratch in copy order; the observed bytes of the
 *              scratch are never written.  c = prod_j j t_mj / ((c_mj + 1) sum_m t_m).
 *              sum_conf: a lane adds its c in locus order; the workgroup's lanes by block_tree_sum; one partial per workgroup,
 *              k_reduce_sum (mchip_em.hip) adds the partials.  The three counts are integers: block_add_counts.
 *              Not yet timed on a device and not tuned (profiles/impute.txt, scripts/impute_bench.py).
 */
#include "mchip_context.h"

constexpr int IMP_LBLOCK = LANE_PASS_LBLOCK;		/* loci per gtS group and per staged block */
constexpr size_t IMP_LDS_BUDGET = 64 * 1024 - 512;	/* dynamic LDS per workgroup (the kernel has 288 static bytes beside it: its
							 * counts and the scratch of the workgroup vote; checked at the launch) */
constexpr size_t IMP_RED_BYTES = 256 * sizeof(double);	/* the tree's space */
constexpr int IMP_MAX_PL = 64;				/* set_shape's limit on the ploidy */

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
	stage_q_rows(qs, KS, Q, qstride, i0, I, K, tid, nthr);
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
			stage_rows(ps, KS, P + (size_t)c0 * K, toff[min(L, l0 + IMP_LBLOCK)] - c0, K, tid, nthr);
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
	block_tree_sum(red, sum);
	if (tid == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = red[0];
	const unsigned long long mine[3] = {n_fill, n_left, n_geno};
	block_add_counts(mine, counts);
}

extern "C" int mchip_impute_missing(mchip_context *ctx, int slot, const int32_t *n_real, uint8_t *geno_out, double *conf_out,
				    uint64_t *n_filled, uint64_t *n_left, uint64_t *n_genotypes, double *sum_conf)
{
	MCHIP_ENTRY();
	if (!ctx) return MCHIP_ERR_INVALID;
	int rc = require_fit(ctx, slot, "impute: the predictive distribution used is the admixture model's");
	if (rc) return rc;
	if (!n_real || !geno_out) return fail(ctx, MCHIP_ERR_INVALID, "null pointer%s", nullptr);
	const int I = ctx->I, L = ctx->L, pl = ctx->ploidy, K = ctx->K;
	for (int l = 0; l < L; l++)
		if (n_real[l] < 0 || n_real[l] > ctx->h_ua[(size_t)l])
			return fail(ctx, MCHIP_ERR_INVALID, "impute: n_real[l] outside [0, uniquealleles[l]]%s", nullptr);
	HIPCHK(hipSetDevice(ctx->device));
	const lane_pass_geometry g = lane_pass_geometry_of(I, L, K, ctx->max_M, ctx->n_cu, IMP_RED_BYTES, 64, IMP_LDS_BUDGET);
	const size_t parts = (size_t)g.n_itiles * g.n_lchunks, n_geno = (size_t)I * L;
	if ((rc = check_lds(ctx, k_impute, g.lds, "impute: the kernel's static LDS has outgrown IMP_LDS_BUDGET"))) return rc;
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
			   lds_pitch(K), g.stage, g.lchunk, ctx->d_gtS, ctx->d_toff, d_nreal.p, ctx->d_p[slot], ctx->d_q[slot], ctx->qstride,
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
