/*
 * mchip_kinship.hip -- kinship between individuals under the fitted admixture model: mchip_kinship_products and its tile pass
 * (include/multiclust_hip.h has the contract, the definitions and the derivation from REAP's estimator; mchip_context.h the
 * per-context state).  Quadratic in the individuals like mchip_residuals.hip: 2 I^2 T multiply-adds, half of them skipped by symmetry.
 *
 * The chunks, the product kernels and the mirror are mchip_gram.h's, shared with mchip_residuals.hip: the same cut of the loci, the
 * same kernel on the same operand R, so `gram` here has the bits of mchip_residual_products' gram.  Per chunk one tile pass and the
 * two symmetric products G += R^T R and V += W^T W; the two I^2 accumulators stay on the device from the first chunk to the last.
 *
 *   k_kin_tile     runtime K, one instance.  Lane = individual, k_resid_tile's pass: a workgroup takes one block of 8 loci (the part
 *                  of it that lies in the chunk) and a tile of individuals; a lane reads its gtS group as aligned 64-bit words.  The
 *                  q rows sit in LDS lds_pitch(K) apart, the P rows of the block are staged when they fit beside the q rows and
 *                  read from memory when they do not (lane_pass_geometry_of).  Per locus: a = observed copies; per column t =
 *                  sum_k q_k p_k by an fma chain in k order, r = fma(-a, t, n), v = t fmax(1 - t, 0) -- a chain that rounds to
 *                  1 + ulp gives 0, not the square root of a negative number -- and w = a sqrt(v); r = w = 0 where a = 0.
 *                  Written as doubles, individual-contiguous: R and W [chunk column][Ipad]; Ipad = I rounded up to RES_TILE, the
 *                  lanes behind I write zeros.  Nothing is kept per allele: 254 alleles run in the registers of two.
 *   k_gram_pair    both products in one launch, grid.z = which (mchip_gram.h): the form kept, see below.
 *   k_resid_gram<true> twice: the same sums in two launches, under MCHIP_KIN_TWO_LAUNCHES; the same bits, which a test asserts.
 *   k_resid_mirror once for G and once for V at the end: both come back symmetric bit for bit.
 *   No floating-point atomics; an element of G or V is owned by one lane of one workgroup from the first chunk to the last, and
 *   the order of its additions is the order of the columns: the same state gives the same bits on any device, under any knob.
 *
 *   Compile report (hipcc of ROCm 7.2, gfx950, -O3, -Rpass-analysis=kernel-resource-usage):  k_kin_tile 32 VGPRs, scratch 0,
 *   dynamic LDS only, 8 waves / SIMD;  k_gram_pair and k_resid_gram<true> 104 VGPRs + 32 AGPRs (the accumulators), scratch 0, 20480
 *   bytes of static LDS, 3 waves / SIMD;  k_resid_mirror 4 VGPRs.  One launch against two: profiles/kinship.txt, scripts/kinship_bench.py.
 */
#include "mchip_gram.h"

/* The loci [lbeg, lend) of one chunk, whose columns start at cbeg = toff[lbeg].  blockIdx.y: the block of 8 loci, counted from the
 * one lbeg lies in.  R and W [column - cbeg][Ipad].  P is a slot's [T][K], Q its [I][K] (qstride = K) or [K] (0). */
__global__ __launch_bounds__(256) void k_kin_tile(int I, int Ipad, int L, int pl, int K, int KS, int stage, int lbeg, int lend,
						  const uint8_t *__restrict__ gtS, const int32_t *__restrict__ toff,
						  const double *__restrict__ P, const double *__restrict__ Q, int qstride,
						  double *__restrict__ R, double *__restrict__ W)
{
	extern __shared__ __attribute__((aligned(16))) double kin_lds[];
	double *qs = kin_lds;					/* [blockDim.x][KS] */
	double *ps = qs + (size_t)blockDim.x * KS;		/* staged P rows of the block, KS apart */
	const int nthr = blockDim.x, tid = threadIdx.x;
	const int i0 = blockIdx.x * nthr, i = i0 + tid;
	const int l0 = (lbeg / RES_LBLOCK + (int)blockIdx.y) * RES_LBLOCK;
	const int jbeg = max(l0, lbeg), jend = min(l0 + RES_LBLOCK, lend);	/* (jbeg < jend: the grid covers the chunk's blocks only) */
	const int cbeg = toff[lbeg], c0 = toff[jbeg];
	stage_q_rows(qs, KS, Q, qstride, i0, I, K, tid, nthr);
	if (stage) stage_rows(ps, KS, P + (size_t)c0 * K, toff[jend] - c0, K, tid, nthr);
	__syncthreads();
	if (i >= Ipad) return;
	const bool live = i < I;
	const double *q = qs + (size_t)tid * KS;
	const uint64_t *gw = reinterpret_cast<const uint64_t *>(gtS + ((size_t)(l0 / RES_LBLOCK) * I + (live ? i : 0)) * ((size_t)RES_LBLOCK * pl));
	const int pstep = stage ? KS : K;
	for (int l = jbeg; l < jend; l++) {
		const int x0 = (l - l0) * pl, cl = toff[l], M = toff[l + 1] - cl;
		int a = 0;
		if (live)
			for (int x = 0; x < pl; x++) a += res_byte(gw, x0 + x) != MCHIP_MISSING;
		const double *prow = stage ? ps + (size_t)(cl - c0) * KS : P + (size_t)cl * K;
		double *rout = R + (size_t)(cl - cbeg) * Ipad + i, *wout = W + (size_t)(cl - cbeg) * Ipad + i;
		for (int m = 0; m < M; m++) {
			double r = 0.0, w = 0.0;
			if (a) {
				int n = 0;
				for (int x = 0; x < pl; x++) n += res_byte(gw, x0 + x) == (unsigned)m;
				const double *p = prow + (size_t)m * pstep;
				double t = 0.0;
				for (int k = 0; k < K; k++) t = fma(q[k], p[k], t);
				r = fma(-(double)a, t, (double)n);
				w = (double)a * sqrt(t * fmax(1.0 - t, 0.0));
			}
			rout[(size_t)m * Ipad] = r;
			wout[(size_t)m * Ipad] = w;
		}
	}
}

extern "C" int mchip_kinship_products(mchip_context *ctx, int slot, double *gram, double *scale)
{
	MCHIP_ENTRY();
	if (!ctx) return MCHIP_ERR_INVALID;
	int rc = require_fit(ctx, slot, "kinship: the individual-specific allele frequencies are the admixture model's");
	if (rc) return rc;
	if (!gram || !scale) return fail(ctx, MCHIP_ERR_INVALID, "null pointer%s", nullptr);
	const int I = ctx->I, L = ctx->L, pl = ctx->ploidy, K = ctx->K;
	const int Ipad = (I + RES_TILE - 1) / RES_TILE * RES_TILE, nt = Ipad / RES_TILE;
	const size_t n2 = (size_t)Ipad * Ipad;
	HIPCHK(hipSetDevice(ctx->device));
	/* lanes per workgroup: a divisor of 256, at least RES_TILE; no reduction space; the blocks of a chunk are the grid's, not the geometry's */
	const lane_pass_geometry g = lane_pass_geometry_of(Ipad, L, K, ctx->max_M, ctx->n_cu, 0, RES_TILE, RES_LDS_BUDGET);
	if ((rc = check_lds(ctx, k_kin_tile, g.lds, "kinship: the kernel's static LDS has outgrown RES_LDS_BUDGET"))) return rc;
	std::vector<int> cut, width;	/* the chunks (mchip_gram.h): chunk ch is loci cut[ch] .. cut[ch + 1] - 1, width[ch] columns */
	res_cut_chunks(ctx->h_ua, L, cut, width);
	scoped_dev<double> d_G, d_V, d_R, d_W;
	if (d_G.alloc(n2) != hipSuccess || d_V.alloc(n2) != hipSuccess || d_R.alloc((size_t)RES_CHUNK * Ipad) != hipSuccess ||
	    d_W.alloc((size_t)RES_CHUNK * Ipad) != hipSuccess) {
		(void)hipGetLastError();
		return fail(ctx, MCHIP_ERR_ALLOC, "kinship: the I x I sums or the chunk buffers do not fit on the device%s", nullptr);
	}
	HIPCHK(hipMemsetAsync(d_G.p, 0, n2 * sizeof(double), ctx->stream));
	HIPCHK(hipMemsetAsync(d_V.p, 0, n2 * sizeof(double), ctx->stream));
	const bool two = ctx->knob.kin_two_launches != 0;
	for (size_t ch = 0; ch + 1 < cut.size(); ch++) {
		const int lbeg = cut[ch], lend = cut[ch + 1];
		const int ncols = width[ch];
		const unsigned nblocks = (unsigned)((lend - 1) / RES_LBLOCK - lbeg / RES_LBLOCK + 1);
		hipLaunchKernelGGL(k_kin_tile, dim3((unsigned)g.n_itiles, nblocks), dim3((unsigned)g.threads), g.lds, ctx->stream, I, Ipad, L, pl, K, lds_pitch(K),
				   g.stage, lbeg, lend, ctx->d_gtS, ctx->d_toff, ctx->d_p[slot], ctx->d_q[slot], ctx->qstride, d_R.p, d_W.p);
		HIPCHK(hipGetLastError());
		if (!ncols) continue;
		if (two) {
			hipLaunchKernelGGL(k_resid_gram<true>, dim3((unsigned)nt, (unsigned)nt), dim3(256), 0, ctx->stream, Ipad, ncols, d_R.p, d_R.p, d_G.p);
			HIPCHK(hipGetLastError());
			hipLaunchKernelGGL(k_resid_gram<true>, dim3((unsigned)nt, (unsigned)nt), dim3(256), 0, ctx->stream, Ipad, ncols, d_W.p, d_W.p, d_V.p);
		} else {
			hipLaunchKernelGGL(k_gram_pair, dim3((unsigned)nt, (unsigned)nt, 2), dim3(256), 0, ctx->stream, Ipad, ncols, d_R.p, d_G.p, d_W.p, d_V.p);
		}
		HIPCHK(hipGetLastError());
	}
	hipLaunchKernelGGL(k_resid_mirror, dim3(nblk((size_t)Ipad), (unsigned)Ipad), dim3(256), 0, ctx->stream, Ipad, d_G.p);
	HIPCHK(hipGetLastError());
	hipLaunchKernelGGL(k_resid_mirror, dim3(nblk((size_t)Ipad), (unsigned)Ipad), dim3(256), 0, ctx->stream, Ipad, d_V.p);
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(ctx->stream));
	/* the caller's arrays are written once everything on the device has succeeded */
	const size_t row = (size_t)I * sizeof(double), pitch = (size_t)Ipad * sizeof(double);
	HIPCHK(hipMemcpy2DAsync(gram, row, d_G.p, pitch, row, (size_t)I, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipMemcpy2DAsync(scale, row, d_V.p, pitch, row, (size_t)I, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	return MCHIP_OK;
}
