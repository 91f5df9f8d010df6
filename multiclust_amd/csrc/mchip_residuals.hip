/*
 * mchip_residuals.hip -- products of the admixture fit's residuals between individuals: mchip_residual_products and its kernels
 * (include/multiclust_hip.h has the contract and the definitions; mchip_context.h the per-context state).  The first analysis here
 * whose cost is quadratic in the individuals: I^2 T + 2 I^2 L multiply-adds, against the I T K of a pass over the data.
 *
 * The loci are cut into chunks on the host and the chunks' products run on the FP64 matrix unit: the cut, k_resid_gram and k_resid_mirror
 * are mchip_gram.h's, shared with mchip_kinship.hip.
 * Per chunk three launches; the two I^2 accumulators stay on the device from the first chunk to the last.
 *
 *   k_resid_tile   runtime K, one instance.  Lane = individual, as k_impute: a workgroup takes one block of 8 loci (the part of it
 *                  that lies in the chunk) and a tile of individuals; a lane reads its gtS group as aligned 64-bit words.  The q
 *                  rows sit in LDS lds_pitch(K) apart (mchip_device_util.h), the P rows of the block are staged when they fit
 *                  beside the q rows and read from memory when they do not (lane_pass_geometry_of, mchip_feature_geometry.h).  Per
 *                  locus: a = observed copies; per column t = sum_k q_k p_k by an fma chain in k order, r = fma(-a, t, n) (0 where
 *                  a = 0), s = fma(r, r, s) in m order.  Written as doubles, individual-contiguous: R [chunk column][Ipad], S and
 *                  O [chunk locus][Ipad]; Ipad = I rounded up to RES_TILE, the lanes behind I write zeros, so the product kernel
 *                  has no edge in the individual dimension.  Nothing is kept per allele: no private array.
 *   k_resid_gram   G += R^T R (SYM: the tiles on and above the diagonal) and D += S^T O (all tiles); k_resid_mirror at the end (mchip_gram.h).
 *   k_resid_diag   D[i][j] = G[i][i]: a data set without a missing copy has o = 1 everywhere, and D is defined as that there.
 *   No floating-point atomics; an element of G or D is owned by one lane of one workgroup from the first chunk to the last, and
 *   the order of its additions is the order of the columns: the same state gives the same bits on any device, under any knob.
 *
 *   Compile report (hipcc of ROCm 7.2, gfx950, -O3, -Rpass-analysis=kernel-resource-usage):  k_resid_tile 26 VGPRs, scratch 0,
 *   dynamic LDS only, 8 waves / SIMD;  k_resid_gram<true> and <false> 104 VGPRs + 32 AGPRs (the accumulators), scratch 0, 20480
 *   bytes of static LDS, 3 waves / SIMD;  k_resid_mirror and k_resid_diag 4 VGPRs.  Timed once, one A/B kept (the rows of the next
 *   stage fetched ahead: 600 -> 419 ms; 32 staged rows instead of 16: worse) and not tuned beyond it: at 10 000 x 100 000 the G kernel
 *   runs at 0.62 of the FP64 peak and D costs as much as G (profiles/resid.txt, scripts/resid_bench.py).
 */
#include "mchip_gram.h"

/* The loci [lbeg, lend) of one chunk, whose columns start at cbeg = toff[lbeg].  blockIdx.y: the block of 8 loci, counted from the
 * one lbeg lies in.  R [column - cbeg][Ipad], S and O [locus - lbeg][Ipad].  P is a slot's [T][K], Q its [I][K] (qstride = K) or
 * [K] (0). */
__global__ __launch_bounds__(256) void k_resid_tile(int I, int Ipad, int L, int pl, int K, int KS, int stage, int lbeg, int lend,
						    const uint8_t *__restrict__ gtS, const int32_t *__restrict__ toff,
						    const double *__restrict__ P, const double *__restrict__ Q, int qstride,
						    double *__restrict__ R, double *__restrict__ S, double *__restrict__ O)
{
	extern __shared__ __attribute__((aligned(16))) double res_lds[];
	double *qs = res_lds;					/* [blockDim.x][KS] */
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
		double *rout = R + (size_t)(cl - cbeg) * Ipad + i;
		double s = 0.0;
		for (int m = 0; m < M; m++) {
			double r = 0.0;
			if (a) {
				int n = 0;
				for (int x = 0; x < pl; x++) n += res_byte(gw, x0 + x) == (unsigned)m;
				const double *p = prow + (size_t)m * pstep;
				double t = 0.0;
				for (int k = 0; k < K; k++) t = fma(q[k], p[k], t);
				r = fma(-(double)a, t, (double)n);
				s = fma(r, r, s);
			}
			rout[(size_t)m * Ipad] = r;
		}
		S[(size_t)(l - lbeg) * Ipad + i] = s;
		O[(size_t)(l - lbeg) * Ipad + i] = a ? 1.0 : 0.0;
	}
}

/* D[i][j] = G[i][i]; grid (Ipad / 256, Ipad) */
__global__ __launch_bounds__(256) void k_resid_diag(int Ipad, const double *__restrict__ G, double *__restrict__ D)
{
	const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
	if (j < Ipad) D[(size_t)i * Ipad + j] = G[(size_t)i * Ipad + i];
}

extern "C" int mchip_residual_products(mchip_context *ctx, int slot, double *gram, double *norms)
{
	MCHIP_ENTRY();
	if (!ctx) return MCHIP_ERR_INVALID;
	int rc = require_fit(ctx, slot, "residuals: the prediction used is the admixture model's");
	if (rc) return rc;
	if (!gram) return fail(ctx, MCHIP_ERR_INVALID, "null pointer%s", nullptr);
	const int I = ctx->I, L = ctx->L, pl = ctx->ploidy, K = ctx->K;
	const int Ipad = (I + RES_TILE - 1) / RES_TILE * RES_TILE, nt = Ipad / RES_TILE;
	const size_t n2 = (size_t)Ipad * Ipad;
	HIPCHK(hipSetDevice(ctx->device));
	/* lanes per workgroup: a divisor of 256, at least RES_TILE; no reduction space; the blocks of a chunk are the grid's, not the geometry's */
	const lane_pass_geometry g = lane_pass_geometry_of(Ipad, L, K, ctx->max_M, ctx->n_cu, 0, RES_TILE, RES_LDS_BUDGET);
	if ((rc = check_lds(ctx, k_resid_tile, g.lds, "residuals: the kernel's static LDS has outgrown RES_LDS_BUDGET"))) return rc;
	std::vector<int> cut, width;	/* the chunks (mchip_gram.h): chunk ch is loci cut[ch] .. cut[ch + 1] - 1, width[ch] columns */
	res_cut_chunks(ctx->h_ua, L, cut, width);
	const bool want_d = norms != nullptr, d_by_product = want_d && ctx->has_missing;
	scoped_dev<double> d_G, d_D, d_R, d_S, d_O;
	if (d_G.alloc(n2) != hipSuccess || (want_d && d_D.alloc(n2) != hipSuccess) || d_R.alloc((size_t)RES_CHUNK * Ipad) != hipSuccess ||
	    d_S.alloc((size_t)RES_CHUNK * Ipad) != hipSuccess || d_O.alloc((size_t)RES_CHUNK * Ipad) != hipSuccess) {
		(void)hipGetLastError();
		return fail(ctx, MCHIP_ERR_ALLOC, "residuals: the I x I sums or the chunk buffers do not fit on the device%s", nullptr);
	}
	HIPCHK(hipMemsetAsync(d_G.p, 0, n2 * sizeof(double), ctx->stream));
	if (d_by_product) HIPCHK(hipMemsetAsync(d_D.p, 0, n2 * sizeof(double), ctx->stream));
	for (size_t ch = 0; ch + 1 < cut.size(); ch++) {
		const int lbeg = cut[ch], lend = cut[ch + 1];
		const int ncols = width[ch];
		const unsigned nblocks = (unsigned)((lend - 1) / RES_LBLOCK - lbeg / RES_LBLOCK + 1);
		hipLaunchKernelGGL(k_resid_tile, dim3((unsigned)g.n_itiles, nblocks), dim3((unsigned)g.threads), g.lds, ctx->stream, I, Ipad, L, pl, K, lds_pitch(K),
				   g.stage, lbeg, lend, ctx->d_gtS, ctx->d_toff, ctx->d_p[slot], ctx->d_q[slot], ctx->qstride, d_R.p, d_S.p, d_O.p);
		HIPCHK(hipGetLastError());
		if (ncols) {
			hipLaunchKernelGGL(k_resid_gram<true>, dim3((unsigned)nt, (unsigned)nt), dim3(256), 0, ctx->stream, Ipad, ncols, d_R.p, d_R.p, d_G.p);
			HIPCHK(hipGetLastError());
		}
		if (d_by_product) {
			hipLaunchKernelGGL(k_resid_gram<false>, dim3((unsigned)nt, (unsigned)nt), dim3(256), 0, ctx->stream, Ipad, lend - lbeg, d_S.p, d_O.p,
					   d_D.p);
			HIPCHK(hipGetLastError());
		}
	}
	hipLaunchKernelGGL(k_resid_mirror, dim3(nblk((size_t)Ipad), (unsigned)Ipad), dim3(256), 0, ctx->stream, Ipad, d_G.p);
	HIPCHK(hipGetLastError());
	if (want_d && !d_by_product) {
		hipLaunchKernelGGL(k_resid_diag, dim3(nblk((size_t)Ipad), (unsigned)Ipad), dim3(256), 0, ctx->stream, Ipad, d_G.p, d_D.p);
		HIPCHK(hipGetLastError());
	}
	HIPCHK(hipStreamSynchronize(ctx->stream));
	/* the caller's arrays are written once everything on the device has succeeded */
	const size_t row = (size_t)I * sizeof(double), pitch = (size_t)Ipad * sizeof(double);
	HIPCHK(hipMemcpy2DAsync(gram, row, d_G.p, pitch, row, (size_t)I, hipMemcpyDeviceToHost, ctx->stream));
	if (want_d) HIPCHK(hipMemcpy2DAsync(norms, row, d_D.p, pitch, row, (size_t)I, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	return MCHIP_OK;
}
