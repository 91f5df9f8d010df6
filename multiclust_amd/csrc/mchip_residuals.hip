/*
 * mchip_residuals.hip -- products of the admixture fit's residuals between individuals: mchip_residual_products and its kernels
 * (include/multiclust_hip.h has the contract and the definitions; mchip_context.h the per-context state).  The first analysis here
 * whose cost is quadratic in the individuals: I^2 T + 2 I^2 L multiply-adds, against the I T K of a pass over the data.
 *
 * The loci are cut into chunks on the host, from uniquealleles alone: whole loci, packed greedily, at most RES_CHUNK columns and
 * RES_CHUNK loci each -- constants, so the chunks and with them the order of every addition depend on the shape and nothing else.
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
 *   k_resid_gram   out += X^T Y over the rows of a chunk with v_mfma_f64_16x16x4_f64.  A workgroup of four waves owns one
 *                  RES_TILE x RES_TILE tile of out, each wave a 32 x 32 quarter as 2 x 2 accumulators of 16 x 16 (16 doubles a
 *                  lane).  It loads the accumulators from out, walks the chunk's rows in order -- RES_DEPTH rows of the two operand
 *                  panels staged in LDS at a time, four rows per instruction, the rows of the next stage on their way from memory
 *                  into registers meanwhile -- and stores them back.  Rows behind the chunk's last are staged as zeros: a tail
 *                  that is no multiple of 4 (or of RES_DEPTH) costs no branch in the product loop.
 *                  A: lane holds X[k = lane >> 4][row = lane & 15], B likewise from Y; C/D: col = lane & 15, row = (lane >> 4) +
 *                  4 reg.  Every staged double feeds two instructions of each of two waves.
 *                  SYM = true (G += R^T R): only the tiles on and above the diagonal run; SYM = false (D += S^T O): all of them.
 *                  FP64 MFMA has the vector units' peak on this chip: what the instruction buys here is operand reuse -- one
 *                  LDS read per 16 multiply-adds of a lane instead of one per multiply-add -- not flops.
 *   k_resid_mirror G[i][j] = G[j][i] for j < i, once at the end: gram comes back symmetric bit for bit.
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
#include "mchip_context.h"

#include <vector>

constexpr int RES_CHUNK = 512;		/* columns, and loci, per chunk at most (tests/test_gpu_resid.py restates it); > 255 = the most columns of a locus */
constexpr int RES_LBLOCK = LANE_PASS_LBLOCK;	/* loci per gtS group */
constexpr int RES_TILE = 64;		/* individuals per side of a workgroup's tile of G; I is padded to it */
constexpr int RES_DEPTH = 16;		/* rows of the operand panels in LDS at a time */
constexpr int RES_PITCH = RES_TILE + 16;	/* doubles between two staged rows: the two rows a half wave reads (k and k + 1, 16 doubles each)
						 * fall into different halves of the banks */
constexpr size_t RES_LDS_BUDGET = 64 * 1024 - 512;	/* dynamic LDS of k_resid_tile (checked with its static LDS at the launch) */

typedef double res_d4 __attribute__((ext_vector_type(4)));

/* byte x of a gtS group held as aligned 64-bit words */
__device__ __forceinline__ unsigned res_byte(const uint64_t *__restrict__ gw, int x)
{
	return (unsigned)(gw[x >> 3] >> ((x & 7) * 8)) & 0xFFu;
}

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

/* out [Ipad][Ipad] += X^T Y over rows 0 .. nrows - 1 of X and Y [nrows][Ipad]; grid (Ipad / RES_TILE)^2, 256 threads.
 * blockIdx.y = tile row bi (index of X's individual), blockIdx.x = tile column bj. */
template <bool SYM>
__global__ __launch_bounds__(256) void k_resid_gram(int Ipad, int nrows, const double *__restrict__ X, const double *__restrict__ Y,
						    double *__restrict__ out)
{
	__shared__ __attribute__((aligned(16))) double xs[RES_DEPTH * RES_PITCH], ys[RES_DEPTH * RES_PITCH];
	const int bi = blockIdx.y, bj = blockIdx.x;
	if (SYM && bi > bj) return;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32;		/* the wave's quarter of the tile */
	const int lr = lane & 15, lk = lane >> 4;
	res_d4 acc[2][2];
	double *obase = out + (size_t)(bi * RES_TILE + wi + lk) * Ipad + (size_t)bj * RES_TILE + wj + lr;
#pragma unroll
	for (int ti = 0; ti < 2; ti++)
#pragma unroll
		for (int tj = 0; tj < 2; tj++)
#pragma unroll
			for (int r = 0; r < 4; r++) acc[ti][tj][r] = obase[(size_t)(ti * 16 + 4 * r) * Ipad + tj * 16];
	const int srow = tid >> 6, scol = tid & 63;	/* staging: thread t loads column t & 63 of rows t >> 6, + 4, + 8, + 12 */
	const double *xg = X + (size_t)bi * RES_TILE + scol, *yg = Y + (size_t)bj * RES_TILE + scol;
	/* the rows of the next stage travel from memory into registers while the products of this one run */
	double px[RES_DEPTH / 4], py[RES_DEPTH / 4];
	auto fetch = [&](int c0) {
#pragma unroll
		for (int x = 0; x < RES_DEPTH / 4; x++) {
			const int c = c0 + srow + 4 * x;
			const bool in = c < nrows;
			px[x] = in ? xg[(size_t)c * Ipad] : 0.0;
			py[x] = in ? yg[(size_t)c * Ipad] : 0.0;
		}
	};
	fetch(0);
	for (int c0 = 0; c0 < nrows; c0 += RES_DEPTH) {
		__syncthreads();	/* everybody is done with the rows staged before */
#pragma unroll
		for (int x = 0; x < RES_DEPTH / 4; x++) {
			xs[(srow + 4 * x) * RES_PITCH + scol] = px[x];
			ys[(srow + 4 * x) * RES_PITCH + scol] = py[x];
		}
		__syncthreads();
		fetch(c0 + RES_DEPTH);	/* (behind the last stage: zeros, no load) */
#pragma unroll
		for (int kk = 0; kk < RES_DEPTH; kk += 4) {
			const double *xr = xs + (kk + lk) * RES_PITCH + wi + lr, *yr = ys + (kk + lk) * RES_PITCH + wj + lr;
			const double a0 = xr[0], a1 = xr[16], b0 = yr[0], b1 = yr[16];
			acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
			acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
			acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
			acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
		}
	}
#pragma unroll
	for (int ti = 0; ti < 2; ti++)
#pragma unroll
		for (int tj = 0; tj < 2; tj++)
#pragma unroll
			for (int r = 0; r < 4; r++) obase[(size_t)(ti * 16 + 4 * r) * Ipad + tj * 16] = acc[ti][tj][r];
}

/* G[i][j] = G[j][i] for j < i; grid (Ipad / 256, Ipad) */
__global__ __launch_bounds__(256) void k_resid_mirror(int Ipad, double *__restrict__ G)
{
	const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
	if (j < i) G[(size_t)i * Ipad + j] = G[(size_t)j * Ipad + i];
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
	/* the chunks: whole loci, greedily, at most RES_CHUNK columns and RES_CHUNK loci each */
	std::vector<int> cut(1, 0), width;	/* chunk ch: loci cut[ch] .. cut[ch + 1] - 1, width[ch] columns */
	int cols = 0;
	for (int l = 0; l < L; l++) {
		const int M = ctx->h_ua[(size_t)l];
		if (l > cut.back() && (cols + M > RES_CHUNK || l - cut.back() >= RES_CHUNK)) {
			cut.push_back(l);
			width.push_back(cols);
			cols = 0;
		}
		cols += M;
	}
	cut.push_back(L);
	width.push_back(cols);
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
