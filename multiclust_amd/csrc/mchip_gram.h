/*
 * mchip_gram.h -- what the units with an I x I sum over the allele columns share (mchip_residuals.hip, mchip_kinship.hip): the cut
 * of the loci into chunks, the FP64-MFMA product of a chunk's operand panels and the mirror of the upper triangle.  Private to
 * those units; every kernel here has internal linkage, so each unit carries its own copy of the code object and no symbol is
 * defined twice.
 *
 * The loci are cut into chunks on the host, from uniquealleles alone: whole loci, packed greedily, at most RES_CHUNK columns and
 * RES_CHUNK loci each -- constants, so the chunks and with them the order of every addition depend on the shape and nothing else.
 *
 *   res_gram_tile  out += X^T Y over the rows of a chunk with v_mfma_f64_16x16x4_f64.  A workgroup of four waves owns one
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
 *   k_resid_gram   one product a launch: grid (Ipad / RES_TILE)^2.
 *   k_gram_pair    two symmetric products a launch, out0 += X0^T X0 and out1 += X1^T X1: blockIdx.z selects the operand and the
 *                  output, the tile's work is res_gram_tile's either way -- an element's additions and their order are those of
 *                  two launches of k_resid_gram<true>, so are its bits; twice the workgroups are in flight.
 *   k_resid_mirror G[i][j] = G[j][i] for j < i, once at the end: the sum comes back symmetric bit for bit.
 *   No floating-point atomics; an element of out is owned by one lane of one workgroup from the first chunk to the last, and
 *   the order of its additions is the order of the columns: the same state gives the same bits on any device, under any knob.
 */
#ifndef MCHIP_GRAM_H
#define MCHIP_GRAM_H

#include "mchip_context.h"

#include <vector>

constexpr int RES_CHUNK = 512;		/* columns, and loci, per chunk at most (tests/test_gpu_resid.py restates it); > 255 = the most columns of a locus */
constexpr int RES_LBLOCK = LANE_PASS_LBLOCK;	/* loci per gtS group */
constexpr int RES_TILE = 64;		/* individuals per side of a workgroup's tile of G; I is padded to it */
constexpr int RES_DEPTH = 16;		/* rows of the operand panels in LDS at a time */
constexpr int RES_PITCH = RES_TILE + 16;	/* doubles between two staged rows: the two rows a half wave reads (k and k + 1, 16 doubles each)
						 * fall into different halves of the banks */
constexpr size_t RES_LDS_BUDGET = 64 * 1024 - 512;	/* dynamic LDS of the tile passes (checked with their static LDS at the launch) */

typedef double res_d4 __attribute__((ext_vector_type(4)));

/* byte x of a gtS group held as aligned 64-bit words */
__device__ __forceinline__ unsigned res_byte(const uint64_t *__restrict__ gw, int x)
{
	return (unsigned)(gw[x >> 3] >> ((x & 7) * 8)) & 0xFFu;
}

/* the chunks: whole loci, greedily, at most RES_CHUNK columns and RES_CHUNK loci each.  Chunk ch: loci cut[ch] .. cut[ch + 1] - 1,
 * width[ch] columns */
static inline void res_cut_chunks(const std::vector<int32_t> &ua, int L, std::vector<int> &cut, std::vector<int> &width)
{
	cut.assign(1, 0);
	width.clear();
	int cols = 0;
	for (int l = 0; l < L; l++) {
		const int M = ua[(size_t)l];
		if (l > cut.back() && (cols + M > RES_CHUNK || l - cut.back() >= RES_CHUNK)) {
			cut.push_back(l);
			width.push_back(cols);
			cols = 0;
		}
		cols += M;
	}
	cut.push_back(L);
	width.push_back(cols);
}

/* the tile (bi, bj) of out [Ipad][Ipad] += X^T Y over rows 0 .. nrows - 1 of X and Y [nrows][Ipad]; 256 threads, all of them call it.
 * bi = tile row (index of X's individual), bj = tile column. */
template <bool SYM>
__device__ __forceinline__ void res_gram_tile(int Ipad, int nrows, const double *__restrict__ X, const double *__restrict__ Y,
					      double *__restrict__ out, int bi, int bj)
{
	__shared__ __attribute__((aligned(16))) double xs[RES_DEPTH * RES_PITCH], ys[RES_DEPTH * RES_PITCH];
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

/* out [Ipad][Ipad] += X^T Y; grid (Ipad / RES_TILE)^2, 256 threads.  blockIdx.y = tile row bi, blockIdx.x = tile column bj. */
template <bool SYM>
static __global__ __launch_bounds__(256) void k_resid_gram(int Ipad, int nrows, const double *__restrict__ X, const double *__restrict__ Y,
							   double *__restrict__ out)
{
	res_gram_tile<SYM>(Ipad, nrows, X, Y, out, (int)blockIdx.y, (int)blockIdx.x);
}

/* out0 += X0^T X0 (blockIdx.z = 0) and out1 += X1^T X1 (blockIdx.z = 1), the tiles on and above the diagonal; grid
 * (Ipad / RES_TILE, Ipad / RES_TILE, 2), 256 threads.  The two outputs and the two panels are four different arrays. */
static __global__ __launch_bounds__(256) void k_gram_pair(int Ipad, int nrows, const double *__restrict__ X0, double *__restrict__ out0,
							  const double *__restrict__ X1, double *__restrict__ out1)
{
	const bool second = blockIdx.z != 0;	/* (uniform over the workgroup) */
	const double *X = second ? X1 : X0;
	res_gram_tile<true>(Ipad, nrows, X, X, second ? out1 : out0, (int)blockIdx.y, (int)blockIdx.x);
}

/* G[i][j] = G[j][i] for j < i; grid (Ipad / 256, Ipad) */
static __global__ __launch_bounds__(256) void k_resid_mirror(int Ipad, double *__restrict__ G)
{
	const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
	if (j < i) G[(size_t)i * Ipad + j] = G[(size_t)j * Ipad + i];
}

#endif
