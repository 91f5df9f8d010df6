/* kernels_k/finalize_q.h -- the Q-side finalisers: slab sums, normalisation and projection of the mixing proportions */
#ifndef MCHIP_KERNELS_K_FINALIZE_Q_H
#define MCHIP_KERNELS_K_FINALIZE_Q_H

#include "kernels_k/common.h"
#include "mchip_finalize.h"

namespace {

/* ---------------------------------------------------------------- simplex.c:109-143 on K registers */
__device__ __forceinline__ void michelot_k(double (&x)[K], double mn)
{
	unsigned long long fixed = 0;
	int n = K;
	while (n) {
		double csum = 0.0;
#pragma unroll
		for (int j = 0; j < K; j++) csum += x[j];
		const double shift = (csum - 1.0) / (double)n;
		bool can_terminate = true;
#pragma unroll
		for (int j = 0; j < K; j++)
			if (!((fixed >> j) & 1ull)) {
				x[j] -= shift;
				if (x[j] < mn) {
					x[j] = mn;
					fixed |= 1ull << j;
					n--;
					can_terminate = false;
				}
			}
		if (can_terminate) break;
	}
}

/* Q[to][i][.] = normalise(q_ik * sum_chunks Spart) then project (em_alg.c:685-701); also stores the
 * expected counts S_ik the writers need (write_file.c:359-381). */
constexpr int FQ_LANES = 8, FQ_IND = MCHIP_BLOCK / FQ_LANES;	/* threads per individual / individuals per block of k_finalize_q */
constexpr int FQ_XCH = (K <= 16 ? FQ_LANES - 1 : 1) * K * FQ_IND;	/* doubles of LDS a block exchanges its partial sums through */
__device__ __forceinline__ void finalize_q_body(int block, double *xch_raw, int I, int n_lchunks, const double *__restrict__ Spart,
		const double *__restrict__ Qfrom, int qstride_from, double *Qto, double *sik,
		int do_mstep, int weighted, int do_projection, double lb, double add)
{
	/* FQ_IND individuals per block, FQ_LANES threads each: thread g of an individual adds slabs g, g + 8, ... (four loads in
	 * flight at a time), the partial sums meet in LDS in the order g = 0 .. 7, and thread 0 of the individual carries on.  Every
	 * slab count is handled here: there is no separate slab-sum launch in front (k_sum_slabs took this scheme's place) */
	constexpr int TURNS = K <= 16 ? 1 : FQ_LANES - 1;	/* K <= 16: all partial sums at once (28 KB of LDS at most); above: in turns */
	double (*xch)[K][FQ_IND] = reinterpret_cast<double (*)[K][FQ_IND]>(xch_raw);	/* [K <= 16 ? FQ_LANES - 1 : 1][K][FQ_IND] */
	const int il = threadIdx.x % FQ_IND, g = threadIdx.x / FQ_IND;
	const int i = block * FQ_IND + il;
	const bool active = i < I;
	double s[K];
#pragma unroll
	for (int k = 0; k < K; k++) s[k] = 0.0;
	if (active) {
		const size_t row = (size_t)I * K;
		const double *src = Spart + (size_t)g * row + (size_t)i * K;
		int ch = g;
		for (; ch + 3 * FQ_LANES < n_lchunks; ch += 4 * FQ_LANES, src += 4 * FQ_LANES * row) {
			double v[4][K];
#pragma unroll
			for (int y = 0; y < 4; y++)
#pragma unroll
				for (int k = 0; k < K; k++) v[y][k] = src[(size_t)y * FQ_LANES * row + k];
#pragma unroll
			for (int y = 0; y < 4; y++)
#pragma unroll
				for (int k = 0; k < K; k++) s[k] += v[y][k];
		}
		for (; ch < n_lchunks; ch += FQ_LANES, src += FQ_LANES * row) {
#pragma unroll
			for (int k = 0; k < K; k++) s[k] += src[k];
		}
	}
	if constexpr (TURNS == 1) {
		if (g) {
#pragma unroll
			for (int k = 0; k < K; k++) xch[g - 1][k][il] = s[k];
		}
		__syncthreads();
		if (g == 0) {
#pragma unroll
			for (int x = 0; x < FQ_LANES - 1; x++)
#pragma unroll
				for (int k = 0; k < K; k++) s[k] += xch[x][k][il];
		}
	} else {
		for (int x = 1; x < FQ_LANES; x++) {
			if (g == x) {
#pragma unroll
				for (int k = 0; k < K; k++) xch[0][k][il] = s[k];
			}
			__syncthreads();
			if (g == 0) {
#pragma unroll
				for (int k = 0; k < K; k++) s[k] += xch[0][k][il];
			}
			__syncthreads();
		}
	}
	if (g || !active) return;
	if (weighted) {
#pragma unroll
		for (int k = 0; k < K; k++) s[k] *= Qfrom[(size_t)i * qstride_from + k];
	}
#pragma unroll
	for (int k = 0; k < K; k++) sik[(size_t)i * K + k] = s[k];
	if (!do_mstep) return;
	double temp = 0.0;
#pragma unroll
	for (int k = 0; k < K; k++) {
		s[k] += add;		/* 0, or the 1 every count of initialize_parameters_admixture starts from (rnd_init.c:624) */
		temp += s[k];
	}
	if (temp == 0.0) {
		/* no observed copy at all: 0 / 0 in the reference.  A finite row is kept here (mchip_get_q reports it as the reference has
		 * it); everything this individual's row is multiplied into carries a zero count */
#pragma unroll
		for (int k = 0; k < K; k++) Qto[(size_t)i * K + k] = 1.0 / K;
		return;
	}
#pragma unroll
	for (int k = 0; k < K; k++) s[k] /= temp;
	if (do_projection) michelot_k(s, lb);
#pragma unroll
	for (int k = 0; k < K; k++) Qto[(size_t)i * K + k] = s[k];
}
__global__ __launch_bounds__(MCHIP_BLOCK) void k_finalize_q(int I, int n_lchunks, const double *__restrict__ Spart,
		const double *__restrict__ Qfrom, int qstride_from, double *Qto, double *sik,
		int do_mstep, int weighted, int do_projection, double lb, const int *stop, double add)
{
	__shared__ double xch[FQ_XCH];
	if (stop && *stop) return;		/* (uniform over the grid) */
	finalize_q_body(blockIdx.x, xch, I, n_lchunks, Spart, Qfrom, qstride_from, Qto, sik, do_mstep, weighted, do_projection, lb, add);
}
/* Both finalisers of an EM step in ONE launch: blocks 0 .. q_blocks-1 are k_finalize_q's, the others k_finalize_p_tile's
 * (mchip_finalize.h).  The two read different sums and write different parameters; a small data set's step is five launches of
 * a few microseconds around its two passes, and this is one of them less (and the two run beside each other).  Same bodies,
 * same bits as the two launches. */
__global__ __launch_bounds__(MCHIP_BLOCK) void k_finalize_qp(int q_blocks, int I, int n_lchunks, const double *__restrict__ Spart,
		const double *__restrict__ Qfrom, int qstride_from, double *Qto, double *sik,
		int do_projection_q, double lb_q, mchip_finalize_p_args p, const int *stop)
{
	__shared__ double lds[FQ_XCH > FP_TILE ? FQ_XCH : FP_TILE];
	if (stop && *stop) return;		/* (uniform over the grid) */
	if ((int)blockIdx.x < q_blocks)		/* (uniform over the block) */
		finalize_q_body(blockIdx.x, lds, I, n_lchunks, Spart, Qfrom, qstride_from, Qto, sik, 1, 1, do_projection_q, lb_q, 0.0);
	else
		finalize_p_tile_body((int)blockIdx.x - q_blocks, lds, p.L, p.K, p.T, p.toff, p.loci_per_block, p.n_slabs, p.Apart, p.Pfrom, p.Pto,
				     p.weighted, p.add_lb, p.do_projection, p.lb);
}

/* projection of nrows rows of K (accelerated updates, accel_em.c:510-511; shared eta row) */
__global__ __launch_bounds__(MCHIP_BLOCK) void k_project_q(int nrows, double *Q, double lb, const int *stop)
{
	const int i = blockIdx.x * MCHIP_BLOCK + threadIdx.x;
	if (i >= nrows || (stop && *stop)) return;
	double s[K];
#pragma unroll
	for (int k = 0; k < K; k++) s[k] = Q[(size_t)i * K + k];
	michelot_k(s, lb);
#pragma unroll
	for (int k = 0; k < K; k++) Q[(size_t)i * K + k] = s[k];
}

}  // namespace

#endif
