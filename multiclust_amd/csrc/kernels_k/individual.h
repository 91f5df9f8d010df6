/* kernels_k/individual.h -- the individual passes (S-side sums) without an LDS tile: dense, and every locus biallelic */
#ifndef MCHIP_KERNELS_K_INDIVIDUAL_H
#define MCHIP_KERNELS_K_INDIVIDUAL_H

#include "kernels_k/common.h"

namespace {

/* ---------------------------------------------------------------- individual pass */
template <int PL>
__global__ __launch_bounds__(QBLOCK) void k_individual_pass(mchip_pass_args a)
{
	if (a.stop && *a.stop) return;		/* batched run already stopped (wave-uniform) */
	if (a.skip_ind && *a.skip_ind) return;	/* sums of these parameters are already in Spart */
	const int i_raw = blockIdx.x * QBLOCK + threadIdx.x;
	const bool active = i_raw < a.I;
	const int i = active ? i_raw : a.I - 1;
	const int pl = PL ? PL : a.ploidy;
	double q[K], acc[K];
#pragma unroll
	for (int k = 0; k < K; k++) {
		q[k] = a.Q[(size_t)i * a.qstride + k];
		acc[k] = 0.0;
	}
	const int l0 = blockIdx.y * a.lchunk;
	const int l1 = min(a.L, l0 + a.lchunk);
	const int lb_end = (l1 + 7) >> 3;
	geno_group<PL> g, gn;
	g.load(a.gtS, (size_t)(l0 >> 3) * a.I + i, pl);
	for (int lb = l0 >> 3; lb < lb_end; lb++) {
		gn.load(a.gtS, (size_t)min(lb + 1, lb_end - 1) * a.I + i, pl);
#pragma unroll
		for (int j = 0; j < 8; j++) {
			const int l = lb * 8 + j;
			if (l >= l1) break;			/* wave-uniform */
			const int c0 = a.toff[l];
			const int M = a.ua[l];
			/* columns of one locus: P rows are contiguous ([T][K]); the next column's row is requested
			 * (scalar loads) before this column's arithmetic so its latency hides under it */
			double pn[K];
#pragma unroll
			for (int k = 0; k < K; k++) pn[k] = a.P[(size_t)c0 * K + k];
			for (int m = 0; m < M; m++) {
				double pc[K];
#pragma unroll
				for (int k = 0; k < K; k++) pc[k] = pn[k];
				const int cn = min(c0 + m + 1, a.T - 1);
#pragma unroll
				for (int k = 0; k < K; k++) pn[k] = a.P[(size_t)cn * K + k];
				const int n = active ? g.count(j, (unsigned)m, pl) : 0;
				if (__ballot(n > 0) == 0ull) continue;	/* nobody in this wave carries allele m */
				double t = q[0] * pc[0];
#pragma unroll
				for (int k = 1; k < K; k++) t = __builtin_fma(q[k], pc[k], t);
				const double r = n ? (double)n * rcp_full(t) : 0.0;	/* lanes that do not carry m: exactly 0, also when t = 0 */
#pragma unroll
				for (int k = 0; k < K; k++) acc[k] = __builtin_fma(pc[k], r, acc[k]);
			}
		}
		g = gn;
	}
	if (active) {
		double *out = a.Spart + ((size_t)blockIdx.y * a.I + i) * K;
#pragma unroll
		for (int k = 0; k < K; k++) out[k] = acc[k];
	}
}

/* ---------------------------------------------------------------- individual pass, every locus biallelic (SNP data)
 * When every locus has exactly two allele columns (diploid data without missing-data phantom slots) column c of locus l is
 * 2l + m and the two rows of a locus are wave-uniform: they come through the scalar cache as SGPR operands of the FMAs, no
 * LDS tile, no per-lane gather.  Both alleles' t are computed for every individual (2K FMAs, the same count as two copies),
 * the genotype only selects which of them enter the log-product, and the S-side sums take P_0 n_0/t_0 + P_1 n_1/t_1 with one
 * reciprocal.  The stand-alone log-likelihood pass, LDS-bound in the general kernel, becomes FP64-bound here. */
template <bool ACCUM, bool NOMISS>
__global__ __launch_bounds__(64 * MCHIP_IND_WAVES_MAX) void k_individual_bial(mchip_pass_args a)
{
	if (a.stop && *a.stop) return;		/* batched run already stopped (uniform over the grid) */
	if (ACCUM && a.skip_ind && *a.skip_ind) return;
	/* cooperating waves, as k_individual_sparse_w: a.ind_waves waves over the same 64 individuals, wave w at sub-chunk w */
	__shared__ double xch[K + 1][64];
	const int lane = threadIdx.x & 63;
	const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	const int W = a.ind_waves;
	const int i_raw = blockIdx.x * 64 + lane;
	const bool active = i_raw < a.I;
	const int i = active ? i_raw : a.I - 1;
	double q[K], acc[K];
#pragma unroll
	for (int k = 0; k < K; k++) {
		q[k] = a.Q[(size_t)i * a.qstride + k];
		acc[k] = 0.0;
	}
	const int l0raw = (int)(blockIdx.y * W + wv) * a.lchunk;
	const bool any = l0raw < a.L;		/* (wave-uniform; a trailing wave of the last workgroup may have nothing: empty loop) */
	const int l0 = any ? l0raw : 0;
	const int l1 = any ? min(a.L, l0 + a.lchunk) : 0;
	const int lb0 = l0 >> 3, lb_end = any ? (l1 + 7) >> 3 : lb0;
	double prod = 1.0;
	int blk = 0, ex = 0;
	geno_group<2> g, gn;
	g.load(a.gtS, (size_t)lb0 * a.I + i, 2);
	for (int lb = lb0; lb < lb_end; lb++) {
		gn.load(a.gtS, (size_t)min(lb + 1, lb_end - 1) * a.I + i, 2);
		const int nloc = l1 - lb * 8;
#pragma unroll
		for (int j = 0; j < 8; j++) {
			if (j < nloc) {		/* wave-uniform */
				const double *__restrict__ r0 = a.P + (size_t)(lb * 8 + j) * 2 * K;	/* rows 2l, 2l+1: wave-uniform, s_load */
				double t0 = q[0] * r0[0], t1 = q[0] * r0[K];
#pragma unroll
				for (int k = 1; k < K; k++) {
					t0 = __builtin_fma(q[k], r0[k], t0);
					t1 = __builtin_fma(q[k], r0[K + k], t1);
				}
				const unsigned ma = g.copy(j, 0, 2), mb = g.copy(j, 1, 2);
				double ta, tb;
				if (NOMISS) {		/* idle lanes duplicate individual I-1 and are dropped at the end */
					ta = ma ? t1 : t0;
					tb = mb ? t1 : t0;
				} else {		/* a missing copy (0xFF) leaves the product alone */
					ta = !active ? 1.0 : (ma == 0u ? t0 : (ma == 1u ? t1 : 1.0));
					tb = !active ? 1.0 : (mb == 0u ? t0 : (mb == 1u ? t1 : 1.0));
				}
				if (ACCUM) {
					const double rp = rcp_full(t0 * t1);
					const double n0 = (double)((int)(ma == 0u) + (int)(mb == 0u)), n1 = (double)((int)(ma == 1u) + (int)(mb == 1u));
					const double R0 = n0 * (rp * t1), R1 = n1 * (rp * t0);
#pragma unroll
					for (int k = 0; k < K; k++) {
						acc[k] = __builtin_fma(r0[k], R0, acc[k]);
						acc[k] = __builtin_fma(r0[K + k], R1, acc[k]);
					}
				}
				prod *= ta * tb;
			}
		}
		if (++blk >= a.flush_blocks) {
			blk = 0;
			rescale(prod, ex);
		}
		g = gn;
	}
	double ll = (double)ex * 0.693147180559945309417 + log(prod);
	for (int x = 1; x < W; x++) {	/* waves 1 .. W-1 hand their sums to wave 0, in wave order */
		if (wv == x) {
#pragma unroll
			for (int k = 0; k < K; k++) xch[k][lane] = acc[k];
			xch[K][lane] = ll;
		}
		__syncthreads();
		if (wv == 0) {
#pragma unroll
			for (int k = 0; k < K; k++) acc[k] += xch[k][lane];
			ll += xch[K][lane];
		}
		__syncthreads();
	}
	if (wv == 0) {
		if (ACCUM && active) {
			double *out = a.Spart + ((size_t)blockIdx.y * a.I + i) * K;
#pragma unroll
			for (int k = 0; k < K; k++) out[k] = acc[k];
		}
		const double tot = wave_total(active ? ll : 0.0);
		if (lane == 0) a.llpart[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = tot;
	}
}

}  // namespace

#endif
