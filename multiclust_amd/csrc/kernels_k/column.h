/* kernels_k/column.h -- the column passes (N-side sums): dense, on packed counts, and with the k range split over lanes */
#ifndef MCHIP_KERNELS_K_COLUMN_H
#define MCHIP_KERNELS_K_COLUMN_H

#include "kernels_k/common.h"

namespace {

/* ---------------------------------------------------------------- column pass */
/* SAFE = false: the log-product is checked once per `flush_blocks` blocks of 8 individuals (host guarantees that
 * 8*ploidy*flush_blocks multiplications cannot underflow a product that starts above 1e-100);
 * SAFE = true: checked after every individual (tiny lower bounds, projection disabled, high ploidy). */
template <int PL, bool ACCUM, bool SAFE, bool LL>
__global__ __launch_bounds__(MCHIP_BLOCK) void k_column_pass(mchip_pass_args a)
{
	if (a.stop && *a.stop) return;		/* batched run already stopped (wave-uniform) */
	__shared__ double red[MCHIP_BLOCK];
	const int c_raw = blockIdx.x * MCHIP_BLOCK + threadIdx.x;
	const bool valid = c_raw < a.T;
	const int c = valid ? c_raw : a.T - 1;
	const int l = a.col_locus[c];
	const unsigned m = valid ? (unsigned)a.col_allele[c] : 0xFEu;	/* 0xFE never matches a genotype byte */
	const int pl = PL ? PL : a.ploidy;

	double p[K], acc[K];
#pragma unroll
	for (int k = 0; k < K; k++) {
		p[k] = a.P[(size_t)c * K + k];
		acc[k] = 0.0;
	}
	const int i0 = blockIdx.y * a.ichunk;
	const int i1 = min(a.I, i0 + a.ichunk);
	const int ib_end = (i1 + 7) >> 3;
	double ll = 0.0, prod = 1.0;
	int blk = 0;

	geno_group<PL> g, gn;
	g.load(a.gtA, (size_t)(i0 >> 3) * a.L + l, pl);
	for (int ib = i0 >> 3; ib < ib_end; ib++) {
		/* software prefetch of the next group (clamped: the last iteration re-reads its own group) */
		gn.load(a.gtA, (size_t)min(ib + 1, ib_end - 1) * a.L + l, pl);
		/* two halves of four individuals: four q rows (4*2K SGPRs) in flight at a time; unrolling all
		 * eight makes hipcc hoist eight s_load_dwordx16 and spill SGPRs through v_writelane */
#pragma unroll 1
		for (int h = 0; h < 2; h++) {
			const geno_group<PL> gh = g.half(h);
#pragma unroll
			for (int j = 0; j < 4; j++) {
				const int i = min(ib * 8 + h * 4 + j, a.I - 1);	/* padded individuals carry 0xFF bytes: n = 0 */
				const double *__restrict__ q = a.Q + (size_t)i * a.qstride;	/* wave-uniform: s_load */
				const int n = gh.count(j, m, pl);
				double t = q[0] * p[0];
#pragma unroll
				for (int k = 1; k < K; k++) t = __builtin_fma(q[k], p[k], t);
				if (ACCUM) {
					/* a zero-count cell contributes exactly 0 whatever t is (em_alg.c:338-342): a column whose P is 0 for
					 * every k (projection off) has t = 0 and 0 * (1/0) would be NaN */
					const double r = n ? (double)n * rcp_full(t) : 0.0;
#pragma unroll
					for (int k = 0; k < K; k++) acc[k] = __builtin_fma(q[k], r, acc[k]);
				}
				/* n log t as log of a product: t^n.  SAFE (projection off): a negative t in a cell that carries copies is
				 * NaN in the reference's log and must not square itself away in a homozygote (found on a 36-allele locus:
				 * tests/test_gpu_cli_differential.py) */
				if (LL) {
					const double tl = (SAFE && t < 0.0) ? __builtin_nan("") : t;
					if (PL == 2) {
						prod *= (n >= 1) ? tl : 1.0;
						prod *= (n >= 2) ? tl : 1.0;
					} else {
						for (int b = 1; b <= pl; b++) prod *= (n >= b) ? tl : 1.0;
					}
				}
				if (LL && SAFE) {
					if (prod < 1e-100) {
						ll += log(prod);
						prod = 1.0;
					}
				}
			}
		}
		if (LL && !SAFE) {
			if (++blk >= a.flush_blocks) {
				blk = 0;
				if (prod < 1e-100) {
					ll += log(prod);
					prod = 1.0;
				}
			}
		}
		g = gn;
	}
	if (ACCUM && valid) {
		double *out = a.Apart + ((size_t)blockIdx.y * a.T + c) * K;
#pragma unroll
		for (int k = 0; k < K; k++) out[k] = acc[k];
	}
	if (LL) {
		ll += log(prod);
		const double tot = block_tree_sum<MCHIP_BLOCK>(red, ll);
		if (threadIdx.x == 0) a.llpart[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = tot;
	}
}

/* ---------------------------------------------------------------- column pass on packed allele counts
 * gtC[g][c] is one 16-byte word per (group of G = 128/BITS individuals, allele column): BITS-bit counts
 * n_ic = ILM[i][l][m] (BITS = 2 for ploidy <= 3, 4 for ploidy <= 15).  One coalesced 16-byte load per lane serves G
 * individuals and the count is a single v_bfe_u32, instead of two byte compares, a select and an add per cell.
 * MIX = false: admixture N-side sums  acc_k += q_ik * n / t;   MIX = true: mixture M step  acc_k += vik * n. */
/* The body: workgroup (bx, by) of counts_grid(); wsum is [K][64] doubles of LDS.  k_column_counts runs it on its own grid,
 * k_estep_pair beside the S-side pass's body. */
template <int BITS, bool MIX, bool SAFE>
__device__ __forceinline__ void column_counts_body(const mchip_pass_args &a, const int bx, const int by, double (*wsum)[64])
{
	constexpr int PERWORD = 32 / BITS;		/* individuals per dword */
	constexpr int G = 4 * PERWORD;			/* individuals per 16-byte word */
	constexpr unsigned MASK = (1u << BITS) - 1u;
	/* individuals per inner step: their q rows must fit the scalar register file (2K SGPRs each, about 100 usable) */
	constexpr int NJ = K <= 12 ? 4 : (K <= 20 ? 2 : 1);
	/* the workgroup's MCHIP_COL_WAVES waves take the same 64 allele columns and consecutive sub-chunks of a.ichunk individuals;
	 * their sums meet in LDS below, in wave order, and wave 0 stores the slab (mchip_internal.h: cooperating waves) */
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;	/* wv is wave-uniform */
	const int c_raw = bx * 64 + lane;
	const bool valid = c_raw < a.T;
	const int c = valid ? c_raw : a.T - 1;
	double p[K], acc[K];
#pragma unroll
	for (int k = 0; k < K; k++) {
		p[k] = MIX ? 0.0 : a.P[(size_t)c * K + k];
		acc[k] = 0.0;
	}
	const int i0 = __builtin_amdgcn_readfirstlane((by * MCHIP_COL_WAVES + wv) * a.ichunk);	/* multiple of G */
	const int i1 = min(a.I, i0 + a.ichunk);
	const int g_end = (i1 + G - 1) / G;		/* (a wave whose sub-chunk starts behind the last individual has no groups) */
	const uint4 *gt = reinterpret_cast<const uint4 *>(a.gtC);
	/* (the q rows are read through the constant address space: Q does not change while a kernel runs, and in k_estep_pair the
	 * clock reading in front of this body is opaque to hipcc -- it would otherwise assume that it may have written Q and read
	 * the rows through the vector memory path into 64 more registers at K = 8) */
	typedef __attribute__((address_space(4))) double const_double;
	const const_double *Qc = (const const_double *)a.Q;
	uint4 w = gt[(size_t)min(i0 / G, (a.I - 1) / G) * a.T + c];
	for (int g = i0 / G; g < g_end; g++) {
		const uint4 wn = gt[(size_t)min(g + 1, g_end - 1) * a.T + c];	/* prefetch (clamped) */
#pragma unroll 1
		for (int wi = 0; wi < 4; wi++) {
			unsigned word = (wi == 0) ? w.x : (wi == 1) ? w.y : (wi == 2) ? w.z : w.w;
#pragma unroll 1
			for (int h = 0; h < PERWORD / NJ; h++) {
				const int ibase = g * G + wi * PERWORD + h * NJ;
				if (ibase >= i1) break;		/* wave-uniform; padded individuals have zero counts anyway */
				/* NJ individuals at a time: their q rows are wave-uniform (scalar loads, used as SGPR operands) */
				const const_double *q[NJ];
				double n[NJ], t[NJ], rc[NJ];
#pragma unroll
				for (int j = 0; j < NJ; j++) {
					q[j] = Qc + (size_t)min(ibase + j, a.I - 1) * a.qstride;
					n[j] = (double)((word >> (BITS * j)) & MASK);
				}
				if (!MIX) {
#pragma unroll
					for (int j = 0; j < NJ; j++) {
						t[j] = q[j][0] * p[0];
#pragma unroll
						for (int k = 1; k < K; k++) t[j] = __builtin_fma(q[j][k], p[k], t[j]);
					}
					if (SAFE) {
						/* projection off / tiny lower bounds (mchip_set_model): t may be 0 in a zero-count cell (a column
						 * whose P is 0 for every k) and a product of four t's may underflow: one reciprocal per cell,
						 * and none where n = 0, so such cells contribute exactly 0 as in em_alg.c:338-342 */
#pragma unroll
						for (int j = 0; j < NJ; j++) rc[j] = (n[j] != 0.0) ? rcp_full(t[j]) : 0.0;
					} else {
						rcp_group(t, rc);
					}
				}
#pragma unroll
				for (int j = 0; j < NJ; j++) {
					const double r = MIX ? n[j] : n[j] * rc[j];
#pragma unroll
					for (int k = 0; k < K; k++) acc[k] = __builtin_fma(q[j][k], r, acc[k]);
				}
				word >>= NJ * BITS;
			}
		}
		w = wn;
	}
	/* (lane, wave and column are worked out again from the thread index, laundered so that hipcc does not keep the first copies
	 * alive across the loop: those four registers were the difference between 7 and 6 waves per SIMD at K = 8) */
	unsigned tid = threadIdx.x;
	asm volatile("" : "+v"(tid));
	const int lane2 = (int)(tid & 63u), wv2 = (int)(tid >> 6);
	for (int x = 1; x < MCHIP_COL_WAVES; x++) {	/* wave x hands its sums to wave 0: one wave's worth of LDS, taken in turns */
		if (wv2 == x) {
#pragma unroll
			for (int k = 0; k < K; k++) wsum[k][lane2] = acc[k];
		}
		__syncthreads();
		if (wv2 == 0) {
#pragma unroll
			for (int k = 0; k < K; k++) acc[k] += wsum[k][lane2];
		}
		__syncthreads();
	}
	const int c2 = bx * 64 + lane2;
	if (wv2 == 0 && c2 < a.T) {
		double *out = a.Apart + ((size_t)by * a.T + c2) * K;
#pragma unroll
		for (int k = 0; k < K; k++) out[k] = acc[k];
	}
}

template <int BITS, bool MIX, bool SAFE = false>
__global__ __launch_bounds__(MCHIP_BLOCK) void k_column_counts(mchip_pass_args a)
{
	if (a.stop && *a.stop) return;		/* batched run already stopped (wave-uniform) */
	__shared__ double wsum[K][64];
	column_counts_body<BITS, MIX, SAFE>(a, (int)blockIdx.x, (int)blockIdx.y, wsum);
}

/* ---------------------------------------------------------------- column pass on packed counts, k range split over CSPLIT lanes
 * K >= 37: CSPLIT = 2 adjacent lanes = one allele column, lane part s holds k in [s CKS, (s+1) CKS) of P_.c and of the
 * accumulators.  The q rows of one dword's worth of individuals (16 at 2 bits per count, 8 at 4) are staged in LDS
 * (double-buffered: the next batch waits in registers while this one is computed); a lane reads its part of a row with
 * ds_read_b128 (the parts of a row sit an odd number of 16-byte units apart: distinct banks), forms its partial dot product, and
 * the lanes of a column add their partials with DPP exchanges (every lane ends on the same bits: a + b = b + a at each level).
 * One reciprocal per cell. */
template <int CTRL> __device__ __forceinline__ double quad_exchange(double v)
{
	return __hiloint2double(__builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false),
				__builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false));
}
/* sum over the four lanes of a quad: v + (the lane whose index differs in bit 0), then the same for bit 1
 * (quad_perm [1,0,3,2] = 0xB1 and [2,3,0,1] = 0x4E) */
__device__ __forceinline__ double quad_sum(double v)
{
	v += quad_exchange<0xB1>(v);
	if (CSPLIT == 4) v += quad_exchange<0x4E>(v);
	return v;
}

template <int BITS, bool SAFE>
__global__ __launch_bounds__(MCHIP_BLOCK) void k_column_counts_split(mchip_pass_args a)
{
	static_assert(CSPLIT == 4 || CSPLIT == 2 || CSPLIT == 1, "quad exchange");
	if (a.stop && *a.stop) return;		/* batched run already stopped (wave-uniform) */
	constexpr int PERWORD = 32 / BITS;		/* individuals per dword = per staged batch */
	constexpr int G = 4 * PERWORD;
	constexpr unsigned MASK = (1u << BITS) - 1u;
	constexpr int ROW = CSPLIT * CQS;		/* LDS doubles per individual */
	constexpr int NST = (PERWORD * K + MCHIP_BLOCK - 1) / MCHIP_BLOCK;	/* staged doubles per thread */
	__shared__ __attribute__((aligned(16))) double qs[2][PERWORD * ROW];
	const int part = threadIdx.x % CSPLIT, k0 = part * CKS;
	const int c_raw = blockIdx.x * (MCHIP_BLOCK / CSPLIT) + threadIdx.x / CSPLIT;
	const bool valid = c_raw < a.T;
	const int c = valid ? c_raw : a.T - 1;
	double p[CKSE], acc[CKSE];
#pragma unroll
	for (int k = 0; k < CKSE; k++) {
		p[k] = (k < CKS && k0 + k < K) ? a.P[(size_t)c * K + k0 + k] : 0.0;
		acc[k] = 0.0;
	}
	const int i0 = blockIdx.y * a.ichunk;		/* multiple of G */
	const int i1 = min(a.I, i0 + a.ichunk);
	const int g_end = (i1 + G - 1) / G;
	/* the padding slots multiply p = 0: they must hold finite values, not whatever the last kernel left in LDS */
	{
		double *flat = &qs[0][0];	/* both buffers, as the one array they are */
		for (int x = threadIdx.x; x < 2 * PERWORD * ROW; x += MCHIP_BLOCK) flat[x] = 0.0;
	}
	__syncthreads();
	auto q_address = [&](int x, int ibase) __attribute__((always_inline)) {	/* element x of a batch: individual x / K, cluster x % K */
		const int j = x / K, k = x % K;
		return a.Q + (size_t)min(ibase + j, a.I - 1) * a.qstride + k;
	};
	auto q_slot = [&](int x) __attribute__((always_inline)) { const int j = x / K, k = x % K; return j * ROW + (k / CKS) * CQS + (k % CKS); };
	for (int y = 0; y < NST; y++) {
		const int x = threadIdx.x + y * MCHIP_BLOCK;
		if (x < PERWORD * K) qs[0][q_slot(x)] = *q_address(x, i0);
	}
	const uint4 *gt = reinterpret_cast<const uint4 *>(a.gtC);
	uint4 w = gt[(size_t)(i0 / G) * a.T + c];
	__syncthreads();
	int buf = 0;
	for (int g = i0 / G; g < g_end; g++) {
		const uint4 wn = gt[(size_t)min(g + 1, g_end - 1) * a.T + c];	/* prefetch (clamped) */
#pragma unroll 1
		for (int wi = 0; wi < 4; wi++) {
			const unsigned word = (wi == 0) ? w.x : (wi == 1) ? w.y : (wi == 2) ? w.z : w.w;
			const int ibase = g * G + wi * PERWORD;
			if (ibase >= i1) break;		/* block-uniform: the remaining batches of the chunk's last word are empty */
			/* the next batch's q rows: requested now, stored behind the arithmetic */
			const int inext = ibase + PERWORD;
			const bool more = inext < i1;	/* block-uniform */
			double st[NST];
			if (more) {
#pragma unroll
				for (int y = 0; y < NST; y++) {
					const int x = threadIdx.x + y * MCHIP_BLOCK;
					st[y] = *q_address(min(x, PERWORD * K - 1), inext);
				}
			}
			const double *rowp = &qs[buf][part * CQS];
#pragma unroll 1
			for (int j = 0; j < PERWORD; j++) {
				if (ibase + j >= i1) break;	/* wave-uniform; padded individuals have zero counts anyway */
				const double2 *qr = reinterpret_cast<const double2 *>(rowp + j * ROW);
				double q[CKSE];
#pragma unroll
				for (int k = 0; k < CKSE / 2; k++) {
					const double2 v = qr[k];
					q[2 * k] = v.x;
					q[2 * k + 1] = v.y;
				}
				double t = q[0] * p[0];
#pragma unroll
				for (int k = 1; k < CKSE; k++) t = __builtin_fma(q[k], p[k], t);
				t = quad_sum(t);
				const double n = (double)((word >> (BITS * j)) & MASK);
				/* SAFE: t may be 0 where n = 0 (projection off: a column whose P is 0 for every k) */
				const double r = SAFE ? ((n != 0.0) ? n * rcp_full(t) : 0.0) : n * rcp_full(t);
#pragma unroll
				for (int k = 0; k < CKSE; k++) acc[k] = __builtin_fma(q[k], r, acc[k]);
			}
			if (more) {
#pragma unroll
				for (int y = 0; y < NST; y++) {
					const int x = threadIdx.x + y * MCHIP_BLOCK;
					if (x < PERWORD * K) qs[buf ^ 1][q_slot(x)] = st[y];
				}
			}
			__syncthreads();	/* the next batch is complete, this one may be overwritten */
			buf ^= 1;
		}
		w = wn;
	}
	if (valid) {
		double *out = a.Apart + ((size_t)blockIdx.y * a.T + c) * K + k0;
#pragma unroll
		for (int k = 0; k < CKS; k++)
			if (k0 + k < K) out[k] = acc[k];
	}
}

}  // namespace

#endif
