/* kernels_k/sparse.h -- the sparse individual pass, lane-split form (K >= 28); the cooperating-waves form is in sparse_w.h */
#ifndef MCHIP_KERNELS_K_SPARSE_H
#define MCHIP_KERNELS_K_SPARSE_H

#include "kernels_k/common.h"

namespace {

/* ---------------------------------------------------------------- individual pass, sparse form
 * lane = individual; only the alleles the individual carries are visited: one term per allele copy
 * (a homozygote contributes its allele twice, which is the reference's n = 2 cell: same t, r and t^2).
 * The P rows of the current block of 8 loci are staged in LDS (double-buffered) and gathered per lane with
 * ds_read_b128; rows of one locus are consecutive, so lanes on different alleles hit different bank groups.
 * Produces the S-side sums and the log likelihood (one multiply per copy, no selects).  ACCUM = false is the
 * stand-alone log-likelihood pass (logL_admixture, log_likelihood.c:96-147). */
/* sum over the SPLIT adjacent lanes of an individual; every lane ends with the same bits (a + b = b + a at every level) */
__device__ __forceinline__ double split_sum(double v)
{
	if (SPLIT >= 2) v += __shfl_xor(v, 1);
	if (SPLIT >= 4) v += __shfl_xor(v, 2);
	return v;
}

#ifndef MCHIP_SPARSE_WAVES
#define MCHIP_SPARSE_WAVES 1
#endif
/* DUAL (with ACCUM, diploid, !SAFE): the same pass also takes the log likelihood of a second parameter set
 * (a.Q2, a.P2 -> a.llpart2), with the arithmetic of the ACCUM = false instance, lane for lane: an accelerated cycle needs
 * log L of its second EM iterate and the E step of the extrapolated point back to back (accel_em.c:53,544); the first is
 * bound by the LDS gather, the second by FP64 issue, and one kernel overlaps some of the two: 2.78-2.88 ms against 1.84 + 1.15
 * at config 3 (scripts/diag/dual.sh).  Tetraploid data loses (1.53 against 0.90 + 0.55 ms at config 5's shape: 170 registers,
 * three waves per SIMD): not instantiated */
/* minimum waves per SIMD the register allocation has to leave room for.  K = 57 ... 64 (four lanes per individual, 16 doubles of
 * q, of the sums and of each gathered row per lane): left alone the diploid S-side instance takes 174 registers = two waves per
 * SIMD, where K = 56 runs three on 150; held to three waves it spills a handful of registers to scratch in the block head
 * and runs 5.3-5.5 -> 4.3-4.6 ms (profiles/r03_k_sweep.txt) */
constexpr int sparse_min_waves(int PL, bool ACCUM)
{
	return MCHIP_SPARSE_WAVES > 1 ? MCHIP_SPARSE_WAVES : ((SPLIT == 4 && KSP == 16 && PL == 2 && ACCUM) ? 3 : 1);
}
template <int PL, bool ACCUM, bool SAFE, bool NOMISS, bool DUAL = false>
__global__ __launch_bounds__(QBLOCK, sparse_min_waves(PL, ACCUM)) void k_individual_sparse(mchip_pass_args a)
{
	static_assert(!DUAL || (ACCUM && !SAFE && PL == 2), "dual pass: ACCUM, shared reciprocals, diploid");
	if (a.stop && *a.stop) return;		/* batched run already stopped (wave-uniform) */
	if (ACCUM && !DUAL && a.skip_ind && *a.skip_ind) return;	/* sums + logL partials of these parameters are already there */
	extern __shared__ __attribute__((aligned(16))) double lds[];	/* [2][tile_cols][KP] (DUAL: twice) then [QBLOCK] reduction scratch */
	double *lds2 = lds + 2 * (size_t)a.tile_cols * KP;
	double *red = lds + (DUAL ? 4 : 2) * (size_t)a.tile_cols * KP;
#ifdef MCHIP_EXP_SCATTER
	/* EXPERIMENT (never in the product build; scripts/diag/scatter_exp.sh): what it would cost this pass to also form the
	 * N-side sums by scattering q_ik * r into per-workgroup LDS accumulators [column of the tile][K] with hardware
	 * ds_add_f64 -- the "(f)" alternative of DESIGN.md 4.3.  Only the atomics are issued (the accumulators are never flushed to
	 * memory, which would cost more): a lower bound on that design's S-side pass. */
	double *nacc = red + QBLOCK;
	for (int x = threadIdx.x; x < a.tile_cols * KP; x += QBLOCK) nacc[x] = 0.0;
#endif
	static_assert(!DUAL || SPLIT == 1, "dual pass: one lane per individual");
	const int part = SPLIT == 1 ? 0 : (int)(threadIdx.x % SPLIT);	/* which k range this lane holds */
	const int k0 = part * KSP;		/* this lane's first cluster */
	const int kl0 = part * PSTR;		/* ... and where its part of a staged row starts in LDS */
	const int i_raw = blockIdx.x * (QBLOCK / SPLIT) + threadIdx.x / SPLIT;
	const bool active = i_raw < a.I;
	const int i = active ? i_raw : a.I - 1;
	const int pl = PL ? PL : a.ploidy;
	double q[KSP], acc[KSP], q2[DUAL ? K : 1];
#pragma unroll
	for (int k = 0; k < KSP; k++) {
		q[k] = (SPLIT == 1 || k0 + k < K) ? a.Q[(size_t)i * a.qstride + k0 + k] : 0.0;
		acc[k] = 0.0;
		if constexpr (DUAL) q2[k] = a.Q2[(size_t)i * a.qstride + k];
	}
	if constexpr (SPLIT > 1 || !NOMISS) {
		/* once per workgroup: every tile slot holds a finite value from here on.  SPLIT > 1: the row slots past K are read by the
		 * last lane part (staging writes k < K only).  Missing data: a missing copy borrows column 0 of its locus and multiplies
		 * it by r = 0; at a locus WITHOUT any allele column (every individual missing: uniquealleles = 0, golden allmiss_*) that
		 * row is the next locus's, or, behind the tile's last column, whatever the previous kernel left in LDS -- 0 x NaN */
		for (int x = threadIdx.x; x < (DUAL ? 4 : 2) * a.tile_cols * KP; x += QBLOCK) lds[x] = 0.0;
		__syncthreads();
	}
	const int l0 = blockIdx.y * a.lchunk;
	const int l1 = min(a.L, l0 + a.lchunk);
	const int lb0 = l0 >> 3, lb_end = (l1 + 7) >> 3;
	double prod = 1.0, prod2 = 1.0;
	int blk = 0, ex = 0, ex2 = 0;
	constexpr int STAGE = 2;
	const bool staged = a.tile_cols * K <= STAGE * QBLOCK;	/* wave-uniform */

	/* column offsets of the current block's and the next block's loci: E[x] = toff[8 lb + x], x = 0..16 (toff is padded by 24
	 * entries equal to T).  Its upper half for the NEXT block is requested at the head of this one and moved in at its end: the
	 * head of a block -- right behind the workgroup barrier, where the waves of a workgroup all stand at the same place -- then
	 * starts its prefetches at once instead of behind three dependent scalar loads (c_lo, then n_lo, then n_hi) */
	int E[17];
#pragma unroll
	for (int x = 0; x < 17; x++) E[x] = a.toff[lb0 * 8 + x];
	/* stage the first tile */
	{
		const int c_lo = E[0], c_hi = E[8];
		const int nel = (c_hi - c_lo) * K;
		for (int x = threadIdx.x; x < nel; x += QBLOCK) {
			lds[(x / K) * KP + lds_k(x % K)] = a.P[(size_t)c_lo * K + x];
			if (DUAL) lds2[(x / K) * KP + lds_k(x % K)] = a.P2[(size_t)c_lo * K + x];
		}
	}
	geno_group<PL> g, gn;
	g.load(a.gtS, (size_t)lb0 * a.I + i, pl);
	__syncthreads();
	for (int lb = lb0; lb < lb_end; lb++) {
		const int buf = (lb - lb0) & 1;
		const double *tile = lds + (size_t)buf * a.tile_cols * KP;
		const double *tile2 = lds2 + (size_t)buf * a.tile_cols * KP;
		const int c_lo = E[0];
		int En[8];
#pragma unroll
		for (int x = 0; x < 8; x++) En[x] = a.toff[(lb + 1) * 8 + 9 + x];
		/* prefetch the next tile and the next genotype group.  Tiles of up to STAGE * QBLOCK doubles (every data set with
		 * <= 4 alleles per locus at K <= 8) wait in registers while this block is computed and go to the other LDS buffer
		 * after it, so no s_waitcnt for them sits in front of the arithmetic; larger tiles are copied through at once */
		double stage[STAGE], stage2[DUAL ? STAGE : 1];
		int nel_next = 0;
		double *dst = lds + (size_t)(buf ^ 1) * a.tile_cols * KP;
		double *dst2 = lds2 + (size_t)(buf ^ 1) * a.tile_cols * KP;
		if (lb + 1 < lb_end) {
			const int n_lo = E[8], n_hi = E[16];
			nel_next = (n_hi - n_lo) * K;
			const double *src = a.P + (size_t)n_lo * K;
			const double *src2 = DUAL ? a.P2 + (size_t)n_lo * K : nullptr;
			if (staged) {
#pragma unroll
				for (int s2 = 0; s2 < STAGE; s2++) {
					const int x = threadIdx.x + s2 * QBLOCK;
					stage[s2] = src[min(x, nel_next - 1)];
					if constexpr (DUAL) stage2[s2] = src2[min(x, nel_next - 1)];
				}
			} else {
				for (int x = threadIdx.x; x < nel_next; x += QBLOCK) {
					dst[(x / K) * KP + lds_k(x % K)] = src[x];
					if (DUAL) dst2[(x / K) * KP + lds_k(x % K)] = src2[x];
				}
			}
		}
		gn.load(a.gtS, (size_t)min(lb + 1, lb_end - 1) * a.I + i, pl);
		int tb[8];
#pragma unroll
		for (int j = 0; j < 8; j++) tb[j] = E[j];
		/* one locus: all of its copies; a lambda so that full blocks run as straight-line code (no per-locus bound check:
		 * the scheduler can then start the next locus's LDS reads under this locus's arithmetic) */
		auto one_locus = [&](int j) __attribute__((always_inline)) {
			const int base = tb[j] - c_lo;
			if constexpr (PL == 2 || PL == 4) {
				/* all copies of the locus first (t), then one shared reciprocal for each pair of copies */
				double pc[PL ? PL : 1][2 * KGP], t[PL ? PL : 1];
				bool miss[PL ? PL : 1];
				unsigned row[PL ? PL : 1];
#pragma unroll
				for (int b = 0; b < PL; b++) {
					const unsigned mraw = g.copy(j, b, pl);
					/* NOMISS: the data set has no missing copy: no selects (idle lanes duplicate individual I-1) */
					miss[b] = NOMISS ? false : ((mraw == MCHIP_MISSING) || !active);
					const unsigned mm = miss[b] ? 0u : mraw;
					row[b] = (unsigned)base + mm;
					/* 16-byte LDS reads (ds_read_b128): twice the bytes per LDS cycle of ds_read2_b64 */
					const double2 *pr = reinterpret_cast<const double2 *>(tile + (size_t)(base + (int)mm) * KP + kl0);
#pragma unroll
					for (int k = 0; k < KGP; k++) {
						const double2 v = pr[k];
						pc[b][2 * k] = v.x;
						pc[b][2 * k + 1] = v.y;
					}
					t[b] = q[0] * pc[b][0];
#pragma unroll
					for (int k = 1; k < KSP; k++) t[b] = __builtin_fma(q[k], pc[b][k], t[b]);
					t[b] = split_sum(t[b]);	/* the lanes' partial dot products; identical in all of them afterwards */
					/* a missing copy borrowed column 0 of its locus; it takes t = 1 so that it leaves the log-product and
					 * its partner's shared reciprocal alone, whatever column 0 holds (all zeros when projection is off and
					 * a bootstrap replicate lacks that allele) */
					if (!NOMISS) t[b] = miss[b] ? 1.0 : t[b];
				}
				if constexpr (PL == 4 && !SAFE && ACCUM) {
					/* tetraploid: the four copies of the locus share one reciprocal (rcp4's scheme: 16 issue slots per
					 * locus instead of 20 for two pairs); the log-product takes the same two pair products as below */
					const double p01 = t[0] * t[1], p23 = t[2] * t[3];
					const double rp = rcp_full(p01 * p23);
					const double r01 = rp * p23, r23 = rp * p01;
					const double r[4] = { miss[0] ? 0.0 : r01 * t[1], miss[1] ? 0.0 : r01 * t[0],
							      miss[2] ? 0.0 : r23 * t[3], miss[3] ? 0.0 : r23 * t[2] };
#pragma unroll
					for (int b = 0; b < 4; b++)
#pragma unroll
						for (int k = 0; k < KSP; k++) acc[k] = __builtin_fma(pc[b][k], r[b], acc[k]);
					prod *= p01;
					prod *= p23;
				} else
#pragma unroll
				for (int b = 0; b < PL; b += 2) {
					const double pp = t[b] * t[b + 1];
					if (ACCUM) {
						double r0, r1;
						if (SAFE) {	/* tiny lower bounds: the product of two t's may underflow */
							r0 = miss[b] ? 0.0 : rcp_full(t[b]);
							r1 = miss[b + 1] ? 0.0 : rcp_full(t[b + 1]);
						} else {
							const double rp = rcp_full(pp);
							r0 = miss[b] ? 0.0 : rp * t[b + 1];
							r1 = miss[b + 1] ? 0.0 : rp * t[b];
						}
#pragma unroll
						for (int k = 0; k < KSP; k++) acc[k] = __builtin_fma(pc[b][k], r0, acc[k]);
#pragma unroll
						for (int k = 0; k < KSP; k++) acc[k] = __builtin_fma(pc[b + 1][k], r1, acc[k]);
#ifdef MCHIP_EXP_SCATTER
#pragma unroll
						for (int k = 0; k < K; k++) unsafeAtomicAdd(&nacc[(size_t)row[b] * KP + k], q[k] * r0);
#pragma unroll
						for (int k = 0; k < K; k++) unsafeAtomicAdd(&nacc[(size_t)row[b + 1] * KP + k], q[k] * r1);
#endif
					}
					if (SAFE) {
						/* projection off: an extrapolated point may have entries outside [0, 1] and t < 0 in a cell that carries a
						 * copy; the reference's log(t) is NaN there and ends the run (em_alg.c:106-110).  Two such factors
						 * must not cancel in the product: a negative t poisons it */
						prod *= t[b] < 0.0 ? __builtin_nan("") : t[b];
						rescale(prod, ex);
						prod *= t[b + 1] < 0.0 ? __builtin_nan("") : t[b + 1];
						rescale(prod, ex);
					} else {
						prod *= pp;
					}
					if constexpr (DUAL) {	/* the second set's t of the same two copies: gather, dot product, into its own log-product
								 * (requesting these rows ahead of the accumulation above costs 30 more registers and a wave
								 * of occupancy: measured slower) */
						double t2[2];
#pragma unroll
						for (int bb = 0; bb < 2; bb++) {
							const double2 *pr = reinterpret_cast<const double2 *>(tile2 + (size_t)row[b + bb] * KP);
							double pc2[KP];
#pragma unroll
							for (int k = 0; k < KP / 2; k++) {
								const double2 v = pr[k];
								pc2[2 * k] = v.x;
								pc2[2 * k + 1] = v.y;
							}
							t2[bb] = q2[0] * pc2[0];
#pragma unroll
							for (int k = 1; k < K; k++) t2[bb] = __builtin_fma(q2[k], pc2[k], t2[bb]);
							if (!NOMISS) t2[bb] = miss[b + bb] ? 1.0 : t2[bb];
						}
						prod2 *= t2[0] * t2[1];
					}
				}
			} else {
				for (int bb = 0; bb < pl; bb++) {	/* any other ploidy: one copy at a time */
					const unsigned mraw = g.copy(j, bb, pl);
					const bool miss = (mraw == MCHIP_MISSING) || !active;
					const unsigned mm = miss ? 0u : mraw;
					const double *pr = tile + (size_t)(base + (int)mm) * KP + kl0;
					double pc[KSP];
#pragma unroll
					for (int k = 0; k < KSP; k++) pc[k] = pr[k];
					double t = q[0] * pc[0];
#pragma unroll
					for (int k = 1; k < KSP; k++) t = __builtin_fma(q[k], pc[k], t);
					t = split_sum(t);
					if (ACCUM) {
						const double r = miss ? 0.0 : rcp_full(t);
#pragma unroll
						for (int k = 0; k < KSP; k++) acc[k] = __builtin_fma(pc[k], r, acc[k]);
					}
					prod *= miss ? 1.0 : (t < 0.0 ? __builtin_nan("") : t);		/* as above: a negative t must end in NaN */
					rescale(prod, ex);
				}
			}
		};
		/* !SAFE: the product is looked at every flush_blocks units of 16 multiplications: a block of 8 diploid loci,
		 * half a block of tetraploid ones (the host sizes flush_blocks for that, mchip_set_model) */
		auto tick = [&]() __attribute__((always_inline)) {
			if (!SAFE) {
				if (++blk >= a.flush_blocks) {
					blk = 0;
					rescale(prod, ex);
					if (DUAL) rescale(prod2, ex2);
				}
			}
		};
		/* unrolled with a scalar bound check per locus: static j keeps the genotype group and the offsets in registers (a
		 * dynamic index would put them in scratch, whose s_waitcnt would also wait for the prefetches) */
		const int nloc = l1 - lb * 8;
		/* (diploid: taking two loci at a time so that four copies share one reciprocal, as the tetraploid locus does, needs the
		 * four gathered rows at once -- 138 registers, three waves per SIMD -- and measured 8-10 % slower than this) */
#pragma unroll
		for (int j = 0; j < 8; j++) {
			if (j < nloc) one_locus(j);
			if (PL == 4 && j == 3) tick();
		}
		tick();
		if (staged) {
#pragma unroll
			for (int s2 = 0; s2 < STAGE; s2++) {
				const int x = threadIdx.x + s2 * QBLOCK;
				if (x < nel_next) dst[(x / K) * KP + lds_k(x % K)] = stage[s2];
				if constexpr (DUAL) { if (x < nel_next) dst2[(x / K) * KP + lds_k(x % K)] = stage2[s2]; }
			}
		}
		g = gn;
#pragma unroll
		for (int x = 0; x <= 8; x++) E[x] = E[x + 8];
#pragma unroll
		for (int x = 0; x < 8; x++) E[9 + x] = En[x];
		__syncthreads();	/* next tile is complete and this one may be overwritten */
	}
	const double ll = (double)ex * 0.693147180559945309417 + log(prod);
	if (ACCUM && active) {
		double *out = a.Spart + ((size_t)blockIdx.y * a.I + i) * K + k0;
#pragma unroll
		for (int k = 0; k < KSP; k++)
			if (SPLIT == 1 || k0 + k < K) out[k] = acc[k];
	}
	/* every lane of an individual carries the same log-product: part 0 speaks for it */
	const double tot = block_tree_sum<QBLOCK>(red, (active && part == 0) ? ll : 0.0);
	if (threadIdx.x == 0) a.llpart[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = tot;
	if (DUAL) {
		const double ll2 = (double)ex2 * 0.693147180559945309417 + log(prod2);
		__syncthreads();	/* red[] is read by thread 0 above */
		const double tot2 = block_tree_sum<QBLOCK>(red, active ? ll2 : 0.0);
		if (threadIdx.x == 0) a.llpart2[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = tot2;
	}
}

/* ---------------------------------------------------------------- its launch: dynamic LDS */
#ifdef MCHIP_EXP_SCATTER
inline size_t sparse_lds_bytes(const mchip_pass_args &a) { return (3 * (size_t)a.tile_cols * KP + QBLOCK) * sizeof(double); }
#else
inline size_t sparse_lds_bytes(const mchip_pass_args &a) { return (2 * (size_t)a.tile_cols * KP + QBLOCK) * sizeof(double); }
#endif

}  // namespace

#endif
