/* kernels_k/pair.h -- the paired E step: the bodies of column.h and sparse_w.h in one launch */
#ifndef MCHIP_KERNELS_K_PAIR_H
#define MCHIP_KERNELS_K_PAIR_H

#include "kernels_k/column.h"
#include "kernels_k/sparse_w.h"

namespace {

/* ---------------------------------------------------------------- paired E step: column pass and S-side pass in one launch
 * The two passes of an E step read the same parameters and write disjoint workspaces (Apart; Spart + llpart), and each leaves idle
 * what the other uses: the column body has no LDS traffic and waits on scalar loads, the individual body waits on LDS gathers.
 * Here their workgroups share one grid (mchip_internal.h: block ids in runs of eight of one kind, the kinds interleaved in the
 * proportion of their counts) and so every CU; each block runs one of the two bodies above unchanged, so every result is the two
 * launches' bit for bit.  256 threads (a.ind_waves = 4); dynamic LDS: the larger of the individual body's tiles and the column
 * body's [K][64] hand-over.
 * a.skip_ind: the individual blocks return at once (the sums are cached), the column blocks work.
 * marks (profiled runs): overlapping kinds have no event-to-event duration, so each working block leaves its first wave start and
 * last wave end (s_memrealtime) in marks[2 * block], [2 * block + 1]; a block that returned leaves start > end.  One lane stores
 * them after the waves' readings met in LDS; mchip_profile.hip's k_pair_spans takes each kind's minimum and maximum.
 * Registers (-Rpass-analysis=kernel-resource-usage): the function takes what the S-side body takes and runs at its waves per
 * SIMD -- K = 8: 93 VGPRs, five waves (S-side instance 90-92, column instance 68 and seven waves); K = 12: 123-125, four waves
 * (122-124).  No vector register spills; the column body's scalar registers are all taken (99 at K = 8), so a few of the
 * launch's own scalars (the marks pointer, the start reading) wait in lanes of one vector register, outside the loops. */
template <int BITS, int PL, bool SAFE, bool NOMISS>
__global__ __launch_bounds__(MCHIP_BLOCK) void k_estep_pair(mchip_pass_args a, mchip_pair_runs runs, unsigned long long *marks)
{
	static_assert(64 * MCHIP_IND_WAVES_MAX == MCHIP_BLOCK, "both bodies at 256 threads");
	extern __shared__ __attribute__((aligned(16))) double lds[];
	unsigned logical;
	const bool ind = mchip_pair_is_ind(blockIdx.x, runs, &logical);	/* uniform over the workgroup */
	const unsigned n_col = (unsigned)((a.T + 63) / 64), n_mine = ind ? (unsigned)(((a.I + 63) / 64) * mchip_ind_slabs(a)) : n_col * (unsigned)mchip_col_slabs(a);
	const bool idle = logical >= n_mine || (a.stop && *a.stop) || (ind && a.skip_ind && *a.skip_ind);
	if (idle) {
		if (marks && threadIdx.x == 0) {
			marks[2 * (size_t)blockIdx.x] = ~0ull;
			marks[2 * (size_t)blockIdx.x + 1] = 0ull;
		}
		return;
	}
	/* (the wave's start waits in registers until the body is done: a store in front of the bodies would be one more thing hipcc
	 * has to assume about memory) */
	const unsigned long long t_start = marks ? __builtin_amdgcn_s_memrealtime() : 0ull;
	if (ind) individual_sparse_w_body<PL, true, SAFE, NOMISS, false>(a, logical, lds);
	else column_counts_body<BITS, false, SAFE>(a, (int)(logical % n_col), (int)(logical / n_col), reinterpret_cast<double (*)[64]>(lds));
	if (marks) {
		/* (the waves' readings meet at the head of the dynamic array: both bodies end behind a barrier that follows their last
		 * LDS read, and a static array beside the tiles would cost config 3 its fifth workgroup per CU -- 5 x 32 KiB fill it) */
		unsigned long long (*wave_mark)[MCHIP_COL_WAVES] = reinterpret_cast<unsigned long long (*)[MCHIP_COL_WAVES]>(lds);
		if ((threadIdx.x & 63) == 0) {
			wave_mark[0][threadIdx.x >> 6] = t_start;
			wave_mark[1][threadIdx.x >> 6] = __builtin_amdgcn_s_memrealtime();
		}
		__syncthreads();
		if (threadIdx.x == 0) {
			unsigned long long t0 = wave_mark[0][0], t1 = wave_mark[1][0];
			for (int w = 1; w < MCHIP_COL_WAVES; w++) {
				t0 = wave_mark[0][w] < t0 ? wave_mark[0][w] : t0;
				t1 = wave_mark[1][w] > t1 ? wave_mark[1][w] : t1;
			}
			marks[2 * (size_t)blockIdx.x] = t0;
			marks[2 * (size_t)blockIdx.x + 1] = t1;
		}
	}
}

}  // namespace

#endif
