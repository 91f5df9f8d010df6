/* kernels_k/partition.h -- the hard partition's passes (first M step) */
#ifndef MCHIP_KERNELS_K_PARTITION_H
#define MCHIP_KERNELS_K_PARTITION_H

#include "kernels_k/common.h"

namespace {

/* ---------------------------------------------------------------- hard partition (first M step)
 * rnd_init.c:456-482: d[i][k][l][m] = 1 for every copy a of allele m assigned to cluster k. */
template <int PL>
__global__ __launch_bounds__(MCHIP_BLOCK) void k_partition_columns(mchip_pass_args a)
{
	const int c_raw = blockIdx.x * MCHIP_BLOCK + threadIdx.x;
	const bool valid = c_raw < a.T;
	const int c = valid ? c_raw : a.T - 1;
	const int l = a.col_locus[c];
	const unsigned m = valid ? (unsigned)a.col_allele[c] : 0xFEu;
	const int pl = PL ? PL : a.ploidy;
	double acc[K];
#pragma unroll
	for (int k = 0; k < K; k++) acc[k] = 0.0;
	const int i0 = blockIdx.y * a.ichunk;
	const int i1 = min(a.I, i0 + a.ichunk);
	for (int ib = i0 >> 3; ib < ((i1 + 7) >> 3); ib++) {
		geno_group<PL> g, s;
		g.load(a.gtA, (size_t)ib * a.L + l, pl);
		s.load(a.asA, (size_t)ib * a.L + l, pl);
#pragma unroll
		for (int j = 0; j < 8; j++) {
			if (a.part_counts) {	/* initialize_parameters_admixture (rnd_init.c:661-684): every copy counts */
				for (int b = 0; b < pl; b++)
					if (g.copy(j, b, pl) == m) {
						const unsigned kb = s.copy(j, b, pl);
#pragma unroll
						for (int k = 0; k < K; k++) acc[k] += (kb == (unsigned)k) ? 1.0 : 0.0;
					}
				continue;
			}
			unsigned long long flags = 0;
			for (int b = 0; b < pl; b++)
				if (g.copy(j, b, pl) == m) flags |= 1ull << (s.copy(j, b, pl) & 63u);
#pragma unroll
			for (int k = 0; k < K; k++) acc[k] += (double)((flags >> k) & 1ull);
		}
	}
	if (valid) {
		double *out = a.Apart + ((size_t)blockIdx.y * a.T + c) * K;
#pragma unroll
		for (int k = 0; k < K; k++) out[k] = acc[k];
	}
}

template <int PL>
__global__ __launch_bounds__(QBLOCK) void k_partition_individuals(mchip_pass_args a)
{
	const int i = blockIdx.x * QBLOCK + threadIdx.x;
	if (i >= a.I) return;
	const int pl = PL ? PL : a.ploidy;
	double acc[K];
#pragma unroll
	for (int k = 0; k < K; k++) acc[k] = 0.0;
	const int l0 = blockIdx.y * a.lchunk;
	const int l1 = min(a.L, l0 + a.lchunk);
	for (int lb = l0 >> 3; lb < ((l1 + 7) >> 3); lb++) {
		geno_group<PL> g, s;
		g.load(a.gtS, (size_t)lb * a.I + i, pl);
		s.load(a.asS, (size_t)lb * a.I + i, pl);
		for (int j = 0; j < 8; j++) {
			if (lb * 8 + j >= l1) break;
			for (int b = 0; b < pl; b++) {
				const unsigned mb = g.copy(j, b, pl), kb = s.copy(j, b, pl);
				if (!a.part_counts) {
					if (mb == MCHIP_MISSING) continue;
					bool dup = false;
					for (int b2 = 0; b2 < b; b2++)
						dup |= (g.copy(j, b2, pl) == mb) && (s.copy(j, b2, pl) == kb);
					if (dup) continue;
				}	/* else initialize_parameters_admixture (rnd_init.c:617-648): every copy of the individual, missing ones too */
#pragma unroll
				for (int k = 0; k < K; k++) acc[k] += (kb == (unsigned)k) ? 1.0 : 0.0;
			}
		}
	}
	double *out = a.Spart + ((size_t)blockIdx.y * a.I + i) * K;
#pragma unroll
	for (int k = 0; k < K; k++) out[k] = acc[k];
}

}  // namespace

#endif
