/* kernels_k/mixture.h -- the mixture model's passes */
#ifndef MCHIP_KERNELS_K_MIXTURE_H
#define MCHIP_KERNELS_K_MIXTURE_H

#include "kernels_k/common.h"

namespace {

/* ---------------------------------------------------------------- mixture model (em_alg.c:763-1011)
 * E step: v_ik = log eta_k + sum_{l,m: n>0} n log p_klm.  log P is tabulated once per step ([T][K], k_logp in
 * mchip.hip); the per-individual sum is a gather-add over the alleles the individual carries (one add per
 * allele copy; n copies of the same allele add the same value n times), lane = individual, rows staged in LDS
 * exactly like the sparse admixture pass.  Vpart (= Spart) holds the per-locus-chunk sums. */
template <int PL, bool STAGED>
__global__ __launch_bounds__(QBLOCK) void k_mix_gather(mchip_pass_args a)
{
	if (a.stop && *a.stop) return;		/* batched run already stopped (wave-uniform) */
	extern __shared__ __attribute__((aligned(16))) double lds[];
	const int i_raw = blockIdx.x * QBLOCK + threadIdx.x;
	const bool active = i_raw < a.I;
	const int i = active ? i_raw : a.I - 1;
	const int pl = PL ? PL : a.ploidy;
	double acc[K];
#pragma unroll
	for (int k = 0; k < K; k++) acc[k] = 0.0;
	const int l0 = blockIdx.y * a.lchunk;
	const int l1 = min(a.L, l0 + a.lchunk);
	const int lb0 = l0 >> 3, lb_end = (l1 + 7) >> 3;
	if (STAGED) {
		const int c_lo = a.toff[lb0 * 8], c_hi = a.toff[min(lb0 * 8 + 8, a.L)];
		const int nel = (c_hi - c_lo) * K;
		for (int x = threadIdx.x; x < nel; x += QBLOCK)
			lds[(x / K) * KP + (x % K)] = a.P[(size_t)c_lo * K + x];
		__syncthreads();
	}
	for (int lb = lb0; lb < lb_end; lb++) {
		const int buf = (lb - lb0) & 1;
		const int c_lo = a.toff[lb * 8];
		const double *tile = STAGED ? lds + (size_t)buf * a.tile_cols * KP : a.P + (size_t)c_lo * K;
		if (STAGED && lb + 1 < lb_end) {
			const int n_lo = a.toff[(lb + 1) * 8], n_hi = a.toff[min((lb + 1) * 8 + 8, a.L)];
			const int nel = (n_hi - n_lo) * K;
			double *dst = lds + (size_t)(buf ^ 1) * a.tile_cols * KP;
			for (int x = threadIdx.x; x < nel; x += QBLOCK)
				dst[(x / K) * KP + (x % K)] = a.P[(size_t)n_lo * K + x];
		}
		geno_group<PL> g;
		g.load(a.gtS, (size_t)lb * a.I + i, pl);
		for (int j = 0; j < 8; j++) {
			const int l = lb * 8 + j;
			if (l >= l1) break;
			const int base = a.toff[l] - c_lo;
			for (int b = 0; b < pl; b++) {
				const unsigned mraw = g.copy(j, b, pl);
				if (mraw == MCHIP_MISSING || !active) continue;
				const double *pr = tile + (size_t)(base + (int)mraw) * (STAGED ? KP : K);
#pragma unroll
				for (int k = 0; k < K; k++) acc[k] += pr[k];
			}
		}
		if (STAGED) __syncthreads();
	}
	if (active) {
		double *out = a.Spart + ((size_t)blockIdx.y * a.I + i) * K;
#pragma unroll
		for (int k = 0; k < K; k++) out[k] = acc[k];
	}
}

/* per individual: combine the chunk sums, then
 *   mode 0 (e_step_mixture, em_alg.c:828-882): v = log eta + sum; max; vik = exp(v - max) / sum; ll_i = log(sum) + max
 *   mode 1 (logL_mixture, log_likelihood.c:203-228): v = sum + log eta; scale only if exp(max) under/overflows */
__global__ __launch_bounds__(MCHIP_BLOCK) void k_mix_finalize(int I, int n_lchunks, const double *__restrict__ Vpart,
		const double *__restrict__ eta, double *vik, double *llpart, int mode, const int *stop)
{
	__shared__ double red[MCHIP_BLOCK];
	if (stop && *stop) return;
	const int i = blockIdx.x * MCHIP_BLOCK + threadIdx.x;
	double ll = 0.0;
	if (i < I) {
		double v[K];
		if (mode == 0) {
#pragma unroll
			for (int k = 0; k < K; k++) v[k] = log(eta[k]);
		} else {
#pragma unroll
			for (int k = 0; k < K; k++) v[k] = 0.0;
		}
		for (int ch = 0; ch < n_lchunks; ch++) {
			const double *src = Vpart + ((size_t)ch * I + i) * K;
#pragma unroll
			for (int k = 0; k < K; k++) v[k] += src[k];
		}
		if (mode == 1) {
#pragma unroll
			for (int k = 0; k < K; k++) v[k] += log(eta[k]);
		}
		double mx = -INFINITY;
#pragma unroll
		for (int k = 0; k < K; k++) if (v[k] > mx) mx = v[k];
		if (mode == 0) {
			double temp = 0.0;
#pragma unroll
			for (int k = 0; k < K; k++) {
				v[k] = exp(v[k] - mx);
				temp += v[k];
			}
#pragma unroll
			for (int k = 0; k < K; k++) vik[(size_t)i * K + k] = v[k] / temp;
			ll = log(temp) + mx;
		} else {
			double temp_exp = exp(mx), scale_exp = 0.0;
			/* The reference halves scale_exp until exp() stops overflowing (log_likelihood.c:212-221).  When no v[k] is an
			 * ordinary number -- every one NaN (a negative extrapolated p with the projection off: log() = NaN in k_logp) or
			 * -inf, or one +inf -- mx is infinite, scale_exp = inf, inf / 2 = inf, and its loop never ends: on the CPU a
			 * process that spins, here a wave the stream never gets back from.  Such an individual's term is NaN instead: the
			 * sum is NaN, and stop() ends the run on "nan" (em_alg.c:106-110), which is where a NaN leads the reference whenever
			 * its loop does end.  A finite mx needs at most log2(DBL_MAX / 709) < 1 016 halvings (a dozen for any sum of logs a
			 * data set can produce); the cap states that bound. */
			if (!(mx > -INFINITY && mx < INFINITY)) {
				ll = __builtin_nan("");
			} else {
				if (temp_exp == 0.0 || temp_exp == HUGE_VAL) {
					scale_exp = (temp_exp == HUGE_VAL) ? mx : -mx;
					int halvings = 0;
					do {
						scale_exp *= 0.5;
						temp_exp = exp(scale_exp);
					} while (temp_exp == HUGE_VAL && ++halvings < 2048);
					scale_exp = mx - scale_exp;
#pragma unroll
					for (int k = 0; k < K; k++) v[k] -= scale_exp;
				}
				temp_exp = 0.0;
#pragma unroll
				for (int k = 0; k < K; k++) temp_exp = temp_exp + exp(v[k]);
				if (temp_exp == HUGE_VAL) {
					/* NOT the reference.  Its halving leaves the shifted maximum anywhere in (354.9, 709.78]; within ln S of
					 * the upper end, with clusters of total weight S relative to the best one (two tied ones are enough), the
					 * sum above overflows and the reference's term is +inf: a log likelihood that passes stop()'s NaN exit and
					 * wins every `ll > emll`.  Such a term is taken in mode 0's form instead, log sum_k exp(v_k - max) + max.
					 * Taken only where the reference's arithmetic gives +inf: every finite result keeps its bits. */
					const double top = mx - scale_exp;	/* the shifted maximum */
					temp_exp = 0.0;
#pragma unroll
					for (int k = 0; k < K; k++) temp_exp = temp_exp + exp(v[k] - top);
					ll = log(temp_exp) + mx;
				} else {
					ll = log(temp_exp) + scale_exp;
				}
			}
		}
	}
	const double tot = block_tree_sum<MCHIP_BLOCK>(red, ll);
	if (threadIdx.x == 0) llpart[blockIdx.x] = tot;
}

/* M step numerators: sum_i vik * n_ic (em_alg.c:972-986), lane = allele column, vik row wave-uniform */
template <int PL>
__global__ __launch_bounds__(MCHIP_BLOCK) void k_mix_column(mchip_pass_args a)
{
	if (a.stop && *a.stop) return;		/* batched run already stopped (wave-uniform) */
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
		geno_group<PL> g;
		g.load(a.gtA, (size_t)ib * a.L + l, pl);
#pragma unroll 4
		for (int j = 0; j < 8; j++) {
			const int i = min(ib * 8 + j, a.I - 1);
			const double *__restrict__ v = a.Q + (size_t)i * K;	/* vik row, wave-uniform */
			const double n = (double)g.count(j, m, pl);
#pragma unroll
			for (int k = 0; k < K; k++) acc[k] = __builtin_fma(v[k], n, acc[k]);
		}
	}
	if (valid) {
		double *out = a.Apart + ((size_t)blockIdx.y * a.T + c) * K;
#pragma unroll
		for (int k = 0; k < K; k++) out[k] = acc[k];
	}
}

}  // namespace

#endif
