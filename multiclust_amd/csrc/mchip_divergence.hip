/*
 * mchip_divergence.hip -- divergence of the fitted clusters from a slot's allele frequencies: mchip_divergence and its kernels
 * (include/multiclust_hip.h has the contract and the definitions; mchip_context.h the per-context state).  Both models: the
 * slot's P is [T][K] under either.  Every quantity is a sum of non-negative terms; nothing is formed by subtracting sums.
 *
 *   k_div_pairs   runtime K, one instance.  The K (K + 1) / 2 entries of the a <= b list are (a, a) -> h_a = sum_c p_a (1 - p_a) and
 *                 (a, b) -> s_ab = sum_c (p_a - p_b)^2 over the T columns.  A workgroup owns one chunk of DIV_CHUNK columns -- a
 *                 constant: the chunk, hence the order of every addition, does not depend on the device's compute units -- and
 *                 reads its part of the [T][K] slot once, DIV_STAGE columns at a time into LDS, rows lds_pitch(K) apart.  Thread t
 *                 owns entries t, t + 256, ... (at most DIV_EPT = 9 at K = 64) in registers and walks the staged columns in column
 *                 order; one partial per entry and chunk, stored [entry][chunk]; launch_reduce_rows (mchip_em.hip) adds each entry's.
 *   k_div_loci    runtime K, lane = locus; the weights sit in LDS (every lane reads the same word: a broadcast).  The M_l K doubles
 *                 of a locus are contiguous from toff[l] K.  Per column: pbar = sum_k w_k p_k as an fma chain in k order, HT +=
 *                 pbar (1 - pbar), then the K values of the column once more (they are in the cache) for V += w_k (p_k - pbar)^2:
 *                 nothing is kept per allele, so 254 alleles run in the registers of 2.  V_l and HT_l go to [L] arrays; a
 *                 workgroup's 256 loci are added by block_tree_sum (lane order = locus order), one partial of each per
 *                 workgroup, stored [2][workgroups]; launch_reduce_rows adds the two rows.
 *   No floating-point atomics anywhere: the same state gives the same bits, on any device and under any geometry knob.
 *   Timed once and not tuned (profiles/divergence.txt, scripts/divergence_bench.py): it runs once per K of a run.
 */
#include "mchip_context.h"

#include <math.h>

constexpr int DIV_CHUNK = 1024;		/* columns per workgroup of the pair kernel (tests/test_gpu_divergence.py restates it) */
constexpr int DIV_STAGE = 64;		/* of which this many are in LDS at a time: 64 (64 | 1) doubles = 33 KB at K = 64 */
constexpr int DIV_THREADS = 256;
constexpr int DIV_EPT = (MCHIP_MAX_K * (MCHIP_MAX_K + 1) / 2 + DIV_THREADS - 1) / DIV_THREADS;	/* entries per thread: 9 */

/* P: a slot's [T][K].  part[e * n_chunks + chunk]: the chunk's partial of entry e of the a <= b list (row a: b = a .. K - 1). */
__global__ __launch_bounds__(DIV_THREADS) void k_div_pairs(int T, int K, int KS, int n_pairs, const double *__restrict__ P,
							   double *__restrict__ part)
{
	extern __shared__ __attribute__((aligned(16))) double div_lds[];	/* [DIV_STAGE][KS] */
	const int tid = threadIdx.x, chunk = blockIdx.x, n_chunks = gridDim.x;
	const int cbeg = chunk * DIV_CHUNK, cend = min(T, cbeg + DIV_CHUNK);
	int ea[DIV_EPT], eb[DIV_EPT];
	double acc[DIV_EPT];
#pragma unroll
	for (int j = 0; j < DIV_EPT; j++) {
		const int e = tid + j * DIV_THREADS;
		int a = 0, rem = e < n_pairs ? e : 0;
		while (rem >= K - a) {
			rem -= K - a;
			a++;
		}
		ea[j] = a;
		eb[j] = a + rem;
		acc[j] = 0.0;
	}
	for (int c0 = cbeg; c0 < cend; c0 += DIV_STAGE) {
		const int ncols = min(DIV_STAGE, cend - c0);
		__syncthreads();	/* everybody is done with the columns staged before */
		stage_rows(div_lds, KS, P + (size_t)c0 * K, ncols, K, tid, DIV_THREADS);
		__syncthreads();
#pragma unroll
		for (int j = 0; j < DIV_EPT; j++) {
			if (tid + j * DIV_THREADS >= n_pairs) continue;
			const int a = ea[j], b = eb[j];
			double s = acc[j];
			if (a == b) {
				for (int c = 0; c < ncols; c++) {
					const double pa = div_lds[c * KS + a];
					s = fma(pa, 1.0 - pa, s);
				}
			} else {
				for (int c = 0; c < ncols; c++) {
					const double d = div_lds[c * KS + a] - div_lds[c * KS + b];
					s = fma(d, d, s);
				}
			}
			acc[j] = s;
		}
	}
#pragma unroll
	for (int j = 0; j < DIV_EPT; j++) {
		const int e = tid + j * DIV_THREADS;
		if (e < n_pairs) part[(size_t)e * n_chunks + chunk] = acc[j];
	}
}

/* w: the K weights.  lv / lht [L]: V_l and HT_l (0 for a locus without a column).  part_v / part_ht: one partial per workgroup. */
__global__ __launch_bounds__(DIV_THREADS) void k_div_loci(int L, int K, const int32_t *__restrict__ toff, const double *__restrict__ P,
							  const double *__restrict__ w, double *__restrict__ lv, double *__restrict__ lht,
							  double *__restrict__ part_v, double *__restrict__ part_ht)
{
	__shared__ double ws[MCHIP_MAX_K];
	__shared__ double red[2][DIV_THREADS];
	const int tid = threadIdx.x, l = blockIdx.x * DIV_THREADS + tid;
	if (tid < K) ws[tid] = w[tid];
	__syncthreads();
	double V = 0.0, HT = 0.0;
	if (l < L) {
		const int c0 = toff[l], c1 = toff[l + 1];
		for (int c = c0; c < c1; c++) {
			const double *__restrict__ p = P + (size_t)c * K;
			double pbar = 0.0;
			for (int k = 0; k < K; k++) pbar = fma(ws[k], p[k], pbar);
			HT = fma(pbar, 1.0 - pbar, HT);
			for (int k = 0; k < K; k++) {
				const double d = p[k] - pbar;
				V = fma(ws[k] * d, d, V);
			}
		}
		lv[l] = V;
		lht[l] = HT;
	}
	const double mine[2] = {V, HT};
	block_tree_sum<DIV_THREADS>(red[0], DIV_THREADS, mine);
	if (tid == 0) {
		part_v[blockIdx.x] = red[0][0];
		part_ht[blockIdx.x] = red[1][0];
	}
}

extern "C" int mchip_divergence(mchip_context *ctx, int slot, const double *weights, double *het, double *sqdiff, double *locus_v,
				double *locus_ht, double *sum_v, double *sum_ht, int32_t *n_loci)
{
	MCHIP_ENTRY();
	if (!ctx) return MCHIP_ERR_INVALID;
	const int rc = require_fit(ctx, slot, nullptr);	/* (both models) */
	if (rc) return rc;
	if (!weights || !het || !sqdiff || !sum_v || !sum_ht || !n_loci) return fail(ctx, MCHIP_ERR_INVALID, "null pointer%s", nullptr);
	const int L = ctx->L, T = ctx->T, K = ctx->K;
	double wsum = 0.0;
	for (int k = 0; k < K; k++) {
		if (!(weights[k] >= 0.0) || !isfinite(weights[k]))	/* (NaN is not >= 0) */
			return fail(ctx, MCHIP_ERR_INVALID, "divergence: a weight is negative, infinite or NaN%s", nullptr);
		wsum += weights[k];
	}
	if (!(wsum > 0.0)) return fail(ctx, MCHIP_ERR_INVALID, "divergence: every weight is zero%s", nullptr);
	HIPCHK(hipSetDevice(ctx->device));
	const int n_pairs = K * (K + 1) / 2, n_chunks = (T + DIV_CHUNK - 1) / DIV_CHUNK, n_lblocks = (L + DIV_THREADS - 1) / DIV_THREADS;
	const size_t lds = (size_t)DIV_STAGE * lds_pitch(K) * sizeof(double);
	scoped_dev<double> d_w, d_part, d_pair, d_lv, d_lht, d_lpart, d_sums;
	HIPCHK(d_w.alloc((size_t)K));
	HIPCHK(d_part.alloc((size_t)n_pairs * n_chunks));
	HIPCHK(d_pair.alloc((size_t)n_pairs));
	HIPCHK(d_lv.alloc((size_t)L));
	HIPCHK(d_lht.alloc((size_t)L));
	HIPCHK(d_lpart.alloc(2 * (size_t)n_lblocks));
	HIPCHK(d_sums.alloc(2));
	HIPCHK(hipMemcpyAsync(d_w.p, weights, (size_t)K * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	hipLaunchKernelGGL(k_div_pairs, dim3((unsigned)n_chunks), dim3(DIV_THREADS), lds, ctx->stream, T, K, lds_pitch(K), n_pairs, ctx->d_p[slot],
			   d_part.p);
	HIPCHK(hipGetLastError());
	launch_reduce_rows(ctx, d_part.p, n_pairs, n_chunks, d_pair.p);
	HIPCHK(hipGetLastError());
	hipLaunchKernelGGL(k_div_loci, dim3((unsigned)n_lblocks), dim3(DIV_THREADS), 0, ctx->stream, L, K, ctx->d_toff, ctx->d_p[slot], d_w.p,
			   d_lv.p, d_lht.p, d_lpart.p, d_lpart.p + n_lblocks);
	HIPCHK(hipGetLastError());
	launch_reduce_rows(ctx, d_lpart.p, 2, n_lblocks, d_sums.p);
	HIPCHK(hipGetLastError());
	std::vector<double> h_pair((size_t)n_pairs);
	double h_sums[2];
	HIPCHK(hipMemcpyAsync(h_pair.data(), d_pair.p, (size_t)n_pairs * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipMemcpyAsync(h_sums, d_sums.p, sizeof h_sums, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));	/* (the weights crossed in pageable memory: done when the stream is) */
	/* the caller's arrays are written once everything on the device has succeeded */
	if (locus_v) HIPCHK(hipMemcpyAsync(locus_v, d_lv.p, (size_t)L * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	if (locus_ht) HIPCHK(hipMemcpyAsync(locus_ht, d_lht.p, (size_t)L * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	for (int a = 0, e = 0; a < K; a++)
		for (int b = a; b < K; b++, e++) {
			if (a == b) {
				het[a] = h_pair[(size_t)e];
				sqdiff[(size_t)a * K + a] = 0.0;
			} else {
				sqdiff[(size_t)a * K + b] = sqdiff[(size_t)b * K + a] = h_pair[(size_t)e];
			}
		}
	int32_t n1 = 0;
	for (int l = 0; l < L; l++) n1 += ctx->h_ua[(size_t)l] > 0;
	*sum_v = h_sums[0];
	*sum_ht = h_sums[1];
	*n_loci = n1;
	return MCHIP_OK;
}
