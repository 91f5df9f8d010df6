/*
 * mchip_query.hip -- mixing proportions of listed individuals with the allele frequencies held fixed: mchip_fit_q_rows and
 * its kernels (include/multiclust_hip.h has the contract; mchip_context.h the per-context state).  Given P the individuals are
 * independent concave problems in K numbers each, so a row is fitted to its own convergence inside one launch.
 *
 *   k_query_gather   a thread per byte: the listed individuals' genotype bytes into a contiguous [n_rows][L][ploidy], read from
 *                    the saved upload-form data set (a hold-out is in force) or from gtA.  The fit then has one input form and
 *                    reads consecutive bytes; n_rows L ploidy bytes of scratch.
 *   k_fit_q_rows     one workgroup of four waves per row, K in buckets of 8, 16, 32 and 64 (the lane's K accumulators are a
 *                    register array; K itself is a run-time argument).  q sits in LDS between iterations and in registers during
 *                    a pass.  Lane x walks the loci l = x, x + 256, ...: toff[l], the copy's allele byte, the K contiguous
 *                    doubles of P's column, t = sum_k q_k p_k by an fma chain in k order, then a_k += p_k (1 / t) and the sum of
 *                    log t in registers; q_k is multiplied in once, after the reduction.  The lanes of a wave are added by a
 *                    shuffle tree (offsets 32, 16, ... 1), the four waves in wave order by thread 0, which then does the update --
 *                    finalize_q_body's arithmetic: s_k = a_k q_k, the sum over k in k order, s_k / sum, the simplex projection
 *                    (michelot_strided) -- and the stopping test, mc_converged's rule on this row's own log likelihood.  The loop
 *                    goes on without leaving the kernel; max_iter bounds it.
 *                    No floating-point atomics, every sum in an order fixed by (L, ploidy, K): the same state gives the same bits.
 *                    Not yet timed on a device (profiles/query_fit.txt, scripts/query_fit_bench.py).
 */
#include "mchip_context.h"
#include "mchip_finalize.h"

/* out[r][l][a] = genotype byte (rows[r], l, a), from the upload form [I][L][ploidy] (upload_form != 0) or from gtA */
__global__ __launch_bounds__(256) void k_query_gather(const uint8_t *__restrict__ src, int upload_form, const int32_t *__restrict__ rows,
						      int n_rows, int L, int pl, uint8_t *__restrict__ out)
{
	const size_t per_row = (size_t)L * pl, n = (size_t)n_rows * per_row, stride = (size_t)gridDim.x * 256;
	for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += stride) {
		const size_t r = idx / per_row, rem = idx % per_row;
		const size_t i = (size_t)rows[r], l = rem / pl, a = rem % pl;
		out[idx] = upload_form ? src[i * per_row + rem] : src[(((i >> 3) * L + l) * 8 + (i & 7)) * (size_t)pl + a];
	}
}

constexpr int FQR_THREADS = 256, FQR_WAVES = FQR_THREADS / 64;

/* the 64 lanes of a wave in a fixed tree; lane 0 holds the sum */
__device__ __forceinline__ double fqr_wave_sum(double v)
{
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
	return v;
}
__device__ __forceinline__ int fqr_wave_sum(int v)
{
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
	return v;
}

/* one workgroup per row of geno [n_rows][L][ploidy]; P a slot's [T][K]; Q0 a slot's [I][K] (the row rows[r] is the start) or NULL
 * (1 / K); the four outputs are device arrays ([n_rows][K], [n_rows], [n_rows], [n_rows]) */
template <int KB>
__global__ __launch_bounds__(FQR_THREADS) void k_fit_q_rows(int L, int pl, int K, const uint8_t *__restrict__ geno, const int32_t *__restrict__ toff,
		const double *__restrict__ P, const double *__restrict__ Q0, const int32_t *__restrict__ rows, int do_projection, double lb,
		int max_iter, double abs_error, double rel_error, double *__restrict__ q_out, double *__restrict__ ll_out,
		int32_t *__restrict__ iter_out, uint8_t *__restrict__ conv_out)
{
	__shared__ double qs[KB];			/* q of the iteration */
	__shared__ double part[FQR_WAVES][KB + 1];	/* the waves' a_k and sum of log t */
	__shared__ int cnt_part[FQR_WAVES];		/* and observed copies */
	__shared__ double ll_now;
	__shared__ int stop_now;
	const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const uint8_t *g = geno + (size_t)r * L * pl;
	if (tid < KB) qs[tid] = tid < K ? (Q0 ? Q0[(size_t)rows[r] * K + tid] : 1.0 / K) : 0.0;
	__syncthreads();
	double prev = 0.0;
	for (int n = 0;; n++) {
		double q[KB], a[KB], ll = 0.0;
		int cnt = 0;
#pragma unroll
		for (int k = 0; k < KB; k++) {
			q[k] = qs[k];
			a[k] = 0.0;
		}
		for (int l = tid; l < L; l += FQR_THREADS) {
			const int c0 = toff[l];
			for (int c = 0; c < pl; c++) {
				const unsigned m = g[(size_t)l * pl + c];
				if (m == MCHIP_MISSING) continue;
				const double *p = P + (size_t)(c0 + (int)m) * K;
				double pv[KB], t = 0.0;
#pragma unroll
				for (int k = 0; k < KB; k++)
					if (k < K) {
						pv[k] = p[k];
						t = fma(q[k], pv[k], t);
					}
				const double rt = 1.0 / t;
#pragma unroll
				for (int k = 0; k < KB; k++)
					if (k < K) a[k] = fma(pv[k], rt, a[k]);
				ll += log(t);
				cnt++;
			}
		}
#pragma unroll
		for (int k = 0; k < KB; k++)
			if (k < K) {
				const double s = fqr_wave_sum(a[k]);
				if (lane == 0) part[wave][k] = s;
			}
		ll = fqr_wave_sum(ll);
		cnt = fqr_wave_sum(cnt);
		if (lane == 0) {
			part[wave][KB] = ll;
			cnt_part[wave] = cnt;
		}
		__syncthreads();
		if (tid == 0) {		/* the row's decision and update: uniform, serial in k */
			double lsum = part[0][KB];
			int copies = cnt_part[0];
			for (int w = 1; w < FQR_WAVES; w++) {
				lsum += part[w][KB];
				copies += cnt_part[w];
			}
			int stop = 0, conv = 0, what = 0;	/* what: 0 = q as it stands, 1 = 1 / K, 2 = NaN */
			if (!copies) {
				stop = 1;
				what = 1;
				lsum = 0.0;
			} else if (!isfinite(lsum)) {
				stop = 1;
				what = 2;
			} else {
				if (n >= 1 && (abs_error != 0 || rel_error != 0)) {
					/* mc_converged's two tests (em_alg.c:163-182), a zero error being a test not made; the difference
					 * is taken whichever test is made, and no test made is no convergence (multiclust_hip.h) */
					const double abs_diff = fabs(lsum - prev);
					conv = 1;
					if (abs_error != 0 && abs_diff > abs_error) conv = 0;
					if (rel_error != 0 && abs_diff / fabs(prev) > rel_error) conv = 0;
				}
				stop = conv || n == max_iter;
			}
			if (stop) {
				for (int k = 0; k < K; k++)
					q_out[(size_t)r * K + k] = what == 1 ? 1.0 / K : (what == 2 ? __longlong_as_double(0x7ff8000000000000ll) : qs[k]);
				ll_out[r] = lsum;
				iter_out[r] = n;
				conv_out[r] = (uint8_t)conv;
			} else {	/* finalize_q_body's arithmetic */
				double temp = 0.0;
				for (int k = 0; k < K; k++) {
					double s = part[0][k];
					for (int w = 1; w < FQR_WAVES; w++) s += part[w][k];
					s *= qs[k];
					qs[k] = s;
					temp += s;
				}
				if (temp == 0.0) {
					for (int k = 0; k < K; k++) qs[k] = 1.0 / K;
				} else {
					for (int k = 0; k < K; k++) qs[k] /= temp;
					if (do_projection) michelot_strided(qs, 1, K, lb, nullptr);	/* (K <= 64: the fixed set is a bit mask) */
				}
			}
			ll_now = lsum;
			stop_now = stop;
		}
		__syncthreads();
		if (stop_now) break;	/* (uniform over the workgroup) */
		prev = ll_now;
	}
}

extern "C" int mchip_fit_q_rows(mchip_context *ctx, int slot, const int32_t *rows, int n_rows, int from_slot, int max_iter, double abs_error,
		     double rel_error, double *q_rows, double *loglik_rows, int32_t *iter_rows, uint8_t *converged_rows)
{
	MCHIP_ENTRY();
	if (!ctx) return MCHIP_ERR_INVALID;
	const int rc = require_fit(ctx, slot, "fit_q_rows: the mixture model has no mixing proportions per individual");
	if (rc) return rc;
	if (!ctx->qstride) return fail(ctx, MCHIP_ERR_UNSUPPORTED, "fit_q_rows: the mixing proportions are shared by all individuals%s", nullptr);
	if (!rows || !q_rows || !loglik_rows || !iter_rows || !converged_rows) return fail(ctx, MCHIP_ERR_INVALID, "null pointer%s", nullptr);
	if (n_rows < 1 || n_rows > ctx->I) return fail(ctx, MCHIP_ERR_INVALID, "fit_q_rows: n_rows must be in [1, I]%s", nullptr);
	if (max_iter < 1) return fail(ctx, MCHIP_ERR_INVALID, "fit_q_rows: max_iter must be >= 1%s", nullptr);
	if (!(abs_error >= 0) || !(rel_error >= 0)) return fail(ctx, MCHIP_ERR_INVALID, "fit_q_rows: an error must be >= 0%s", nullptr);
	{
		std::vector<uint8_t> listed((size_t)ctx->I, 0);
		for (int r = 0; r < n_rows; r++) {
			if (rows[r] < 0 || rows[r] >= ctx->I) return fail(ctx, MCHIP_ERR_INVALID, "fit_q_rows: a row outside [0, I)%s", nullptr);
			if (listed[(size_t)rows[r]]) return fail(ctx, MCHIP_ERR_INVALID, "fit_q_rows: a row is listed twice%s", nullptr);
			listed[(size_t)rows[r]] = 1;
		}
	}
	HIPCHK(hipSetDevice(ctx->device));
	const int L = ctx->L, pl = ctx->ploidy, K = ctx->K;
	const size_t nr = (size_t)n_rows;
	scoped_dev<int32_t> d_rows, d_iter;
	scoped_dev<uint8_t> d_geno, d_conv;
	scoped_dev<double> d_q, d_ll;
	HIPCHK(d_rows.alloc(nr));
	HIPCHK(d_iter.alloc(nr));
	HIPCHK(d_geno.alloc(nr * L * pl));
	HIPCHK(d_conv.alloc(nr));
	HIPCHK(d_q.alloc(nr * K));
	HIPCHK(d_ll.alloc(nr));
	HIPCHK(hipMemcpyAsync(d_rows.p, rows, nr * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
	/* the full data set: the saved one while a fold is held out of the installed one */
	const bool saved = ctx->cv_fold >= 0 && ctx->cv_full.d_raw;
	hipLaunchKernelGGL(k_query_gather, dim3(nblk_capped(nr * L * pl, 256, (size_t)1 << 20)), dim3(256), 0, ctx->stream,
			   saved ? ctx->cv_full.d_raw : ctx->d_gtA, saved ? 1 : 0, d_rows.p, n_rows, L, pl, d_geno.p);
	HIPCHK(hipGetLastError());
	const double *Q0 = from_slot ? ctx->d_q[slot] : nullptr;
#define FQR_LAUNCH(KB)                                                                                                                   \
	hipLaunchKernelGGL(k_fit_q_rows<KB>, dim3((unsigned)n_rows), dim3(FQR_THREADS), 0, ctx->stream, L, pl, K, d_geno.p, ctx->d_toff, \
			   ctx->d_p[slot], Q0, d_rows.p, ctx->do_projection, ctx->eta_lb, max_iter, abs_error, rel_error, d_q.p, d_ll.p, \
			   d_iter.p, d_conv.p)
	if (K <= 8) FQR_LAUNCH(8);
	else if (K <= 16) FQR_LAUNCH(16);
	else if (K <= 32) FQR_LAUNCH(32);
	else FQR_LAUNCH(64);
#undef FQR_LAUNCH
	HIPCHK(hipGetLastError());
	/* (the rows array and the results cross in pageable memory: the copies are done when the stream is) */
	std::vector<double> h_q(nr * K), h_ll(nr);
	std::vector<int32_t> h_iter(nr);
	std::vector<uint8_t> h_conv(nr);
	HIPCHK(hipMemcpyAsync(h_q.data(), d_q.p, nr * K * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipMemcpyAsync(h_ll.data(), d_ll.p, nr * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipMemcpyAsync(h_iter.data(), d_iter.p, nr * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipMemcpyAsync(h_conv.data(), d_conv.p, nr, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	/* the caller's arrays are written once everything has succeeded */
	memcpy(q_rows, h_q.data(), nr * K * sizeof(double));
	memcpy(loglik_rows, h_ll.data(), nr * sizeof(double));
	memcpy(iter_rows, h_iter.data(), nr * sizeof(int32_t));
	memcpy(converged_rows, h_conv.data(), nr);
	return MCHIP_OK;
}
