/*
 * mchip_em.hip -- the EM step: the K-independent reductions and finalisers behind the passes of mchip_kernels_k.hip (kernels_k/), the E step of
 * either model with its M step (run_estep, run_mixture), graph capture, and the entry points that run steps and take log likelihoods.
 */
#include "mchip_context.h"
#include "mchip_finalize.h"

#include <math.h>

__global__ __launch_bounds__(MCHIP_BLOCK) void k_reduce_sum(const double *__restrict__ in, int n, double *out, const int *stop = nullptr)
{
	__shared__ double red[MCHIP_BLOCK];
	if (stop && *stop) return;
	const double v = block_ordered_sum(in, n, red);
	if (threadIdx.x == 0) *out = v;
}
/* out[r] = the sum of row r of in [gridDim.x][n]: block r is k_reduce_sum on its row */
__global__ __launch_bounds__(MCHIP_BLOCK) void k_reduce_rows(const double *__restrict__ in, int n, double *__restrict__ out)
{
	__shared__ double red[MCHIP_BLOCK];
	const double v = block_ordered_sum(in + (size_t)blockIdx.x * n, n, red);
	if (threadIdx.x == 0) out[blockIdx.x] = v;
}

/* out[e] = sum over slabs of slabs[j][e], in a fixed order: a block handles 32 elements x 8 slab lanes (lane s adds
 * slabs s, s+8, ...; the 8 partial sums are then added in lane order), so the many per-chunk partial-sum slabs of the
 * individual pass are combined with element- AND slab-level parallelism instead of one serial loop per individual */
__global__ __launch_bounds__(MCHIP_BLOCK) void k_sum_slabs(const double *__restrict__ slabs, int n_slabs, size_t n, double *out,
		const int *stop)
{
	__shared__ double part[8][32];
	if (stop && *stop) return;
	const int e_local = threadIdx.x & 31, s = threadIdx.x >> 5;
	const size_t e = (size_t)blockIdx.x * 32 + e_local;
	double acc = 0.0;
	if (e < n && s < n_slabs) acc = ordered_sum(0.0, slabs, (size_t)s * n + e, 8 * n, (n_slabs - s + 7) / 8);
	part[s][e_local] = acc;
	__syncthreads();
	if (s == 0 && e < n) {
		double t = part[0][e_local];
#pragma unroll
		for (int x = 1; x < 8; x++) t += part[x][e_local];
		out[e] = t;
	}
}

/* P[to][l,.][k] = normalise(P[from] * sum_chunks Apart) then project (em_alg.c:706-752); thread = (l,k).  Loci with at most 8
 * alleles (nearly always) are summed, normalised and projected in registers and written once; longer ones go through memory */
__global__ __launch_bounds__(MCHIP_BLOCK) void k_finalize_p(int L, int K, int T, const int32_t *__restrict__ toff,
		int n_ichunks, const double *__restrict__ Apart, const double *Pfrom, double *Pto,
		int weighted, double add_lb, int do_projection, double lb, uint8_t *flags, const int *stop = nullptr)
{
	const size_t idx = (size_t)blockIdx.x * MCHIP_BLOCK + threadIdx.x;
	if (idx >= (size_t)L * K || (stop && *stop)) return;
	const int k = (int)(idx % K);
	const int l = (int)(idx / K);
	const int c0 = toff[l], M = toff[l + 1] - c0;
	double temp = 0.0;
	if (M <= 8) {
		double v[8];
#pragma unroll
		for (int m = 0; m < 8; m++) {
			v[m] = 0.0;
			if (m < M) {
				const size_t e = (size_t)(c0 + m) * K + k;
				double s = ordered_sum(0.0, Apart, e, (size_t)T * K, n_ichunks);
				if (weighted) s *= Pfrom[e];
				s += add_lb;
				v[m] = s;
				temp += s;
			}
		}
#pragma unroll
		for (int m = 0; m < 8; m++)
			if (m < M) v[m] /= temp;
		if (do_projection) michelot_small(v, M, lb);
#pragma unroll
		for (int m = 0; m < 8; m++)
			if (m < M) Pto[(size_t)(c0 + m) * K + k] = v[m];
		return;
	}
	for (int m = 0; m < M; m++) {
		const size_t e = (size_t)(c0 + m) * K + k;
		double s = ordered_sum(0.0, Apart, e, (size_t)T * K, n_ichunks);
		if (weighted) s *= Pfrom[e];
		s += add_lb;		/* mixture M step starts every sum at p_lower_bound (em_alg.c:972); 0 otherwise */
		Pto[e] = s;
		temp += s;
	}
	for (int m = 0; m < M; m++) Pto[(size_t)(c0 + m) * K + k] /= temp;
	if (do_projection) michelot_strided(Pto + (size_t)c0 * K + k, K, M, lb, flags ? flags + (size_t)c0 * K + k : nullptr);
}

/* k_finalize_p with the memory side done by whole blocks (mchip_finalize.h: finalize_p_tile_body) */
__global__ __launch_bounds__(MCHIP_BLOCK) void k_finalize_p_tile(int L, int K, int T, const int32_t *__restrict__ toff, int loci_per_block,
		int n_slabs, const double *__restrict__ Apart, const double *Pfrom, double *Pto,
		int weighted, double add_lb, int do_projection, double lb, const int *stop = nullptr)
{
	__shared__ double tile[FP_TILE];
	if (stop && *stop) return;
	finalize_p_tile_body(blockIdx.x, tile, L, K, T, toff, loci_per_block, n_slabs, Apart, Pfrom, Pto, weighted, add_lb, do_projection, lb);
}

/* projection of every (l,k) block of a P slot (accelerated updates, accel_em.c:474-475) */
__global__ __launch_bounds__(MCHIP_BLOCK) void k_project_p(int L, int K, const int32_t *__restrict__ toff, double *P,
		double lb, uint8_t *flags, const int *stop = nullptr)
{
	const size_t idx = (size_t)blockIdx.x * MCHIP_BLOCK + threadIdx.x;
	if (idx >= (size_t)L * K || (stop && *stop)) return;
	const int k = (int)(idx % K);
	const int l = (int)(idx / K);
	const int c0 = toff[l], M = toff[l + 1] - c0;
	if (M <= 8) {
		double v[8];
#pragma unroll
		for (int m = 0; m < 8; m++) v[m] = m < M ? P[(size_t)(c0 + m) * K + k] : 0.0;
		michelot_small(v, M, lb);
#pragma unroll
		for (int m = 0; m < 8; m++)
			if (m < M) P[(size_t)(c0 + m) * K + k] = v[m];
		return;
	}
	michelot_strided(P + (size_t)c0 * K + k, K, M, lb, flags ? flags + (size_t)c0 * K + k : nullptr);
}

/* shared eta (eta_constrained): eta_k = sum_i S_ik / sum, project (em_alg.c:604-648): one block per k */
__global__ __launch_bounds__(MCHIP_BLOCK) void k_column_sums(const double *__restrict__ sik, int I, int K, double *out, const int *stop = nullptr)
{
	__shared__ double red[MCHIP_BLOCK];
	if (stop && *stop) return;
	const int k = blockIdx.x;
	double s = 0.0;
	for (int i = threadIdx.x; i < I; i += MCHIP_BLOCK) s += sik[(size_t)i * K + k];
	block_tree_sum<MCHIP_BLOCK>(red, s);
	if (threadIdx.x == 0) out[k] = red[0];
}
__global__ void k_normalize_row(const double *__restrict__ sums, int K, double *eta, const int *stop = nullptr, double add = 0.0)
{
	if (threadIdx.x || blockIdx.x || (stop && *stop)) return;
	double temp = 0.0;
	for (int k = 0; k < K; k++) temp += sums[k] + add;
	for (int k = 0; k < K; k++) eta[k] = (sums[k] + add) / temp;
}

/* mixture model: log P table; the E step skips p == 0 cells (em_alg.c:797-804), logL_mixture does not
 * (log_likelihood.c:197-200) */
__global__ void k_logp(const double *__restrict__ p, double *__restrict__ out, size_t n, int skip_zero, const int *stop = nullptr)
{
	const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= n || (stop && *stop)) return;
	const double v = p[idx];
	out[idx] = (skip_zero && v == 0.0) ? 0.0 : log(v);
}

/* stop() + stop_condition() + converged() of em_alg.c:101-182 on the device (time limit excepted).  One block: when `part` is
 * given the block first sums the E step's n partial log likelihoods exactly as k_reduce_sum does (same strided order, same tree:
 * the batched loops stay bit-identical to the call-by-call ones) and stores the sum in *ll -- one launch less per iteration,
 * which is what a small data set's step time is made of; then thread 0 applies the rule. */
__global__ __launch_bounds__(MCHIP_BLOCK) void k_stop_check(mchip_run_state *s, double *ll, const double *__restrict__ part = nullptr, int n = 0)
{
	__shared__ double red[MCHIP_BLOCK];
	if (s->stopped) return;		/* uniform */
	double loglik = 0.0;
	if (part) loglik = block_ordered_sum(part, n, red);
	if (threadIdx.x) return;
	if (part) *ll = loglik;
	else loglik = *ll;
	s->n_iter++;
	if (loglik != loglik) {
		s->fatal = 1;
		s->bad_loglik = loglik;
		s->stopped = 1;
		return;
	}
	int stop;
	if (s->max_iter && s->n_iter > s->max_iter) {
		s->iter_stop = 1;
		stop = 1;
	} else {
		double abs_diff = 0, rel_diff = 0;
		stop = 1;
		if (s->abs_error != 0) abs_diff = fabs(loglik - s->logL);
		if (s->rel_error != 0) rel_diff = abs_diff / fabs(s->logL);
		if (s->abs_error != 0 && abs_diff > s->abs_error) stop = 0;
		if (s->rel_error != 0 && rel_diff > s->rel_error) stop = 0;
		if (stop) s->converged = 1;
	}
	s->stopped = stop;
	if (loglik < s->logL && !stop) {
		s->fatal = 2;
		s->bad_loglik = loglik;
		s->stopped = 1;
		return;
	}
	s->logL = loglik;
}

/* P[to] from n_slabs slabs of N-side sums: the tiled form where the data set allows it */
static void launch_finalize_p(mchip_context *ctx, int n_slabs, const double *slabs, int from, int to, int weighted, double add_lb,
			      int do_projection, const int *stop)
{
	const int per = finalize_p_loci(ctx->K, ctx->max_M);
	if (per)
		hipLaunchKernelGGL(k_finalize_p_tile, dim3((ctx->L + per - 1) / per), dim3(MCHIP_BLOCK), 0, ctx->stream,
				   ctx->L, ctx->K, ctx->T, ctx->d_toff, per, n_slabs, slabs, ctx->d_p[from], ctx->d_p[to],
				   weighted, add_lb, do_projection, ctx->p_lb, stop);
	else
		hipLaunchKernelGGL(k_finalize_p, dim3(nblk((size_t)ctx->L * ctx->K)), dim3(MCHIP_BLOCK), 0, ctx->stream,
				   ctx->L, ctx->K, ctx->T, ctx->d_toff, n_slabs, slabs, ctx->d_p[from], ctx->d_p[to],
				   weighted, add_lb, do_projection, ctx->p_lb, ctx->d_flags, stop);
}
/* the hard partition's: k_finalize_p itself whatever the data set, in place in slot `to`, unweighted, with the byte flags */
void launch_finalize_p_untiled(mchip_context *ctx, int n_slabs, int to, double add_lb, int do_projection)
{
	hipLaunchKernelGGL(k_finalize_p, dim3(nblk((size_t)ctx->L * ctx->K)), dim3(MCHIP_BLOCK), 0, ctx->stream,
			   ctx->L, ctx->K, ctx->T, ctx->d_toff, n_slabs, ctx->d_Apart, ctx->d_p[to], ctx->d_p[to],
			   0, add_lb, do_projection, ctx->p_lb, ctx->d_flags);
}
void launch_reduce_sum(mchip_context *ctx, const double *in, int n, double *out)
{
	hipLaunchKernelGGL(k_reduce_sum, dim3(1), dim3(MCHIP_BLOCK), 0, ctx->stream, in, n, out, (const int *)nullptr);
}
void launch_reduce_rows(mchip_context *ctx, const double *in, int n_rows, int n, double *out)
{
	hipLaunchKernelGGL(k_reduce_rows, dim3((unsigned)n_rows), dim3(MCHIP_BLOCK), 0, ctx->stream, in, n, out);
}

/* out[0 .. count) = the `count` doubles of d_scalars that begin at `field`; a null out asks for nothing: no copy, no wait */
int fetch_scalars(mchip_context *ctx, const double *field, int count, double *out)
{
	if (!out) return MCHIP_OK;
	HIPCHK(hipMemcpyAsync(ctx->h_pinned, field, count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	for (int x = 0; x < count; x++) out[x] = ctx->h_pinned[x];
	return MCHIP_OK;
}

/* shared eta: eta[to] = normalise(sum_i S_ik), project (em_alg.c:604-648) */
int finalize_shared_eta(mchip_context *ctx, int to, const int *stop, double add, int project)
{
	double *sums = ctx->d_scalars->eta_sums;	/* one per block of k_column_sums: K <= MCHIP_MAX_K of them */
	hipLaunchKernelGGL(k_column_sums, dim3(ctx->K), dim3(MCHIP_BLOCK), 0, ctx->stream, ctx->d_sik, ctx->I, ctx->K, sums, stop);
	hipLaunchKernelGGL(k_normalize_row, dim3(1), dim3(64), 0, ctx->stream, sums, ctx->K, ctx->d_q[to], stop, add);
	if (ctx->do_projection && project) ctx->kt->project_q(1, ctx->K, ctx->d_q[to], ctx->eta_lb, stop, ctx->stream);
	HIPCHK(hipGetLastError());
	return MCHIP_OK;
}

/* *ll (a field of d_scalars) = the sum of the n partial log likelihoods a pass left in d_llpart */
static void reduce_ll(mchip_context *ctx, int n, double *ll, const int *stop)
{
	hipLaunchKernelGGL(k_reduce_sum, dim3(1), dim3(MCHIP_BLOCK), 0, ctx->stream, ctx->d_llpart, n, ll, stop);
}
/* the stop rule of the batched loops on the E step that has just run; it adds that step's partial log likelihoods up itself */
void stop_check(mchip_context *ctx)
{
	hipLaunchKernelGGL(k_stop_check, dim3(1), dim3(MCHIP_BLOCK), 0, ctx->stream, ctx->d_run, &ctx->d_scalars->logL, ctx->d_llpart, ctx->ll_parts);
}

/* one pass that takes the log likelihood (kt->accum_q or kt->loglik), between the marks of a profiled run; ll given: its partial
 * sums' sum goes to that field of d_scalars (else the caller's next kernel adds them up) */
void ll_pass(mchip_context *ctx, int kind, ll_pass_fn launch, const mchip_pass_args &a, const mchip_plan &p, double *ll, const int *stop)
{
	prof_mark(ctx, kind, true);
	launch(a, p, ctx->stream);
	prof_mark(ctx, kind, false);
	if (ll) reduce_ll(ctx, p.ll_parts, ll, stop);
}

/* mixture model: E step (mode 0, optionally followed by the M step) or logL_mixture (mode 1); ll: the field of d_scalars that
 * receives the log likelihood, by default logL for an E step and emll for logL_mixture */
int run_mixture(mchip_context *ctx, int from, int to, int do_mstep, int mode, const int *stop, double *ll, bool defer_ll)
{
	if (!ll) ll = mode ? &ctx->d_scalars->emll : &ctx->d_scalars->logL;
	const size_t KT = (size_t)ctx->K * ctx->T;
	hipLaunchKernelGGL(k_logp, dim3(nblk(KT)), dim3(256), 0, ctx->stream, ctx->d_p[from], ctx->d_logp, KT, mode == 0, stop);
	mchip_pass_args a = pass_args(ctx, from);
	a.P = ctx->d_logp;
	a.stop = stop;
	const mchip_plan plan = plan_for(ctx->kt, a, ctx->knob);
	prof_mark(ctx, mode == 0 ? MCHIP_KERN_ACCUM_Q : MCHIP_KERN_LOGLIK, true);
	ctx->kt->mix_gather(a, plan, ctx->stream);
	prof_mark(ctx, mode == 0 ? MCHIP_KERN_ACCUM_Q : MCHIP_KERN_LOGLIK, false);
	const int nb = mix_ll_parts(ctx->I);
	ctx->kt->mix_finalize(ctx->I, ctx->geo.n_lchunks, ctx->d_Spart, ctx->d_q[from], ctx->d_sik, ctx->d_llpart, mode, stop, ctx->stream);
	ctx->ll_parts = nb;
	if (!defer_ll) reduce_ll(ctx, nb, ll, stop);
	if (do_mstep) {
		int rc = finalize_shared_eta(ctx, to, stop);		/* em_alg.c:916-962 */
		if (rc) return rc;
		mchip_pass_args b = pass_args(ctx, from);
		b.Q = ctx->d_sik;				/* vik rows */
		b.qstride = ctx->K;
		b.stop = stop;
		prof_mark(ctx, MCHIP_KERN_ACCUM_P, true);
		ctx->kt->mix_column(b, plan, ctx->stream);
		prof_mark(ctx, MCHIP_KERN_ACCUM_P, false);
		launch_finalize_p(ctx, plan.mix_col_slabs, ctx->d_Apart, from, to, 0, ctx->p_lb, ctx->do_projection, stop);
	}
	HIPCHK(hipGetLastError());
	if (mode == 0) ctx->have_ll = 1;
	return MCHIP_OK;
}

/* defer_ll: the caller's k_stop_check sums the partial log likelihoods (ctx->ll_parts of them in d_llpart) itself */
int run_estep(mchip_context *ctx, int from, int to, int do_mstep, const int *stop, const int *skip_ind, bool defer_ll)
{
	if (!ctx->admixture) return run_mixture(ctx, from, to, do_mstep, 0, stop, nullptr, defer_ll);
	mchip_pass_args a = pass_args(ctx, from);
	a.stop = stop;
	a.skip_ind = skip_ind;
	const mchip_plan plan = plan_for(ctx->kt, a, ctx->knob);
	const int indiv = ctx->qstride != 0;
	double *ll = defer_ll ? nullptr : &ctx->d_scalars->logL;
	const estep_finish fin = finish_for(plan, ctx->K, ctx->max_M, indiv, do_mstep, ctx->knob);
	/* the individual pass over these very parameters already ran (mchip_loglik_prefetch): its sums are in Spart, its log likelihood
	 * in d_scalars->ll_point */
	const bool s_cached = !plan.col.ll && do_mstep && !stop && ctx->s_cache_slot == from;
	if (do_mstep && !s_cached && plan.pair) {
		/* both passes of this E step as one launch (k_estep_pair: the same bodies, the same bits).  The choice depends on the model
		 * and the data set alone: captured, eager and call-by-call steps take it alike */
		unsigned long long *marks = nullptr;
		if (ctx->profiling) {
			int rc = pair_profile_slot(ctx, plan.pair_blocks, &marks);
			if (rc) return rc;
		}
		ctx->kt->estep_pair(a, plan, marks, ctx->stream);
		if (marks) launch_pair_spans(ctx, marks, plan);
		ctx->ll_parts = plan.ll_parts;
		if (ll) reduce_ll(ctx, plan.ll_parts, ll, stop);
	} else {
		/* the column pass: N-side sums of an M step; where it is the pass that takes the log likelihood, on every E step */
		if (do_mstep || plan.col.ll) {
			prof_mark(ctx, MCHIP_KERN_ACCUM_P, true);
			if (do_mstep) ctx->kt->accum_p(a, plan, ctx->stream); else ctx->kt->loglik(a, plan, ctx->stream);
			prof_mark(ctx, MCHIP_KERN_ACCUM_P, false);
		}
		if (s_cached) {
			HIPCHK(hipMemcpyAsync(&ctx->d_scalars->logL, &ctx->d_scalars->ll_point, sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
		} else {
			ll_pass(ctx, MCHIP_KERN_ACCUM_Q, ctx->kt->accum_q, a, plan, ll, stop);
			ctx->ll_parts = plan.ll_parts;
		}
	}
	ctx->s_cache_slot = -1;		/* Spart is consumed below; slot `to` is about to change */
	ctx->have_ll = 1;
	if (fin.fused) {
		mchip_finalize_p_args p;
		p.L = ctx->L; p.K = ctx->K; p.T = ctx->T; p.loci_per_block = fin.p_loci; p.n_slabs = plan.col_slabs; p.weighted = 1;
		p.do_projection = ctx->do_projection; p.toff = ctx->d_toff; p.Apart = ctx->d_Apart; p.Pfrom = ctx->d_p[from];
		p.Pto = ctx->d_p[to]; p.add_lb = 0.0; p.lb = ctx->p_lb;
		ctx->kt->finalize_qp(ctx->I, plan.ind_slabs, ctx->d_Spart, ctx->d_q[from], ctx->qstride, ctx->d_q[to], ctx->d_sik,
				     ctx->do_projection, ctx->eta_lb, p, stop, ctx->stream);
		ctx->empty_rows_nan[to] = 1;
		HIPCHK(hipGetLastError());
		return MCHIP_OK;
	}
	/* k_finalize_q adds the slabs itself, eight threads per individual (no slab-sum launch in front of it: at config 2 that launch
	 * was 4 of the 137 us of a step, at config 3 two of the cycle's small kernels) */
	ctx->kt->finalize_q(ctx->I, ctx->K, plan.ind_slabs, ctx->d_Spart, ctx->d_q[from], ctx->qstride,
			    ctx->d_q[to], ctx->d_sik, do_mstep && indiv, 1, ctx->do_projection, ctx->eta_lb, stop, ctx->stream, 0.0);
	if (do_mstep && indiv) ctx->empty_rows_nan[to] = 1;
	if (do_mstep) {
		if (!indiv) {
			int rc = finalize_shared_eta(ctx, to, stop);
			if (rc) return rc;
		}
		if (fin.slab_sum) {
			/* many N-side slabs: k_sum_slabs adds them at 5 TB/s (element- and slab-level parallelism, fully coalesced; the
			 * (l, k) threads of k_finalize_p reach 2.7 TB/s on the same bytes), k_finalize_p then reads one slab */
			const size_t n = (size_t)ctx->K * ctx->T;
			hipLaunchKernelGGL(k_sum_slabs, dim3(nblk(n, 32)), dim3(MCHIP_BLOCK), 0, ctx->stream, ctx->d_Apart, plan.col_slabs, n, ctx->d_stage, stop);
			launch_finalize_p(ctx, 1, ctx->d_stage, from, to, 1, 0.0, ctx->do_projection, stop);
		} else {
			launch_finalize_p(ctx, plan.col_slabs, ctx->d_Apart, from, to, 1, 0.0, ctx->do_projection, stop);
		}
	}
	HIPCHK(hipGetLastError());
	return MCHIP_OK;
}

/* A launch-bound sequence as a hipGraph: unless *exec holds one, what enqueue() puts on the stream is captured into it.  Returns
 * whether there is a graph to launch; if not (capture unavailable, or enqueue failed) the caller enqueues eagerly, and no error of
 * the attempt is left behind for its HIPCHK(hipGetLastError()). */
bool captured(mchip_context *ctx, hipGraphExec_t *exec, const std::function<int()> &enqueue)
{
	hipGraph_t graph = nullptr;
	if (*exec || MCHIP_WAIT(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal)) != hipSuccess) return *exec != nullptr;
	const int rc = enqueue();
	const hipError_t e = MCHIP_WAIT(hipStreamEndCapture(ctx->stream, &graph));
	if (rc || e != hipSuccess || !graph || MCHIP_WAIT(hipGraphInstantiate(exec, graph, nullptr, nullptr, 0)) != hipSuccess) *exec = nullptr;
	if (graph) (void)MCHIP_WAIT(hipGraphDestroy(graph));
	(void)hipGetLastError();
	return *exec != nullptr;
}

int project_slot(mchip_context *ctx, int to, const int *stop)
{
	if (!ctx->do_projection) return MCHIP_OK;
	hipLaunchKernelGGL(k_project_p, dim3(nblk((size_t)ctx->L * ctx->K)), dim3(MCHIP_BLOCK), 0, ctx->stream,
			   ctx->L, ctx->K, ctx->d_toff, ctx->d_p[to], ctx->p_lb, ctx->d_flags, stop);
	ctx->kt->project_q(ctx->qstride ? ctx->I : 1, ctx->K, ctx->d_q[to], ctx->eta_lb, stop, ctx->stream);
	HIPCHK(hipGetLastError());
	return MCHIP_OK;
}

extern "C" {

int mchip_em_run(mchip_context *ctx, int slot, int n_steps, mchip_run_state *state)
{
	MCHIP_ENTRY();
	int rc = check_slot(ctx, slot);
	if (rc) return rc;
	if (!state || n_steps < 1) return fail(ctx, MCHIP_ERR_INVALID, "em_run: bad arguments%s", nullptr);
	if (ctx->qstride) ctx->empty_rows_nan[slot] = 1;	/* (set here too: a replayed graph does not pass through the enqueueing code) */
	HIPCHK(hipSetDevice(ctx->device));
	HIPCHK(hipMemcpyAsync(ctx->d_run, state, sizeof *state, hipMemcpyHostToDevice, ctx->stream));
	const int *stop = &ctx->d_run->stopped;
	/* The step is a launch-bound chain of 6-7 kernels on small data sets: capture it once into a hipGraph and replay it
	 * (eager launches cost ~8 us of host time each here, graph nodes ~1.5 us of device time).  Event marks cannot be
	 * captured, so profiled runs stay eager. */
	const auto step = [&] { const int r = run_estep(ctx, slot, slot, 1, stop, nullptr, true); if (!r) stop_check(ctx); return r; };
	const bool use_graph = !ctx->profiling && n_steps >= 4 && !ctx->knob.no_graph && captured(ctx, &ctx->step_graph[slot], step);
	for (int s = 0; s < n_steps; s++) {
		if (use_graph) HIPCHK(hipGraphLaunch(ctx->step_graph[slot], ctx->stream));
		else if ((rc = step())) return rc;
	}
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(state, ctx->d_run, sizeof *state, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	return MCHIP_OK;
}

int mchip_em_step(mchip_context *ctx, int from, int to, double *loglik)
{
	MCHIP_ENTRY();
	int rc = check_slot(ctx, from);
	if (rc) return rc;
	if ((rc = check_slot(ctx, to))) return rc;
	HIPCHK(hipSetDevice(ctx->device));
	if ((rc = run_estep(ctx, from, to, 1))) return rc;
	if (ctx->qstride) ctx->empty_rows_nan[to] = 1;
	return fetch_scalars(ctx, &ctx->d_scalars->logL, 1, loglik);
}

int mchip_last_loglik(mchip_context *ctx, double *loglik)
{
	MCHIP_ENTRY();
	if (!ctx || !loglik) return MCHIP_ERR_INVALID;
	if (!ctx->have_ll) return fail(ctx, MCHIP_ERR_STATE, "no log likelihood computed yet%s", nullptr);
	HIPCHK(hipSetDevice(ctx->device));
	return fetch_scalars(ctx, &ctx->d_scalars->logL, 1, loglik);
}

int mchip_e_step(mchip_context *ctx, int slot, double *loglik)
{
	MCHIP_ENTRY();
	int rc = check_slot(ctx, slot);
	if (rc) return rc;
	HIPCHK(hipSetDevice(ctx->device));
	if ((rc = run_estep(ctx, slot, slot, 0))) return rc;
	return fetch_scalars(ctx, &ctx->d_scalars->logL, 1, loglik);
}

int mchip_loglik(mchip_context *ctx, int slot, double *loglik)
{
	MCHIP_ENTRY();
	int rc = check_slot(ctx, slot);
	if (rc) return rc;
	HIPCHK(hipSetDevice(ctx->device));
	if (!ctx->admixture) {
		if ((rc = run_mixture(ctx, slot, slot, 0, 1))) return rc;
		return fetch_scalars(ctx, &ctx->d_scalars->emll, 1, loglik);
	}
	const mchip_pass_args a = pass_args(ctx, slot);
	ll_pass(ctx, MCHIP_KERN_LOGLIK, ctx->kt->loglik, a, plan_for(ctx->kt, a, ctx->knob), &ctx->d_scalars->emll);
	HIPCHK(hipGetLastError());
	return fetch_scalars(ctx, &ctx->d_scalars->emll, 1, loglik);
}

int mchip_loglik_prefetch(mchip_context *ctx, int slot, double *loglik)
{
	MCHIP_ENTRY();
	int rc = check_slot(ctx, slot);
	if (rc) return rc;
	const mchip_pass_args a = pass_args(ctx, slot);
	const mchip_plan plan = plan_for(ctx->kt, a, ctx->knob);
	if (!ctx->admixture || plan.col.ll) return mchip_loglik(ctx, slot, loglik);	/* nothing to share on those paths */
	HIPCHK(hipSetDevice(ctx->device));
	ll_pass(ctx, MCHIP_KERN_ACCUM_Q, ctx->kt->accum_q, a, plan, &ctx->d_scalars->ll_point);	/* S-side sums -> Spart */
	HIPCHK(hipGetLastError());
	ctx->s_cache_slot = slot;
	return fetch_scalars(ctx, &ctx->d_scalars->ll_point, 1, loglik);
}

}	/* extern "C" */
