/*
 * mchip_accel.hip -- the acceleration of the EM iteration (SQUAREM, quasi-Newton): secants, their dot products and the updates
 * as vector kernels, the batched cycle that takes every decision on the device, and their entry points.
 */
#include "mchip_context.h"

#include <math.h>

/* the end of a batched accelerated cycle in one single-block launch: emll (when in1 is given: the dual pass's second log
 * likelihood) -> sc->emll, the extrapolated point's log likelihood -> sc->ll_point (k_reduce_sum's sums), accept iff ll > emll */
__global__ __launch_bounds__(MCHIP_BLOCK) void k_reduce_accept(const double *__restrict__ in1, const double *__restrict__ in2, int n, mchip_scalars *sc,
		mchip_cycle_flags *cyc, const int *stop)
{
	__shared__ double red[MCHIP_BLOCK];
	if (stop && *stop) return;
	if (in1) {
		const double v = block_ordered_sum(in1, n, red);
		if (threadIdx.x == 0) sc->emll = v;
	}
	const double v2 = block_ordered_sum(in2, n, red);
	if (threadIdx.x == 0) {
		sc->ll_point = v2;
		cyc->accepted = (!cyc->no_update && sc->ll_point > sc->emll) ? 1 : 0;
	}
}

/* the 2 * nout sums of a dot-product pass in one launch (block x < nout: eta part x -> sc->dots[DOT_ETA + x]; the others: p part ->
 * sc->dots[DOT_P + .]): each block is k_reduce_sum on its array, same order, same tree */
__global__ __launch_bounds__(MCHIP_BLOCK) void k_reduce_dots(const double *__restrict__ part_q, int gq, const double *__restrict__ part_p, int gp,
		int nout, mchip_scalars *sc, const int *stop)
{
	__shared__ double red[MCHIP_BLOCK];
	if (stop && *stop) return;
	const int x = blockIdx.x;
	const double *in = x < nout ? part_q + (size_t)x * gq : part_p + (size_t)(x - nout) * gp;
	const int n = x < nout ? gq : gp;
	double *out = x < nout ? sc->dots + DOT_ETA + x : sc->dots + DOT_P + (x - nout);
	const double v = block_ordered_sum(in, n, red);
	if (threadIdx.x == 0) *out = v;
}

/* secant: out = x_to - x_from (em_alg.c:1104-1161) */
__global__ void k_diff(const double *__restrict__ a, const double *__restrict__ b, double *out, size_t n, const int *stop = nullptr)
{
	const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (stop && *stop) return;
	if (idx < n) out[idx] = a[idx] - b[idx];
}

/* three dot products of accel_em.c:143-184 (mode 0: utu, u(v-u), (v-u)^2) or the two of 291-310
 * (mode 1: u1.u2, u1.v2) over one array pair; block partials, combined by k_reduce_sum */
__global__ __launch_bounds__(MCHIP_BLOCK) void k_dots(const double *__restrict__ u, const double *__restrict__ v,
		const double *__restrict__ u2, size_t n, int mode, double *part, const int *stop = nullptr)
{
	__shared__ double red[3][MCHIP_BLOCK];
	if (stop && *stop) return;
	double s0 = 0, s1 = 0, s2 = 0;
	for (size_t x = (size_t)blockIdx.x * MCHIP_BLOCK + threadIdx.x; x < n; x += (size_t)gridDim.x * MCHIP_BLOCK) {
		if (mode == 0) {
			const double uu = u[x], d = v[x] - uu;
			s0 += uu * uu; s1 += uu * d; s2 += d * d;
		} else {
			const double uu = u[x];
			s0 += uu * u2[x]; s1 += uu * v[x];
		}
	}
	const double mine[3] = {s0, s1, s2};
	block_tree_sum<MCHIP_BLOCK>(red[0], MCHIP_BLOCK, mine);
	if (threadIdx.x == 0) {
		part[blockIdx.x] = red[0][0];
		part[gridDim.x + blockIdx.x] = red[1][0];
		part[2 * gridDim.x + blockIdx.x] = red[2][0];
	}
}

/* k_dots (mode 0) and k_accel_update of a batched cycle straight from the three iterates: u = x1 - x0 and v = x2 - x1 are formed
 * where they are used -- the values k_diff would have stored, so the sums and the update keep their bits -- and the cycle has
 * four launches and 100 MB of traffic less */
/* block `bid` of `gdim` of the dot-product pass over one array (u = x1 - x0, v = x2 - x1 formed here): grid-stride partial sums, a
 * fixed tree per block, three partials per block */
__device__ __forceinline__ void dots_slots_body(const double *__restrict__ x0, const double *__restrict__ x1, const double *__restrict__ x2,
		size_t n, double *part, unsigned bid, unsigned gdim, double (*red)[MCHIP_BLOCK])
{
	double s0 = 0, s1 = 0, s2 = 0;
	for (size_t x = (size_t)bid * MCHIP_BLOCK + threadIdx.x; x < n; x += (size_t)gdim * MCHIP_BLOCK) {
		const double uu = x1[x] - x0[x], vv = x2[x] - x1[x];
		const double d = vv - uu;
		s0 += uu * uu; s1 += uu * d; s2 += d * d;
	}
	const double mine[3] = {s0, s1, s2};
	block_tree_sum<MCHIP_BLOCK>(red[0], MCHIP_BLOCK, mine);
	if (threadIdx.x == 0) {
		part[bid] = red[0][0];
		part[gdim + bid] = red[1][0];
		part[2 * gdim + bid] = red[2][0];
	}
}
/* the eta part (blocks 0 .. gq-1) and the p part (the other gp blocks) of the step-size dot products in one launch; every block
 * does what it did when the two parts were two launches */
__global__ __launch_bounds__(MCHIP_BLOCK) void k_dots_slots(const double *__restrict__ q0, const double *__restrict__ q1,
		const double *__restrict__ q2, size_t nq, double *part_q, unsigned gq, const double *__restrict__ p0,
		const double *__restrict__ p1, const double *__restrict__ p2, size_t np, double *part_p, const int *stop)
{
	__shared__ double red[3][MCHIP_BLOCK];
	if (stop && *stop) return;
	if (blockIdx.x < gq) dots_slots_body(q0, q1, q2, nq, part_q, blockIdx.x, gq, red);
	else dots_slots_body(p0, p1, p2, np, part_p, blockIdx.x - gq, gridDim.x - gq, red);
}
/* x_B = x_A - 2 s u + s^2 (v - u) (or x_A + u + s v) for the eta array (threads below nq) and the p array in one launch */
__global__ void k_accel_update_slots(const double *__restrict__ q0, const double *q1, const double *__restrict__ q2, double *qout, size_t nq,
				     const double *__restrict__ p0, const double *p1, const double *__restrict__ p2, double *pout, size_t np,
				     int qn_form, const double *s_dev, const int *stop)
{
#pragma clang fp contract(off)
	size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= nq + np || (stop && *stop)) return;
	const double *x0 = q0, *x1 = q1, *x2 = q2;
	double *out = qout;
	if (idx >= nq) { idx -= nq; x0 = p0; x1 = p1; x2 = p2; out = pout; }
	const double s = *s_dev;
	const double u = x1[idx] - x0[idx], v = x2[idx] - x1[idx];	/* (out may be x1: read before written, element by element) */
	if (qn_form) out[idx] = x0[idx] + u + s * v;
	else out[idx] = x0[idx] - 2 * s * u + s * s * (v - u);
}

/* accel_em.c:444-541 element updates (projection follows in k_project_*).  Evaluated exactly as the reference's expression
 * (left to right, every product and sum rounded: no fused multiply-add): where the extrapolation cancels to about zero, the
 * last bits decide whether the projection clamps the entry to the lower bound */
__global__ void k_accel_update(const double *__restrict__ base, const double *__restrict__ u, const double *__restrict__ v,
			       double *out, size_t n, double s, int qn_form, const double *s_dev = nullptr, const int *stop = nullptr)
{
#pragma clang fp contract(off)
	const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= n || (stop && *stop)) return;
	if (s_dev) s = *s_dev;		/* batched accelerated runs: the step size was computed on the device */
	if (qn_form) out[idx] = base[idx] + u[idx] + s * v[idx];
	else out[idx] = base[idx] - 2 * s * u[idx] + s * s * (v[idx] - u[idx]);
}
__global__ void k_axpy2(const double *__restrict__ v, double *out, size_t n, double ca, double cb)
{
#pragma clang fp contract(off)
	const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx < n) out[idx] += v[idx] * ca * cb;	/* accel_em.c:387-393: v * Ainv * cutu */
}
__global__ void k_add(const double *__restrict__ a, const double *__restrict__ b, double *out, size_t n)
{
	const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx < n) out[idx] = a[idx] + b[idx];
}

/* step_size() of accel_em.c:130-243 on the device (batched accelerated runs): sc->dots from DOT_ETA / DOT_P on are the eta / p
 * parts of utu, u(v-u), (v-u)^2 (eta terms first, accel_em.c:143-184); the step goes to sc->step; cyc->no_update = 1 when the
 * reference would leave the cycle without an update (NaN / infinite step, S3's sqrt(utu) < 1e-8 guard) */
__device__ __forceinline__ void step_size_body(mchip_scalars *sc, int scheme, mchip_cycle_flags *cyc)
{
	const double *eta = sc->dots + DOT_ETA, *p = sc->dots + DOT_P;
	const double utu = eta[0] + p[0], utvu = eta[1] + p[1], vutvu = eta[2] + p[2];
	double s;
	if (scheme == 1) s = utu / utvu;
	else if (scheme == 2) s = utvu / vutvu;
	else if (scheme == 3) s = (sqrt(utu) < 1e-8) ? (double)NAN : -sqrt(utu / vutvu);
	else s = -utu / utvu;				/* QN with one secant */
	if (scheme < 4 && s > -1) s = -1;		/* SQUAREM clamp (accel_em.c:236-237); false for NaN */
	sc->step = s;
	cyc->no_update = (s != s || s - s != 0.0) ? 1 : 0;	/* isnan || isinf */
}
/* the six sums of the step-size dot products (k_reduce_dots's blocks, one after the other: same order, same tree, same bits) and
 * step_size (accel_em.c:130-243) in one single-block launch */
__global__ __launch_bounds__(MCHIP_BLOCK) void k_reduce_dots_step(const double *__restrict__ part_q, int gq, const double *__restrict__ part_p,
		int gp, mchip_scalars *sc, int scheme, mchip_cycle_flags *cyc, const int *stop)
{
	__shared__ double red[MCHIP_BLOCK];
	if (stop && *stop) return;
	for (int x = 0; x < 6; x++) {
		const double *in = x < 3 ? part_q + (size_t)x * gq : part_p + (size_t)(x - 3) * gp;
		const int n = x < 3 ? gq : gp;
		const double v = block_ordered_sum(in, n, red);
		if (threadIdx.x == 0) sc->dots[(x < 3 ? DOT_ETA : DOT_P) + (x % 3)] = v;
	}
	if (threadIdx.x == 0) step_size_body(sc, scheme, cyc);
}
__global__ void k_accept(const mchip_scalars *sc, mchip_cycle_flags *cyc, const int *stop)
{
	if (threadIdx.x || blockIdx.x || (stop && *stop)) return;
	cyc->accepted = (!cyc->no_update && sc->ll_point > sc->emll) ? 1 : 0;
}

/* the cycle's outcome goes back to the slot every cycle starts from: the extrapolated point if accepted, else the second
 * EM iterate (pindex = tindex / findex, accel_em.c:89-101), so that the slot roles are the same in every cycle */
__global__ void k_select_copy(double *qdst, const double *__restrict__ q_if_accepted, const double *__restrict__ q_otherwise, size_t nq,
			      double *pdst, const double *__restrict__ p_if_accepted, const double *__restrict__ p_otherwise, size_t np,
			      const mchip_cycle_flags *cyc, const int *stop)
{
	size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= nq + np || (stop && *stop)) return;
	if (idx < nq) qdst[idx] = cyc->accepted ? q_if_accepted[idx] : q_otherwise[idx];
	else { idx -= nq; pdst[idx] = cyc->accepted ? p_if_accepted[idx] : p_otherwise[idx]; }
}

/* secant j's p and eta parts: of the u pair (which = 0) or of the v pair */
static double *secant_p(mchip_context *ctx, int which, int j) { return which ? ctx->d_vp[j] : ctx->d_up[j]; }
static double *secant_q(mchip_context *ctx, int which, int j) { return which ? ctx->d_vq[j] : ctx->d_uq[j]; }

extern "C" {

/* ---- acceleration ---- */
static int check_secant(mchip_context *ctx, int j)
{
	if (!ctx) return MCHIP_ERR_INVALID;
	if (!ctx->K) return fail(ctx, MCHIP_ERR_STATE, "no model set%s", nullptr);
	if (j < 0 || j >= ctx->nsec) return fail(ctx, MCHIP_ERR_INVALID, "secant index out of range%s", nullptr);
	return MCHIP_OK;
}

/* the secant buffers as model state (mod->u_pklm / v_pklm / u_etaik / v_etaik, multiclust.h:284-293): written and read whole, in
 * the parameter slots' own flat order, so that a quasi-Newton run with q > 1 can be resumed from a recorded state */
int mchip_set_secant(mchip_context *ctx, int which, int j, const double *p_part, const double *q_part)
{
	MCHIP_ENTRY();
	int rc = check_secant(ctx, j);
	if (rc) return rc;
	if (!p_part || !q_part || (which != 0 && which != 1)) return fail(ctx, MCHIP_ERR_INVALID, "set_secant: bad arguments%s", nullptr);
	const size_t KT = (size_t)ctx->K * ctx->T;
	HIPCHK(hipSetDevice(ctx->device));
	HIPCHK(hipMemcpyAsync(ctx->d_stage, p_part, KT * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	launch_transpose(ctx, ctx->d_stage, secant_p(ctx, which, j), true);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(secant_q(ctx, which, j), q_part, (size_t)ctx->nq * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	return MCHIP_OK;
}
int mchip_get_secant(mchip_context *ctx, int which, int j, double *p_part, double *q_part)
{
	MCHIP_ENTRY();
	int rc = check_secant(ctx, j);
	if (rc) return rc;
	if (!p_part || !q_part || (which != 0 && which != 1)) return fail(ctx, MCHIP_ERR_INVALID, "get_secant: bad arguments%s", nullptr);
	const size_t KT = (size_t)ctx->K * ctx->T;
	HIPCHK(hipSetDevice(ctx->device));
	launch_transpose(ctx, secant_p(ctx, which, j), ctx->d_stage, false);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(p_part, ctx->d_stage, KT * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipMemcpyAsync(q_part, secant_q(ctx, which, j), (size_t)ctx->nq * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	return MCHIP_OK;
}

int mchip_secant(mchip_context *ctx, int which, int j, int to, int from)
{
	MCHIP_ENTRY();
	int rc = check_secant(ctx, j);
	if (rc) return rc;
	if ((rc = check_slot(ctx, to)) || (rc = check_slot(ctx, from))) return rc;
	HIPCHK(hipSetDevice(ctx->device));
	const size_t KT = (size_t)ctx->K * ctx->T;
	double *dp = secant_p(ctx, which, j), *dq = secant_q(ctx, which, j);
	hipLaunchKernelGGL(k_diff, dim3(nblk(KT)), dim3(256), 0, ctx->stream, ctx->d_p[to], ctx->d_p[from], dp, KT);
	hipLaunchKernelGGL(k_diff, dim3(nblk(ctx->nq)), dim3(256), 0, ctx->stream, ctx->d_q[to], ctx->d_q[from], dq, (size_t)ctx->nq);
	HIPCHK(hipGetLastError());
	return MCHIP_OK;
}

/* the dot products' eta parts land in d_scalars->dots[DOT_ETA + x], the p parts in d_scalars->dots[DOT_P + x] */
static void dots_enqueue(mchip_context *ctx, const double *uq, const double *vq, const double *u2q,
			 const double *up, const double *vp, const double *u2p, int mode, int nout, const int *stop = nullptr)
{
	const size_t KT = (size_t)ctx->K * ctx->T;
	const int gq = dot_blocks((size_t)ctx->nq), gp = dot_blocks(KT);
	double *part_q = dot_part_eta(ctx->d_redpart), *part_p = dot_part_p(ctx->d_redpart);
	hipLaunchKernelGGL(k_dots, dim3(gq), dim3(MCHIP_BLOCK), 0, ctx->stream, uq, vq, u2q, (size_t)ctx->nq, mode, part_q, stop);
	hipLaunchKernelGGL(k_dots, dim3(gp), dim3(MCHIP_BLOCK), 0, ctx->stream, up, vp, u2p, KT, mode, part_p, stop);
	hipLaunchKernelGGL(k_reduce_dots, dim3(2 * nout), dim3(MCHIP_BLOCK), 0, ctx->stream, part_q, gq, part_p, gp, nout, ctx->d_scalars, stop);
}

static int dots_common(mchip_context *ctx, const double *uq, const double *vq, const double *u2q,
		       const double *up, const double *vp, const double *u2p, int mode, int nout, double *out)
{
	dots_enqueue(ctx, uq, vq, u2q, up, vp, u2p, mode, nout);
	HIPCHK(hipGetLastError());
	double tmp[8];
	int rc = fetch_scalars(ctx, ctx->d_scalars->dots, 8, tmp);
	if (rc) return rc;
	for (int x = 0; x < nout; x++) out[x] = tmp[DOT_ETA + x] + tmp[DOT_P + x];	/* eta terms first, then p (accel_em.c:143-184) */
	return MCHIP_OK;
}

int mchip_step_dots(mchip_context *ctx, int j, double *out3)
{
	MCHIP_ENTRY();
	int rc = check_secant(ctx, j);
	if (rc) return rc;
	if (!out3) return MCHIP_ERR_INVALID;
	HIPCHK(hipSetDevice(ctx->device));
	return dots_common(ctx, ctx->d_uq[j], ctx->d_vq[j], nullptr, ctx->d_up[j], ctx->d_vp[j], nullptr, 0, 3, out3);
}

int mchip_secant_dots(mchip_context *ctx, int j1, int j2, double *out2)
{
	MCHIP_ENTRY();
	int rc = check_secant(ctx, j1);
	if (rc) return rc;
	if ((rc = check_secant(ctx, j2))) return rc;
	if (!out2) return MCHIP_ERR_INVALID;
	HIPCHK(hipSetDevice(ctx->device));
	return dots_common(ctx, ctx->d_uq[j1], ctx->d_vq[j2], ctx->d_uq[j2], ctx->d_up[j1], ctx->d_vp[j2], ctx->d_up[j2], 1, 2, out2);
}

int mchip_accel_update(mchip_context *ctx, int to, int base, int j, double s, int qn_form)
{
	MCHIP_ENTRY();
	int rc = check_secant(ctx, j);
	if (rc) return rc;
	ctx->s_cache_slot = -1;
	if ((rc = check_slot(ctx, to)) || (rc = check_slot(ctx, base))) return rc;
	HIPCHK(hipSetDevice(ctx->device));
	const size_t KT = (size_t)ctx->K * ctx->T;
	hipLaunchKernelGGL(k_accel_update, dim3(nblk(KT)), dim3(256), 0, ctx->stream, ctx->d_p[base], ctx->d_up[j], ctx->d_vp[j], ctx->d_p[to], KT, s, qn_form);
	hipLaunchKernelGGL(k_accel_update, dim3(nblk(ctx->nq)), dim3(256), 0, ctx->stream, ctx->d_q[base], ctx->d_uq[j], ctx->d_vq[j], ctx->d_q[to], (size_t)ctx->nq, s, qn_form);
	HIPCHK(hipGetLastError());
	ctx->empty_rows_nan[to] = ctx->empty_rows_nan[base];	/* x + (anything of NaN secants) is NaN in the reference */
	return project_slot(ctx, to);
}

/* One accelerated cycle = accelerated_em_step (accel_em.c:35-114) with one secant pair and no back-tracking, enqueued
 * without a host round trip: slot A holds the cycle's starting iterate, B = A+1 its first EM iterate and later the
 * extrapolated point, C = A+2 the second EM iterate.  Every decision the reference takes on the host is taken by a
 * one-thread kernel (stop rule twice, step size, accept test); the cycle's outcome is copied back to A so that the next
 * cycle has the same slot roles, which is what lets one captured graph serve every cycle. */
static int accel_cycle_enqueue(mchip_context *ctx, int A, int scheme)
{
	const int B = (A + 1) % 3, C = (A + 2) % 3;
	const int *stop = &ctx->d_run->stopped;
	mchip_cycle_flags *cyc = ctx->d_cyc;
	mchip_scalars *sc = ctx->d_scalars;
	const size_t KT = (size_t)ctx->K * ctx->T, nq = (size_t)ctx->nq;
	int rc;
	/* em_2_steps (em_alg.c:1072-1211): E(A) M(->B) stop, u = B - A; E(B) M(->C) stop, v = C - B */
	if ((rc = run_estep(ctx, A, B, 1, stop, &cyc->accepted, true))) return rc;
	stop_check(ctx);
	if ((rc = run_estep(ctx, B, C, 1, stop, nullptr, true))) return rc;
	stop_check(ctx);
	/* emll = log_likelihood(findex = C) -> sc->emll (accel_em.c:53).  Admixture model: where the dual individual pass
	 * exists, emll is taken below, by the pass that visits the extrapolated point (same kernel arithmetic, same bits) */
	mchip_pass_args dual = pass_args(ctx, B);
	dual.stop = stop;
	dual.P2 = ctx->d_p[C];
	dual.Q2 = ctx->d_q[C];
	dual.llpart2 = ctx->d_llpart2;
	const mchip_plan plan = plan_for(ctx->kt, dual, ctx->knob);	/* (of slot C's arguments too: a plan does not depend on the slot) */
	const bool use_dual = ctx->admixture && plan.dual;
	if (!ctx->admixture) {
		if ((rc = run_mixture(ctx, C, C, 0, 1, stop, &sc->emll))) return rc;	/* logL_mixture */
	} else if (!use_dual) {
		mchip_pass_args a = pass_args(ctx, C);
		a.stop = stop;
		ll_pass(ctx, MCHIP_KERN_LOGLIK, ctx->kt->loglik, a, plan, &sc->emll, stop);
	}
	{	/* (the secants u = B - A, v = C - B are formed inside the kernels that use them: nothing stores them in a batched cycle) */
		const int gq = dot_blocks(nq), gp = dot_blocks(KT);
		double *part_q = dot_part_eta(ctx->d_redpart), *part_p = dot_part_p(ctx->d_redpart);
		hipLaunchKernelGGL(k_dots_slots, dim3(gq + gp), dim3(MCHIP_BLOCK), 0, ctx->stream, ctx->d_q[A], ctx->d_q[B], ctx->d_q[C], nq, part_q, (unsigned)gq,
				   ctx->d_p[A], ctx->d_p[B], ctx->d_p[C], KT, part_p, stop);
		/* step size (accel_em.c:130-243) -> sc->step, by the launch that adds up the partial dot products */
		hipLaunchKernelGGL(k_reduce_dots_step, dim3(1), dim3(MCHIP_BLOCK), 0, ctx->stream, part_q, gq, part_p, gp, sc, scheme, cyc, stop);
	}
	/* accelerated_update (accel_em.c:422-551): B = A - 2 s u + s^2 (v - u) (or A + u + s v), projected; its log likelihood,
	 * taken by the pass that also leaves the S-side sums -> sc->ll_point */
	hipLaunchKernelGGL(k_accel_update_slots, dim3(nblk(nq + KT)), dim3(256), 0, ctx->stream, ctx->d_q[A], ctx->d_q[B], ctx->d_q[C], ctx->d_q[B], nq,
			   ctx->d_p[A], ctx->d_p[B], ctx->d_p[C], ctx->d_p[B], KT, scheme == 4, &sc->step, stop);
	if ((rc = project_slot(ctx, B, stop))) return rc;
	if (!ctx->admixture) {
		if ((rc = run_mixture(ctx, B, B, 0, 1, stop, &sc->ll_point))) return rc;	/* nothing of this pass serves the next E step */
	} else {
		if (use_dual) {
			prof_mark(ctx, MCHIP_KERN_DUAL, true);
			ctx->kt->accum_q_dual(dual, plan, ctx->stream);
			prof_mark(ctx, MCHIP_KERN_DUAL, false);
		} else {
			mchip_pass_args a = pass_args(ctx, B);
			a.stop = stop;
			ll_pass(ctx, MCHIP_KERN_ACCUM_Q, ctx->kt->accum_q, a, plan, nullptr);	/* (k_reduce_accept adds its partial sums up) */
		}
	}
	/* the two log likelihoods' sums and accept iff ll > emll, one launch; the outcome goes back to slot A */
	if (ctx->admixture)
		hipLaunchKernelGGL(k_reduce_accept, dim3(1), dim3(MCHIP_BLOCK), 0, ctx->stream, use_dual ? ctx->d_llpart2 : (const double *)nullptr, ctx->d_llpart,
				   plan.ll_parts, sc, cyc, stop);
	else
		hipLaunchKernelGGL(k_accept, dim3(1), dim3(64), 0, ctx->stream, sc, cyc, stop);
	hipLaunchKernelGGL(k_select_copy, dim3(nblk(nq + KT)), dim3(256), 0, ctx->stream, ctx->d_q[A], ctx->d_q[B], ctx->d_q[C], nq,
			   ctx->d_p[A], ctx->d_p[B], ctx->d_p[C], KT, cyc, stop);
	HIPCHK(hipGetLastError());
	return MCHIP_OK;
}

int mchip_accel_run(mchip_context *ctx, int slot, int scheme, int n_cycles, mchip_run_state *state)
{
	MCHIP_ENTRY();
	int rc = check_slot(ctx, slot);
	if (rc) return rc;
	if (!state || n_cycles < 1 || scheme < 1 || scheme > 4) return fail(ctx, MCHIP_ERR_INVALID, "accel_run: bad arguments%s", nullptr);
	if ((ctx->admixture && !ctx->geo.sparse) || ctx->nsec < 1)
		return fail(ctx, MCHIP_ERR_UNSUPPORTED, "accel_run: needs a secant pair; loci with more than 32 alleles run cycle by cycle%s", nullptr);
	if (ctx->qstride) ctx->empty_rows_nan[0] = ctx->empty_rows_nan[1] = ctx->empty_rows_nan[2] = 1;	/* every slot is written by the cycle's M steps */
	HIPCHK(hipSetDevice(ctx->device));
	HIPCHK(hipMemcpyAsync(ctx->d_run, state, sizeof *state, hipMemcpyHostToDevice, ctx->stream));
	/* does Spart hold the S-side sums of this very slot (mchip_loglik_prefetch, or the accepted cycle that ended the
	 * previous call)?  The first E step of the batch is told through the device flag the later cycles set themselves */
	mchip_cycle_flags flags = { 0, (ctx->admixture && ctx->s_cache_slot == slot) ? 1 : 0 };
	HIPCHK(hipMemcpyAsync(ctx->d_cyc, &flags, sizeof flags, hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));	/* flags is on the stack */
	ctx->s_cache_slot = -1;
	const auto cycle = [&] { return accel_cycle_enqueue(ctx, slot, scheme); };
	hipGraphExec_t *exec = &ctx->cycle_graph[slot][scheme];
	const bool use_graph = !ctx->profiling && !ctx->knob.no_graph && captured(ctx, exec, cycle);
	for (int c = 0; c < n_cycles; c++) {
		if (use_graph) HIPCHK(hipGraphLaunch(*exec, ctx->stream));
		else if ((rc = cycle())) return rc;
	}
	HIPCHK(hipMemcpyAsync(state, ctx->d_run, sizeof *state, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipMemcpyAsync(&flags, ctx->d_cyc, sizeof flags, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	/* a batch that ran to its end on an accepted cycle leaves that cycle's sums for whoever continues from this slot */
	ctx->s_cache_slot = (ctx->admixture && !state->stopped && flags.accepted) ? slot : -1;
	ctx->have_ll = 1;
	return MCHIP_OK;
}

int mchip_multisecant_update(mchip_context *ctx, int to, int base, int u_index, int n_terms,
			     const int *v_index, const double *coef_a, const double *coef_b)
{
	MCHIP_ENTRY();
	int rc = check_secant(ctx, u_index);
	if (rc) return rc;
	ctx->s_cache_slot = -1;
	if ((rc = check_slot(ctx, to)) || (rc = check_slot(ctx, base))) return rc;
	if (n_terms < 0 || (n_terms && (!v_index || !coef_a || !coef_b))) return MCHIP_ERR_INVALID;
	for (int t = 0; t < n_terms; t++) if ((rc = check_secant(ctx, v_index[t]))) return rc;
	HIPCHK(hipSetDevice(ctx->device));
	const size_t KT = (size_t)ctx->K * ctx->T;
	hipLaunchKernelGGL(k_add, dim3(nblk(KT)), dim3(256), 0, ctx->stream, ctx->d_p[base], ctx->d_up[u_index], ctx->d_p[to], KT);
	hipLaunchKernelGGL(k_add, dim3(nblk(ctx->nq)), dim3(256), 0, ctx->stream, ctx->d_q[base], ctx->d_uq[u_index], ctx->d_q[to], (size_t)ctx->nq);
	for (int t = 0; t < n_terms; t++) {
		hipLaunchKernelGGL(k_axpy2, dim3(nblk(KT)), dim3(256), 0, ctx->stream, ctx->d_vp[v_index[t]], ctx->d_p[to], KT, coef_a[t], coef_b[t]);
		hipLaunchKernelGGL(k_axpy2, dim3(nblk(ctx->nq)), dim3(256), 0, ctx->stream, ctx->d_vq[v_index[t]], ctx->d_q[to], (size_t)ctx->nq, coef_a[t], coef_b[t]);
	}
	HIPCHK(hipGetLastError());
	ctx->empty_rows_nan[to] = ctx->empty_rows_nan[base];
	return project_slot(ctx, to);
}

}	/* extern "C" */
