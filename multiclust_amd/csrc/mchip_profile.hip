/*
 * mchip_profile.hip -- the measurement hooks: event marks around the passes, the spans of a paired E step's two kinds of block,
 * and mchip_profile_begin / mchip_profile_end.
 */
#include "mchip_context.h"

void prof_mark(mchip_context *ctx, int kind, bool start)
{
	if (!ctx->profiling) return;
	if (ctx->ev_used >= ctx->ev_pool.size()) {
		hipEvent_t e;
		if (hipEventCreate(&e) != hipSuccess) return;
		ctx->ev_pool.push_back(e);
	}
	(void)hipEventRecord(ctx->ev_pool[ctx->ev_used++], ctx->stream);
	if (start) ctx->ev_kind.push_back(kind);
}

/* Profiled paired E steps (k_estep_pair).  The two kinds of block of such a launch overlap, so no pair of events brackets either
 * pass: every block leaves two clock readings in d_pair_marks, and this one-block launch behind it takes, per kind, the first
 * start and the last end of the blocks that worked (mchip_pair_span; start > end where none did).  mchip_profile_end turns the
 * spans into the two passes' durations. */
constexpr size_t PAIR_SPAN_CHUNK = 1024;	/* spans per device allocation */
constexpr int PAIR_SPAN_THREADS = 1024;		/* one thread per run of MCHIP_PAIR_RUN blocks: the kind is worked out once per run */
__global__ __launch_bounds__(PAIR_SPAN_THREADS) void k_pair_spans(const unsigned long long *__restrict__ marks, unsigned n_blocks, mchip_pair_runs runs,
								  mchip_pair_span *out)
{
	__shared__ unsigned long long red[4][PAIR_SPAN_THREADS];
	unsigned long long lo[2] = { ~0ull, ~0ull }, hi[2] = { 0ull, 0ull };
	for (unsigned r = threadIdx.x; r < n_blocks / MCHIP_PAIR_RUN; r += PAIR_SPAN_THREADS) {	/* (n_blocks: whole runs, mchip_plan::pair_blocks) */
		unsigned logical;
		const int kind = mchip_pair_is_ind(r * MCHIP_PAIR_RUN, runs, &logical) ? 1 : 0;
#pragma unroll
		for (int x = 0; x < MCHIP_PAIR_RUN; x++) {
			const size_t b = (size_t)r * MCHIP_PAIR_RUN + x;
			const unsigned long long t0 = marks[2 * b], t1 = marks[2 * b + 1];
			if (t0 > t1) continue;		/* the block returned at once */
			lo[kind] = t0 < lo[kind] ? t0 : lo[kind];
			hi[kind] = t1 > hi[kind] ? t1 : hi[kind];
		}
	}
	red[0][threadIdx.x] = lo[0]; red[1][threadIdx.x] = lo[1]; red[2][threadIdx.x] = hi[0]; red[3][threadIdx.x] = hi[1];
	__syncthreads();
	for (int s = PAIR_SPAN_THREADS / 2; s > 0; s >>= 1) {
		if ((int)threadIdx.x < s) {
			for (int x = 0; x < 2; x++) {
				const unsigned long long l2 = red[x][threadIdx.x + s], h2 = red[2 + x][threadIdx.x + s];
				if (l2 < red[x][threadIdx.x]) red[x][threadIdx.x] = l2;
				if (h2 > red[2 + x][threadIdx.x]) red[2 + x][threadIdx.x] = h2;
			}
		}
		__syncthreads();
	}
	if (threadIdx.x == 0) {
		out->start[0] = red[0][0]; out->start[1] = red[1][0];
		out->end[0] = red[2][0]; out->end[1] = red[3][0];
	}
}

/* room for the next profiled paired launch: its blocks' clock readings and its span */
int pair_profile_slot(mchip_context *ctx, size_t n_blocks, unsigned long long **marks)
{
	if (n_blocks > ctx->pair_marks_cap) {
		HIPCHK(hipStreamSynchronize(ctx->stream));	/* (an earlier launch may still be writing the smaller buffer) */
		dfree(ctx->d_pair_marks);
		ctx->pair_marks_cap = 0;
		HIPCHK(hipMalloc((void **)&ctx->d_pair_marks, 2 * n_blocks * sizeof(unsigned long long)));
		ctx->pair_marks_cap = n_blocks;
	}
	if (ctx->pair_used / PAIR_SPAN_CHUNK >= ctx->pair_spans.size()) {
		mchip_pair_span *chunk = nullptr;
		HIPCHK(hipMalloc((void **)&chunk, PAIR_SPAN_CHUNK * sizeof(mchip_pair_span)));
		ctx->pair_spans.push_back(chunk);
	}
	*marks = ctx->d_pair_marks;
	return MCHIP_OK;
}

/* behind a profiled paired launch: its span into the slot pair_profile_slot made room for */
void launch_pair_spans(mchip_context *ctx, const unsigned long long *marks, const mchip_plan &plan)
{
	hipLaunchKernelGGL(k_pair_spans, dim3(1), dim3(PAIR_SPAN_THREADS), 0, ctx->stream, marks, plan.pair_blocks, plan.pair_runs,
			   ctx->pair_spans[ctx->pair_used / PAIR_SPAN_CHUNK] + ctx->pair_used % PAIR_SPAN_CHUNK);
	ctx->pair_used++;
}

extern "C" {

/* ---- measurement hooks ---- */
int mchip_profile_begin(mchip_context *ctx)
{
	MCHIP_ENTRY();
	if (!ctx) return MCHIP_ERR_INVALID;
	HIPCHK(hipSetDevice(ctx->device));
	ctx->profiling = 1;
	ctx->ev_used = 0;
	ctx->ev_kind.clear();
	ctx->pair_used = 0;
	HIPCHK(hipEventRecord(ctx->ev_begin, ctx->stream));
	return MCHIP_OK;
}

int mchip_profile_end(mchip_context *ctx, double *total_ms, double *kernel_ms, int *launches)
{
	MCHIP_ENTRY();
	if (!ctx) return MCHIP_ERR_INVALID;
	if (!ctx->profiling) return fail(ctx, MCHIP_ERR_STATE, "profile_end without profile_begin%s", nullptr);
	HIPCHK(hipSetDevice(ctx->device));
	HIPCHK(hipEventRecord(ctx->ev_end, ctx->stream));
	HIPCHK(hipEventSynchronize(ctx->ev_end));
	ctx->profiling = 0;
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, ctx->ev_begin, ctx->ev_end));
	if (total_ms) *total_ms = ms;
	double km[MCHIP_KERN_COUNT] = {0}, longest[MCHIP_KERN_COUNT] = {0};
	int kl[MCHIP_KERN_COUNT] = {0};
	std::vector<float> each(ctx->ev_kind.size(), 0.0f);
	std::vector<int> kind_of(ctx->ev_kind);
	for (size_t p = 0; 2 * p + 1 < ctx->ev_used && p < ctx->ev_kind.size(); p++)
		HIPCHK(hipEventElapsedTime(&each[p], ctx->ev_pool[2 * p], ctx->ev_pool[2 * p + 1]));
	/* paired E steps: each kind's blocks' span inside the launch, from the device's constant-rate clock, is that pass's launch.
	 * The two spans of a launch overlap (that is the point of the pair), so their sum exceeds the time the launch took */
	if (ctx->pair_used) {
		int khz = 0;
		if (MCHIP_WAIT(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device)) != hipSuccess || khz <= 0) khz = 100000;
		std::vector<mchip_pair_span> spans(ctx->pair_used);
		for (size_t p = 0; p < ctx->pair_used; p += PAIR_SPAN_CHUNK) {
			const size_t n = ctx->pair_used - p < PAIR_SPAN_CHUNK ? ctx->pair_used - p : PAIR_SPAN_CHUNK;
			HIPCHK(hipMemcpy(&spans[p], ctx->pair_spans[p / PAIR_SPAN_CHUNK], n * sizeof(mchip_pair_span), hipMemcpyDeviceToHost));
		}
		for (const mchip_pair_span &sp : spans)
			for (int x = 0; x < 2; x++) {
				each.push_back(sp.end[x] > sp.start[x] ? (float)((double)(sp.end[x] - sp.start[x]) / khz) : 0.0f);
				kind_of.push_back(x ? MCHIP_KERN_ACCUM_Q : MCHIP_KERN_ACCUM_P);
			}
		ctx->pair_used = 0;
	}
	for (size_t p = 0; p < each.size(); p++)
		if (each[p] > longest[kind_of[p]]) longest[kind_of[p]] = each[p];
	/* a launch that returned at once (the S-side pass of a batched accelerated cycle whose sums were already in place, any
	 * kernel after the stopping rule fired) did no pass over the data: it is not a launch of that kernel for these figures */
	for (size_t p = 0; p < each.size(); p++) {
		const int kind = kind_of[p];
		if (each[p] <= 0.0f || each[p] < 0.05 * longest[kind]) continue;	/* (a kind's blocks of a paired launch that all returned: exactly 0) */
		km[kind] += each[p];
		kl[kind]++;
	}
	for (int x = 0; x < MCHIP_KERN_COUNT; x++) {
		if (kernel_ms) kernel_ms[x] = km[x];
		if (launches) launches[x] = kl[x];
	}
	return MCHIP_OK;
}

}	/* extern "C" */
