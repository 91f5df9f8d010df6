/*
 * mchip.hip -- a context and what it holds: create / destroy, the knobs, the per-K table lookup, the progress record, the one
 * path by which a data set is installed (with its layout kernels) and the model with its parameter slots.  gfx950 only; no CPU
 * fallback: every entry point fails with MCHIP_ERR_NO_DEVICE / MCHIP_ERR_HIP when the GPU path cannot run.  The launch geometry
 * and the plan are in mchip_plan.hip, the EM step in mchip_em.hip, the acceleration in mchip_accel.hip, the initialisations in
 * mchip_init.hip, the measurement hooks in mchip_profile.hip.
 */
#include "mchip_context.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/syscall.h>
#include <unistd.h>

/* ------------------------------------------------------------------ progress record (mchip_progress.h) */
mchip_progress_slot mchip_progress_slots[MCHIP_PROGRESS_SLOTS];
std::atomic<unsigned long long> mchip_progress_events{0};
static std::atomic<int> progress_next_slot{0};

mchip_progress_slot *mchip_progress_my_slot(void)
{
	static thread_local mchip_progress_slot *mine = nullptr;
	if (!mine) {
		int x = progress_next_slot.fetch_add(1, std::memory_order_relaxed);
		if (x >= MCHIP_PROGRESS_SLOTS) x = MCHIP_PROGRESS_SLOTS - 1;	/* more threads than slots: the last one is shared */
		mine = &mchip_progress_slots[x];
		mine->tid.store((long)syscall(SYS_gettid), std::memory_order_relaxed);
	}
	return mine;
}

/* ------------------------------------------------------------------ per-K tables */
#define DECL_KT(n) const mchip_ktable *mchip_ktable_get_##n();
MCHIP_FOR_EACH_K(DECL_KT)
#undef DECL_KT

const mchip_ktable *mchip_get_ktable(int K)
{
	typedef const mchip_ktable *(*getter)();
#define KT_ENTRY(n) mchip_ktable_get_##n,
	static const getter tabs[] = { nullptr, MCHIP_FOR_EACH_K(KT_ENTRY) };
#undef KT_ENTRY
	static_assert(MCHIP_MAX_K == 64 && sizeof(tabs) / sizeof(tabs[0]) == MCHIP_MAX_K + 1,
		      "one kernel translation unit per K (mchip_internal.h: MCHIP_FOR_EACH_K; Makefile: KS)");
	return (K >= 1 && K <= MCHIP_MAX_K) ? tabs[K]() : nullptr;
}

/* ------------------------------------------------------------------ context */
void read_knobs(mchip_knobs *knob)
{
	auto on = [](const char *name) { return getenv(name) != nullptr ? 1 : 0; };
	auto num = [](const char *name, int dflt) { const char *e = getenv(name); return (e && atoi(e) > 0) ? atoi(e) : dflt; };
	knob->no_bial = on("MCHIP_NO_BIAL");
	knob->no_counts = on("MCHIP_NO_COUNTS");
	knob->force_dense = on("MCHIP_FORCE_DENSE");
	knob->force_safe = on("MCHIP_FORCE_SAFE");
	knob->no_graph = on("MCHIP_NO_GRAPH");
	knob->no_dual = on("MCHIP_NO_DUAL");
	knob->no_slab_sum = on("MCHIP_NO_SLAB_SUM");
	knob->no_fused_finalize = on("MCHIP_NO_FUSED_FINALIZE");
	knob->no_pair = on("MCHIP_NO_PAIR");
	knob->kin_two_launches = on("MCHIP_KIN_TWO_LAUNCHES");
	knob->no_col_split = on("MCHIP_NO_COL_SPLIT");
	knob->part_no_tile = on("MCHIP_PART_NO_TILE");
	knob->sim_no_tile = on("MCHIP_SIM_NO_TILE");
	const int both = num("MCHIP_BLOCKS_PER_CU", 64);
	knob->per_cu_col = num("MCHIP_BLOCKS_PER_CU_COL", both);
	knob->per_cu_ind = num("MCHIP_BLOCKS_PER_CU_IND", both);
	const char *f = getenv("MCHIP_SLAB_FRAC");
	knob->slab_frac = (f && atof(f) > 0) ? atof(f) : 0.3;
	knob->no_roundup = on("MCHIP_NO_CHUNK_ROUNDUP");
	knob->geometry_given = on("MCHIP_BLOCKS_PER_CU") || on("MCHIP_BLOCKS_PER_CU_COL") || on("MCHIP_SLAB_FRAC");
}

/* ------------------------------------------------------------------ kernels of the install path and of the parameter slots */

/* raw [I][L][pl] bytes -> gtA [ceil(I/8)][L][8][pl] and gtS [ceil(L/8)][I][8][pl]; pads with 0xFF;
 * validates allele indices when ua != nullptr (limit = ua[l]) or against `limit` otherwise.
 * A workgroup moves one tile of RT_I individuals x RT_L loci through LDS: the rows of the tile are read once, contiguously
 * (RT_L * pl bytes per row), and both layouts are written in runs of whole 8 * pl-byte groups that are contiguous in memory
 * (gtA: consecutive loci of one block of 8 individuals; gtS: consecutive individuals of one block of 8 loci).  The first
 * version read raw[] once per OUTPUT byte in output order -- 8 rows per group, a few bytes of every 64-byte line at a time:
 * 28.5 GB of HBM traffic for a 2 GB genotype (profiles/r01_v5_c3_traffic.json); it is paid per initialisation (the
 * partition takes the same route) and per bootstrap replicate. */
constexpr int RT_I = 64;	/* individuals per tile; loci per tile: 64 up to ploidy 8, fewer above (32 KiB of LDS) */

__global__ __launch_bounds__(256) void k_relayout(const uint8_t *__restrict__ raw, int I, int L, int pl, const int32_t *__restrict__ ua,
			   int limit, uint8_t *gtA, uint8_t *gtS, int n_ltiles, int RT_L, int *bad)
{
	extern __shared__ __attribute__((aligned(16))) uint8_t tile[];	/* [RT_I][RT_L * pl] */
	const int rowb = RT_L * pl;		/* bytes per tile row: a multiple of 8 */
	const int l0 = (blockIdx.x % n_ltiles) * RT_L, i0 = (blockIdx.x / n_ltiles) * RT_I;
	int flags = 0;
	const int roww = rowb / 4;		/* dwords per tile row */
	/* rows are read four bytes at a time when every row of the tile starts on a 4-byte boundary of raw[] and lies inside it */
	const bool words = ((((size_t)L * pl) | ((size_t)l0 * pl) | (size_t)raw) & 3) == 0 && l0 + RT_L <= L;
	for (int x = threadIdx.x; x < RT_I * roww; x += 256) {
		const int r = x / roww, w = x % roww;
		const int i = i0 + r;
		uint32_t v4 = 0xFFFFFFFFu;
		if (i < I) {
			const uint8_t *src = raw + ((size_t)i * L + l0) * pl + (size_t)w * 4;
			if (words) {
				v4 = *reinterpret_cast<const uint32_t *>(src);
			} else {
				v4 = 0;
				for (int y = 0; y < 4; y++) {
					const int l = l0 + (w * 4 + y) / pl;
					const uint32_t v = l < L ? src[y] : 0xFFu;
					v4 |= v << (8 * y);
				}
			}
			for (int y = 0; y < 4; y++) {
				const int l = l0 + (w * 4 + y) / pl;
				const uint32_t v = (v4 >> (8 * y)) & 0xFFu;
				if (l >= L) continue;
				const int lim = ua ? ua[l] : limit;
				if (v != 0xFFu && (int)v >= lim) flags |= 1;
				if (v == 0xFFu) flags |= 2;	/* bit 1: the data set has missing copies */
			}
		}
		reinterpret_cast<uint32_t *>(tile)[x] = v4;
	}
	if (flags) atomicOr(bad, flags);
	__syncthreads();
	const int grp = 8 * pl, grpw = 2 * pl;	/* bytes / dwords per group of 8 entries */
	/* gtA: block ib of 8 individuals, loci l0 .. l0+RT_L-1: RT_L groups, contiguous; one dword (4 of the group's bytes) per thread */
	for (int x = threadIdx.x; x < (RT_I / 8) * RT_L * grpw; x += 256) {
		const int w = x % grpw, ll = (x / grpw) % RT_L, ibl = x / (grpw * RT_L);
		const int l = l0 + ll;
		const size_t ib = (size_t)(i0 / 8) + ibl;
		if (l >= L || ib * 8 >= (size_t)I) continue;
		uint32_t v4 = 0;
		for (int y = 0; y < 4; y++) {
			const int e = w * 4 + y, j = e / pl, a = e % pl;
			v4 |= (uint32_t)tile[(ibl * 8 + j) * rowb + ll * pl + a] << (8 * y);
		}
		reinterpret_cast<uint32_t *>(gtA + (ib * L + l) * (size_t)grp)[w] = v4;
	}
	/* gtS: block lb of 8 loci, individuals i0 .. i0+RT_I-1: RT_I groups, contiguous; the group's bytes are contiguous in the tile row */
	for (int x = threadIdx.x; x < (RT_L / 8) * RT_I * grpw; x += 256) {
		const int w = x % grpw, r = (x / grpw) % RT_I, lbl = x / (grpw * RT_I);
		const int i = i0 + r;
		const size_t lb = (size_t)(l0 / 8) + lbl;
		if (i >= I || lb * 8 >= (size_t)L) continue;
		reinterpret_cast<uint32_t *>(gtS + (lb * I + i) * (size_t)grp)[w] = reinterpret_cast<const uint32_t *>(tile + r * rowb + lbl * grp)[w];
	}
}

/* launch: one workgroup per tile; LDS = RT_I * RT_L * pl <= 32 KiB */
int launch_relayout(hipStream_t stream, const uint8_t *raw, int I, int L, int pl, const int32_t *ua, int limit,
		    uint8_t *gtA, uint8_t *gtS, int *bad)
{
	int RT_L = 64;
	while (RT_L > 8 && RT_I * RT_L * pl > 32 * 1024) RT_L -= 8;
	const int n_ltiles = (L + RT_L - 1) / RT_L, n_itiles = (I + RT_I - 1) / RT_I;
	const size_t blocks = (size_t)n_ltiles * n_itiles;
	if (blocks >= ((size_t)1 << 31) || (size_t)RT_I * RT_L * pl > 64 * 1024) return -1;
	hipLaunchKernelGGL(k_relayout, dim3((unsigned)blocks), dim3(256), (size_t)RT_I * RT_L * pl, stream, raw, I, L, pl, ua, limit, gtA, gtS,
			   n_ltiles, RT_L, bad);
	return 0;
}

/* gtA -> raw [I][L][pl] (mchip_get_genotypes) */
__global__ void k_unlayout(const uint8_t *__restrict__ gtA, int I, int L, int pl, uint8_t *raw)
{
	const size_t n = (size_t)I * L * pl, stride = (size_t)gridDim.x * blockDim.x;
	for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += stride) {
		size_t r = idx;
		const int a = (int)(r % pl); r /= pl;
		const int l = (int)(r % L);
		const size_t i = r / L;
		raw[idx] = gtA[(((i >> 3) * L + l) * 8 + (i & 7)) * (size_t)pl + a];
	}
}

/* gtA -> packed counts gtC[g][c]: thread = (group g of G individuals, column c) */
template <int BITS>
__global__ void k_build_counts(const uint8_t *__restrict__ gtA, int I, int L, int pl, int T,
			       const int32_t *__restrict__ col_locus, const uint8_t *__restrict__ col_allele, uint4 *gtC)
{
	constexpr int PERWORD = 32 / BITS, G = 4 * PERWORD;
	const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	const size_t ngroups = (size_t)(I + G - 1) / G;
	if (idx >= ngroups * T) return;
	const int c = (int)(idx % T);
	const size_t g = idx / T;
	const int l = col_locus[c];
	const unsigned m = col_allele[c];
	unsigned out[4] = {0, 0, 0, 0};
	for (int x = 0; x < G; x++) {
		const size_t i = g * G + x;
		if (i >= (size_t)I) break;
		const uint8_t *src = gtA + (((i >> 3) * L + l) * 8 + (i & 7)) * (size_t)pl;
		unsigned n = 0;
		for (int b = 0; b < pl; b++) n += (src[b] == m);
		out[x / PERWORD] |= n << (BITS * (x % PERWORD));
	}
	gtC[idx] = make_uint4(out[0], out[1], out[2], out[3]);
}

/* non-empty cells (i, c) with n_ic > 0 -- the unit SURVEY.md section 8d counts flops in -- and non-missing allele copies;
 * thread = (block of 8 individuals, column) over gtA, block partial sums, one atomic per block */
__global__ __launch_bounds__(256) void k_count_cells(const uint8_t *__restrict__ gtA, int I, int L, int pl, int T,
		const int32_t *__restrict__ col_locus, const uint8_t *__restrict__ col_allele, unsigned long long *out)
{
	__shared__ unsigned red[2][256];
	const size_t n = (size_t)((I + 7) / 8) * T, stride = (size_t)gridDim.x * 256;
	unsigned cells = 0, copies = 0;
	for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += stride) {
		const int c = (int)(idx % T);
		const size_t ib = idx / T;
		const int l = col_locus[c];
		const unsigned m = col_allele[c];
		const uint8_t *src = gtA + (ib * L + l) * 8 * (size_t)pl;
		for (int j = 0; j < 8; j++) {
			unsigned cnt = 0;
			for (int b = 0; b < pl; b++) cnt += (src[j * pl + b] == m);	/* padded individuals carry 0xFF */
			cells += cnt != 0;
			copies += cnt;
		}
	}
	const unsigned mine[2] = {cells, copies};
	block_tree_sum<256>(red[0], 256, mine);
	if (threadIdx.x == 0) {
		atomicAdd(&out[0], (unsigned long long)red[0][0]);
		atomicAdd(&out[1], (unsigned long long)red[1][0]);
	}
}

/* host order [K][T] <-> device order [T][K] */
__global__ void k_transpose_kt_to_tk(const double *__restrict__ src, double *__restrict__ dst, int K, int T)
{
	const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= (size_t)K * T) return;
	const int k = (int)(idx % K);
	const size_t c = idx / K;
	dst[idx] = src[(size_t)k * T + c];
}
__global__ void k_transpose_tk_to_kt(const double *__restrict__ src, double *__restrict__ dst, int K, int T)
{
	const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= (size_t)K * T) return;
	const size_t c = idx % T;
	const int k = (int)(idx / T);
	dst[idx] = src[c * K + k];
}
void launch_transpose(mchip_context *ctx, const double *src, double *dst, bool to_tk)
{
	const size_t KT = (size_t)ctx->K * ctx->T;
	if (to_tk) hipLaunchKernelGGL(k_transpose_kt_to_tk, dim3(nblk(KT)), dim3(256), 0, ctx->stream, src, dst, ctx->K, ctx->T);
	else hipLaunchKernelGGL(k_transpose_tk_to_kt, dim3(nblk(KT)), dim3(256), 0, ctx->stream, src, dst, ctx->K, ctx->T);
}

/* ------------------------------------------------------------------ helpers */
int check_slot(mchip_context *ctx, int slot)
{
	if (!ctx) return MCHIP_ERR_INVALID;
	if (!ctx->K) return fail(ctx, MCHIP_ERR_STATE, "no model set%s", nullptr);
	if (slot < 0 || slot > 2) return fail(ctx, MCHIP_ERR_INVALID, "slot out of range%s", nullptr);
	return MCHIP_OK;
}

/* the captured steps carry their kernel arguments by value (buffer addresses, the data set's has_missing flag) */
static void drop_graphs(mchip_context *ctx)
{
	for (int s = 0; s < 3; s++)
		if (ctx->step_graph[s]) { (void)MCHIP_WAIT(hipGraphExecDestroy(ctx->step_graph[s])); ctx->step_graph[s] = nullptr; }
	for (int s = 0; s < 3; s++)
		for (int m = 0; m < 5; m++)
			if (ctx->cycle_graph[s][m]) { (void)MCHIP_WAIT(hipGraphExecDestroy(ctx->cycle_graph[s][m])); ctx->cycle_graph[s][m] = nullptr; }
}

void free_model(mchip_context *ctx)
{
	drop_graphs(ctx);
	for (int s = 0; s < 3; s++) { dfree(ctx->d_p[s]); dfree(ctx->d_q[s]); }
	for (int s = 0; s < MCHIP_MAX_SECANTS; s++) { dfree(ctx->d_up[s]); dfree(ctx->d_vp[s]); dfree(ctx->d_uq[s]); dfree(ctx->d_vq[s]); }
	dfree(ctx->d_sik); dfree(ctx->d_stage); dfree(ctx->d_logp); dfree(ctx->d_Apart); dfree(ctx->d_Spart); dfree(ctx->d_llpart); dfree(ctx->d_llpart2);
	dfree(ctx->d_redpart); dfree(ctx->d_flags);
	ctx->K = 0;
	ctx->parked_K = 0;
	ctx->kt = nullptr;
	ctx->have_ll = 0;
	ctx->s_cache_slot = -1;
}

void drop_saved(saved_set &set)
{
	dfree(set.d_raw);
	set.L = 0;
	set.ua.clear();
	set.empty.clear();
}

void free_data(mchip_context *ctx, int keep)
{
	drop_cv(ctx);
	drop_generators(ctx);
	if (!(keep & KEEP_RS_BASE)) drop_saved(ctx->rs_base);
	dfree(ctx->d_ua); dfree(ctx->d_toff); dfree(ctx->d_col_locus); dfree(ctx->d_col_allele);
	dfree(ctx->d_gtA); dfree(ctx->d_gtS); dfree(ctx->d_gtC); dfree(ctx->d_asA); dfree(ctx->d_asS);
	dfree(ctx->d_initA); dfree(ctx->d_initS);
	dfree(ctx->d_draw);
	dfree(ctx->d_cand_span); dfree(ctx->d_cand_centers); dfree(ctx->d_cand_off);
	ctx->cand_span_bytes = ctx->cand_loci = ctx->cand_center_bytes = 0;
	dfree(ctx->d_cen_part); dfree(ctx->d_cen_work);
	ctx->cen_part_bytes = ctx->cen_work_bytes = 0;
	ctx->init_geno_set = 0;
	ctx->h_ua.clear();
	ctx->I = ctx->L = ctx->T = 0;
}

/* ------------------------------------------------------------------ C-ABI */
extern "C" {

int mchip_abi_version(void) { return MCHIP_ABI_VERSION; }

int mchip_device_count(int *count)
{
	MCHIP_ENTRY();
	if (!count) return MCHIP_ERR_INVALID;
	int n = 0;
	if (MCHIP_WAIT(hipGetDeviceCount(&n)) != hipSuccess) n = 0;
	*count = n;
	return MCHIP_OK;
}

int mchip_create(mchip_context **out, int device)
{
	MCHIP_ENTRY();
	if (!out) return MCHIP_ERR_INVALID;
	*out = nullptr;
	int n = 0;
	if (MCHIP_WAIT(hipGetDeviceCount(&n)) != hipSuccess || n <= 0) return MCHIP_ERR_NO_DEVICE;	/* a process's first runtime call: hipInit */
	if (device < 0 || device >= n) return MCHIP_ERR_INVALID;
	mchip_context *ctx = new mchip_context();
	ctx->first_empty = -1;
	ctx->cv_fold = -1;
	ctx->device = device;
	ctx->err[0] = 0;
	ctx->geo.ind_waves = 1;
	read_knobs(&ctx->knob);
	if (MCHIP_WAIT(hipSetDevice(device)) != hipSuccess || MCHIP_WAIT(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess) {
		delete ctx;
		return MCHIP_ERR_HIP;
	}
	hipDeviceProp_t prop;
	ctx->n_cu = (MCHIP_WAIT(hipGetDeviceProperties(&prop, device)) == hipSuccess) ? prop.multiProcessorCount : 256;
	if (MCHIP_WAIT(hipHostMalloc((void **)&ctx->h_pinned, sizeof(mchip_scalars), hipHostMallocDefault)) != hipSuccess ||
	    MCHIP_WAIT(hipMalloc((void **)&ctx->d_scalars, sizeof(mchip_scalars))) != hipSuccess ||
	    MCHIP_WAIT(hipMalloc((void **)&ctx->d_run, sizeof(mchip_run_state))) != hipSuccess ||
	    MCHIP_WAIT(hipMalloc((void **)&ctx->d_cyc, sizeof(mchip_cycle_flags))) != hipSuccess ||
	    MCHIP_WAIT(hipEventCreate(&ctx->ev_begin)) != hipSuccess || MCHIP_WAIT(hipEventCreate(&ctx->ev_end)) != hipSuccess) {
		delete ctx;
		return MCHIP_ERR_ALLOC;
	}
	*out = ctx;
	return MCHIP_OK;
}

int mchip_destroy(mchip_context *ctx)
{
	MCHIP_ENTRY();
	if (!ctx) return MCHIP_OK;
	(void)MCHIP_WAIT(hipSetDevice(ctx->device));
	(void)MCHIP_WAIT(hipStreamSynchronize(ctx->stream));
	free_model(ctx);
	free_data(ctx);
	dfree(ctx->d_scalars);
	dfree(ctx->d_cyc);
	dfree(ctx->d_run);
	if (ctx->h_pinned) (void)MCHIP_WAIT(hipHostFree(ctx->h_pinned));
	for (hipEvent_t e : ctx->ev_pool) (void)MCHIP_WAIT(hipEventDestroy(e));
	dfree(ctx->d_pair_marks);
	for (mchip_pair_span *&chunk : ctx->pair_spans) dfree(chunk);
	(void)MCHIP_WAIT(hipEventDestroy(ctx->ev_begin));
	(void)MCHIP_WAIT(hipEventDestroy(ctx->ev_end));
	(void)MCHIP_WAIT(hipStreamDestroy(ctx->stream));
	delete ctx;
	return MCHIP_OK;
}

const char *mchip_last_error(const mchip_context *ctx) { return ctx ? ctx->err : "null context"; }

int mchip_synchronize(mchip_context *ctx)
{
	MCHIP_ENTRY();
	if (!ctx) return MCHIP_ERR_INVALID;
	HIPCHK(hipStreamSynchronize(ctx->stream));
	return MCHIP_OK;
}

int mchip_device_info(mchip_context *ctx, char *name, int name_len, int *compute_units, double *hbm_bytes)
{
	MCHIP_ENTRY();
	if (!ctx) return MCHIP_ERR_INVALID;
	hipDeviceProp_t prop;
	HIPCHK(hipGetDeviceProperties(&prop, ctx->device));
	if (name && name_len > 0) snprintf(name, name_len, "%s (%s)", prop.name, prop.gcnArchName);
	if (compute_units) *compute_units = prop.multiProcessorCount;
	if (hbm_bytes) *hbm_bytes = (double)prop.totalGlobalMem;
	return MCHIP_OK;
}

}	/* extern "C" */

/* ------------------------------------------------------------------ installing a data set (mchip_context.h declares what the
 * feature units call) */
static int set_shape_impl(mchip_context *ctx, int I, int L, int ploidy, const int32_t *ua, int keep)
{
	if (I <= 0 || L <= 0 || ploidy <= 0 || ploidy > 64 || !ua)
		return fail(ctx, MCHIP_ERR_INVALID, "set_genotypes: bad shape or null pointer%s", nullptr);
	read_knobs(&ctx->knob);
	HIPCHK(hipSetDevice(ctx->device));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	drop_cv(ctx);	/* folds, the saved full data set and a hold-out in force belong to the data set that goes */
	if (!(keep & KEEP_RS_BASE)) drop_saved(ctx->rs_base);	/* so does the base of its selections of loci (a new selection keeps it) */
	/* The same shape and allele lists as the data set held (the next bootstrap replicate, a re-upload): every buffer stays;
	 * the model is dropped as the contract says, but its buffers are parked for an mchip_set_model with the same arguments.
	 * Freeing and re-allocating ~10 GB per replicate costs little per call, but the runtime returns freed memory lazily and
	 * stalls for seconds once the card's memory has been through its hands (measured: every 11th config-5 replicate) */
	if (ctx->T && ctx->I == I && ctx->L == L && ctx->ploidy == ploidy && (int)ctx->h_ua.size() == L &&
	    !memcmp(ctx->h_ua.data(), ua, sizeof(int32_t) * (size_t)L)) {
		if (ctx->K) ctx->parked_K = ctx->K;
		ctx->K = 0;
		ctx->have_ll = 0;
		ctx->s_cache_slot = -1;
		if (!(keep & KEEP_INIT)) ctx->init_geno_set = 0;
		return MCHIP_OK;
	}
	free_model(ctx);	/* workspaces depend on T */
	free_data(ctx, keep);

	std::vector<int32_t> toff(L + 25);	/* padded: kernels read the offsets of a block of 8 loci and of the two blocks behind it */
	toff[0] = 0;
	int maxM = 0, minM = 1 << 30;
	for (int l = 0; l < L; l++) {
		if (ua[l] < minM) minM = ua[l];
		if (ua[l] < 0 || ua[l] > 255) return fail(ctx, MCHIP_ERR_INVALID, "uniquealleles[l] must be in [0,255]%s", nullptr);
		if ((long long)toff[l] + ua[l] > 2000000000LL) return fail(ctx, MCHIP_ERR_INVALID, "too many allele columns%s", nullptr);
		toff[l + 1] = toff[l] + ua[l];
		if (ua[l] > maxM) maxM = ua[l];
	}
	const int T = toff[L];
	for (int x = L + 1; x < L + 25; x++) toff[x] = T;
	if (T <= 0) return fail(ctx, MCHIP_ERR_INVALID, "no alleles%s", nullptr);
	std::vector<int32_t> col_locus(T);
	std::vector<uint8_t> col_allele(T);
	for (int l = 0; l < L; l++)
		for (int m = 0; m < ua[l]; m++) {
			col_locus[toff[l] + m] = l;
			col_allele[toff[l] + m] = (uint8_t)m;
		}
	ctx->I = I; ctx->L = L; ctx->ploidy = ploidy; ctx->T = T; ctx->max_M = maxM; ctx->min_M = minM;
	ctx->h_ua.assign(ua, ua + L);
	ctx->geno_bytes_A = (size_t)((I + 7) / 8) * L * 8 * ploidy;
	ctx->geno_bytes_S = (size_t)((L + 7) / 8) * I * 8 * ploidy;
	HIPCHK(hipMalloc((void **)&ctx->d_ua, sizeof(int32_t) * L));
	HIPCHK(hipMalloc((void **)&ctx->d_toff, sizeof(int32_t) * (L + 25)));
	HIPCHK(hipMalloc((void **)&ctx->d_col_locus, sizeof(int32_t) * T));
	HIPCHK(hipMalloc((void **)&ctx->d_col_allele, T));
	HIPCHK(hipMalloc((void **)&ctx->d_gtA, ctx->geno_bytes_A));
	HIPCHK(hipMalloc((void **)&ctx->d_gtS, ctx->geno_bytes_S));
	HIPCHK(hipMemcpyAsync(ctx->d_ua, ua, sizeof(int32_t) * L, hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(hipMemcpyAsync(ctx->d_toff, toff.data(), sizeof(int32_t) * (L + 25), hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(hipMemcpyAsync(ctx->d_col_locus, col_locus.data(), sizeof(int32_t) * T, hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(hipMemcpyAsync(ctx->d_col_allele, col_allele.data(), T, hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));	/* the host vectors go out of scope */
	return MCHIP_OK;
}

int set_shape(mchip_context *ctx, int I, int L, int ploidy, const int32_t *ua, int keep)
{
	const int rc = set_shape_impl(ctx, I, L, ploidy, ua, keep);
	if (rc == MCHIP_ERR_HIP || rc == MCHIP_ERR_ALLOC) {	/* an allocation that failed half way: no data set, no model */
		free_model(ctx);
		free_data(ctx, keep);
	}
	return rc;
}

/* one byte per allele copy in stream order, padded to whole generator chunks: the device-drawn partition, a generated data
 * set before it goes into the kernels' layouts, an uploaded genotype on its way there.  Kept for the life of the data set. */
int stream_buffer(mchip_context *ctx)
{
	if (ctx->d_draw) return MCHIP_OK;
	const size_t n = (size_t)ctx->I * ctx->L * ctx->ploidy;
	HIPCHK(hipMalloc((void **)&ctx->d_draw, ((n + RNG_CHUNK - 1) / RNG_CHUNK) * RNG_CHUNK));
	return MCHIP_OK;
}

int install_layouts(mchip_context *ctx, int has_missing)
{
	const int I = ctx->I, L = ctx->L, ploidy = ctx->ploidy, T = ctx->T;
	if (ctx->has_missing != has_missing) drop_graphs(ctx);	/* parked model buffers: the kernel variant changes */
	ctx->has_missing = has_missing;
	ctx->counts_valid = 0;	/* counted when asked for (mchip_data_counts): a bootstrap replicate never asks */
	ctx->count_bits = count_bits_for(ploidy, ctx->knob);
	if (ctx->count_bits) {
		const int G = 128 / ctx->count_bits;
		const size_t nwords = (size_t)((I + G - 1) / G) * T;
		if (!ctx->d_gtC) HIPCHK(hipMalloc((void **)&ctx->d_gtC, nwords * 16));
		if (ctx->count_bits == 2)
			hipLaunchKernelGGL(k_build_counts<2>, dim3(nblk(nwords)), dim3(256), 0, ctx->stream, ctx->d_gtA, I, L, ploidy, T,
					   ctx->d_col_locus, ctx->d_col_allele, (uint4 *)ctx->d_gtC);
		else
			hipLaunchKernelGGL(k_build_counts<4>, dim3(nblk(nwords)), dim3(256), 0, ctx->stream, ctx->d_gtA, I, L, ploidy, T,
					   ctx->d_col_locus, ctx->d_col_allele, (uint4 *)ctx->d_gtC);
		HIPCHK(hipGetLastError());
		HIPCHK(hipStreamSynchronize(ctx->stream));
	}
	return MCHIP_OK;
}

/* genotype held on the device as [I][L][ploidy] bytes -> the kernels' layouts (validated), packed counts */
int install_raw(mchip_context *ctx, const uint8_t *d_raw)
{
	const int I = ctx->I, L = ctx->L, ploidy = ctx->ploidy;
	int *d_bad = bad_flag(ctx);
	HIPCHK(hipMemsetAsync(d_bad, 0, sizeof(int), ctx->stream));
	if (launch_relayout(ctx->stream, d_raw, I, L, ploidy, ctx->d_ua, 0, ctx->d_gtA, ctx->d_gtS, d_bad))
		return fail(ctx, MCHIP_ERR_UNSUPPORTED, "data set too large for the layout kernel%s", nullptr);
	HIPCHK(hipGetLastError());
	int bad = 0;
	HIPCHK(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	if (bad & 1) {
		free_data(ctx);
		return fail(ctx, MCHIP_ERR_INVALID, "genotype allele index >= uniquealleles[l]%s", nullptr);
	}
	return install_layouts(ctx, (bad & 2) ? 1 : 0);
}

/* (a generated data set has no empty rows, and its call passes none: that the slots' NaN marks are reset there too cannot be
 * observed, because they stand for rows of this list) */
void set_empty_rows(mchip_context *ctx, std::vector<int> rows)
{
	ctx->empty_rows = std::move(rows);
	ctx->first_empty = ctx->empty_rows.empty() ? -1 : ctx->empty_rows[0];
	for (int sl = 0; sl < 3; sl++) ctx->empty_rows_nan[sl] = 0;
}

void set_empty_rows_unseen(mchip_context *ctx, const std::vector<uint8_t> &seen)
{
	std::vector<int> rows;
	for (size_t i = 0; i < seen.size(); i++)
		if (!seen[i]) rows.push_back((int)i);
	set_empty_rows(ctx, std::move(rows));
}

static void launch_unlayout(mchip_context *ctx, uint8_t *d_raw)
{
	const size_t n = (size_t)ctx->I * ctx->L * ctx->ploidy;
	hipLaunchKernelGGL(k_unlayout, dim3(nblk_capped(n)), dim3(256), 0, ctx->stream, ctx->d_gtA, ctx->I, ctx->L, ctx->ploidy, d_raw);
}

int save_installed(mchip_context *ctx, saved_set &set)
{
	HIPCHK(hipMalloc((void **)&set.d_raw, (size_t)ctx->I * ctx->L * ctx->ploidy));
	launch_unlayout(ctx, set.d_raw);
	if (MCHIP_WAIT(hipGetLastError()) != hipSuccess || MCHIP_WAIT(hipStreamSynchronize(ctx->stream)) != hipSuccess) {
		dfree(set.d_raw);
		return fail(ctx, MCHIP_ERR_HIP, "saving the installed data set failed%s", nullptr);
	}
	set.L = ctx->L;
	set.ua = ctx->h_ua;
	set.empty = ctx->empty_rows;
	return MCHIP_OK;
}

int install_saved(mchip_context *ctx, const saved_set &set)
{
	const int rc = install_raw(ctx, set.d_raw);
	if (!rc) set_empty_rows(ctx, set.empty);
	return rc;
}

int install_derived(mchip_context *ctx, const std::function<void(uint8_t *d_out, uint8_t *d_seen)> &fill)
{
	int rc = stream_buffer(ctx);
	if (rc) return rc;
	const size_t I = (size_t)ctx->I;
	scoped_dev<uint8_t> d_seen;
	HIPCHK(d_seen.alloc(I));
	HIPCHK(hipMemsetAsync(d_seen.p, 0, I, ctx->stream));
	fill(ctx->d_draw, d_seen.p);
	HIPCHK(hipGetLastError());
	std::vector<uint8_t> seen(I);
	HIPCHK(hipMemcpyAsync(seen.data(), d_seen.p, I, hipMemcpyDeviceToHost, ctx->stream));
	if ((rc = install_raw(ctx, ctx->d_draw))) return rc;	/* (synchronises the stream) */
	set_empty_rows_unseen(ctx, seen);
	return MCHIP_OK;
}

extern "C" {

int mchip_set_genotypes(mchip_context *ctx, int I, int L, int ploidy, const int32_t *ua, const uint8_t *geno)
{
	MCHIP_ENTRY();
	if (!ctx) return MCHIP_ERR_INVALID;
	if (!geno) return fail(ctx, MCHIP_ERR_INVALID, "set_genotypes: bad shape or null pointer%s", nullptr);
	int rc = set_shape(ctx, I, L, ploidy, ua);
	if (rc) return rc;
	const size_t raw_bytes = (size_t)I * L * ploidy;
	/* an individual whose every copy is missing (one pass that stops at each individual's first observed copy: O(I) on real data) */
	std::vector<int> empty;
	for (int i = 0; i < I; i++) {
		const uint8_t *row = geno + (size_t)i * L * ploidy;
		size_t x = 0;
		while (x < (size_t)L * ploidy && row[x] == MCHIP_MISSING) x++;
		if (x == (size_t)L * ploidy) empty.push_back(i);
	}
	set_empty_rows(ctx, std::move(empty));
	if ((rc = stream_buffer(ctx))) return rc;
	HIPCHK(hipMemcpyAsync(ctx->d_draw, geno, raw_bytes, hipMemcpyHostToDevice, ctx->stream));
	return install_raw(ctx, ctx->d_draw);
}

int mchip_copy_genotypes(mchip_context *ctx, const mchip_context *src)
{
	MCHIP_ENTRY();
	if (!ctx || !src || ctx == src) return MCHIP_ERR_INVALID;
	if (!src->T) return fail(ctx, MCHIP_ERR_STATE, "copy_genotypes: the source holds no data set%s", nullptr);
	if (src->device != ctx->device) return fail(ctx, MCHIP_ERR_UNSUPPORTED, "copy_genotypes: contexts on different devices%s", nullptr);
	int rc = set_shape(ctx, src->I, src->L, src->ploidy, src->h_ua.data(), KEEP_INIT);
	if (rc) return rc;
	HIPCHK(hipStreamSynchronize(src->stream));
	HIPCHK(hipMemcpyAsync(ctx->d_gtA, src->d_gtA, ctx->geno_bytes_A, hipMemcpyDeviceToDevice, ctx->stream));
	HIPCHK(hipMemcpyAsync(ctx->d_gtS, src->d_gtS, ctx->geno_bytes_S, hipMemcpyDeviceToDevice, ctx->stream));
	if (src->count_bits) {
		const int G = 128 / src->count_bits;
		const size_t bytes = (size_t)((ctx->I + G - 1) / G) * ctx->T * 16;
		if (!ctx->d_gtC) HIPCHK(hipMalloc((void **)&ctx->d_gtC, bytes));
		HIPCHK(hipMemcpyAsync(ctx->d_gtC, src->d_gtC, bytes, hipMemcpyDeviceToDevice, ctx->stream));
	}
	if (ctx->has_missing != src->has_missing) drop_graphs(ctx);
	ctx->has_missing = src->has_missing;
	set_empty_rows(ctx, src->empty_rows);
	ctx->count_bits = src->count_bits;
	ctx->counts_valid = src->counts_valid;
	ctx->nnz_cells = src->nnz_cells;
	ctx->n_copies = src->n_copies;
	HIPCHK(hipStreamSynchronize(ctx->stream));
	return MCHIP_OK;
}

int mchip_set_init_genotypes(mchip_context *ctx, const uint8_t *geno)
{
	MCHIP_ENTRY();
	if (!ctx) return MCHIP_ERR_INVALID;
	if (!ctx->T) return fail(ctx, MCHIP_ERR_STATE, "no genotypes set%s", nullptr);
	HIPCHK(hipSetDevice(ctx->device));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	ctx->init_geno_set = 0;
	if (!geno) {
		dfree(ctx->d_initA);
		dfree(ctx->d_initS);
		return MCHIP_OK;
	}
	const size_t n = (size_t)ctx->I * ctx->L * ctx->ploidy;
	int *d_bad = bad_flag(ctx);
	int rc = stream_buffer(ctx);
	if (rc) return rc;
	uint8_t *d_obs = ctx->d_draw;
	if (!ctx->d_initA) HIPCHK(hipMalloc((void **)&ctx->d_initA, ctx->geno_bytes_A));
	if (!ctx->d_initS) HIPCHK(hipMalloc((void **)&ctx->d_initS, ctx->geno_bytes_S));
	HIPCHK(hipMemcpyAsync(d_obs, geno, n, hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(hipMemsetAsync(d_bad, 0, sizeof(int), ctx->stream));
	if (launch_relayout(ctx->stream, d_obs, ctx->I, ctx->L, ctx->ploidy, ctx->d_ua, 0, ctx->d_initA, ctx->d_initS, d_bad))
		return fail(ctx, MCHIP_ERR_UNSUPPORTED, "data set too large for the layout kernel%s", nullptr);
	HIPCHK(hipGetLastError());
	int bad = 0;
	HIPCHK(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	if (bad & 1) {
		dfree(ctx->d_initA);
		dfree(ctx->d_initS);
		return fail(ctx, MCHIP_ERR_INVALID, "init genotype allele index >= uniquealleles[l]%s", nullptr);
	}
	ctx->init_geno_set = 1;
	return MCHIP_OK;
}

int mchip_data_counts(mchip_context *ctx, uint64_t *nonempty_cells, uint64_t *allele_copies)
{
	MCHIP_ENTRY();
	if (!ctx) return MCHIP_ERR_INVALID;
	if (!ctx->T) return fail(ctx, MCHIP_ERR_STATE, "no genotypes set%s", nullptr);
	if (!ctx->counts_valid) {	/* integer sums: order does not matter */
		HIPCHK(hipSetDevice(ctx->device));
		unsigned long long *d_cnt = ctx->d_scalars->cells, h_cnt[2] = {0, 0};
		HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof h_cnt, ctx->stream));
		const size_t n = (size_t)((ctx->I + 7) / 8) * ctx->T;
		hipLaunchKernelGGL(k_count_cells, dim3(nblk_capped(n, 256, 65536)), dim3(256), 0, ctx->stream, ctx->d_gtA,
				   ctx->I, ctx->L, ctx->ploidy, ctx->T, ctx->d_col_locus, ctx->d_col_allele, d_cnt);
		HIPCHK(hipGetLastError());
		HIPCHK(hipMemcpyAsync(h_cnt, d_cnt, sizeof h_cnt, hipMemcpyDeviceToHost, ctx->stream));
		HIPCHK(hipStreamSynchronize(ctx->stream));
		ctx->nnz_cells = h_cnt[0];
		ctx->n_copies = h_cnt[1];
		ctx->counts_valid = 1;
	}
	if (nonempty_cells) *nonempty_cells = ctx->nnz_cells;
	if (allele_copies) *allele_copies = ctx->n_copies;
	return MCHIP_OK;
}

int mchip_get_genotypes(mchip_context *ctx, uint8_t *geno)
{
	MCHIP_ENTRY();
	if (!ctx || !geno) return MCHIP_ERR_INVALID;
	if (!ctx->T) return fail(ctx, MCHIP_ERR_STATE, "no genotypes set%s", nullptr);
	HIPCHK(hipSetDevice(ctx->device));
	const size_t n = (size_t)ctx->I * ctx->L * ctx->ploidy;
	scoped_dev<uint8_t> d_raw;
	HIPCHK(d_raw.alloc(n));
	launch_unlayout(ctx, d_raw.p);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(geno, d_raw, n, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	return MCHIP_OK;
}

static int set_model_impl(mchip_context *ctx, int K, int admixture, int eta_constrained, int do_projection,
			  double eta_lb, double p_lb, int n_secants)
{
	if (!ctx->T) return fail(ctx, MCHIP_ERR_STATE, "set_model before set_genotypes%s", nullptr);
	if (K < 1) return fail(ctx, MCHIP_ERR_INVALID, "K must be >= 1%s", nullptr);
	if (K > MCHIP_MAX_K) return fail(ctx, MCHIP_ERR_UNSUPPORTED, "K > MCHIP_MAX_K is not built%s", nullptr);
	if (n_secants < 0 || n_secants > MCHIP_MAX_SECANTS) return fail(ctx, MCHIP_ERR_INVALID, "n_secants out of range%s", nullptr);
	/* the element-per-thread kernels over parameters take one work-item per entry of P or Q */
	if ((size_t)K * ctx->T >= ((size_t)1 << 31) || (size_t)K * ctx->I >= ((size_t)1 << 31))
		return fail(ctx, MCHIP_ERR_UNSUPPORTED, "K*T or K*I of 2^31 or more is not supported%s", nullptr);
	read_knobs(&ctx->knob);
	HIPCHK(hipSetDevice(ctx->device));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	{	/* the buffers of this very model are still allocated (same data shape, same arguments): zero the parameters and go */
		const int have = ctx->K ? ctx->K : ctx->parked_K;
		if (have == K && ctx->d_p[0] && ctx->sig_admixture == admixture && ctx->sig_constrained == (eta_constrained ? 1 : 0) &&
		    ctx->sig_projection == do_projection && ctx->sig_nsec == n_secants && ctx->sig_eta_lb == eta_lb && ctx->sig_p_lb == p_lb) {
			const size_t KTr = (size_t)K * ctx->T;
			for (int s = 0; s < 3; s++) {
				HIPCHK(hipMemsetAsync(ctx->d_p[s], 0, KTr * sizeof(double), ctx->stream));
				HIPCHK(hipMemsetAsync(ctx->d_q[s], 0, (size_t)ctx->nq * sizeof(double), ctx->stream));
			}
			HIPCHK(hipMemsetAsync(ctx->d_sik, 0, (size_t)ctx->I * K * sizeof(double), ctx->stream));
			ctx->K = K;
			ctx->parked_K = 0;
			ctx->have_ll = 0;
			ctx->s_cache_slot = -1;
			HIPCHK(hipStreamSynchronize(ctx->stream));
			return MCHIP_OK;
		}
	}
	free_model(ctx);
	ctx->sig_admixture = admixture; ctx->sig_constrained = eta_constrained ? 1 : 0; ctx->sig_projection = do_projection;
	ctx->sig_nsec = n_secants; ctx->sig_eta_lb = eta_lb; ctx->sig_p_lb = p_lb;
	ctx->K = K; ctx->admixture = admixture; ctx->constrained = eta_constrained ? 1 : 0;
	ctx->do_projection = do_projection; ctx->eta_lb = eta_lb; ctx->p_lb = p_lb; ctx->nsec = n_secants;
	ctx->kt = mchip_get_ktable(K);
	const int shared_eta = (!admixture || eta_constrained);
	ctx->nq = shared_eta ? K : ctx->I * K;
	ctx->qstride = shared_eta ? 0 : K;
	const size_t KT = (size_t)K * ctx->T;
	for (int s = 0; s < 3; s++) {
		HIPCHK(hipMalloc((void **)&ctx->d_p[s], KT * sizeof(double)));
		HIPCHK(hipMalloc((void **)&ctx->d_q[s], (size_t)ctx->nq * sizeof(double)));
		HIPCHK(hipMemsetAsync(ctx->d_p[s], 0, KT * sizeof(double), ctx->stream));
		HIPCHK(hipMemsetAsync(ctx->d_q[s], 0, (size_t)ctx->nq * sizeof(double), ctx->stream));
	}
	for (int s = 0; s < n_secants; s++) {
		HIPCHK(hipMalloc((void **)&ctx->d_up[s], KT * sizeof(double)));
		HIPCHK(hipMalloc((void **)&ctx->d_vp[s], KT * sizeof(double)));
		HIPCHK(hipMalloc((void **)&ctx->d_uq[s], (size_t)ctx->nq * sizeof(double)));
		HIPCHK(hipMalloc((void **)&ctx->d_vq[s], (size_t)ctx->nq * sizeof(double)));
	}
	HIPCHK(hipMalloc((void **)&ctx->d_sik, (size_t)ctx->I * K * sizeof(double)));
	HIPCHK(hipMemsetAsync(ctx->d_sik, 0, (size_t)ctx->I * K * sizeof(double), ctx->stream));
	HIPCHK(hipMalloc((void **)&ctx->d_stage, KT * sizeof(double)));
	if (!admixture) HIPCHK(hipMalloc((void **)&ctx->d_logp, KT * sizeof(double)));

	ctx->geo = model_geometry(shape_of(ctx), K, admixture, do_projection, p_lb, ctx->knob, ctx->n_cu);
	HIPCHK(hipMalloc((void **)&ctx->d_Apart, (size_t)ctx->geo.n_ichunks * KT * sizeof(double)));
	HIPCHK(hipMalloc((void **)&ctx->d_Spart, (size_t)ctx->geo.n_lchunks * ctx->I * K * sizeof(double)));
	HIPCHK(hipMalloc((void **)&ctx->d_llpart, (size_t)ctx->geo.n_llpart * sizeof(double)));
	HIPCHK(hipMalloc((void **)&ctx->d_llpart2, (size_t)ctx->geo.n_llpart * sizeof(double)));
	HIPCHK(hipMalloc((void **)&ctx->d_redpart, DOT_PARTIALS * sizeof(double)));
	if (needs_byte_flags(ctx->max_M)) {
		HIPCHK(hipMalloc((void **)&ctx->d_flags, KT));
	}
	HIPCHK(hipStreamSynchronize(ctx->stream));
	return MCHIP_OK;
}

int mchip_set_model(mchip_context *ctx, int K, int admixture, int eta_constrained, int do_projection,
		    double eta_lb, double p_lb, int n_secants)
{
	MCHIP_ENTRY();
	if (!ctx) return MCHIP_ERR_INVALID;
	const int rc = set_model_impl(ctx, K, admixture, eta_constrained, do_projection, eta_lb, p_lb, n_secants);
	if (rc == MCHIP_ERR_HIP || rc == MCHIP_ERR_ALLOC) free_model(ctx);	/* an allocation that failed half way leaves no model, not a partial one */
	return rc;
}

int mchip_q_length(const mchip_context *ctx, int *n)
{
	MCHIP_ENTRY();
	if (!ctx || !n || !ctx->K) return MCHIP_ERR_STATE;
	*n = ctx->nq;
	return MCHIP_OK;
}
int mchip_p_length(const mchip_context *ctx, int *n)
{
	MCHIP_ENTRY();
	if (!ctx || !n || !ctx->K) return MCHIP_ERR_STATE;
	*n = ctx->K * ctx->T;
	return MCHIP_OK;
}

int mchip_set_p(mchip_context *ctx, int slot, const double *p)
{
	MCHIP_ENTRY();
	int rc = check_slot(ctx, slot);
	if (rc) return rc;
	ctx->s_cache_slot = -1;
	if (!p) return fail(ctx, MCHIP_ERR_INVALID, "null pointer%s", nullptr);
	const size_t KT = (size_t)ctx->K * ctx->T;
	HIPCHK(hipSetDevice(ctx->device));
	HIPCHK(hipMemcpyAsync(ctx->d_stage, p, KT * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	launch_transpose(ctx, ctx->d_stage, ctx->d_p[slot], true);
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(ctx->stream));	/* the host buffer may be reused on return */
	return MCHIP_OK;
}

int mchip_get_p(mchip_context *ctx, int slot, double *p)
{
	MCHIP_ENTRY();
	int rc = check_slot(ctx, slot);
	if (rc) return rc;
	if (!p) return fail(ctx, MCHIP_ERR_INVALID, "null pointer%s", nullptr);
	const size_t KT = (size_t)ctx->K * ctx->T;
	HIPCHK(hipSetDevice(ctx->device));
	launch_transpose(ctx, ctx->d_p[slot], ctx->d_stage, false);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(p, ctx->d_stage, KT * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	return MCHIP_OK;
}

int mchip_set_q(mchip_context *ctx, int slot, const double *q)
{
	MCHIP_ENTRY();
	int rc = check_slot(ctx, slot);
	if (rc) return rc;
	ctx->s_cache_slot = -1;
	if (!q) return fail(ctx, MCHIP_ERR_INVALID, "null pointer%s", nullptr);
	HIPCHK(hipSetDevice(ctx->device));
	/* A row of an individual without a single observed copy that comes in as NaN (what mchip_get_q reports for it after an M
	 * step: a warm start, a checkpoint) is kept on the device as the finite 1 / K k_finalize_q keeps -- a NaN there would reach
	 * every column's N-side sum through 0 * (1 / NaN) -- and the slot goes on reporting it as NaN; a finite row is taken as it is */
	int nan_rows = 0;
	if (ctx->qstride)
		for (int i : ctx->empty_rows)
			for (int k = 0; k < ctx->K; k++) nan_rows |= (q[(size_t)i * ctx->K + k] != q[(size_t)i * ctx->K + k]);
	if (nan_rows) {
		std::vector<double> clean(q, q + ctx->nq);
		for (int i : ctx->empty_rows) {
			bool bad = false;
			for (int k = 0; k < ctx->K; k++) bad |= (clean[(size_t)i * ctx->K + k] != clean[(size_t)i * ctx->K + k]);
			if (bad)
				for (int k = 0; k < ctx->K; k++) clean[(size_t)i * ctx->K + k] = 1.0 / ctx->K;
		}
		HIPCHK(hipMemcpyAsync(ctx->d_q[slot], clean.data(), (size_t)ctx->nq * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
		HIPCHK(hipStreamSynchronize(ctx->stream));	/* `clean` goes out of scope */
	} else {
		HIPCHK(hipMemcpyAsync(ctx->d_q[slot], q, (size_t)ctx->nq * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
		HIPCHK(hipStreamSynchronize(ctx->stream));
	}
	ctx->empty_rows_nan[slot] = nan_rows;
	return MCHIP_OK;
}

int mchip_get_q(mchip_context *ctx, int slot, double *q)
{
	MCHIP_ENTRY();
	int rc = check_slot(ctx, slot);
	if (rc) return rc;
	if (!q) return fail(ctx, MCHIP_ERR_INVALID, "null pointer%s", nullptr);
	HIPCHK(hipSetDevice(ctx->device));
	HIPCHK(hipMemcpyAsync(q, ctx->d_q[slot], (size_t)ctx->nq * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	/* An individual without a single observed copy: the reference's M step gives it 0 / 0 (em_alg.c:685-690; printed "-nan") and the
	 * row then sits in its arrays untouched by anything else, every zero-count cell being skipped.  The device keeps a finite row
	 * for it (k_finalize_q: 1 / K) so that nothing it is multiplied into turns NaN, and it is reported here as the reference has it */
	if (ctx->qstride && ctx->empty_rows_nan[slot])
		for (int i : ctx->empty_rows)
			for (int k = 0; k < ctx->K; k++) q[(size_t)i * ctx->K + k] = -__builtin_nan("");
	return MCHIP_OK;
}

int mchip_empty_individuals(const mchip_context *ctx, int *first)
{
	MCHIP_ENTRY();
	if (!ctx) return 0;
	if (first) *first = ctx->first_empty;
	return (int)ctx->empty_rows.size();
}

int mchip_copy_slot(mchip_context *ctx, int to, int from)
{
	MCHIP_ENTRY();
	int rc = check_slot(ctx, to);
	if (rc || (rc = check_slot(ctx, from))) return rc;
	if (to == from) return MCHIP_OK;
	ctx->s_cache_slot = -1;
	HIPCHK(hipSetDevice(ctx->device));
	HIPCHK(hipMemcpyAsync(ctx->d_p[to], ctx->d_p[from], (size_t)ctx->K * ctx->T * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
	HIPCHK(hipMemcpyAsync(ctx->d_q[to], ctx->d_q[from], (size_t)ctx->nq * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
	ctx->empty_rows_nan[to] = ctx->empty_rows_nan[from];
	return MCHIP_OK;
}

int mchip_get_expected_counts(mchip_context *ctx, double *sik)
{
	MCHIP_ENTRY();
	if (!ctx || !sik) return MCHIP_ERR_INVALID;
	if (!ctx->K) return fail(ctx, MCHIP_ERR_STATE, "no model set%s", nullptr);
	HIPCHK(hipSetDevice(ctx->device));
	HIPCHK(hipMemcpyAsync(sik, ctx->d_sik, (size_t)ctx->I * ctx->K * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	return MCHIP_OK;
}

/* ---- where the process stands (mchip_progress.h) ---- */
int mchip_progress_note(const char *what)
{
	mchip_progress_slot *s = mchip_progress_my_slot();
	s->note.store(what, std::memory_order_relaxed);
	s->since_ns.store(mchip_progress_now(), std::memory_order_relaxed);
	mchip_progress_events.fetch_add(1, std::memory_order_relaxed);
	return MCHIP_OK;
}

int mchip_progress_report(char *buf, int buf_len, unsigned long long *events)
{
	if (events) *events = mchip_progress_events.load(std::memory_order_relaxed);
	if (!buf || buf_len <= 0) return MCHIP_OK;
	int n = progress_next_slot.load(std::memory_order_relaxed), used = 0;
	if (n > MCHIP_PROGRESS_SLOTS) n = MCHIP_PROGRESS_SLOTS;
	const long long now = mchip_progress_now();
	buf[0] = 0;
	for (int x = 0; x < n && used < buf_len - 1; x++) {
		const mchip_progress_slot &s = mchip_progress_slots[x];
		const char *entry = s.entry.load(std::memory_order_relaxed), *wait = s.wait.load(std::memory_order_relaxed);
		const char *note = s.note.load(std::memory_order_relaxed);
		const int w = snprintf(buf + used, (size_t)(buf_len - used), "thread %ld: %s%s%s%s%s%s, %.1f s since its last event\n",
				       s.tid.load(std::memory_order_relaxed), entry ? "in " : "outside the library", entry ? entry : "",
				       wait ? ", waiting in " : "", wait ? wait : "", note ? "; last phase: " : "", note ? note : "",
				       1e-9 * (double)(now - s.since_ns.load(std::memory_order_relaxed)));
		if (w < 0) break;
		used += w < buf_len - used ? w : buf_len - used - 1;
	}
	return MCHIP_OK;
}

}  /* extern "C" */
