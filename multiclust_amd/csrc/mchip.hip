/*
 * mchip.hip -- context management, K-independent kernels and the C-ABI entry points of
 * libmulticlust_hip.so (include/multiclust_hip.h).  gfx950 only; no CPU fallback: every entry point
 * fails with MCHIP_ERR_NO_DEVICE / MCHIP_ERR_HIP when the GPU path cannot run.
 */
#include "mchip_context.h"
#include "mchip_finalize.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
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
DECL_KT(1) DECL_KT(2) DECL_KT(3) DECL_KT(4) DECL_KT(5) DECL_KT(6) DECL_KT(7) DECL_KT(8)
DECL_KT(9) DECL_KT(10) DECL_KT(11) DECL_KT(12) DECL_KT(13) DECL_KT(14) DECL_KT(15) DECL_KT(16)
DECL_KT(17) DECL_KT(18) DECL_KT(19) DECL_KT(20) DECL_KT(21) DECL_KT(22) DECL_KT(23) DECL_KT(24)
DECL_KT(25) DECL_KT(26) DECL_KT(27) DECL_KT(28) DECL_KT(29) DECL_KT(30) DECL_KT(31) DECL_KT(32)
DECL_KT(33) DECL_KT(34) DECL_KT(35) DECL_KT(36) DECL_KT(37) DECL_KT(38) DECL_KT(39) DECL_KT(40)
DECL_KT(41) DECL_KT(42) DECL_KT(43) DECL_KT(44) DECL_KT(45) DECL_KT(46) DECL_KT(47) DECL_KT(48)
DECL_KT(49) DECL_KT(50) DECL_KT(51) DECL_KT(52) DECL_KT(53) DECL_KT(54) DECL_KT(55) DECL_KT(56)
DECL_KT(57) DECL_KT(58) DECL_KT(59) DECL_KT(60) DECL_KT(61) DECL_KT(62) DECL_KT(63) DECL_KT(64)

const mchip_ktable *mchip_get_ktable(int K)
{
	typedef const mchip_ktable *(*getter)();
	static const getter tabs[MCHIP_MAX_K + 1] = {
		nullptr,
		mchip_ktable_get_1, mchip_ktable_get_2, mchip_ktable_get_3, mchip_ktable_get_4, mchip_ktable_get_5, mchip_ktable_get_6, mchip_ktable_get_7, mchip_ktable_get_8,
		mchip_ktable_get_9, mchip_ktable_get_10, mchip_ktable_get_11, mchip_ktable_get_12, mchip_ktable_get_13, mchip_ktable_get_14, mchip_ktable_get_15, mchip_ktable_get_16,
		mchip_ktable_get_17, mchip_ktable_get_18, mchip_ktable_get_19, mchip_ktable_get_20, mchip_ktable_get_21, mchip_ktable_get_22, mchip_ktable_get_23, mchip_ktable_get_24,
		mchip_ktable_get_25, mchip_ktable_get_26, mchip_ktable_get_27, mchip_ktable_get_28, mchip_ktable_get_29, mchip_ktable_get_30, mchip_ktable_get_31, mchip_ktable_get_32,
		mchip_ktable_get_33, mchip_ktable_get_34, mchip_ktable_get_35, mchip_ktable_get_36, mchip_ktable_get_37, mchip_ktable_get_38, mchip_ktable_get_39, mchip_ktable_get_40,
		mchip_ktable_get_41, mchip_ktable_get_42, mchip_ktable_get_43, mchip_ktable_get_44, mchip_ktable_get_45, mchip_ktable_get_46, mchip_ktable_get_47, mchip_ktable_get_48,
		mchip_ktable_get_49, mchip_ktable_get_50, mchip_ktable_get_51, mchip_ktable_get_52, mchip_ktable_get_53, mchip_ktable_get_54, mchip_ktable_get_55, mchip_ktable_get_56,
		mchip_ktable_get_57, mchip_ktable_get_58, mchip_ktable_get_59, mchip_ktable_get_60, mchip_ktable_get_61, mchip_ktable_get_62, mchip_ktable_get_63, mchip_ktable_get_64,
	};
	static_assert(MCHIP_MAX_K == 64, "one kernel translation unit per K (Makefile: KS)");
	return (K >= 1 && K <= MCHIP_MAX_K) ? tabs[K]() : nullptr;
}

/* ------------------------------------------------------------------ context */
static void read_knobs(mchip_knobs *knob)
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

/* ------------------------------------------------------------------ K-independent kernels */

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
static int launch_relayout(hipStream_t stream, const uint8_t *raw, int I, int L, int pl, const int32_t *ua, int limit,
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

/* ------------------------------------------------------------------ mixture model: initialisation from individual centers
 * random_individual_center + initialize_parameters_mixture (rnd_init.c:192-339) given the K centers the host drew.
 *
 * k_center_distance: ONE pass over the genotype for all K centers.  Workgroup = blockDim.x individuals x a chunk of blocks of
 * 8 loci; thread = individual reading its contiguous gtS runs; the K center rows of a tile of locus blocks are staged in LDS
 * (read from gtS too: the centers are individuals of the data set), so every lane reads the same center bytes (broadcast).
 * Per (i, k, l): sum_m |n_ilm - n_c(k)lm| over observed copies = n_i + n_c - 2 * (size of the multiset intersection of the two
 * lists of observed copies), the intersection found by matching every copy of the individual with an unused equal copy of the
 * center.  Integer sums, kept per thread in LDS ([K][blockDim.x], 32 bits: a chunk holds at most 2 * 8 * chunk_groups * ploidy),
 * written as part[chunk][k][i]; k_center_assign adds the chunks in 64 bits.  MISSING bytes (also the loci that pad the last
 * block of 8) match nothing and count for nothing.
 * PLT = ploidy 1..8: the run of 8 loci in registers.  PLT = 0: any ploidy; the thread's copies of one locus go through a
 * private LDS row so that global memory is still read once. */
template <int PLT>
__global__ __launch_bounds__(256) void k_center_distance(const uint8_t *__restrict__ gtS, int I, int L, int pl_rt, int K,
		const int32_t *__restrict__ centers, int chunk_groups, int tile_groups, uint32_t *__restrict__ part)
{
	extern __shared__ uint32_t cd_lds[];
	const int pl = PLT ? PLT : pl_rt, nthr = blockDim.x, tid = threadIdx.x, grp = 8 * pl;
	uint32_t *acc = cd_lds;					/* [K][nthr] */
	uint32_t *cen32 = acc + (size_t)K * nthr;		/* [tile_groups][K][8][pl] bytes */
	const uint8_t *cen = reinterpret_cast<const uint8_t *>(cen32);
	uint8_t *own = reinterpret_cast<uint8_t *>(cen32 + (size_t)tile_groups * K * 2 * pl);	/* PLT = 0: [pl][nthr] */
	const int i = blockIdx.x * nthr + tid;
	const bool live = i < I;
	const int n_groups = (L + 7) >> 3;
	const int g_begin = blockIdx.y * chunk_groups, g_end = n_groups - g_begin < chunk_groups ? n_groups : g_begin + chunk_groups;
	for (int k = 0; k < K; k++) acc[k * nthr + tid] = 0;
	for (int g0 = g_begin; g0 < g_end; g0 += tile_groups) {
		const int ng = g_end - g0 < tile_groups ? g_end - g0 : tile_groups;
		__syncthreads();	/* the previous tile has been read */
		for (int x = tid; x < ng * K * 2 * pl; x += nthr) {
			const int w = x % (2 * pl), k = (x / (2 * pl)) % K, g = x / (2 * pl * K);
			cen32[x] = reinterpret_cast<const uint32_t *>(gtS + ((size_t)(g0 + g) * I + centers[k]) * grp)[w];
		}
		__syncthreads();
		if (!live) continue;
		for (int g = 0; g < ng; g++) {
			const uint8_t *src = gtS + ((size_t)(g0 + g) * I + i) * grp;
			if constexpr (PLT > 0) {
				unsigned long long run[PLT ? PLT : 1];
#pragma unroll
				for (int x = 0; x < PLT; x++) run[x] = reinterpret_cast<const unsigned long long *>(src)[x];
				for (int k = 0; k < K; k++) {
					unsigned long long crun[PLT ? PLT : 1];
#pragma unroll
					for (int x = 0; x < PLT; x++) crun[x] = reinterpret_cast<const unsigned long long *>(cen + (size_t)(g * K + k) * grp)[x];
					int d = 0;
#pragma unroll
					for (int t = 0; t < 8; t++) {
						unsigned used = 0;
#pragma unroll
						for (int b = 0; b < PLT; b++) {
							const int at = t * PLT + b;
							d += ((unsigned)(crun[at >> 3] >> (8 * (at & 7))) & 0xFFu) != MCHIP_MISSING;
						}
#pragma unroll
						for (int a = 0; a < PLT; a++) {
							const int at = t * PLT + a;
							const unsigned gi = (unsigned)(run[at >> 3] >> (8 * (at & 7))) & 0xFFu;
							const bool obs = gi != MCHIP_MISSING;
							bool found = false;
#pragma unroll
							for (int b = 0; b < PLT; b++) {
								const int bt = t * PLT + b;
								const unsigned cb = (unsigned)(crun[bt >> 3] >> (8 * (bt & 7))) & 0xFFu;
								const bool hit = obs && !found && !((used >> b) & 1u) && cb == gi;
								used |= (unsigned)hit << b;
								found = found || hit;
							}
							d += (int)obs - 2 * (int)found;
						}
					}
					acc[k * nthr + tid] += (uint32_t)d;
				}
			} else {
				for (int t = 0; t < 8; t++) {
					for (int a = 0; a < pl; a++) own[a * nthr + tid] = src[t * pl + a];
					for (int k = 0; k < K; k++) {
						const uint8_t *ck = cen + (size_t)(g * K + k) * grp + t * pl;
						unsigned long long used = 0;
						int d = 0;
						for (int b = 0; b < pl; b++) d += ck[b] != MCHIP_MISSING;
						for (int a = 0; a < pl; a++) {
							const unsigned gi = own[a * nthr + tid];
							if (gi == MCHIP_MISSING) continue;
							d++;
							for (int b = 0; b < pl; b++)
								if (!((used >> b) & 1ull) && ck[b] == gi) { used |= 1ull << b; d -= 2; break; }
						}
						acc[k * nthr + tid] += (uint32_t)d;
					}
				}
			}
		}
	}
	if (live)
		for (int k = 0; k < K; k++) part[((size_t)blockIdx.y * K + k) * I + i] = acc[k * nthr + tid];
}

template <int PLT>
static void launch_center_distance(mchip_context *ctx, unsigned n_iblocks, unsigned n_chunks, int nthr, size_t lds, const int32_t *d_centers,
				   int chunk_groups, int tile_groups)
{
	hipLaunchKernelGGL(k_center_distance<PLT>, dim3(n_iblocks, n_chunks), dim3(nthr), lds, ctx->stream, ctx->d_gtS, ctx->I, ctx->L, ctx->ploidy,
			   ctx->K, d_centers, chunk_groups, tile_groups, ctx->d_cen_part);
}

/* the assignment: a center k joins itself (the reference breaks out of its loop there, even when an earlier center is at
 * distance 0); every other individual joins the FIRST center of minimal distance (diff < min_diff, strict).  n_k counted. */
__global__ __launch_bounds__(256) void k_center_assign(const uint32_t *__restrict__ part, int n_chunks, int I, int K,
		const int32_t *__restrict__ centers, int32_t *__restrict__ assign, uint32_t *__restrict__ nk)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= I) return;
	int best = -1;
	for (int k = 0; k < K; k++)
		if (centers[k] == i) best = k;
	if (best < 0) {
		unsigned long long min_diff = ~0ull;
		best = 0;
		for (int k = 0; k < K; k++) {
			unsigned long long diff = 0;
			for (int c = 0; c < n_chunks; c++) diff += part[((size_t)c * K + k) * I + i];
			if (diff < min_diff) { best = k; min_diff = diff; }
		}
	}
	assign[i] = best;
	atomicAdd(&nk[best], 1u);
}

/* c[column][k] = observed copies of the allele among the individuals assigned to k.  Workgroup = 256 individuals x a chunk of
 * loci, thread = individual reading its gtS runs once, word by word; the counts of a tile of loci in LDS (integer atomics: the
 * sums are order-free), added to the global table per tile; tile = 0 (a locus block's counters do not fit): global atomics. */
__global__ __launch_bounds__(256) void k_center_counts(const uint8_t *__restrict__ gtS, int I, int L, int pl, int K,
		const int32_t *__restrict__ toff, const int32_t *__restrict__ assign, int chunk_loci, int tile, uint32_t *__restrict__ cnt)
{
	extern __shared__ uint32_t cc_lds[];
	const int i = blockIdx.y * 256 + threadIdx.x;
	const bool live = i < I;
	const int k = live ? assign[i] : 0;
	const int l_begin = blockIdx.x * chunk_loci, l_end = L - l_begin < chunk_loci ? L : l_begin + chunk_loci;
	const int step = tile ? tile : chunk_loci;
	for (int t0 = l_begin; t0 < l_end; t0 += step) {
		const int t1 = l_end - t0 < step ? l_end : t0 + step;
		const int col0 = toff[t0], nwords = (toff[t1] - col0) * K;
		if (tile) {
			for (int x = threadIdx.x; x < nwords; x += 256) cc_lds[x] = 0;
			__syncthreads();
		}
		if (live)
			for (int g = t0 >> 3; g * 8 < t1; g++) {
				const uint32_t *src = reinterpret_cast<const uint32_t *>(gtS + ((size_t)g * I + i) * 8 * pl);
				for (int w = 0; w < 2 * pl; w++) {
					const uint32_t v4 = src[w];
#pragma unroll
					for (int y = 0; y < 4; y++) {
						const uint32_t mb = (v4 >> (8 * y)) & 0xFFu;
						const int l = g * 8 + (w * 4 + y) / pl;
						if (mb == MCHIP_MISSING || l >= t1) continue;
						const int c = toff[l] + (int)mb;
						if (tile) atomicAdd(&cc_lds[(size_t)(c - col0) * K + k], 1u);
						else atomicAdd(&cnt[(size_t)c * K + k], 1u);
					}
				}
			}
		if (tile) {
			__syncthreads();
			for (int x = threadIdx.x; x < nwords; x += 256)
				if (cc_lds[x]) atomicAdd(&cnt[(size_t)col0 * K + x], cc_lds[x]);
			__syncthreads();
		}
	}
}

/* eta[k] = (1 + n_k) / (I + K); per (k, l), left to right over m: e = 1 + (K - k) * c (the reference re-adds every individual's
 * counts inside its loop over k, rnd_init.c:296-318), temp += e, p = e / temp.  Exact integers below 2^53 divided by correctly
 * rounded IEEE divisions: the bits of the host form. */
__global__ void k_center_finish(int I, int L, int K, const int32_t *__restrict__ toff, const uint32_t *__restrict__ cnt,
		const uint32_t *__restrict__ nk, double *__restrict__ eta, double *__restrict__ P)
{
	const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx < (size_t)K) eta[idx] = (double)(1u + nk[idx]) / (double)(I + K);
	if (idx >= (size_t)K * L) return;
	const int k = (int)(idx % K), l = (int)(idx / K);
	const int c0 = toff[l], M = toff[l + 1] - c0;
	double temp = 0.0;
	for (int m = 0; m < M; m++) temp += 1.0 + (double)(K - k) * (double)cnt[(size_t)(c0 + m) * K + k];
	for (int m = 0; m < M; m++) P[(size_t)(c0 + m) * K + k] = (1.0 + (double)(K - k) * (double)cnt[(size_t)(c0 + m) * K + k]) / temp;
}

/* random_allele_center's assignment (rnd_init.c:552-580) given the centers the host drew: copy (i, a) of locus l goes to the
 * first cluster k whose center allele it carries; a copy that matches no center (a missing copy never does) takes the next
 * value of rand() % K, in i, a order within the locus.  lane = locus: the locus's non-matching copies are numbered by the
 * lane's own running count, their draws start draw_offset[l] into the byte stream `draws` (rand() % K of the candidate's
 * whole stream span, from k_draw_partition).  Writes the partition in stream-independent raw order [I][L][pl]. */
__global__ __launch_bounds__(256) void k_assign_by_centers(const uint8_t *__restrict__ gtA, int I, int L, int pl, int K,
		const uint8_t *__restrict__ centers, const unsigned long long *__restrict__ draw_offset,
		const uint8_t *__restrict__ draws, unsigned long long n_draws, uint8_t *raw, int *bad)
{
	const int l = blockIdx.x * 256 + threadIdx.x;
	if (l >= L) return;
	uint8_t cen[MCHIP_MAX_K];
	for (int k = 0; k < K; k++) cen[k] = centers[(size_t)l * K + k];
	unsigned long long next = draw_offset[l];
	for (int ib = 0; ib < (I + 7) / 8; ib++) {
		const uint8_t *src = gtA + ((size_t)ib * L + l) * 8 * (size_t)pl;
		for (int j = 0; j < 8; j++) {
			const int i = ib * 8 + j;
			if (i >= I) break;
			for (int b = 0; b < pl; b++) {
				const uint8_t g = src[j * pl + b];
				int kk = -1;
				if (g != MCHIP_MISSING)
					for (int k = 0; k < K; k++) {
						if (cen[k] == 0xFF) break;	/* center[k] == -1 ends the list (rnd_init.c:562-563) */
						if (cen[k] == g) { kk = k; break; }
					}
				if (kk < 0) {
					if (K == 1) kk = 0;			/* every copy to cluster 0, nothing drawn */
					else if (next < n_draws) kk = draws[next++];
					else { kk = 0; atomicOr(bad, 1); }	/* the host counted other genotypes than the device holds */
				}
				raw[((size_t)i * L + l) * pl + b] = (uint8_t)kk;
			}
		}
	}
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

/* acc + in[first] + in[first + stride] + ... (count terms, added in that order): the loads of eight terms are issued
 * together, the additions keep their order, so the result is the plain loop's to the last bit */
__device__ __forceinline__ double ordered_sum(double acc, const double *__restrict__ in, size_t first, size_t stride, int count)
{
	int x = 0;
	for (; x + 8 <= count; x += 8) {
		double v[8];
#pragma unroll
		for (int y = 0; y < 8; y++) v[y] = in[first + (size_t)(x + y) * stride];
#pragma unroll
		for (int y = 0; y < 8; y++) acc += v[y];
	}
	for (; x < count; x++) acc += in[first + (size_t)x * stride];
	return acc;
}

/* deterministic sum of n doubles by one block (fixed strided order, then a fixed tree); every thread must call it; the result is
 * valid in thread 0 (and red[] may be reused after the trailing barrier) */
__device__ __forceinline__ double block_ordered_sum(const double *__restrict__ in, int n, double *red)
{
	const double s = (int)threadIdx.x < n ? ordered_sum(0.0, in, threadIdx.x, MCHIP_BLOCK, (n - (int)threadIdx.x + MCHIP_BLOCK - 1) / MCHIP_BLOCK) : 0.0;
	const double v = block_tree_sum<MCHIP_BLOCK>(red, s);
	__syncthreads();
	return v;
}
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

/* loci per block of k_finalize_p_tile for this data set and K, or 0 where a locus can outgrow the tile (k_finalize_p then) */
static int finalize_p_loci(int K, int max_M)
{
	if (max_M > 64 || max_M < 1) return 0;
	const int n = FP_TILE / (max_M * K);
	return n >= 4 ? n : 0;
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

/* ------------------------------------------------------------------ helpers */
int check_slot(mchip_context *ctx, int slot)
{
	if (!ctx) return MCHIP_ERR_INVALID;
	if (!ctx->K) return fail(ctx, MCHIP_ERR_STATE, "no model set%s", nullptr);
	if (slot < 0 || slot > 2) return fail(ctx, MCHIP_ERR_INVALID, "slot out of range%s", nullptr);
	return MCHIP_OK;
}

static void prof_mark(mchip_context *ctx, int kind, bool start)
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
static int pair_profile_slot(mchip_context *ctx, size_t n_blocks, unsigned long long **marks)
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

/* what a data set's shape is to the launch geometry and the plan */
struct mchip_shape { int I, L, T, ploidy, min_M, max_M, count_bits; };

/* bits per packed allele count of the column pass's second genotype layout (gtC), 0 = none */
static int count_bits_for(int ploidy, const mchip_knobs &kn)
{
	if (kn.no_counts) return 0;
	return ploidy <= 3 ? 2 : (ploidy <= 15 ? 4 : 0);
}

/* Launch geometry of a model on a data set: a function of the shape, the model, the knobs and the device's CU count alone (it
 * touches neither the device nor a context: mchip_describe_plan runs it on a machine without a GPU). */
static mchip_geometry model_geometry(const mchip_shape &sh, int K, int admixture, int do_projection, double p_lb, const mchip_knobs &kn, int n_cu)
{
	mchip_geometry g = {};
	/* launch geometry.  Both passes are FP64-issue-bound and every workgroup does the same amount of work, so
	 * the grid's last partial "round" of workgroups runs at low occupancy: measured at config 3, 8 workgroups
	 * per CU cost 6.9 ms per EM step, 64 per CU 5.4 ms (profiles/r01_geometry_sweep.txt).  More chunks mean
	 * more partial-sum slabs (Apart/Spart are written and re-read once per step), so the chunk count is capped
	 * where the slab bytes reach ~30 % of the genotype bytes the pass streams (config 2: 0.188 -> 0.179 ms per step against 15 %;
	 * config 3 reaches its 64 workgroups per CU before either cap).  The column pass stops at 15 % once the grid fills the
	 * device twice over: its slabs are K*T doubles each and k_finalize_p reads them all (config 5: 28 -> 15 slabs, 1.61 ->
	 * 1.56 ms per step; scripts/diag/geom.sh).  Chunk sizes are multiples of 8. */
	const int per_cu_col = kn.per_cu_col, per_cu_ind = kn.per_cu_ind;	/* tuning knobs (default 64) */
	int target = per_cu_col * n_cu;
	const int col_tiles = (sh.T + MCHIP_BLOCK - 1) / MCHIP_BLOCK;
	const int iblocks = (sh.I + 7) / 8, lblocks = (sh.L + 7) / 8;
	const double slab_frac = kn.slab_frac;	/* tuning knob (default 0.3) */
	/* column pass: slab bytes per chunk 8*K*T, genotype bytes per chunk ichunk*L*ploidy */
	int min_ichunk = (int)ceil(8.0 * K * sh.T / (slab_frac * sh.L * sh.ploidy));
	int want = (target + col_tiles - 1) / col_tiles;
	int cap = sh.I / (min_ichunk > 0 ? min_ichunk : 1);
	{
		const int cap_lo = cap / 2;						/* half the slab budget */
		const int fill = (2 * 8 * n_cu + col_tiles - 1) / col_tiles;	/* two rounds of 8 resident workgroups per CU */
		const int soft = cap_lo > (fill < cap ? fill : cap) ? cap_lo : (fill < cap ? fill : cap);
		if (!kn.geometry_given && want > soft) want = soft;
	}
	if (want > cap) want = cap;
	if (want < 1) want = 1;
	if (want > iblocks) want = iblocks;
	if (sh.count_bits && !kn.no_roundup) {	/* the packed-count column pass puts MCHIP_COL_WAVES chunks into a workgroup: whole workgroups where the caps allow */
		const int up = ((want + MCHIP_COL_WAVES - 1) / MCHIP_COL_WAVES) * MCHIP_COL_WAVES;
		if (up <= cap && up <= iblocks) want = up;
	}
	{
		const int gran = sh.count_bits ? 128 / sh.count_bits : 8;	/* individuals per packed word */
		const int per = (sh.I + want - 1) / want;
		g.ichunk = ((per + gran - 1) / gran) * gran;
	}
	g.n_ichunks = (sh.I + g.ichunk - 1) / g.ichunk;
	/* individual pass: slab bytes per chunk 8*K*I, genotype bytes per chunk lchunk*I*ploidy */
	/* (the sparse pass gives an individual mchip_ind_split(K) lanes; the dense and mixture kernels one, and do not use n_ll_ind) */
	const int ind_per_block = mchip_qblock(K) / (admixture ? mchip_ind_split(K) : 1);
	const int ind_tiles = (sh.I + ind_per_block - 1) / ind_per_block;
	int min_lchunk = (int)ceil(8.0 * K / (slab_frac * sh.ploidy));
	target = per_cu_ind * n_cu;
	want = (target + ind_tiles - 1) / ind_tiles;
	cap = sh.L / (min_lchunk > 0 ? min_lchunk : 1);
	if (want > cap) want = cap;
	if (want < 1) want = 1;
	if (want > lblocks) want = lblocks;
	{	/* the sparse individual pass stages two tiles of 8 loci of P rows in LDS: use it while they fit 64 KiB */
		const size_t kp = (size_t)mchip_kp(K);
		const size_t lds = (2 * 8 * (size_t)sh.max_M * kp + mchip_qblock(K)) * sizeof(double);
		g.sparse = (sh.max_M <= MCHIP_SPARSE_MAX_M) && lds <= 65536 && !kn.force_dense;
	}
	/* cooperating waves (mchip_internal.h): chunks are still what ONE WAVE takes; a workgroup of the sparse individual-side kernels
	 * is ind_waves of them, so a whole number of workgroups wants a multiple of that many chunks where the caps allow it */
	const bool ind_coop = admixture && g.sparse && mchip_ind_split(K) == 1;
	g.ind_waves = ind_coop ? mchip_ind_waves(K, 8 * sh.max_M) : 1;
	if (ind_coop) {
		/* ... and a multiple of eight slab rows where possible: the sparse kernel then keeps a row on one XCD (coop_rows() in
		 * mchip_kernels_k.hip), and eight XCDs with 52 rows between them would have 7 and 6 each */
		const int w8 = 8 * g.ind_waves, w1 = g.ind_waves;
		const int up8 = ((want + w8 - 1) / w8) * w8, up1 = ((want + w1 - 1) / w1) * w1;
		if (up8 <= cap && up8 <= lblocks) want = up8;
		else if (up1 <= cap && up1 <= lblocks) want = up1;
	}
	g.lchunk = ((lblocks + want - 1) / want) * 8;
	g.n_lchunks = (sh.L + g.lchunk - 1) / g.lchunk;
	g.xcd_rows = (ind_coop && ((g.n_lchunks + g.ind_waves - 1) / g.ind_waves) % 8 == 0) ? 1 : 0;
	{	/* partial log likelihoods any pass can leave: one per workgroup; no individual-side kernel has fewer than 64 individuals
		 * per workgroup, no column-side one fewer than 64 columns */
		const int by_col = ((sh.T + 63) / 64) * g.n_ichunks, by_ind = ((sh.I + 63) / 64) * g.n_lchunks;
		(void)col_tiles; (void)ind_tiles;
		g.n_llpart = by_col > by_ind ? by_col : by_ind;
	}
	/* log-product check interval: with every parameter >= its lower bound, t = sum_k q_k p_k >= p_lb / K, so
	 * floor(200 / -log10(t_min)) multiplications keep a product that starts above 1e-100 above 1e-300
	 * (DESIGN.md section 4).  A block of 8 loci (or individuals) multiplies 8*ploidy times. */
	{
		const double tmin = p_lb / K;
		int blocks = 0;
		if (do_projection && tmin > 0 && tmin < 1) {
			const double mults = floor(200.0 / -log10(tmin));
			/* the sparse tetraploid pass checks twice per block (every 4 loci = 16 multiplications) */
			blocks = (int)(mults / (sh.ploidy == 4 ? 16.0 : 8.0 * sh.ploidy));
			if (blocks > 1 << 16) blocks = 1 << 16;
		}
		g.flush_blocks = blocks;
		/* Supported lower bounds (--bound): any value >= 0.  The fast kernels share one reciprocal among the four cells of a
		 * column-pass step (1 / (t0 t1 t2 t3)) and between the two copies of a locus, which needs every t > 0 and
		 * t^4 >= DBL_MIN: guaranteed when projection is on and p_lb >= 1e-75 (t >= p_lb).  Otherwise -- projection off
		 * (--projection: an unobserved allele column, e.g. the phantom slot of a locus with missing data or an allele a
		 * bootstrap replicate lacks, has P = 0 for every k, so t = 0 in its zero-count cells) or a smaller bound -- the
		 * kernels take one reciprocal per non-empty cell and zero-count cells contribute exactly 0, as in em_alg.c:338-342.
		 * A non-empty cell with t = 0 is NaN here as it is in the reference (n * 0 / 0). */
		g.safe_rcp = (!do_projection || !(p_lb >= 1e-75)) ? 1 : 0;
		if (kn.force_safe) g.safe_rcp = 1;
		if (g.safe_rcp) g.flush_blocks = 0;
	}
	return g;
}

/* the pass arguments that shape, geometry and knobs give: everything the plan reads, no buffer */
static mchip_pass_args shape_args(const mchip_shape &sh, const mchip_geometry &g, const mchip_knobs &kn, int K, int qstride, int has_missing)
{
	mchip_pass_args a;
	memset(&a, 0, sizeof a);
	a.I = sh.I; a.L = sh.L; a.T = sh.T; a.ploidy = sh.ploidy; a.K = K;
	a.count_bits = sh.count_bits; a.has_missing = has_missing;
	a.qstride = qstride;
	a.ichunk = g.ichunk; a.n_ichunks = g.n_ichunks;
	a.flush_blocks = g.flush_blocks;
	a.safe_rcp = g.safe_rcp;
	a.lchunk = g.lchunk; a.n_lchunks = g.n_lchunks;
	a.sparse = g.sparse; a.tile_cols = 8 * sh.max_M;
	a.biallelic = (sh.min_M == 2 && sh.max_M == 2 && !kn.no_bial) ? 1 : 0;
	a.ind_waves = g.ind_waves;
	a.xcd_rows = g.xcd_rows;
	a.no_col_split = kn.no_col_split;
	return a;
}

static mchip_shape shape_of(const mchip_context *ctx)
{
	return mchip_shape{ ctx->I, ctx->L, ctx->T, ctx->ploidy, ctx->min_M, ctx->max_M, ctx->count_bits };
}

static mchip_pass_args pass_args(mchip_context *ctx, int slot)
{
	mchip_pass_args a = shape_args(shape_of(ctx), ctx->geo, ctx->knob, ctx->K, ctx->qstride, ctx->has_missing);
	a.gtA = ctx->d_gtA; a.gtS = ctx->d_gtS; a.gtC = ctx->d_gtC;
	a.ua = ctx->d_ua; a.toff = ctx->d_toff; a.col_locus = ctx->d_col_locus; a.col_allele = ctx->d_col_allele;
	a.P = ctx->d_p[slot]; a.Q = ctx->d_q[slot];
	a.Apart = ctx->d_Apart; a.llpart = ctx->d_llpart; a.Spart = ctx->d_Spart;
	a.asA = ctx->d_asA; a.asS = ctx->d_asS;
	return a;
}

/* partial log likelihoods k_mix_finalize leaves: one per workgroup */
static int mix_ll_parts(int I) { return (I + MCHIP_BLOCK - 1) / MCHIP_BLOCK; }
/* the projection of P keeps its "fixed" flags in registers up to 64 alleles per locus, above that in d_flags */
static bool needs_byte_flags(int max_M) { return max_M > 64; }

/* the plan of these arguments, less what the knobs switch off */
static mchip_plan plan_for(const mchip_ktable *kt, const mchip_pass_args &a, const mchip_knobs &kn)
{
	mchip_plan p;
	kt->plan(a, &p);
	if (kn.no_pair) p.pair = 0;
	if (kn.no_dual) p.dual = 0;
	return p;
}

/* the finalisers behind an E step's passes: both in one launch (k_finalize_qp: an M step with individual mixing proportions whose P
 * side takes the tiled form), or k_finalize_q and the P side's, the latter behind k_sum_slabs where the column pass left many slabs */
struct estep_finish { int p_loci; bool slab_sum, fused; };
static estep_finish finish_for(const mchip_plan &p, int K, int max_M, bool indiv, int do_mstep, const mchip_knobs &kn)
{
	estep_finish f;
	f.p_loci = finalize_p_loci(K, max_M);
	f.slab_sum = p.col_slabs > 8 && !kn.no_slab_sum;
	f.fused = do_mstep && indiv && f.p_loci && !f.slab_sum && !kn.no_fused_finalize;
	return f;
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

/* How an instance is spelled: its kernel's name and, in the order of the kernel's template arguments, the fields of mchip_instance
 * that are those arguments (p pl, b bits, A accum, S safe, N nomiss, L ll, M mix, D dual, G staged). */
static const struct { const char *name, *args; } kernel_names[MCHIP_K_KINDS] = {
	{ "", "" },
	{ "k_column_pass", "pASL" },
	{ "k_column_counts", "bMS" },
	{ "k_column_counts_split", "bS" },
	{ "k_individual_pass", "p" },
	{ "k_individual_sparse", "pASND" },
	{ "k_individual_sparse_w", "pASND" },
	{ "k_individual_bial", "AN" },
	{ "k_estep_pair", "bpSN" },
	{ "k_mix_gather", "pG" },
	{ "k_mix_column", "p" },
};
static std::string instance_name(const mchip_instance &k)
{
	std::string out = kernel_names[k.kernel].name;
	for (const char *c = kernel_names[k.kernel].args; *c; c++) {
		const bool flag = *c == 'A' ? k.accum : *c == 'S' ? k.safe : *c == 'N' ? k.nomiss : *c == 'L' ? k.ll : *c == 'M' ? k.mix : *c == 'D' ? k.dual : k.staged;
		out += c == kernel_names[k.kernel].args ? "<" : ",";
		out += *c == 'p' ? std::to_string(k.pl) : *c == 'b' ? std::to_string(k.bits) : flag ? "true" : "false";
	}
	return out + ">";
}

int mchip_describe_plan(const mchip_plan_query *q, char *buf, int buf_len)
{
	if (!q || !buf || buf_len < 1) return MCHIP_ERR_INVALID;
	if (q->K < 1 || q->I < 1 || q->L < 1 || q->T < 1 || q->ploidy < 1 || q->ploidy > 64 || q->min_alleles > q->max_alleles ||
	    q->max_alleles < 1 || q->max_alleles > 255 || q->n_cu < 1)
		return MCHIP_ERR_INVALID;
	if (q->K > MCHIP_MAX_K) return MCHIP_ERR_UNSUPPORTED;
	mchip_knobs kn;
	read_knobs(&kn);
	const int K = q->K, indiv = q->admixture && !q->eta_constrained;
	const mchip_shape sh = { q->I, q->L, q->T, q->ploidy, q->min_alleles, q->max_alleles, count_bits_for(q->ploidy, kn) };
	const mchip_geometry g = model_geometry(sh, K, q->admixture, q->do_projection, q->p_lb, kn, q->n_cu);
	const mchip_pass_args a = shape_args(sh, g, kn, K, indiv ? K : 0, q->has_missing);
	const mchip_plan p = plan_for(mchip_get_ktable(K), a, kn);
	const estep_finish fin = finish_for(p, K, sh.max_M, indiv, 1, kn);
	std::vector<std::string> lines;
	auto launch = [&](const std::string &name) {
		for (const std::string &l : lines) if (l == name) return;
		lines.push_back(name);
	};
	auto fact = [&](const char *key, long v) { lines.push_back(std::string(key) + "=" + std::to_string(v)); };
	const char *finalize_p = fin.p_loci ? "k_finalize_p_tile" : "k_finalize_p";	/* (launch_finalize_p) */
	if (!q->admixture) {	/* run_mixture, with and without the M step, whatever the calls */
		launch(instance_name(p.mix_gather));
		launch("k_mix_finalize");
		launch(instance_name(p.mix_col));
		launch(finalize_p);
	} else {
		if (q->accel_cycle && p.col.ll) return MCHIP_ERR_UNSUPPORTED;	/* (mchip_accel_run: the dense pair runs cycle by cycle) */
		/* run_estep with the M step: the passes, then the finalisers */
		if (p.pair) launch(instance_name(p.pair_pass));	/* (one launch that runs the bodies of the two below) */
		launch(instance_name(p.col));
		launch(instance_name(p.sside));
		if (fin.fused) launch("k_finalize_qp");
		else {
			launch("k_finalize_q");
			if (fin.slab_sum) launch("k_sum_slabs");
			launch(finalize_p);
		}
		if (q->accel_cycle) {	/* accel_cycle_enqueue: log L of the second EM iterate and of the extrapolated point */
			if (p.dual) launch(instance_name(p.dual_pass));
			else { launch(instance_name(p.ll)); launch(instance_name(p.sside)); }
		} else {
			launch(instance_name(p.ll));						/* mchip_loglik */
			if (p.col.ll) launch(instance_name(p.ll));				/* mchip_e_step: run_estep without the M step */
			launch(instance_name(p.sside));
			launch("k_finalize_q");
			launch(instance_name(p.col.ll ? p.ll : p.sside));			/* mchip_loglik_prefetch */
		}
	}
	fact("n_ichunks", g.n_ichunks); fact("lchunk", g.lchunk); fact("n_lchunks", g.n_lchunks);
	fact("ind_waves", g.ind_waves); fact("xcd_rows", g.xcd_rows); fact("sparse", g.sparse);
	fact("col_slabs", q->admixture ? p.col_slabs : p.mix_col_slabs);
	fact("ind_slabs", p.ind_slabs);
	fact("ll_parts", q->admixture ? p.ll_parts : mix_ll_parts(q->I));
	fact("pair", q->admixture ? p.pair : 0); fact("dual", q->admixture ? p.dual : 0);
	fact("shared_eta", !indiv); fact("byte_flags", needs_byte_flags(sh.max_M));
	std::string out;
	for (const std::string &l : lines) out += l + "\n";
	if (out.size() >= (size_t)buf_len) return MCHIP_ERR_INVALID;
	memcpy(buf, out.c_str(), out.size() + 1);
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
	hipLaunchKernelGGL(k_transpose_kt_to_tk, dim3(nblk(KT)), dim3(256), 0, ctx->stream, ctx->d_stage, ctx->d_p[slot], ctx->K, ctx->T);
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
	hipLaunchKernelGGL(k_transpose_tk_to_kt, dim3(nblk(KT)), dim3(256), 0, ctx->stream, ctx->d_p[slot], ctx->d_stage, ctx->K, ctx->T);
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

/* out[0 .. count) = the `count` doubles of d_scalars that begin at `field` */
static int fetch_scalars(mchip_context *ctx, const double *field, int count, double *out)
{
	HIPCHK(hipMemcpyAsync(ctx->h_pinned, field, count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	for (int x = 0; x < count; x++) out[x] = ctx->h_pinned[x];
	return MCHIP_OK;
}

/* shared eta: eta[to] = normalise(sum_i S_ik), project (em_alg.c:604-648) */
static int finalize_shared_eta(mchip_context *ctx, int to, const int *stop = nullptr, double add = 0.0, int project = 1)
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
static void stop_check(mchip_context *ctx)
{
	hipLaunchKernelGGL(k_stop_check, dim3(1), dim3(MCHIP_BLOCK), 0, ctx->stream, ctx->d_run, &ctx->d_scalars->logL, ctx->d_llpart, ctx->ll_parts);
}

/* one pass that takes the log likelihood (kt->accum_q or kt->loglik), between the marks of a profiled run; ll given: its partial
 * sums' sum goes to that field of d_scalars (else the caller's next kernel adds them up) */
typedef void (*ll_pass_fn)(const mchip_pass_args &a, const mchip_plan &p, hipStream_t s);
static void ll_pass(mchip_context *ctx, int kind, ll_pass_fn launch, const mchip_pass_args &a, const mchip_plan &p, double *ll, const int *stop = nullptr)
{
	prof_mark(ctx, kind, true);
	launch(a, p, ctx->stream);
	prof_mark(ctx, kind, false);
	if (ll) reduce_ll(ctx, p.ll_parts, ll, stop);
}

/* mixture model: E step (mode 0, optionally followed by the M step) or logL_mixture (mode 1); ll: the field of d_scalars that
 * receives the log likelihood, by default logL for an E step and emll for logL_mixture */
static int run_mixture(mchip_context *ctx, int from, int to, int do_mstep, int mode, const int *stop = nullptr, double *ll = nullptr,
		       bool defer_ll = false)
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
static int run_estep(mchip_context *ctx, int from, int to, int do_mstep, const int *stop = nullptr, const int *skip_ind = nullptr,
		     bool defer_ll = false)
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
		if (marks) {
			hipLaunchKernelGGL(k_pair_spans, dim3(1), dim3(PAIR_SPAN_THREADS), 0, ctx->stream, marks, plan.pair_blocks, plan.pair_runs,
					   ctx->pair_spans[ctx->pair_used / PAIR_SPAN_CHUNK] + ctx->pair_used % PAIR_SPAN_CHUNK);
			ctx->pair_used++;
		}
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
static bool captured(mchip_context *ctx, hipGraphExec_t *exec, const std::function<int()> &enqueue)
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
	if (loglik) return fetch_scalars(ctx, &ctx->d_scalars->logL, 1, loglik);
	return MCHIP_OK;
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
	if (loglik) return fetch_scalars(ctx, &ctx->d_scalars->logL, 1, loglik);
	return MCHIP_OK;
}

int mchip_loglik(mchip_context *ctx, int slot, double *loglik)
{
	MCHIP_ENTRY();
	int rc = check_slot(ctx, slot);
	if (rc) return rc;
	HIPCHK(hipSetDevice(ctx->device));
	if (!ctx->admixture) {
		if ((rc = run_mixture(ctx, slot, slot, 0, 1))) return rc;
		if (loglik) return fetch_scalars(ctx, &ctx->d_scalars->emll, 1, loglik);
		return MCHIP_OK;
	}
	const mchip_pass_args a = pass_args(ctx, slot);
	ll_pass(ctx, MCHIP_KERN_LOGLIK, ctx->kt->loglik, a, plan_for(ctx->kt, a, ctx->knob), &ctx->d_scalars->emll);
	HIPCHK(hipGetLastError());
	if (loglik) return fetch_scalars(ctx, &ctx->d_scalars->emll, 1, loglik);
	return MCHIP_OK;
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
	if (loglik) return fetch_scalars(ctx, &ctx->d_scalars->ll_point, 1, loglik);
	return MCHIP_OK;
}

}	/* extern "C" */

/* the hard-partition counts are in Spart ([n_lchunks][I][K]) and in n_aslabs slabs of Apart: normalise (and project) into slot `to` */
int partition_finalize(mchip_context *ctx, int to, int counts, int n_aslabs)
{
	int rc;
	const int indiv = ctx->qstride != 0;
	const int project = counts ? 0 : ctx->do_projection;
	const double add = counts ? 1.0 : 0.0;
	ctx->empty_rows_nan[to] = counts ? 0 : (ctx->qstride ? 1 : 0);	/* an M step of the hard partition: 0 / 0 for such a row (rnd_init.c:356); with counts
									 * every count starts at 1 (rnd_init.c:624): 1 / K, as the device holds it */
	ctx->kt->finalize_q(ctx->I, ctx->K, ctx->geo.n_lchunks, ctx->d_Spart, ctx->d_q[to], ctx->qstride,
			    ctx->d_q[to], ctx->d_sik, indiv, 0, project, ctx->eta_lb, nullptr, ctx->stream, add);
	if (!indiv && (rc = finalize_shared_eta(ctx, to, nullptr, add, !counts))) return rc;
	hipLaunchKernelGGL(k_finalize_p, dim3(nblk((size_t)ctx->L * ctx->K)), dim3(MCHIP_BLOCK), 0, ctx->stream,
			   ctx->L, ctx->K, ctx->T, ctx->d_toff, n_aslabs, ctx->d_Apart, ctx->d_p[to], ctx->d_p[to],
			   0, add, project, ctx->p_lb, ctx->d_flags);
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(ctx->stream));
	return MCHIP_OK;
}

/* relayout of a partition held on the device in stream order, then the hard-partition M step into slot `to`
 * (counts = 0: random_initialize_admixture, rnd_init.c:349-357), or initialize_parameters_admixture (rnd_init.c:603-705)
 * from that partition (counts = 1: one count per copy on top of 1, normalised, never projected) */
int partition_mstep(mchip_context *ctx, const uint8_t *d_raw, int to, int counts)
{
	if (!ctx->d_asA) HIPCHK(hipMalloc((void **)&ctx->d_asA, ctx->geno_bytes_A));
	if (!ctx->d_asS) HIPCHK(hipMalloc((void **)&ctx->d_asS, ctx->geno_bytes_S));
	int *d_bad = bad_flag(ctx);
	HIPCHK(hipMemsetAsync(d_bad, 0, sizeof(int), ctx->stream));
	if (launch_relayout(ctx->stream, d_raw, ctx->I, ctx->L, ctx->ploidy, nullptr, ctx->K, ctx->d_asA, ctx->d_asS, d_bad))
		return fail(ctx, MCHIP_ERR_UNSUPPORTED, "data set too large for the layout kernel%s", nullptr);
	HIPCHK(hipGetLastError());
	int bad = 0;
	HIPCHK(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	if (bad) return fail(ctx, MCHIP_ERR_INVALID, "partition assignment >= K%s", nullptr);

	mchip_pass_args a = pass_args(ctx, to);
	if (ctx->init_geno_set) {	/* bootstrap fits: the partition indicators come from the observed haplotypes (rnd_init.c:471) */
		a.gtA = ctx->d_initA;
		a.gtS = ctx->d_initS;
	}
	a.part_counts = counts;
	ctx->kt->part_p(a, ctx->stream);
	ctx->kt->part_q(a, ctx->stream);
	return partition_finalize(ctx, to, counts, ctx->geo.n_ichunks);
}

int check_partition_call(mchip_context *ctx, const void *arg, int to)
{
	int rc = check_slot(ctx, to);
	if (rc) return rc;
	ctx->s_cache_slot = -1;
	if (!arg) return fail(ctx, MCHIP_ERR_INVALID, "null pointer%s", nullptr);
	if (!ctx->admixture) return fail(ctx, MCHIP_ERR_STATE, "allele partitions initialise the admixture model only%s", nullptr);
	return MCHIP_OK;
}

void launch_reduce_sum(mchip_context *ctx, const double *in, int n, double *out)
{
	hipLaunchKernelGGL(k_reduce_sum, dim3(1), dim3(MCHIP_BLOCK), 0, ctx->stream, in, n, out, (const int *)nullptr);
}
void launch_reduce_rows(mchip_context *ctx, const double *in, int n_rows, int n, double *out)
{
	hipLaunchKernelGGL(k_reduce_rows, dim3((unsigned)n_rows), dim3(MCHIP_BLOCK), 0, ctx->stream, in, n, out);
}

extern "C" {

int mchip_mstep_from_partition(mchip_context *ctx, const uint8_t *assign, int to)
{
	MCHIP_ENTRY();
	int rc = check_partition_call(ctx, assign, to);
	if (rc) return rc;
	HIPCHK(hipSetDevice(ctx->device));
	const size_t raw_bytes = (size_t)ctx->I * ctx->L * ctx->ploidy;
	scoped_dev<uint8_t> d_raw;
	HIPCHK(d_raw.alloc(raw_bytes));
	HIPCHK(hipMemcpyAsync(d_raw, assign, raw_bytes, hipMemcpyHostToDevice, ctx->stream));
	return partition_mstep(ctx, d_raw, to);
}

int mchip_init_from_allele_centers(mchip_context *ctx, const uint8_t *centers, const uint64_t *draw_offset, const uint32_t *window,
				   uint64_t n_draws, int to)
{
	MCHIP_ENTRY();
	int rc = check_partition_call(ctx, centers, to);
	if (rc) return rc;
	if (!draw_offset || !window) return fail(ctx, MCHIP_ERR_INVALID, "null pointer%s", nullptr);
	HIPCHK(hipSetDevice(ctx->device));
	/* rand() % K for the candidate's whole span of the stream (center draws included: the host knows which draws are whose).
	 * No allocation per candidate: the span, centers and offsets live in the context (grown when a candidate needs more), the
	 * assignment goes to the stream-order scratch buffer -- a hipFree would synchronise the whole device and stall the other
	 * --streams workers, n_rand_em_init times per initialisation */
	if ((rc = stream_buffer(ctx))) return rc;
	uint8_t *d_raw = ctx->d_draw;
	if (n_draws) {
		const size_t span = (((size_t)n_draws + RNG_CHUNK - 1) / RNG_CHUNK) * RNG_CHUNK;	/* whole chunks are written */
		HIPCHK(grow_dev(ctx, &ctx->d_cand_span, &ctx->cand_span_bytes, span + span / 8));
		if ((rc = draw_mod_stream(ctx, window, (size_t)n_draws, ctx->K, ctx->d_cand_span))) return rc;
	} else {
		HIPCHK(grow_dev(ctx, &ctx->d_cand_span, &ctx->cand_span_bytes, 16));	/* no copy draws: never read */
	}
	/* every offset must leave room for the locus's copies inside the span: a locus reads at most I*ploidy draws */
	for (int l = 0; l < ctx->L; l++)
		if (draw_offset[l] > n_draws) return fail(ctx, MCHIP_ERR_INVALID, "draw offset beyond the stream span%s", nullptr);
	HIPCHK(grow_dev(ctx, &ctx->d_cand_centers, &ctx->cand_center_bytes, (size_t)ctx->L * ctx->K));
	{
		size_t have = ctx->cand_loci * sizeof(unsigned long long);
		HIPCHK(grow_dev(ctx, &ctx->d_cand_off, &have, (size_t)ctx->L * sizeof(unsigned long long)));
		ctx->cand_loci = have / sizeof(unsigned long long);
	}
	uint8_t *d_span = ctx->d_cand_span, *d_cen = ctx->d_cand_centers;
	unsigned long long *d_off = ctx->d_cand_off;
	HIPCHK(hipMemcpyAsync(d_cen, centers, (size_t)ctx->L * ctx->K, hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(hipMemcpyAsync(d_off, draw_offset, sizeof(uint64_t) * (size_t)ctx->L, hipMemcpyHostToDevice, ctx->stream));
	int *d_bad = bad_flag(ctx);
	HIPCHK(hipMemsetAsync(d_bad, 0, sizeof(int), ctx->stream));
	hipLaunchKernelGGL(k_assign_by_centers, dim3(nblk((size_t)ctx->L)), dim3(256), 0, ctx->stream,
			   ctx->init_geno_set ? ctx->d_initA : ctx->d_gtA, ctx->I, ctx->L, ctx->ploidy, ctx->K, d_cen, d_off, d_span,
			   (unsigned long long)n_draws, d_raw, d_bad);
	HIPCHK(hipGetLastError());
	int bad = 0;
	HIPCHK(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	if (bad) return fail(ctx, MCHIP_ERR_INVALID, "allele-center draws run past the stream span: offsets do not match the genotype held%s", nullptr);
	rc = partition_mstep(ctx, d_raw, to, 1);
	(void)MCHIP_WAIT(hipStreamSynchronize(ctx->stream));	/* centers / draw_offset are the caller's: uploaded by now */
	return rc;
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

int mchip_init_from_individual_centers(mchip_context *ctx, const int32_t *centers, int to, int32_t *assign_out)
{
	MCHIP_ENTRY();
	int rc = check_slot(ctx, to);
	if (rc) return rc;
	ctx->s_cache_slot = -1;
	if (!centers) return fail(ctx, MCHIP_ERR_INVALID, "null pointer%s", nullptr);
	if (ctx->admixture) return fail(ctx, MCHIP_ERR_STATE, "individual centers initialise the mixture model only%s", nullptr);
	const int I = ctx->I, L = ctx->L, K = ctx->K, pl = ctx->ploidy, T = ctx->T;
	for (int k = 0; k < K; k++) {
		if (centers[k] < 0 || centers[k] >= I) return fail(ctx, MCHIP_ERR_INVALID, "center out of range%s", nullptr);
		for (int j = 0; j < k; j++)
			if (centers[j] == centers[k]) return fail(ctx, MCHIP_ERR_INVALID, "centers are not distinct%s", nullptr);
	}
	HIPCHK(hipSetDevice(ctx->device));
	/* work: counts [T][K], n_k [K], centers [K], assignment [I] */
	const size_t n_cnt = (size_t)T * K;
	HIPCHK(grow_dev(ctx, &ctx->d_cen_work, &ctx->cen_work_bytes, (n_cnt + 2 * (size_t)K + (size_t)I) * sizeof(uint32_t)));
	uint32_t *d_cnt = ctx->d_cen_work, *d_nk = d_cnt + n_cnt;
	int32_t *d_centers = reinterpret_cast<int32_t *>(d_nk + K), *d_assign = d_centers + K;
	HIPCHK(hipMemsetAsync(d_cnt, 0, (n_cnt + (size_t)K) * sizeof(uint32_t), ctx->stream));
	HIPCHK(hipMemcpyAsync(d_centers, centers, sizeof(int32_t) * (size_t)K, hipMemcpyHostToDevice, ctx->stream));
	const int n_groups = (L + 7) / 8;
	int n_dist_chunks = 0;
	if (K > 1) {
		/* threads per workgroup: the K accumulators of a thread live in LDS ([K][threads] words, at most 32 KiB) */
		const int tiled = pl <= 8;
		const int nthr = tiled ? (K <= 32 ? 256 : 128) : (K <= 32 ? 128 : 64);
		const unsigned n_iblocks = (unsigned)((I + nthr - 1) / nthr);
		int want = (int)(2048 / n_iblocks);
		if (want < 1) want = 1;
		int chunk_groups = (n_groups + want - 1) / want;
		if (chunk_groups < 8) chunk_groups = 8;
		if (chunk_groups > n_groups) chunk_groups = n_groups;
		const unsigned n_chunks = (unsigned)((n_groups + chunk_groups - 1) / chunk_groups);
		int tile_groups = 16384 / (K * 8 * pl);		/* staged center rows near 16 KiB */
		if (tile_groups < 1) tile_groups = 1;
		if (tile_groups > chunk_groups) tile_groups = chunk_groups;
		const size_t lds = ((size_t)K * nthr + (size_t)tile_groups * K * 2 * pl) * sizeof(uint32_t) + (tiled ? 0 : (size_t)pl * nthr);
		if (lds > 64 * 1024) return fail(ctx, MCHIP_ERR_UNSUPPORTED, "center distances: the shape does not fit the kernel%s", nullptr);
		HIPCHK(grow_dev(ctx, &ctx->d_cen_part, &ctx->cen_part_bytes, (size_t)n_chunks * K * I * sizeof(uint32_t)));
		if (tiled)
			with_ploidy(pl, [&](auto PL) { launch_center_distance<PL()>(ctx, n_iblocks, n_chunks, nthr, lds, d_centers, chunk_groups, tile_groups); });
		else
			launch_center_distance<0>(ctx, n_iblocks, n_chunks, nthr, lds, d_centers, chunk_groups, tile_groups);
		HIPCHK(hipGetLastError());
		n_dist_chunks = (int)n_chunks;
	}
	/* K = 1: no chunk, every distance 0, every individual joins cluster 0 (rnd_init.c:199-204) */
	hipLaunchKernelGGL(k_center_assign, dim3(nblk((size_t)I)), dim3(256), 0, ctx->stream, ctx->d_cen_part, n_dist_chunks, I, K, d_centers,
			   d_assign, d_nk);
	HIPCHK(hipGetLastError());
	{
		const unsigned n_iblocks = (unsigned)((I + 255) / 256);
		int want = (int)(2048 / n_iblocks);
		if (want < 1) want = 1;
		int chunk_loci = (((L + want - 1) / want) + 7) & ~7;
		if (chunk_loci < 64) chunk_loci = 64;
		/* counters of a tile: tile * max_M * K words, at most 32 KiB, a multiple of 8 loci; none when 8 loci do not fit */
		int tile = (int)((8192 / ((size_t)ctx->max_M * K)) & ~(size_t)7);
		if (tile > chunk_loci) tile = chunk_loci;
		const size_t lds = (size_t)tile * ctx->max_M * K * sizeof(uint32_t);
		hipLaunchKernelGGL(k_center_counts, dim3((unsigned)((L + chunk_loci - 1) / chunk_loci), n_iblocks), dim3(256), lds, ctx->stream,
				   ctx->d_gtS, I, L, pl, K, ctx->d_toff, d_assign, chunk_loci, tile, d_cnt);
		HIPCHK(hipGetLastError());
	}
	hipLaunchKernelGGL(k_center_finish, dim3(nblk((size_t)K * L)), dim3(256), 0, ctx->stream, I, L, K, ctx->d_toff, d_cnt, d_nk, ctx->d_q[to],
			   ctx->d_p[to]);
	HIPCHK(hipGetLastError());
	ctx->empty_rows_nan[to] = 0;	/* as mchip_set_q leaves the slot for finite rows */
	if (assign_out) HIPCHK(hipMemcpyAsync(assign_out, d_assign, sizeof(int32_t) * (size_t)I, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));	/* centers is the caller's: uploaded by now */
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
	hipLaunchKernelGGL(k_transpose_kt_to_tk, dim3(nblk(KT)), dim3(256), 0, ctx->stream, ctx->d_stage, which ? ctx->d_vp[j] : ctx->d_up[j], ctx->K, ctx->T);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(which ? ctx->d_vq[j] : ctx->d_uq[j], q_part, (size_t)ctx->nq * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
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
	hipLaunchKernelGGL(k_transpose_tk_to_kt, dim3(nblk(KT)), dim3(256), 0, ctx->stream, which ? ctx->d_vp[j] : ctx->d_up[j], ctx->d_stage, ctx->K, ctx->T);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(p_part, ctx->d_stage, KT * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipMemcpyAsync(q_part, which ? ctx->d_vq[j] : ctx->d_uq[j], (size_t)ctx->nq * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
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
	double *dp = which ? ctx->d_vp[j] : ctx->d_up[j];
	double *dq = which ? ctx->d_vq[j] : ctx->d_uq[j];
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

static int project_slot(mchip_context *ctx, int to, const int *stop = nullptr)
{
	if (!ctx->do_projection) return MCHIP_OK;
	hipLaunchKernelGGL(k_project_p, dim3(nblk((size_t)ctx->L * ctx->K)), dim3(MCHIP_BLOCK), 0, ctx->stream,
			   ctx->L, ctx->K, ctx->d_toff, ctx->d_p[to], ctx->p_lb, ctx->d_flags, stop);
	ctx->kt->project_q(ctx->qstride ? ctx->I : 1, ctx->K, ctx->d_q[to], ctx->eta_lb, stop, ctx->stream);
	HIPCHK(hipGetLastError());
	return MCHIP_OK;
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
