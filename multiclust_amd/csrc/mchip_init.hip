/*
 * mchip_init.hip -- initialisations that run on the device: the mixture model's from individual centers, the admixture model's
 * from allele centers, and the M step of a hard partition (which mchip_generators.hip calls for the partitions it draws).
 */
#include "mchip_context.h"

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
	launch_finalize_p_untiled(ctx, n_aslabs, to, add, project);
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

}	/* extern "C" */
