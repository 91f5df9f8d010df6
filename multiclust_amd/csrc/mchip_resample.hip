/*
 * mchip_resample.hip -- a data set made of a selection of loci with repeats: mchip_resample_loci and its kernel
 * (include/multiclust_hip.h has the contract; mchip_context.h the per-context state and the install path).
 *
 *   k_resample_gather   out[i][j][.] = base[i][src[j]][.], both in upload form.  A workgroup takes a chunk of RS_CHUNK output
 *                       loci and stages their source indices in LDS once; it then walks individuals (blockIdx.y, grid stride).
 *                       Within an individual consecutive threads take consecutive output loci, so a wave writes 64 * ploidy
 *                       contiguous bytes of one individual's output row and its reads stay inside that individual's base row
 *                       (L_base * ploidy bytes: 200 KB at the headline shape, which the L2 cache holds while the chunks of the
 *                       row are gathered).  Every index is 64-bit: I * L * ploidy is 2 * 10^9 at the headline shape.
 *                       A thread that met an observed copy marks its individual, as k_cv_mask does.
 *                       Measured cost: profiles/locus_bootstrap.txt.
 */
#include "mchip_context.h"

constexpr int RS_CHUNK = 1024;	/* output loci per workgroup: 4 KB of staged indices, four loci per thread and individual */

/* base: the saved data set in upload form [I][L_base][ploidy]; src: L2 locus indices, each in [0, L_base) (checked by the caller);
 * out in upload form [I][L2][ploidy]; seen[i] (zeroed by the caller) = 1 for every individual that keeps an observed copy */
__global__ __launch_bounds__(256) void k_resample_gather(const uint8_t *__restrict__ base, const int32_t *__restrict__ src, int I,
							 int L_base, int L2, int pl, uint8_t *__restrict__ out, uint8_t *seen)
{
	__shared__ int32_t s_src[RS_CHUNK];
	const int j0 = blockIdx.x * RS_CHUNK, nj = min(RS_CHUNK, L2 - j0);
	for (int x = threadIdx.x; x < nj; x += 256) s_src[x] = src[j0 + x];
	__syncthreads();
	for (int i = blockIdx.y; i < I; i += gridDim.y) {
		const uint8_t *__restrict__ brow = base + (size_t)i * L_base * pl;
		uint8_t *__restrict__ orow = out + ((size_t)i * L2 + j0) * pl;
		bool any = false;
		for (int x = threadIdx.x; x < nj; x += 256) {
			const uint8_t *g = brow + (size_t)s_src[x] * pl;
			for (int a = 0; a < pl; a++) {
				const uint8_t v = g[a];
				any |= v != MCHIP_MISSING;
				orow[(size_t)x * pl + a] = v;
			}
		}
		if (any) seen[i] = 1;	/* (every writer stores the same value) */
	}
}

/* the selection src[0 .. L2) of the saved base -> the installed data set, whose shape is the selection's by now */
static int install_selection(mchip_context *ctx, const int32_t *src, int L2)
{
	scoped_dev<int32_t> d_src;
	HIPCHK(d_src.alloc((size_t)L2));
	HIPCHK(hipMemcpyAsync(d_src.p, src, sizeof(int32_t) * (size_t)L2, hipMemcpyHostToDevice, ctx->stream));
	return install_derived(ctx, [&](uint8_t *d_out, uint8_t *d_seen) {
		const unsigned chunks = (unsigned)((L2 + RS_CHUNK - 1) / RS_CHUNK);
		/* enough workgroups to fill the device many times over, each staging its indices for several individuals */
		const unsigned want = (65536u + chunks - 1) / chunks;
		const unsigned rows = nblk_capped((size_t)ctx->I, 1, want < 65535u ? want : 65535u);
		hipLaunchKernelGGL(k_resample_gather, dim3(chunks, rows), dim3(256), 0, ctx->stream, ctx->rs_base.d_raw, d_src.p, ctx->I,
				   ctx->rs_base.L, L2, ctx->ploidy, d_out, d_seen);
	});
}

extern "C" int mchip_resample_loci(mchip_context *ctx, const int32_t *src, int L2)
{
	MCHIP_ENTRY();
	if (!ctx) return MCHIP_ERR_INVALID;
	if (!ctx->T) return fail(ctx, MCHIP_ERR_STATE, "no genotypes set%s", nullptr);
	if (ctx->cv_fold >= 0) return fail(ctx, MCHIP_ERR_STATE, "resample_loci: a cross-validation fold is held out%s", nullptr);
	saved_set &base = ctx->rs_base;
	if (!src && !base.d_raw) return fail(ctx, MCHIP_ERR_STATE, "resample_loci: no saved base to install again%s", nullptr);
	const int I = ctx->I, pl = ctx->ploidy;
	const int Lb = base.d_raw ? base.L : ctx->L;
	std::vector<int32_t> ua2;
	if (src) {	/* everything that can be refused is refused before anything is touched */
		if (L2 < 1) return fail(ctx, MCHIP_ERR_INVALID, "resample_loci: L2 must be at least 1%s", nullptr);
		const std::vector<int32_t> &ua_base = base.d_raw ? base.ua : ctx->h_ua;
		long long T2 = 0;
		ua2.resize((size_t)L2);
		for (int j = 0; j < L2; j++) {
			if (src[j] < 0 || src[j] >= Lb) return fail(ctx, MCHIP_ERR_INVALID, "resample_loci: locus index outside [0, L_base)%s", nullptr);
			T2 += (ua2[j] = ua_base[src[j]]);
		}
		if (T2 > 2000000000LL) return fail(ctx, MCHIP_ERR_INVALID, "too many allele columns%s", nullptr);
		if (T2 <= 0) return fail(ctx, MCHIP_ERR_INVALID, "no alleles%s", nullptr);
	} else {
		L2 = Lb;
	}
	HIPCHK(hipSetDevice(ctx->device));
	int rc;
	/* the data set installed now is the base: keep it */
	if (!base.d_raw && (rc = save_installed(ctx, base))) return rc;
	/* the new shape: tables, buffers, no model, no init genotypes, no cross-validation state -- and the base stays */
	rc = set_shape(ctx, I, L2, pl, src ? ua2.data() : base.ua.data(), KEEP_RS_BASE);
	if (!rc) rc = src ? install_selection(ctx, src, L2) : install_saved(ctx, base);
	if (rc) {	/* a failure half way: no data set (set_shape), or one whose bytes are not what was asked for */
		free_model(ctx);
		free_data(ctx);
		return rc;
	}
	return MCHIP_OK;
}
