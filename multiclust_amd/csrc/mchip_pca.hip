/*
 * mchip_pca.hip -- principal components of packed PLINK records: mchip_bed_pca_apply, mchip_bed_pca and their kernels
 * (include/multiclust_hip.h has the matrix and the contracts; mchip_pca_algebra.h the iteration and its host algebra;
 * mchip_context.h the context and what every unit shares of the records: bed_word, bed_stage_tile, bed_upload).  Installs nothing.
 *
 * G = Z Z^T / L' is never formed: Y = G X is two products over the 2-bit records, W = Z^T X and Y = Z W / L', both on
 * v_mfma_f64_16x16x4_f64 with the A operand decoded from the codes on the way in.  The column count b is a multiple of 16 here
 * (the entry points pad); NB = b / 16 is a template argument, so the accumulators are registers.
 *
 *   k_pca_scale    a wave per variant, four to a workgroup: the counts n0, n2, n3 of the record by population count over 64-bit
 *                  words (the word loop and mask of k_qc_variants, the mask formed from I), then lane 0 the used flag, mu, inv, the
 *                  four-entry table z[code] and t_l.  Integers up to mu.  L' and the trace are summed on the host in index order.
 *   k_pca_project  W[l][c] = sum_i z_il X[i][c].  A workgroup owns BT_L = 64 variants, a wave 16 of them, and walks ALL individuals
 *                  in ascending tiles of BT_I = 256 staged by bed_stage_tile; per 64 individuals the X rows go to LDS, those of the
 *                  next 64 on their way from memory into registers meanwhile.  A lane
 *                  keeps the table of its variant in three registers: A = select by the code, B = one LDS read per instruction.
 *                  No split along I, no atomics: the order of the additions of an element depends on (I, b) alone.
 *                  A: lane holds z[variant = lane & 15][individual = lane >> 4]; B: X[individual = lane >> 4][column = lane & 15];
 *                  C/D: column = lane & 15, variant = (lane >> 4) + 4 reg (the map of k_resid_gram, mchip_residuals.hip).
 *   k_pca_expand   partial[slab][i][c] = sum over the slab's variants of z_il W[l][c].  A workgroup owns PCA_ITILE = 64 individuals, a
 *                  wave 16 of them, and one slab of PCA_LSLAB variants (a constant, mchip_feature_geometry.h: the cut is a function of
 *                  L alone, no launch knob shows in any bit); per 64 variants their codes (16 bytes a record), tables and W rows go
 *                  to LDS, the W rows fetched ahead likewise.  A = the table entry of (variant, code), one LDS read; B = a W row element.
 *   k_pca_fold     Y[i][c] = (partial[0][i][c] + partial[1][i][c] + ...) / L', the slabs in index order.
 *   Staged X / W rows are pca_pitch(b) doubles apart: the two rows a half wave reads fall into different halves of the banks.
 *   Rows of individuals behind I: X is staged as zeros there (project) and the rows of partial are never read (fold), so garbage in
 *   the padding bits of a record reaches nothing.
 *
 *   Compile report (hipcc of ROCm 7.2, gfx950, -O3, -Rpass-analysis=kernel-resource-usage):  k_pca_scale 26 VGPRs, k_pca_fold 16;
 *   k_pca_project<1..4> 52 / 85 / 104 / 102 VGPRs + 8 NB AGPRs (the accumulators), 8 / 4 / 4 / 3 waves / SIMD, 4352 bytes of static
 *   LDS; k_pca_expand<1..4> 50 / 76 / 138 / 122 VGPRs + 8 NB AGPRs, 8 / 5 / 3 / 3 waves / SIMD, 3328 bytes; scratch 0 everywhere.
 *   Timed once, one A/B kept (the rows of the next stage fetched ahead: 4.78 -> 3.46 and 3.61 -> 2.79 ms at 64 columns) and not tuned
 *   beyond it: at 10 000 x 100 000 the expansion runs at 46 TF/s, the rate of k_resid_gram in the same run (48), the projection at
 *   27 - 37 TF/s, rising with the width: what it pays per four individuals for the decode does not scale with the columns
 *   (profiles/pca.txt, scripts/pca_bench.py).
 */
#include "mchip_context.h"
#include "mchip_pca_algebra.h"

static_assert(PCA_MAX_BLOCK == MCHIP_PCA_MAX_VECTORS, "the host algebra and the header agree on the widest block");
static_assert(PCA_VARIANTS == BT_L && PCA_ITILE == 64 && PCA_LSLAB % BT_L == 0 && MCHIP_PCA_MAX_VECTORS == 64,
	      "k_pca_project and k_pca_expand are written for these");

typedef double pca_d4 __attribute__((ext_vector_type(4)));
constexpr int PCA_CROW = 5;	/* dwords between the staged codes of two records in k_pca_expand: four of data, one of padding */

__host__ __device__ constexpr int pca_pitch(int b) { return b % 32 == 0 ? b + 16 : b; }

/* The operand rows of a stage: the 64 rows r0 ... r0 + 63 of M [n_rows][16 NB], zeros behind row n_rows - 1, travel from memory into
 * 4 NB registers a thread (element t, t + 256, ... of the 64 x 16 NB block) while the products of the stage before run, as in
 * k_resid_gram, and go to LDS pca_pitch apart once that stage has been read. */
template <int NB> __device__ __forceinline__ void pca_fetch_rows(double (&pre)[4 * NB], const double *__restrict__ M, long long r0, long long n_rows, int tid)
{
	constexpr int b = 16 * NB;
#pragma unroll
	for (int x = 0; x < 4 * NB; x++) {
		const int e = tid + 256 * x, r = e / b, c = e % b;
		pre[x] = r0 + r < n_rows ? M[(size_t)(r0 + r) * b + c] : 0.0;
	}
}
template <int NB> __device__ __forceinline__ void pca_store_rows(double *rows, const double (&pre)[4 * NB], int tid)
{
	constexpr int b = 16 * NB, pitch = pca_pitch(b);
#pragma unroll
	for (int x = 0; x < 4 * NB; x++) {
		const int e = tid + 256 * x;
		rows[(e / b) * pitch + e % b] = pre[x];
	}
}

/* tab[l][code] = z of the code at variant l (0 for a missing call and on an unused variant), scale[l] = {mu, inv} (0, 0 unused),
 * t[l] = the variant's part of the trace (0 unused), used[l] = 1 / 0 */
__global__ __launch_bounds__(256) void k_pca_scale(const uint8_t *__restrict__ bed, size_t rb, int I, int L, double *__restrict__ tab,
						   double *__restrict__ scale, double *__restrict__ t, int32_t *__restrict__ used)
{
#pragma clang fp contract(off)
	const int lane = threadIdx.x & 63;
	const long long l = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (l >= L) return;	/* (a whole wave) */
	const int n_words = (I + 31) / 32;
	const uint64_t low = 0x5555555555555555ull;
	uint32_t c0 = 0, c2 = 0, c3 = 0;
	for (int w = lane; w < n_words; w += 64) {
		const size_t off = 8 * (size_t)w;
		uint64_t v = bed_word(bed, (size_t)l * rb + off);
		if (off + 4 < rb) v |= (uint64_t)bed_word(bed, (size_t)l * rb + off + 4) << 32;
		const int n = I - 32 * w;	/* individuals in this word: bits behind them are padding, or the next record */
		const uint64_t m = n >= 32 ? low : (((1ull << (2 * n)) - 1ull) & low);
		const uint64_t lo = v & m, hi = (v >> 1) & m;
		c0 += (uint32_t)__popcll(m & ~lo & ~hi);
		c2 += (uint32_t)__popcll(hi & ~lo);
		c3 += (uint32_t)__popcll(lo & hi);
	}
	c0 = wave_sum_u32(c0); c2 = wave_sum_u32(c2); c3 = wave_sum_u32(c3);
	if (lane) return;
	const int64_t n = (int64_t)c0 + c2 + c3, s = (int64_t)c2 + 2 * (int64_t)c3;
	double z[4] = { 0.0, 0.0, 0.0, 0.0 }, mu = 0.0, inv = 0.0, tl = 0.0;
	const bool use = s > 0 && s < 2 * n;
	if (use) {
		mu = (double)s / (double)n;
		inv = 1.0 / sqrt(mu * (1.0 - 0.5 * mu));
		z[0] = (0.0 - mu) * inv;
		z[2] = (1.0 - mu) * inv;
		z[3] = (2.0 - mu) * inv;
		tl = ((double)c0 * (mu * mu) + (double)c2 * ((1.0 - mu) * (1.0 - mu)) + (double)c3 * ((2.0 - mu) * (2.0 - mu))) * (inv * inv);
	}
	for (int c = 0; c < 4; c++) tab[4 * (size_t)l + c] = z[c];
	scale[2 * (size_t)l] = mu;
	scale[2 * (size_t)l + 1] = inv;
	t[l] = tl;
	used[l] = use ? 1 : 0;
}

/* W [L][16 NB] = Z^T X for X [I][16 NB]; grid ceil(L / BT_L), 256 threads, 64 * pca_pitch(16 NB) doubles of dynamic LDS */
template <int NB>
__global__ __launch_bounds__(256) void k_pca_project(const uint8_t *__restrict__ bed, size_t rb, int I, int L, const double *__restrict__ tab,
						     const double *__restrict__ X, double *__restrict__ W)
{
	constexpr int b = 16 * NB, pitch = pca_pitch(b);
	extern __shared__ __attribute__((aligned(16))) double pca_rows[];	/* [64][pitch] */
	__shared__ uint32_t tile[BT_L * BT_ROW];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4;
	const int l0 = blockIdx.x * BT_L, ll = 16 * wave + lr;
	double z0 = 0.0, z2 = 0.0, z3 = 0.0;	/* the table of this lane's variant; behind L the staged codes are 0 and so is z0 */
	if ((long long)l0 + ll < L) {
		const double *tl = tab + 4 * ((size_t)l0 + ll);
		z0 = tl[0]; z2 = tl[2]; z3 = tl[3];
	}
	pca_d4 acc[NB];
#pragma unroll
	for (int cb = 0; cb < NB; cb++) acc[cb] = pca_d4{ 0.0, 0.0, 0.0, 0.0 };
	double pre[4 * NB];
	pca_fetch_rows<NB>(pre, X, 0, I, tid);
	for (int ibase = 0; ibase < I; ibase += 64) {
		const int sub = (ibase % BT_I) / 64;
		__syncthreads();	/* the X rows before, and every fourth time the tile before, have been read */
		if (!sub) bed_stage_tile(tile, bed, rb, L, l0, ibase);
		pca_store_rows<NB>(pca_rows, pre, tid);
		__syncthreads();
		pca_fetch_rows<NB>(pre, X, (long long)ibase + 64, I, tid);	/* (behind the last individual: zeros, no load) */
		const uint32_t *trow = tile + ll * BT_ROW + 4 * sub;
#pragma unroll
		for (int q = 0; q < 4; q++) {
			const uint32_t word = trow[q];	/* the individuals ibase + 16 q ... + 15 of this lane's variant */
#pragma unroll
			for (int s = 0; s < 4; s++) {
				const uint32_t c = (word >> (2 * (4 * s + lk))) & 3u;
				const double a = c == 0u ? z0 : c == 2u ? z2 : c == 3u ? z3 : 0.0;
				const double *xr = pca_rows + (16 * q + 4 * s + lk) * pitch + lr;
#pragma unroll
				for (int cb = 0; cb < NB; cb++) acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, xr[16 * cb], acc[cb], 0, 0, 0);
			}
		}
	}
#pragma unroll
	for (int r = 0; r < 4; r++) {
		const long long l = (long long)l0 + 16 * wave + lk + 4 * r;
		if (l >= L) continue;
#pragma unroll
		for (int cb = 0; cb < NB; cb++) W[(size_t)l * b + 16 * cb + lr] = acc[cb][r];
	}
}

/* partial [n_slabs][Ipad][16 NB]: slab blockIdx.y's part of Z W for the individuals 64 blockIdx.x ...; 256 threads, 64 *
 * pca_pitch(16 NB) doubles of dynamic LDS */
template <int NB>
__global__ __launch_bounds__(256) void k_pca_expand(const uint8_t *__restrict__ bed, size_t rb, int L, int Ipad, const double *__restrict__ tab,
						    const double *__restrict__ W, double *__restrict__ partial)
{
	constexpr int b = 16 * NB, pitch = pca_pitch(b);
	extern __shared__ __attribute__((aligned(16))) double pca_rows[];	/* [64][pitch] */
	__shared__ double tabs[BT_L * 4];
	__shared__ uint32_t codes[BT_L * PCA_CROW];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4;
	const int i0 = blockIdx.x * PCA_ITILE;
	const long long lbeg = (long long)blockIdx.y * PCA_LSLAB;
	const int lend = (int)min((long long)L, lbeg + PCA_LSLAB);
	pca_d4 acc[NB];
#pragma unroll
	for (int cb = 0; cb < NB; cb++) acc[cb] = pca_d4{ 0.0, 0.0, 0.0, 0.0 };
	double pre[4 * NB];
	pca_fetch_rows<NB>(pre, W, lbeg, lend, tid);
	for (int l0 = (int)lbeg; l0 < lend; l0 += BT_L) {
		__syncthreads();	/* the variants before have been read */
		{	/* 64 records x the 16 bytes of this tile's individuals, 64 tables of four; behind lend zeros */
			const int ll = tid / 4, w = tid % 4;
			const bool in = l0 + ll < lend;
			const size_t off = (size_t)(i0 / 4) + 4 * (size_t)w;
			codes[ll * PCA_CROW + w] = (in && off < rb) ? bed_word(bed, (size_t)(l0 + ll) * rb + off) : 0u;
			tabs[tid] = in ? tab[4 * (size_t)l0 + tid] : 0.0;
		}
		pca_store_rows<NB>(pca_rows, pre, tid);
		__syncthreads();
		pca_fetch_rows<NB>(pre, W, (long long)l0 + BT_L, lend, tid);	/* (behind the slab's last variant: zeros, no load) */
#pragma unroll 4
		for (int s = 0; s < BT_L / 4; s++) {
			const int ll = 4 * s + lk;
			const uint32_t c = (codes[ll * PCA_CROW + wave] >> (2 * lr)) & 3u;	/* individual i0 + 16 wave + lr */
			const double a = tabs[4 * ll + c];
			const double *wr = pca_rows + ll * pitch + lr;
#pragma unroll
			for (int cb = 0; cb < NB; cb++) acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, wr[16 * cb], acc[cb], 0, 0, 0);
		}
	}
	double *out = partial + ((size_t)blockIdx.y * Ipad + i0 + 16 * wave + lk) * b + lr;
#pragma unroll
	for (int r = 0; r < 4; r++)
#pragma unroll
		for (int cb = 0; cb < NB; cb++) out[(size_t)(4 * r) * b + 16 * cb] = acc[cb][r];
}

/* Y [I][b] = the slabs of partial [n_slabs][Ipad][b] added in index order, divided by L' */
__global__ __launch_bounds__(256) void k_pca_fold(const double *__restrict__ partial, int n_slabs, size_t slab /* Ipad b */, size_t n /* I b */,
						  int n_used, double *__restrict__ Y)
{
	for (size_t x = (size_t)blockIdx.x * 256 + threadIdx.x; x < n; x += (size_t)gridDim.x * 256) {
		double s = partial[x];
		for (int k = 1; k < n_slabs; k++) s += partial[(size_t)k * slab + x];
		Y[x] = s / (double)n_used;
	}
}

/* what both entry points hold on the device from the first launch to the last */
struct pca_device {
	int I = 0, L = 0, b = 0, Ipad = 0, n_slabs = 0, n_used = 0;
	size_t rb = 0;
	double trace = 0.0;
	scoped_dev<uint8_t> bed;
	scoped_dev<int32_t> used;
	scoped_dev<double> tab, scale, t, X, W, Y, partial;
};

/* The records go up, the buffers are allocated, k_pca_scale runs, and L' and the trace are summed in index order.  b = the padded
 * column count.  `who` names the entry point in the messages. */
static int pca_prepare(mchip_context *ctx, pca_device &d, int I, int L, const uint8_t *bed, size_t rb, int b, const char *who)
{
	if (I > 0x7FFFFFFF - PCA_ITILE || ((long long)L + PCA_LSLAB - 1) / PCA_LSLAB > 65535)
		return fail(ctx, MCHIP_ERR_UNSUPPORTED, "%s: too many individuals, or more than 65535 slabs of variants, for one launch", who);
	const pca_geometry g = pca_geometry_of(I, L);
	d.I = I; d.L = L; d.b = b; d.rb = rb;
	d.Ipad = g.Ipad;
	d.n_slabs = g.n_slabs;
	HIPCHK(hipSetDevice(ctx->device));
	const hipError_t uploaded = bed_upload(ctx, d.bed, bed, (size_t)L * rb);
	if (!d.bed.p || d.tab.alloc(4 * (size_t)L) != hipSuccess || d.scale.alloc(2 * (size_t)L) != hipSuccess || d.t.alloc((size_t)L) != hipSuccess ||
	    d.used.alloc((size_t)L) != hipSuccess || d.X.alloc((size_t)I * b) != hipSuccess || d.W.alloc((size_t)L * b) != hipSuccess ||
	    d.Y.alloc((size_t)I * b) != hipSuccess || d.partial.alloc((size_t)d.n_slabs * d.Ipad * b) != hipSuccess) {
		(void)hipGetLastError();
		return fail(ctx, MCHIP_ERR_ALLOC, "%s: the records, the tables, the vectors or the slabs' partial sums do not fit on the device", who);
	}
	HIPCHK(uploaded);
	hipLaunchKernelGGL(k_pca_scale, dim3(nblk((size_t)L, 4)), dim3(256), 0, ctx->stream, d.bed.p, rb, I, L, d.tab.p, d.scale.p, d.t.p, d.used.p);
	HIPCHK(hipGetLastError());
	std::vector<double> t((size_t)L);
	std::vector<int32_t> used((size_t)L);
	HIPCHK(hipMemcpyAsync(t.data(), d.t.p, sizeof(double) * (size_t)L, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipMemcpyAsync(used.data(), d.used.p, sizeof(int32_t) * (size_t)L, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	double sum = 0.0;
	int n_used = 0;
	for (int l = 0; l < L; l++) { sum += t[(size_t)l]; n_used += used[(size_t)l]; }
	if (!n_used) return fail(ctx, MCHIP_ERR_INVALID, "%s: no polymorphic variant: every variant is monomorphic or without a call", who);
	d.n_used = n_used;
	d.trace = sum / (double)n_used;
	HIPCHK(hipMemsetAsync(d.X.p, 0, sizeof(double) * (size_t)I * b, ctx->stream));	/* the padding columns of X */
	return MCHIP_OK;
}

template <int NB> static void pca_launch(mchip_context *ctx, pca_device &d)
{
	const size_t lds = sizeof(double) * 64 * (size_t)pca_pitch(16 * NB);
	hipLaunchKernelGGL(k_pca_project<NB>, dim3(nblk((size_t)d.L, PCA_VARIANTS)), dim3(256), lds, ctx->stream, d.bed.p, d.rb, d.I, d.L, d.tab.p, d.X.p,
			   d.W.p);
	hipLaunchKernelGGL(k_pca_expand<NB>, dim3((unsigned)(d.Ipad / PCA_ITILE), (unsigned)d.n_slabs), dim3(256), lds, ctx->stream, d.bed.p, d.rb, d.L,
			   d.Ipad, d.tab.p, d.W.p, d.partial.p);
}

/* Y = Z (Z^T X) / L' on the device, W left in place */
static int pca_multiply(mchip_context *ctx, pca_device &d)
{
	switch (d.b / 16) {
	case 1: pca_launch<1>(ctx, d); break;
	case 2: pca_launch<2>(ctx, d); break;
	case 3: pca_launch<3>(ctx, d); break;
	default: pca_launch<4>(ctx, d); break;
	}
	HIPCHK(hipGetLastError());
	const size_t n = (size_t)d.I * d.b;
	hipLaunchKernelGGL(k_pca_fold, dim3(nblk_capped(n)), dim3(256), 0, ctx->stream, d.partial.p, d.n_slabs, (size_t)d.Ipad * d.b, n, d.n_used, d.Y.p);
	HIPCHK(hipGetLastError());
	return MCHIP_OK;
}

/* n columns of a host matrix [rows][n] <-> the first n columns of a device matrix [rows][b] */
static hipError_t pca_columns_up(mchip_context *ctx, double *dev, int b, const double *host, int n, int rows)
{
	return hipMemcpy2DAsync(dev, sizeof(double) * (size_t)b, host, sizeof(double) * (size_t)n, sizeof(double) * (size_t)n, (size_t)rows,
				hipMemcpyHostToDevice, ctx->stream);
}
static hipError_t pca_columns_down(mchip_context *ctx, double *host, int n, const double *dev, int b, int rows)
{
	return hipMemcpy2DAsync(host, sizeof(double) * (size_t)n, dev, sizeof(double) * (size_t)b, sizeof(double) * (size_t)n, (size_t)rows,
				hipMemcpyDeviceToHost, ctx->stream);
}

extern "C" int mchip_bed_pca_apply(mchip_context *ctx, int I, int L, const uint8_t *bed, size_t record_bytes, int n_vec, const double *x, double *y,
				   double *w, double *scale, int *n_used, double *trace)
{
	MCHIP_ENTRY();
	if (!ctx) return MCHIP_ERR_INVALID;
	if (!bed_shape_ok(I, L, bed, record_bytes) || !x || !y || !n_used)
		return fail(ctx, MCHIP_ERR_INVALID, "bed_pca_apply: bad shape, null pointer or records shorter than ceil(I/4) bytes%s", nullptr);
	if (n_vec < 1 || n_vec > MCHIP_PCA_MAX_VECTORS)
		return fail(ctx, MCHIP_ERR_INVALID, "bed_pca_apply: the number of vectors lies outside 1 ... 64%s", nullptr);
	pca_device d;
	const int b = (n_vec + 15) / 16 * 16;
	int rc = pca_prepare(ctx, d, I, L, bed, record_bytes, b, "bed_pca_apply");
	if (rc) return rc;
	HIPCHK(pca_columns_up(ctx, d.X.p, b, x, n_vec, I));
	if ((rc = pca_multiply(ctx, d))) return rc;
	HIPCHK(hipStreamSynchronize(ctx->stream));
	/* the caller's arrays are written once everything on the device has succeeded */
	HIPCHK(pca_columns_down(ctx, y, n_vec, d.Y.p, b, I));
	if (w) HIPCHK(pca_columns_down(ctx, w, n_vec, d.W.p, b, L));
	if (scale) HIPCHK(hipMemcpyAsync(scale, d.scale.p, sizeof(double) * 2 * (size_t)L, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	*n_used = d.n_used;
	if (trace) *trace = d.trace;
	return MCHIP_OK;
}

extern "C" int mchip_bed_pca(mchip_context *ctx, int I, int L, const uint8_t *bed, size_t record_bytes, int n_pc, int n_extra, int max_iter, double tol,
			     double *eigenvalues, double *eigenvectors, double *residuals, double *trace, int *n_used, int *n_iter)
{
	MCHIP_ENTRY();
	if (!ctx) return MCHIP_ERR_INVALID;
	if (!bed_shape_ok(I, L, bed, record_bytes) || !eigenvalues || !eigenvectors || !residuals || !trace || !n_used || !n_iter)
		return fail(ctx, MCHIP_ERR_INVALID, "bed_pca: bad shape, null pointer or records shorter than ceil(I/4) bytes%s", nullptr);
	if (n_pc < 1 || n_extra < 0 || (long long)n_pc + n_extra > MCHIP_PCA_MAX_VECTORS || n_pc > I || max_iter < 1 || !(tol > 0.0 && tol < 1.0))
		return fail(ctx, MCHIP_ERR_INVALID, "bed_pca: components outside 1 ... min(I, 64 - extra vectors), no iteration allowed or a tolerance outside (0, 1)%s",
			    nullptr);
	const int b = pca_block_width(I, n_pc, n_extra), bdev = (b + 15) / 16 * 16;
	pca_device d;
	int rc = pca_prepare(ctx, d, I, L, bed, record_bytes, bdev, "bed_pca");
	if (rc) return rc;
	std::vector<double> val((size_t)n_pc), vec((size_t)I * n_pc), res((size_t)n_pc);
	int it = 0;
	/* only the I x b blocks cross, once each way an iteration: the records, the tables, W and the partial sums stay where they are */
	rc = pca_subspace_iteration(I, b, n_pc, max_iter, tol, [&](const double *X, double *Y) -> int {
		HIPCHK(pca_columns_up(ctx, d.X.p, bdev, X, b, I));
		const int mrc = pca_multiply(ctx, d);
		if (mrc) return mrc;
		HIPCHK(pca_columns_down(ctx, Y, b, d.Y.p, bdev, I));
		HIPCHK(hipStreamSynchronize(ctx->stream));
		return MCHIP_OK;
	}, val.data(), vec.data(), res.data(), &it);
	if (rc) return rc;
	memcpy(eigenvalues, val.data(), sizeof(double) * (size_t)n_pc);
	memcpy(eigenvectors, vec.data(), sizeof(double) * (size_t)I * n_pc);
	memcpy(residuals, res.data(), sizeof(double) * (size_t)n_pc);
	*trace = d.trace;
	*n_used = d.n_used;
	*n_iter = it;
	return MCHIP_OK;
}
