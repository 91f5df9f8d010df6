/*
 * mchip_bed.hip -- PLINK 1 .bed records (2 bits per genotype, variant-major) unpacked on the device: mchip_set_genotypes_bed
 * and its kernels (include/multiclust_hip.h has the format and the contract; mchip_context.h the context and the install path).
 *
 * Two passes over the packed records, I * L / 4 bytes each:
 *   k_bed_locus   one wave per locus: which of A1, A2 and "missing" occur among the I samples of the record -> uniquealleles[l]
 *                 as the STRUCTURE reader counts it and whether A1 is observed (the recoding of a locus depends on nothing else:
 *                 homozygous A1 -> 0 0, heterozygous -> 0 1, missing -> FF FF, homozygous A2 -> 1 1 when A1 is observed, else 0 0);
 *   k_bed_expand  one workgroup per tile of 64 loci x 256 individuals (4 KB of packed bytes staged in LDS): writes the tile's part
 *                 of gtA [ceil(I/8)][L][8][2] and of gtS [ceil(L/8)][I][8][2] as whole 16-byte groups, 1 KB contiguous per wave on
 *                 either side, and marks the individuals that have an observed call.
 * The upload form [I][L][2] never exists.
 */
#include "mchip_context.h"

constexpr int BED_PAD = 8;	/* bytes allocated behind the last record: records are read as dwords from any byte offset */
constexpr int BT_L = 64;	/* loci per tile */
constexpr int BT_I = 256;	/* individuals per tile: 64 staged bytes of each record */
constexpr int BT_ROW = 17;	/* dwords between staged records: 16 of data and one of padding, so that the 64 lanes that read the
				 * same byte pair of 64 consecutive records (gtA side) fall on 64 different banks */

/* four packed bytes from any byte offset of the buffer: records are record_bytes apart, whatever that is modulo 4.  Two aligned
 * loads; the second may reach BED_PAD - 1 bytes behind the last record */
__device__ __forceinline__ uint32_t bed_word(const uint8_t *__restrict__ bed, size_t off)
{
	const uint32_t *w = reinterpret_cast<const uint32_t *>(bed + (off & ~(size_t)3));
	const unsigned sh = 8u * (unsigned)(off & 3);
	const uint32_t lo = w[0];
	return sh ? (lo >> sh) | (w[1] << (32u - sh)) : lo;
}

/* locus pass: ua[l] as the STRUCTURE reader counts it, a1[l] = 1 when allele A1 is observed at locus l (the one thing the recoding
 * of a locus depends on), bit 1 of *flags set when any call is missing */
__global__ __launch_bounds__(256) void k_bed_locus(const uint8_t *__restrict__ bed, size_t rb, int I, int L, int32_t *__restrict__ ua,
						   uint8_t *__restrict__ a1_out, int *flags)
{
	const int lane = threadIdx.x & 63, l = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (l >= L) return;	/* (a whole wave) */
	const int nwords = (I + 15) / 16;
	uint32_t a1 = 0, a2 = 0, ms = 0;
	for (int w = lane; w < nwords; w += 64) {
		const uint32_t v = bed_word(bed, (size_t)l * rb + 4 * (size_t)w);
		const int n = I - 16 * w;	/* samples in this word: bits behind them are padding, or the next record */
		const uint32_t valid = n >= 16 ? 0x55555555u : (((1u << (2 * n)) - 1u) & 0x55555555u);
		const uint32_t lo = v & valid, hi = (v >> 1) & valid;
		a1 |= ~lo & valid;	/* codes 0 and 2 carry A1 */
		a2 |= hi;		/* codes 2 and 3 carry A2 */
		ms |= lo & ~hi;		/* code 1 */
	}
	const int A1 = __ballot(a1 != 0) != 0, A2 = __ballot(a2 != 0) != 0, MS = __ballot(ms != 0) != 0;
	if (lane == 0) {
		const int nu = A1 + A2;
		ua[l] = nu ? nu + MS : 0;	/* no observed call: the reader leaves the locus without allele columns */
		a1_out[l] = (uint8_t)A1;
		if (MS) atomicOr(flags, 2);
	}
}

/* the byte pairs of the four codes, 16 bits each, code 0 lowest */
__device__ __forceinline__ uint64_t bed_pairs(uint32_t hom2)
{
	return 0xFFFF0000ull | (0x0100ull << 32) | ((uint64_t)hom2 << 48);
}

/* expand pass: gtA and gtS of the ploidy-2 data set, padded with 0xFF like k_relayout's; seen[i] (zeroed by the caller) = 1 for
 * every individual with an observed call */
__global__ __launch_bounds__(256) void k_bed_expand(const uint8_t *__restrict__ bed, size_t rb, int I, int L, const uint8_t *__restrict__ a1,
						    uint8_t *__restrict__ gtA, uint8_t *__restrict__ gtS, uint8_t *seen, int n_ltiles)
{
	__shared__ __attribute__((aligned(16))) uint32_t tile[BT_L * BT_ROW];
	__shared__ uint32_t hom2[BT_L];		/* byte pair of a homozygous A2 call of the locus */
	const int l0 = (blockIdx.x % n_ltiles) * BT_L, i0 = (blockIdx.x / n_ltiles) * BT_I;
	const size_t b0 = (size_t)(i0 / 4);	/* first staged byte of every record */
	for (int x = threadIdx.x; x < BT_L * 16; x += 256) {
		const int ll = x / 16, w = x % 16, l = l0 + ll;
		const size_t off = b0 + 4 * (size_t)w;
		tile[ll * BT_ROW + w] = (l < L && off < rb) ? bed_word(bed, (size_t)l * rb + off) : 0u;
	}
	if (threadIdx.x < BT_L) hom2[threadIdx.x] = (l0 + (int)threadIdx.x < L && a1[l0 + threadIdx.x]) ? 0x0101u : 0u;
	__syncthreads();
	const uint8_t *tb = reinterpret_cast<const uint8_t *>(tile);
	/* gtA: a thread owns (block of 8 individuals, locus) = 16 staged bits; consecutive threads take consecutive loci */
	for (int x = threadIdx.x; x < (BT_I / 8) * BT_L; x += 256) {
		const int ll = x % BT_L, ibl = x / BT_L, l = l0 + ll, ifirst = i0 + ibl * 8;
		if (l >= L || ifirst >= I) continue;
		const uint32_t bits = *reinterpret_cast<const uint16_t *>(tb + ll * (BT_ROW * 4) + ibl * 2);
		const uint64_t pairs = bed_pairs(hom2[ll]);
		uint32_t out[4] = { 0, 0, 0, 0 };
#pragma unroll
		for (int j = 0; j < 8; j++) {
			const uint32_t c = (bits >> (2 * j)) & 3u;
			const uint32_t pr = ifirst + j < I ? (uint32_t)(pairs >> (16 * c)) & 0xFFFFu : 0xFFFFu;
			out[j / 2] |= pr << (16 * (j & 1));
		}
		*reinterpret_cast<uint4 *>(gtA + ((size_t)(ifirst / 8) * L + l) * 16) = make_uint4(out[0], out[1], out[2], out[3]);
	}
	/* gtS: a thread owns (block of 8 loci, individual); consecutive threads take consecutive individuals, and a thread stays with
	 * its individual through the eight locus blocks of the tile */
	bool any = false;
	for (int x = threadIdx.x; x < (BT_L / 8) * BT_I; x += 256) {
		const int r = x % BT_I, lbl = x / BT_I, i = i0 + r, lfirst = l0 + lbl * 8;
		if (i >= I || lfirst >= L) continue;
		uint32_t out[4] = { 0, 0, 0, 0 };
#pragma unroll
		for (int j = 0; j < 8; j++) {
			const int ll = lbl * 8 + j;
			const uint32_t c = ((uint32_t)tb[ll * (BT_ROW * 4) + r / 4] >> (2 * (r & 3))) & 3u;
			const bool in = lfirst + j < L;
			const uint32_t pr = in ? (uint32_t)(bed_pairs(hom2[ll]) >> (16 * c)) & 0xFFFFu : 0xFFFFu;
			any |= in && c != 1u;
			out[j / 2] |= pr << (16 * (j & 1));
		}
		*reinterpret_cast<uint4 *>(gtS + ((size_t)(lfirst / 8) * I + i) * 16) = make_uint4(out[0], out[1], out[2], out[3]);
	}
	if (any) seen[i0 + threadIdx.x] = 1;	/* (every writer stores the same value) */
}

/* The packed records go up as they are; the locus pass tells the host the allele counts set_shape sizes the column tables from,
 * the expand pass fills gtA / gtS.  No stream buffer (d_draw) and no k_relayout on this route. */
extern "C" int mchip_set_genotypes_bed(mchip_context *ctx, int I, int L, const uint8_t *bed, size_t record_bytes, int32_t *uniquealleles_out)
{
	MCHIP_ENTRY();
	if (!ctx) return MCHIP_ERR_INVALID;
	if (I <= 0 || L <= 0 || !bed || record_bytes < ((size_t)I + 3) / 4)
		return fail(ctx, MCHIP_ERR_INVALID, "set_genotypes_bed: bad shape, null pointer or records shorter than ceil(I/4) bytes%s", nullptr);
	HIPCHK(hipSetDevice(ctx->device));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	const size_t bed_bytes = (size_t)L * record_bytes;
	scoped_dev<uint8_t> d_bed, d_a1, d_seen;
	scoped_dev<int32_t> d_ua;
	HIPCHK(d_bed.alloc(bed_bytes + BED_PAD));
	HIPCHK(d_a1.alloc((size_t)L));
	HIPCHK(d_seen.alloc((size_t)I));
	HIPCHK(d_ua.alloc((size_t)L));
	int *d_bad = bad_flag(ctx);
	HIPCHK(hipMemcpyAsync(d_bed.p, bed, bed_bytes, hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(hipMemsetAsync(d_bed.p + bed_bytes, 0, BED_PAD, ctx->stream));
	HIPCHK(hipMemsetAsync(d_seen.p, 0, (size_t)I, ctx->stream));
	HIPCHK(hipMemsetAsync(d_bad, 0, sizeof(int), ctx->stream));
	hipLaunchKernelGGL(k_bed_locus, dim3((unsigned)((L + 3) / 4)), dim3(256), 0, ctx->stream, d_bed.p, record_bytes, I, L, d_ua.p, d_a1.p, d_bad);
	HIPCHK(hipGetLastError());
	std::vector<int32_t> ua((size_t)L);
	int bad = 0;
	HIPCHK(hipMemcpyAsync(ua.data(), d_ua.p, sizeof(int32_t) * (size_t)L, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	if (uniquealleles_out) memcpy(uniquealleles_out, ua.data(), sizeof(int32_t) * (size_t)L);
	int rc = set_shape(ctx, I, L, 2, ua.data());
	if (rc) return rc;
	const int n_ltiles = (L + BT_L - 1) / BT_L, n_itiles = (I + BT_I - 1) / BT_I;
	const size_t blocks = (size_t)n_ltiles * n_itiles;
	if (blocks >= ((size_t)1 << 31)) {
		free_data(ctx);
		return fail(ctx, MCHIP_ERR_UNSUPPORTED, "data set too large for the layout kernel%s", nullptr);
	}
	hipLaunchKernelGGL(k_bed_expand, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, d_bed.p, record_bytes, I, L, d_a1.p, ctx->d_gtA,
			   ctx->d_gtS, d_seen.p, n_ltiles);
	HIPCHK(hipGetLastError());
	std::vector<uint8_t> seen((size_t)I);
	HIPCHK(hipMemcpyAsync(seen.data(), d_seen.p, (size_t)I, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	set_empty_rows_unseen(ctx, seen);
	return install_layouts(ctx, (bad & 2) ? 1 : 0);
}
