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
 *
 * mchip_bed_ld_band reads the same records for another purpose and installs nothing: the band of r^2 between every variant and
 * its `window` successors (the definition is in the header), L * window * I / 32 word pairs.
 *   k_ld_band     one workgroup per LD_TILE first variants x LD_DCHUNK offsets x a run of individuals (ld_band_geometry_of,
 *                 mchip_feature_geometry.h).  Per stage of LD_STAGE 64-bit words (32 individuals each) it forms three bit planes of
 *                 its LD_TILE first and LD_TILE + LD_DCHUNK - 1 second records in LDS (15 KB): valid, dosage 1, dosage 2.  A lane
 *                 owns one first variant and LD_DCHUNK / 4 offsets and counts with __popcll into 6 integer registers per pair; the
 *                 64 lanes of a wave read 64 consecutive words of a plane (no bank conflict).  At the end the six sums of a pair
 *                 go to memory with integer atomics: runs of individuals combine in any order, the sums are the same.
 *   k_ld_r2       one lane per pair: the six sums -> C, Vx, Vy in 64-bit integers -> r2, NaN where a variance is 0 or the second
 *                 variant does not exist.
 *   Compile report (hipcc of ROCm 7.2, gfx950, -O3, -Rpass-analysis=kernel-resource-usage):  k_ld_band 81 VGPRs, scratch 0, 15360
 *   bytes of static LDS, 5 waves / SIMD (the loop over a stage's words is kept rolled: unrolled it takes 135 VGPRs and 3 waves);
 *   k_ld_r2 25 VGPRs, scratch 0, 8 waves / SIMD.  Timed once and not tuned (profiles/ld.txt, scripts/ld_bench.py).
 *
 * mchip_bed_king reads the records for a third purpose and installs nothing either: the KING-robust kinship of a slab of individuals
 * with all individuals (the definition is in the header), n_rows * I * ceil(L / 64) word pairs.
 *   k_king_planes the records turned round: per individual three bit planes over the variants (valid, heterozygous, homozygous A2),
 *                 64 variants to a 64-bit word, [plane][word][Ipad] with the individuals contiguous.  One workgroup per word x 256
 *                 individuals, the record bytes staged as k_bed_expand stages them; a wave-wide __ballot over 64 variants' codes of
 *                 one individual is one plane word.
 *   k_king_pairs  one workgroup per KING_TILE x KING_TILE individuals x a run of words (king_geometry_of, mchip_feature_geometry.h).
 *                 Per stage of KING_STAGE words it holds four planes (hom A1 = valid & ~het & ~hom A2 formed on the way in) of its
 *                 row and column individuals in LDS (16 KB); a lane owns 4 x 4 pairs and counts with five __popcll per pair and
 *                 word into 80 integer registers -- n, hh, op, h_ij, and h_ji from the same pass.  At the end the five counts of a
 *                 pair go to memory with integer atomics: runs of variants combine in any order, the counts are the same.
 *   k_king_phi    one lane per pair: the counts -> m, num in 64-bit integers -> phi, NaN where m = 0.
 *   Compile report (same compiler and flags):  k_king_planes 33 VGPRs, scratch 0, 4352 bytes of static LDS, 8 waves / SIMD;
 *   k_king_pairs 153 VGPRs, scratch 0, 16384 bytes of static LDS, 3 waves / SIMD; k_king_phi 24 VGPRs, scratch 0, 8 waves / SIMD.
 *   Timed once and not tuned (profiles/king.txt, scripts/king_bench.py).
 *
 * mchip_bed_qc reads the records for a fourth purpose and installs nothing either: the four genotype counts of every individual and
 * of every variant (over the individuals a keep mask names) and the Hardy-Weinberg exact test of every variant (the definition is in
 * the header): what --mind, --geno, --maf and --hwe filter by.
 *   k_qc_mask        the keep bytes expanded once to bit 2 j of word j / 32 for every kept individual j < I: the padding is cleared here.
 *   k_qc_variants    a wave per variant, QC_VARIANTS to a workgroup, x a run of individuals (qc_geometry_of,
 *                    mchip_feature_geometry.h): a lane reads its record as 64-bit words, 64 consecutive ones a wave, forms the two
 *                    bit planes of the word under the mask and takes four population counts; the wave's sums go to memory with
 *                    integer atomics.
 *   k_qc_individuals the transposed direction in k_king_planes' pattern: a workgroup per QC_ITILE individuals x a run of 64-variant
 *                    words, the record bytes staged as k_bed_expand stages them; a wave-wide __ballot over 64 variants' codes of
 *                    one individual is that individual's word of a code's plane, and its population count stays in a register of
 *                    the individual's lane: no plane is stored.  At the end integer atomics.
 *   k_qc_hwe         a lane per variant, FP64: the walk of the definition twice, nothing staged in memory; lanes of a wave differ
 *                    in their trip counts, so the workgroups are single waves.
 */
#include "mchip_context.h"

constexpr long long QUIET_NAN_BITS = 0x7FF8000000000000ll;	/* the NaN of a pair without a value (k_ld_r2, k_king_phi) */

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
	bed_stage_tile(tile, bed, rb, L, l0, i0);
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
	if (!bed_shape_ok(I, L, bed, record_bytes))
		return fail(ctx, MCHIP_ERR_INVALID, "set_genotypes_bed: bad shape, null pointer or records shorter than ceil(I/4) bytes%s", nullptr);
	HIPCHK(hipSetDevice(ctx->device));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	scoped_dev<uint8_t> d_bed, d_a1, d_seen;
	scoped_dev<int32_t> d_ua;
	HIPCHK(bed_upload(ctx, d_bed, bed, (size_t)L * record_bytes));
	HIPCHK(d_a1.alloc((size_t)L));
	HIPCHK(d_seen.alloc((size_t)I));
	HIPCHK(d_ua.alloc((size_t)L));
	int *d_bad = bad_flag(ctx);
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

/* ---- linkage disequilibrium between neighbouring variants: mchip_bed_ld_band (include/multiclust_hip.h has the definition) ---- */
constexpr int LD_YROWS = LD_TILE + LD_DCHUNK - 1;	/* second variants a workgroup meets */
constexpr int LD_PER_LANE = LD_DCHUNK / 4;		/* offsets of a lane: wave q of the four takes offsets q * LD_PER_LANE ... */

/* the three bit planes of word wg (individuals 32 wg ... 32 wg + 31, bit 2 j for the j-th of them) of the record at rec:
 * valid = not missing, b0 = dosage 1 (code 2), b1 = dosage 2 (code 3); bits behind individual I - 1 are 0 in all three */
__device__ __forceinline__ void ld_planes(const uint8_t *__restrict__ bed, size_t rb, int I, size_t rec, int wg, uint64_t &valid, uint64_t &b0,
					  uint64_t &b1)
{
	const size_t off = 8 * (size_t)wg;
	const int n = I - 32 * wg;	/* samples in this word: bits behind them are padding, or the next record */
	valid = b0 = b1 = 0;
	if (n <= 0 || off >= rb) return;
	uint64_t v = bed_word(bed, rec * rb + off);
	if (off + 4 < rb) v |= (uint64_t)bed_word(bed, rec * rb + off + 4) << 32;
	const uint64_t low = 0x5555555555555555ull;
	const uint64_t m = n >= 32 ? low : (((1ull << (2 * n)) - 1ull) & low);
	const uint64_t lo = v & m, hi = (v >> 1) & m;
	valid = m & ~(lo & ~hi);	/* code 1 is the missing call */
	b0 = hi & ~lo;
	b1 = hi & lo;
}

/* sums[(a * window + d - 1) * 6 + 0..5] += n, Sx, Sy, Sxx, Syy, Sxy of the pair (a, a + d) over this workgroup's run of
 * individuals; rows count from the first uploaded record.  blockIdx.x = tile of first variants + n_tiles * chunk of offsets,
 * blockIdx.y = run of individuals.  Lane = first variant ax of the tile, wave q = offsets q * LD_PER_LANE + 1 ... of the chunk: the
 * 64 lanes of a wave read 64 consecutive words of a plane.  With c1 / c2 the carriers of dosage 1 / 2 among the individuals typed
 * at both variants, Sx = c1x + 2 c2x and Sxx = c1x + 4 c2x; b0 and b1 are 0 where the call is missing, so the products of Sxy need
 * no mask. */
__global__ __launch_bounds__(256) void k_ld_band(const uint8_t *__restrict__ bed, size_t rb, int I, int n_up, int n_first, int window,
						 ld_band_geometry g, uint32_t *__restrict__ sums)
{
	__shared__ uint64_t xs[3][LD_STAGE][LD_TILE];
	__shared__ uint64_t ys[3][LD_STAGE][LD_YROWS + 1];
	const int tile = blockIdx.x % g.n_tiles, dch = blockIdx.x / g.n_tiles;
	const int a0 = tile * LD_TILE, y0 = a0 + dch * LD_DCHUNK + 1;
	if (y0 >= n_up) return;		/* (the whole workgroup) no pair of this tile and chunk lies inside the records */
	const int nwords = (I + 31) / 32;
	const int w_begin = (int)blockIdx.y * g.stages_per_split * LD_STAGE;
	const int w_end = min(nwords, w_begin + g.stages_per_split * LD_STAGE);
	const int ax = threadIdx.x & 63, q = threadIdx.x >> 6;
	uint32_t acc[LD_PER_LANE][6];
#pragma unroll
	for (int j = 0; j < LD_PER_LANE; j++)
#pragma unroll
		for (int s = 0; s < 6; s++) acc[j][s] = 0;
	for (int ws = w_begin; ws < w_end; ws += LD_STAGE) {
		__syncthreads();	/* the stage before has been read */
		for (int x = threadIdx.x; x < (LD_TILE + LD_YROWS) * LD_STAGE; x += 256) {
			const int row = x / LD_STAGE, w = x % LD_STAGE;
			const bool first = row < LD_TILE;
			const int r = first ? a0 + row : y0 + row - LD_TILE;
			uint64_t v = 0, b0 = 0, b1 = 0;
			if (r < n_up && ws + w < w_end) ld_planes(bed, rb, I, (size_t)r, ws + w, v, b0, b1);
			if (first) { xs[0][w][row] = v; xs[1][w][row] = b0; xs[2][w][row] = b1; }
			else { ys[0][w][row - LD_TILE] = v; ys[1][w][row - LD_TILE] = b0; ys[2][w][row - LD_TILE] = b1; }
		}
		__syncthreads();
#pragma unroll 1
		for (int w = 0; w < LD_STAGE; w++) {	/* (words behind w_end are staged as zeros) */
			const uint64_t vx = xs[0][w][ax], b0x = xs[1][w][ax], b1x = xs[2][w][ax];
#pragma unroll
			for (int j = 0; j < LD_PER_LANE; j++) {
				const int yr = ax + q * LD_PER_LANE + j;	/* < LD_YROWS */
				const uint64_t vy = ys[0][w][yr], b0y = ys[1][w][yr], b1y = ys[2][w][yr];
				acc[j][0] += (uint32_t)__popcll(vx & vy);
				acc[j][1] += (uint32_t)__popcll(b0x & vy);
				acc[j][2] += (uint32_t)__popcll(b1x & vy);
				acc[j][3] += (uint32_t)__popcll(b0y & vx);
				acc[j][4] += (uint32_t)__popcll(b1y & vx);
				acc[j][5] += (uint32_t)__popcll(b0x & b0y) + 2u * (uint32_t)(__popcll(b0x & b1y) + __popcll(b1x & b0y)) +
					     4u * (uint32_t)__popcll(b1x & b1y);
			}
		}
	}
	const int a = a0 + ax;
	if (a >= n_first) return;
#pragma unroll
	for (int j = 0; j < LD_PER_LANE; j++) {
		const int d = dch * LD_DCHUNK + q * LD_PER_LANE + j + 1;
		if (d > window || a + d >= n_up) continue;
		uint32_t *s = sums + ((size_t)a * (size_t)window + (size_t)(d - 1)) * 6;
		atomicAdd(s + 0, acc[j][0]);
		atomicAdd(s + 1, acc[j][1] + 2u * acc[j][2]);
		atomicAdd(s + 2, acc[j][3] + 2u * acc[j][4]);
		atomicAdd(s + 3, acc[j][1] + 4u * acc[j][2]);
		atomicAdd(s + 4, acc[j][3] + 4u * acc[j][4]);
		atomicAdd(s + 5, acc[j][5]);
	}
}

/* r2 of every pair from its six sums, in exact 64-bit integers up to the two products and the division of the definition; NaN where
 * either variance is 0 and where the second variant lies behind the last record */
__global__ __launch_bounds__(256) void k_ld_r2(const uint32_t *__restrict__ sums, size_t n_pairs, int window, int n_up, double *__restrict__ r2)
{
	for (size_t x = (size_t)blockIdx.x * 256 + threadIdx.x; x < n_pairs; x += (size_t)gridDim.x * 256) {
		const size_t a = x / (size_t)window, d = x % (size_t)window + 1;
		double out = __longlong_as_double(QUIET_NAN_BITS);
		if (a + d < (size_t)n_up) {
			const uint32_t *s = sums + x * 6;
			const int64_t n = s[0], Sx = s[1], Sy = s[2], Sxx = s[3], Syy = s[4], Sxy = s[5];
			const int64_t C = n * Sxy - Sx * Sy, Vx = n * Sxx - Sx * Sx, Vy = n * Syy - Sy * Sy;
			if (Vx != 0 && Vy != 0) out = ((double)C * (double)C) / ((double)Vx * (double)Vy);
		}
		r2[x] = out;
	}
}

extern "C" int mchip_bed_ld_band(mchip_context *ctx, int I, int L, const uint8_t *bed, size_t record_bytes, int l0, int n_first, int window,
				 double *r2)
{
	MCHIP_ENTRY();
	if (!ctx) return MCHIP_ERR_INVALID;
	if (!bed_shape_ok(I, L, bed, record_bytes) || !r2)
		return fail(ctx, MCHIP_ERR_INVALID, "bed_ld_band: bad shape, null pointer or records shorter than ceil(I/4) bytes%s", nullptr);
	if (l0 < 0 || n_first < 0 || (long long)l0 + n_first > L || window < 1 || window > MCHIP_LD_MAX_WINDOW)
		return fail(ctx, MCHIP_ERR_INVALID, "bed_ld_band: first variants outside the records, or a window outside 1 ... 4096%s", nullptr);
	if (!n_first) return MCHIP_OK;
	const long long reach = (long long)n_first + window;
	const int n_up = (int)((long long)(L - l0) < reach ? (long long)(L - l0) : reach);	/* records that cross: rows count from l0 */
	const ld_band_geometry g = ld_band_geometry_of(I, n_first, window, (long long)ctx->knob.per_cu_ind * (ctx->n_cu > 0 ? ctx->n_cu : 256));
	if ((long long)g.n_tiles * g.n_dchunks >= (1ll << 24))
		return fail(ctx, MCHIP_ERR_UNSUPPORTED, "bed_ld_band: too many first variants times offsets for one launch; call it in slabs%s", nullptr);
	HIPCHK(hipSetDevice(ctx->device));
	const size_t up_bytes = (size_t)n_up * record_bytes, n_pairs = (size_t)n_first * (size_t)window;
	scoped_dev<uint8_t> d_bed;
	scoped_dev<uint32_t> d_sums;
	scoped_dev<double> d_r2;
	const hipError_t uploaded = bed_upload(ctx, d_bed, bed + (size_t)l0 * record_bytes, up_bytes);
	if (!d_bed.p || d_sums.alloc(n_pairs * 6) != hipSuccess || d_r2.alloc(n_pairs) != hipSuccess) {
		(void)hipGetLastError();
		return fail(ctx, MCHIP_ERR_ALLOC, "bed_ld_band: the records, the sums or the band do not fit on the device%s", nullptr);
	}
	HIPCHK(uploaded);
	HIPCHK(hipMemsetAsync(d_sums.p, 0, n_pairs * 6 * sizeof(uint32_t), ctx->stream));
	hipLaunchKernelGGL(k_ld_band, dim3((unsigned)(g.n_tiles * g.n_dchunks), (unsigned)g.n_split), dim3(256), 0, ctx->stream, d_bed.p, record_bytes,
			   I, n_up, n_first, window, g, d_sums.p);
	HIPCHK(hipGetLastError());
	hipLaunchKernelGGL(k_ld_r2, dim3(nblk_capped(n_pairs)), dim3(256), 0, ctx->stream, d_sums.p, n_pairs, window, n_up, d_r2.p);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(r2, d_r2.p, sizeof(double) * n_pairs, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	return MCHIP_OK;
}

/* ---- KING-robust kinship between the individuals: mchip_bed_king (include/multiclust_hip.h has the definition) ---- */
constexpr int KING_PER = KING_TILE / 16;	/* row individuals and column individuals of a lane: KING_PER x KING_PER pairs */

/* the records turned round: planes[(p * n_words + w) * Ipad + i] = plane p (0 valid, 1 heterozygous, 2 homozygous A2) of individual i
 * over the variants 64 w ... 64 w + 63, bit v for variant 64 w + v; bits behind variant L - 1 and the rows I ... Ipad - 1 are 0.  One
 * workgroup per word x BT_I individuals: the 64 bytes of each of its 64 records staged as in k_bed_expand (a lane then reads its
 * record's byte, BT_ROW dwords apart: 64 different banks); lane = variant, a wave walks its 64 individuals and a ballot over the
 * lanes' codes of one individual is that individual's word; lane k keeps the k-th, so the stores run along the individuals. */
__global__ __launch_bounds__(256) void k_king_planes(const uint8_t *__restrict__ bed, size_t rb, int I, int L, int n_words, int Ipad,
						     uint64_t *__restrict__ planes)
{
	__shared__ uint32_t tile[BT_L * BT_ROW];
	const int w = blockIdx.x % n_words, l0 = w * BT_L, i0 = (blockIdx.x / n_words) * BT_I;
	bed_stage_tile(tile, bed, rb, L, l0, i0);
	__syncthreads();
	const uint8_t *tb = reinterpret_cast<const uint8_t *>(tile);
	const int lane = threadIdx.x & 63, first = (threadIdx.x >> 6) * 64;
	const bool l_in = l0 + lane < L;
	uint64_t v = 0, h = 0, b = 0;
	for (int k = 0; k < 64; k++) {
		const int r = first + k;
		const uint32_t c = ((uint32_t)tb[lane * (BT_ROW * 4) + r / 4] >> (2 * (r & 3))) & 3u;
		const bool in = l_in && i0 + r < I;	/* padding bits and staged zeros carry no call */
		const uint64_t bv = __ballot(in && c != 1u), bh = __ballot(in && c == 2u), bb = __ballot(in && c == 3u);
		if (lane == k) { v = bv; h = bh; b = bb; }
	}
	const int i = i0 + first + lane;
	if (i >= Ipad) return;
	const size_t plane = (size_t)n_words * (size_t)Ipad, at = (size_t)w * (size_t)Ipad + (size_t)i;
	planes[at] = v;
	planes[plane + at] = h;
	planes[2 * plane + at] = b;
}

/* sums[((i - i0) * I + j) * 4 + 0..3] += n, hh, op, h_ij and hji[(i - i0) * I + j] += h_ji of the pair (i, j) over this workgroup's
 * run of words.  blockIdx.x = tile of rows + n_rtiles * tile of columns, blockIdx.y = run of words.  Per stage the four planes
 * (valid, het, hom A1 = valid & ~het & ~hom A2, hom A2) of the tile's row and column individuals go to LDS (16 KB).  Lane (tx, ty)
 * of 16 x 16 owns the rows 4 ty ... 4 ty + 3 and the columns tx, tx + 16, tx + 32, tx + 48 of the tile: the 16 lanes tx of a wave
 * read 16 consecutive words of a plane, the four ty the same ones (broadcast). */
__global__ __launch_bounds__(256) void k_king_pairs(const uint64_t *__restrict__ planes, int n_words, int Ipad, int I, int i0, int n_rows,
						    king_geometry g, uint32_t *__restrict__ sums, uint32_t *__restrict__ hji)
{
	__shared__ uint64_t rs[4][KING_STAGE][KING_TILE];
	__shared__ uint64_t cs[4][KING_STAGE][KING_TILE];
	const int rt = blockIdx.x % g.n_rtiles, ct = blockIdx.x / g.n_rtiles;
	const int r0 = i0 + rt * KING_TILE, c0 = ct * KING_TILE;
	const int w_begin = (int)blockIdx.y * g.stages_per_split * KING_STAGE;
	const int w_end = min(n_words, w_begin + g.stages_per_split * KING_STAGE);
	const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
	const size_t plane = (size_t)n_words * (size_t)Ipad;
	uint32_t acc[KING_PER][KING_PER][5];
#pragma unroll
	for (int r = 0; r < KING_PER; r++)
#pragma unroll
		for (int c = 0; c < KING_PER; c++)
#pragma unroll
			for (int s = 0; s < 5; s++) acc[r][c][s] = 0;
	for (int ws = w_begin; ws < w_end; ws += KING_STAGE) {
		__syncthreads();	/* the stage before has been read */
		for (int x = threadIdx.x; x < 2 * KING_STAGE * KING_TILE; x += 256) {
			const int side = x / (KING_STAGE * KING_TILE), w = (x / KING_TILE) % KING_STAGE, k = x % KING_TILE;
			const int idx = (side ? c0 : r0) + k;
			uint64_t v = 0, h = 0, b = 0;
			if (idx < Ipad && ws + w < w_end) {	/* (a slab's last row tile may reach behind the padded individuals) */
				const size_t at = (size_t)(ws + w) * (size_t)Ipad + (size_t)idx;
				v = planes[at]; h = planes[plane + at]; b = planes[2 * plane + at];
			}
			uint64_t (*dst)[KING_STAGE][KING_TILE] = side ? cs : rs;
			dst[0][w][k] = v; dst[1][w][k] = h; dst[2][w][k] = v & ~h & ~b; dst[3][w][k] = b;
		}
		__syncthreads();
#pragma unroll 1
		for (int w = 0; w < KING_STAGE; w++) {	/* (words behind w_end are staged as zeros) */
			uint64_t cv[KING_PER], ch[KING_PER], ca[KING_PER], cb[KING_PER];
#pragma unroll
			for (int c = 0; c < KING_PER; c++) {
				const int k = tx + 16 * c;
				cv[c] = cs[0][w][k]; ch[c] = cs[1][w][k]; ca[c] = cs[2][w][k]; cb[c] = cs[3][w][k];
			}
#pragma unroll
			for (int r = 0; r < KING_PER; r++) {
				const int k = ty * KING_PER + r;
				const uint64_t rv = rs[0][w][k], rh = rs[1][w][k], ra = rs[2][w][k], rb2 = rs[3][w][k];
#pragma unroll
				for (int c = 0; c < KING_PER; c++) {
					acc[r][c][0] += (uint32_t)__popcll(rv & cv[c]);
					acc[r][c][1] += (uint32_t)__popcll(rh & ch[c]);
					acc[r][c][2] += (uint32_t)__popcll((ra & cb[c]) | (rb2 & ca[c]));
					acc[r][c][3] += (uint32_t)__popcll(rh & cv[c]);
					acc[r][c][4] += (uint32_t)__popcll(ch[c] & rv);
				}
			}
		}
	}
#pragma unroll
	for (int r = 0; r < KING_PER; r++) {
		const int i = r0 + ty * KING_PER + r;
		if (i >= i0 + n_rows) continue;
#pragma unroll
		for (int c = 0; c < KING_PER; c++) {
			const int j = c0 + tx + 16 * c;
			if (j >= I) continue;
			const size_t p = (size_t)(i - i0) * (size_t)I + (size_t)j;
			atomicAdd(sums + 4 * p + 0, acc[r][c][0]);
			atomicAdd(sums + 4 * p + 1, acc[r][c][1]);
			atomicAdd(sums + 4 * p + 2, acc[r][c][2]);
			atomicAdd(sums + 4 * p + 3, acc[r][c][3]);
			atomicAdd(hji + p, acc[r][c][4]);
		}
	}
}

/* phi of every pair from its counts, in exact 64-bit integers up to the one division of the definition; NaN where m = 0 */
__global__ __launch_bounds__(256) void k_king_phi(const uint32_t *__restrict__ sums, const uint32_t *__restrict__ hji, size_t n_pairs,
						  double *__restrict__ phi)
{
	for (size_t x = (size_t)blockIdx.x * 256 + threadIdx.x; x < n_pairs; x += (size_t)gridDim.x * 256) {
		const int64_t hh = sums[4 * x + 1], op = sums[4 * x + 2], hij = sums[4 * x + 3], hj = hji[x];
		const int64_t m = hij < hj ? hij : hj;
		const int64_t num = 2 * hh - 4 * op - hij - hj + 2 * m;
		phi[x] = m ? (double)num / (double)(4 * m) : __longlong_as_double(QUIET_NAN_BITS);
	}
}

extern "C" int mchip_bed_king(mchip_context *ctx, int I, int L, const uint8_t *bed, size_t record_bytes, int i0, int n_rows, double *phi,
			      uint32_t *counts)
{
	MCHIP_ENTRY();
	if (!ctx) return MCHIP_ERR_INVALID;
	if (!bed_shape_ok(I, L, bed, record_bytes) || !phi)
		return fail(ctx, MCHIP_ERR_INVALID, "bed_king: bad shape, null pointer or records shorter than ceil(I/4) bytes%s", nullptr);
	if (i0 < 0 || n_rows < 0 || (long long)i0 + n_rows > I)
		return fail(ctx, MCHIP_ERR_INVALID, "bed_king: rows outside the individuals%s", nullptr);
	if (!n_rows) return MCHIP_OK;
	if (I > 0x7FFFFFFF - KING_TILE)
		return fail(ctx, MCHIP_ERR_UNSUPPORTED, "bed_king: too many individuals%s", nullptr);
	const int n_words = (int)(((long long)L + 63) / 64), Ipad = (I + KING_TILE - 1) / KING_TILE * KING_TILE;
	const king_geometry g = king_geometry_of(I, n_rows, L, (long long)ctx->knob.per_cu_ind * (ctx->n_cu > 0 ? ctx->n_cu : 256));
	const size_t t_blocks = (size_t)n_words * (size_t)((I + BT_I - 1) / BT_I);
	if ((long long)g.n_rtiles * g.n_ctiles >= (1ll << 31) || t_blocks >= ((size_t)1 << 31))
		return fail(ctx, MCHIP_ERR_UNSUPPORTED, "bed_king: too many individuals or variants for one launch; call it in slabs of rows%s", nullptr);
	HIPCHK(hipSetDevice(ctx->device));
	const size_t bed_bytes = (size_t)L * record_bytes, n_planes = 3 * (size_t)n_words * (size_t)Ipad, n_pairs = (size_t)n_rows * (size_t)I;
	scoped_dev<uint8_t> d_bed;
	scoped_dev<uint64_t> d_planes;
	scoped_dev<uint32_t> d_sums, d_hji;
	scoped_dev<double> d_phi;
	const hipError_t uploaded = bed_upload(ctx, d_bed, bed, bed_bytes);
	if (!d_bed.p || d_planes.alloc(n_planes) != hipSuccess || d_sums.alloc(n_pairs * 4) != hipSuccess ||
	    d_hji.alloc(n_pairs) != hipSuccess || d_phi.alloc(n_pairs) != hipSuccess) {
		(void)hipGetLastError();
		return fail(ctx, MCHIP_ERR_ALLOC, "bed_king: the records, the planes or the slab's counts and kinships do not fit on the device%s", nullptr);
	}
	HIPCHK(uploaded);
	HIPCHK(hipMemsetAsync(d_sums.p, 0, n_pairs * 4 * sizeof(uint32_t), ctx->stream));
	HIPCHK(hipMemsetAsync(d_hji.p, 0, n_pairs * sizeof(uint32_t), ctx->stream));
	hipLaunchKernelGGL(k_king_planes, dim3((unsigned)t_blocks), dim3(256), 0, ctx->stream, d_bed.p, record_bytes, I, L, n_words, Ipad, d_planes.p);
	HIPCHK(hipGetLastError());
	hipLaunchKernelGGL(k_king_pairs, dim3((unsigned)(g.n_rtiles * g.n_ctiles), (unsigned)g.n_split), dim3(256), 0, ctx->stream, d_planes.p, n_words,
			   Ipad, I, i0, n_rows, g, d_sums.p, d_hji.p);
	HIPCHK(hipGetLastError());
	hipLaunchKernelGGL(k_king_phi, dim3(nblk_capped(n_pairs)), dim3(256), 0, ctx->stream, d_sums.p, d_hji.p, n_pairs, d_phi.p);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(phi, d_phi.p, sizeof(double) * n_pairs, hipMemcpyDeviceToHost, ctx->stream));
	if (counts) HIPCHK(hipMemcpyAsync(counts, d_sums.p, sizeof(uint32_t) * 4 * n_pairs, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	return MCHIP_OK;
}

/* ---- genotype counts along both axes and the Hardy-Weinberg exact test: mchip_bed_qc (include/multiclust_hip.h has the definition) ---- */
static_assert(QC_ITILE == BT_I && QC_VARIANTS * 64 == 256 && QC_STEP == 64, "k_qc_variants and k_qc_individuals are written for these");

/* mask[w] = bit 2 j for every individual 32 w + j < I with keep[i] != 0 (keep = null: every one): the low bit of each kept
 * individual's two, nothing where a record holds padding */
__global__ __launch_bounds__(256) void k_qc_mask(const uint8_t *__restrict__ keep, int I, int n_words, uint64_t *__restrict__ mask)
{
	const int w = blockIdx.x * 256 + threadIdx.x;
	if (w >= n_words) return;
	uint64_t m = 0;
	for (int j = 0; j < 32; j++) {
		const long long i = 32ll * w + j;
		if (i < I && (!keep || keep[i])) m |= 1ull << (2 * j);
	}
	mask[w] = m;
}

/* var[4 l + c] += the kept individuals of this workgroup's run with code c at variant l.  blockIdx.x = group of QC_VARIANTS
 * variants, a wave each; blockIdx.y = run of individuals.  Word w of a record is its bytes 8 w ... 8 w + 7 (w < n_words =
 * ceil(I / 32), so byte 8 w lies inside the record); what it holds behind the record's last byte is never read into the high half
 * and masked in the low one. */
__global__ __launch_bounds__(256) void k_qc_variants(const uint8_t *__restrict__ bed, size_t rb, int L, int n_words,
						     const uint64_t *__restrict__ mask, qc_geometry g, uint32_t *__restrict__ var)
{
	const int lane = threadIdx.x & 63;
	const long long l = (long long)blockIdx.x * QC_VARIANTS + (threadIdx.x >> 6);
	if (l >= L) return;	/* (a whole wave) */
	const long long w_begin = (long long)blockIdx.y * g.steps_per_split * QC_STEP;
	const int w_end = (int)min((long long)n_words, w_begin + (long long)g.steps_per_split * QC_STEP);
	uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
	for (long long w = w_begin + lane; w < w_end; w += QC_STEP) {
		const size_t off = 8 * (size_t)w;
		uint64_t v = bed_word(bed, (size_t)l * rb + off);
		if (off + 4 < rb) v |= (uint64_t)bed_word(bed, (size_t)l * rb + off + 4) << 32;
		const uint64_t m = mask[w], lo = v & m, hi = (v >> 1) & m;
		c0 += (uint32_t)__popcll(m & ~lo & ~hi);
		c1 += (uint32_t)__popcll(lo & ~hi);
		c2 += (uint32_t)__popcll(hi & ~lo);
		c3 += (uint32_t)__popcll(lo & hi);
	}
	c0 = wave_sum_u32(c0); c1 = wave_sum_u32(c1); c2 = wave_sum_u32(c2); c3 = wave_sum_u32(c3);
	if (lane == 0) {
		uint32_t *out = var + 4 * (size_t)l;
		atomicAdd(out + 0, c0); atomicAdd(out + 1, c1); atomicAdd(out + 2, c2); atomicAdd(out + 3, c3);
	}
}

/* ind[4 i + c] += the variants of this workgroup's run at which individual i has code c.  blockIdx.x = tile of QC_ITILE individuals,
 * blockIdx.y = run of words of 64 variants.  Per word the tile is staged and read as in k_king_planes: lane = variant, a wave walks
 * its 64 individuals, the ballot of a code over the lanes is the k-th individual's word and lane k counts it.  Code 0 is what is
 * left of the run's variants. */
__global__ __launch_bounds__(256) void k_qc_individuals(const uint8_t *__restrict__ bed, size_t rb, int I, int L, int n_words, qc_geometry g,
							uint32_t *__restrict__ ind)
{
	__shared__ uint32_t tile[BT_L * BT_ROW];
	const int i0 = blockIdx.x * QC_ITILE;
	const long long w_begin = (long long)blockIdx.y * g.words_per_split;
	const int w_end = (int)min((long long)n_words, w_begin + g.words_per_split);
	const uint8_t *tb = reinterpret_cast<const uint8_t *>(tile);
	const int lane = threadIdx.x & 63, first = (threadIdx.x >> 6) * 64;
	uint32_t c1 = 0, c2 = 0, c3 = 0;
	for (int w = (int)w_begin; w < w_end; w++) {
		__syncthreads();	/* the word before has been read */
		bed_stage_tile(tile, bed, rb, L, w * BT_L, i0);
		__syncthreads();
		const bool l_in = (long long)w * BT_L + lane < L;
		for (int k = 0; k < 64; k++) {
			const int r = first + k;
			const uint32_t c = ((uint32_t)tb[lane * (BT_ROW * 4) + r / 4] >> (2 * (r & 3))) & 3u;
			const bool in = l_in && i0 + r < I;	/* padding bits and staged zeros carry no call */
			const uint64_t b1 = __ballot(in && c == 1u), b2 = __ballot(in && c == 2u), b3 = __ballot(in && c == 3u);
			if (lane == k) { c1 += (uint32_t)__popcll(b1); c2 += (uint32_t)__popcll(b2); c3 += (uint32_t)__popcll(b3); }
		}
	}
	const int i = i0 + first + lane;
	if (i >= I || w_begin >= w_end) return;
	const long long l_end = 64ll * w_end < L ? 64ll * w_end : (long long)L;
	const uint32_t n = (uint32_t)(l_end - 64ll * w_begin);
	uint32_t *out = ind + 4 * (size_t)i;
	atomicAdd(out + 0, n - c1 - c2 - c3); atomicAdd(out + 1, c1); atomicAdd(out + 2, c2); atomicAdd(out + 3, c3);
}

/* the walk of the definition from h = mid: visit(h, w) for mid, then downwards, then upwards.  One multiply and one divide a step,
 * in this order; the integer products are exact in 64 bits for N < 2^30 */
template <typename F> __device__ __forceinline__ void qc_hwe_walk(int64_t N, int64_t r, int64_t mid, F &&visit)
{
#pragma clang fp contract(off)
	int64_t h = mid, a = (r - mid) / 2, b = N - h - a;
	double w = 1.0;
	visit(h, w);
	while (h >= 2) {
		w = (w * (double)(h * (h - 1))) / (double)(4 * (a + 1) * (b + 1));
		h -= 2; a += 1; b += 1;
		visit(h, w);
	}
	h = mid; a = (r - mid) / 2; b = N - h - a; w = 1.0;
	while (h <= r - 2) {
		w = (w * (double)(4 * a * b)) / (double)((h + 2) * (h + 1));
		h += 2; a -= 1; b -= 1;
		visit(h, w);
	}
}

/* p[l] of the counts var[4 l + 0, 2, 3]: the walk twice, the second time with the same bits, no weight kept */
__global__ __launch_bounds__(64) void k_qc_hwe(const uint32_t *__restrict__ var, int L, double *__restrict__ p)
{
#pragma clang fp contract(off)
	const long long l = (long long)blockIdx.x * 64 + threadIdx.x;
	if (l >= L) return;
	const int64_t n0 = var[4 * l], n2 = var[4 * l + 2], n3 = var[4 * l + 3], N = n0 + n2 + n3;
	if (N == 0) { p[l] = 1.0; return; }
	const int64_t r = 2 * (n0 < n3 ? n0 : n3) + n2;
	int64_t mid = (r * (2 * N - r)) / (2 * N);
	if ((mid ^ r) & 1) mid += 1;
	double S = 0.0, w_obs = 0.0, T = 0.0;
	qc_hwe_walk(N, r, mid, [&](int64_t h, double w) { S += w; if (h == n2) w_obs = w; });
	const double bound = w_obs * 1.0000001;
	qc_hwe_walk(N, r, mid, [&](int64_t, double w) { if (w <= bound) T += w; });
	const double q = T / S;
	p[l] = q > 1.0 ? 1.0 : q;
}

extern "C" int mchip_bed_qc(mchip_context *ctx, int I, int L, const uint8_t *bed, size_t record_bytes, const uint8_t *ind_keep,
			    uint32_t *ind_counts, uint32_t *var_counts, double *hwe_p)
{
	MCHIP_ENTRY();
	if (!ctx) return MCHIP_ERR_INVALID;
	if (!bed_shape_ok(I, L, bed, record_bytes) || (!ind_counts && !var_counts && !hwe_p))
		return fail(ctx, MCHIP_ERR_INVALID, "bed_qc: bad shape, null records, records shorter than ceil(I/4) bytes or no output array%s", nullptr);
	if (I >= (1 << 30))
		return fail(ctx, MCHIP_ERR_UNSUPPORTED, "bed_qc: 2^30 or more individuals: the products of the exact test leave 64 bits%s", nullptr);
	const int n_mwords = (I + 31) / 32, n_lwords = (int)(((long long)L + 63) / 64);
	const qc_geometry g = qc_geometry_of(I, L, (long long)ctx->knob.per_cu_ind * (ctx->n_cu > 0 ? ctx->n_cu : 256));
	const bool by_variant = var_counts || hwe_p;
	HIPCHK(hipSetDevice(ctx->device));
	scoped_dev<uint8_t> d_bed, d_keep;
	scoped_dev<uint64_t> d_mask;
	scoped_dev<uint32_t> d_var, d_ind;
	scoped_dev<double> d_p;
	const hipError_t uploaded = bed_upload(ctx, d_bed, bed, (size_t)L * record_bytes);
	if (!d_bed.p || (by_variant && (d_mask.alloc((size_t)n_mwords) != hipSuccess || d_var.alloc(4 * (size_t)L) != hipSuccess)) ||
	    (by_variant && ind_keep && d_keep.alloc((size_t)I) != hipSuccess) || (hwe_p && d_p.alloc((size_t)L) != hipSuccess) ||
	    (ind_counts && d_ind.alloc(4 * (size_t)I) != hipSuccess)) {
		(void)hipGetLastError();
		return fail(ctx, MCHIP_ERR_ALLOC, "bed_qc: the records, the mask, the counts or the p values do not fit on the device%s", nullptr);
	}
	HIPCHK(uploaded);
	if (by_variant) {
		if (ind_keep) HIPCHK(hipMemcpyAsync(d_keep.p, ind_keep, (size_t)I, hipMemcpyHostToDevice, ctx->stream));
		HIPCHK(hipMemsetAsync(d_var.p, 0, 4 * (size_t)L * sizeof(uint32_t), ctx->stream));
		hipLaunchKernelGGL(k_qc_mask, dim3(nblk((size_t)n_mwords)), dim3(256), 0, ctx->stream, d_keep.p, I, n_mwords, d_mask.p);
		HIPCHK(hipGetLastError());
		hipLaunchKernelGGL(k_qc_variants, dim3((unsigned)g.n_vgroups, (unsigned)g.v_split), dim3(256), 0, ctx->stream, d_bed.p, record_bytes, L,
				   n_mwords, d_mask.p, g, d_var.p);
		HIPCHK(hipGetLastError());
	}
	if (hwe_p) {
		hipLaunchKernelGGL(k_qc_hwe, dim3(nblk((size_t)L, 64)), dim3(64), 0, ctx->stream, d_var.p, L, d_p.p);
		HIPCHK(hipGetLastError());
	}
	if (ind_counts) {
		HIPCHK(hipMemsetAsync(d_ind.p, 0, 4 * (size_t)I * sizeof(uint32_t), ctx->stream));
		hipLaunchKernelGGL(k_qc_individuals, dim3((unsigned)g.n_itiles, (unsigned)g.i_split), dim3(256), 0, ctx->stream, d_bed.p, record_bytes, I,
				   L, n_lwords, g, d_ind.p);
		HIPCHK(hipGetLastError());
	}
	if (ind_counts) HIPCHK(hipMemcpyAsync(ind_counts, d_ind.p, 4 * (size_t)I * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
	if (var_counts) HIPCHK(hipMemcpyAsync(var_counts, d_var.p, 4 * (size_t)L * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
	if (hwe_p) HIPCHK(hipMemcpyAsync(hwe_p, d_p.p, sizeof(double) * (size_t)L, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	return MCHIP_OK;
}
