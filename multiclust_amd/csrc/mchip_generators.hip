/*
 * mchip_generators.hip -- the libc-compatible rand() stream on the device and what is drawn from it: the random allele partition
 * with its first M step (mchip_mstep_from_rand_partition), the parametric-bootstrap data sets of the admixture model
 * (mchip_simulate_genotypes) and of the mixture model (mchip_simulate_genotypes_mixture), and draw_mod_stream, the plain
 * rand() % m bytes that the cross-validation folds and the Rand-EM candidates take (include/multiclust_hip.h has the contracts;
 * mchip_context.h the per-context state, the install path and the hard-partition M step this unit calls back into).
 *
 * The format of the stream is known here and nowhere else: lag 31, taps 31 and 3, the reduction polynomial x^31 - x^28 - 1
 * (rng_polymul_wide), a thread's generator as a [31][256] ring in LDS (rng_ring), the base window extended by its next 30 values
 * (rng_window_from).  So are the output layouts of a generated tile (sim_tile_begin, sim_tile_store_locus, sim_tile_store_run).
 *
 *   k_draw_partition             rand() % K, one byte per draw, in stream order; thread = chunk of RNG_CHUNK draws
 *   k_jump_powers                jump polynomials x^(A*n) of a regular lattice of stream positions, once per data-set shape
 *   k_walk_tables                the inverse-CDF walks over eta and p as integer thresholds on the value rand() returned
 *   k_simulate_admixture<FAST>   admixture bootstrap data set in stream order (raw [I][L][pl]); thread = chunk of draws
 *   k_simulate_tile<PL>          the same tile by tile, straight into gtA / gtS; thread = individual (K <= 8, <= 4 alleles, PL <= 8)
 *   k_simulate_mixture_source    mixture bootstrap: the cluster of every individual
 *   k_simulate_mixture_tile<PL>  its copies tile by tile, straight into gtA / gtS (<= 4 alleles, PL <= 8, any K)
 *   k_simulate_mixture_general   its copies in raw [I][L][pl] order (any shape)
 *   k_partition_tile<PL>         random partition + the counts of the first M step in one pass, nothing stored per copy
 *   k_partition_finish           adds the N-side slabs of k_partition_tile
 */
#include "mchip_context.h"

/* ------------------------------------------------------------------ libc-compatible rand() on the device
 * glibc's TYPE_3 generator is the additive lagged Fibonacci recurrence x_j = x_{j-31} + x_{j-3} (mod 2^32) with
 * rand() = x_j >> 1.  It is linear, so x^n mod (x^31 - x^28 - 1) over Z/2^32 carries a 31-word window n draws
 * ahead.  Thread c draws the RNG_CHUNK consecutive values that start RNG_CHUNK*c draws into the stream: its jump
 * polynomial is the product of two tabulated ones (hi = c / 256, lo = c % 256), so the stream is the serial one
 * whatever the launch geometry (random_allele_partition, rnd_init.c:456-467: one rand() % K per allele copy). */
struct rng_window { uint32_t s[2 * RNG_LAG - 1]; };	/* x_{j-31} .. x_{j+29}: window, then its next 30 values */

/* the 31 words behind a draw, extended by their next 30 values */
static rng_window rng_window_from(const uint32_t *window)
{
	rng_window base;
	for (int t = 0; t < RNG_LAG; t++) base.s[t] = window[t];
	for (int t = 0; t < RNG_LAG - 1; t++) base.s[RNG_LAG + t] = base.s[t] + base.s[RNG_LAG - 3 + t];
	return base;
}

/* t[0 .. 30] = (a * b) mod (x^31 - x^28 - 1) over Z/2^32: the product's 61 words, folded from degree 60 down.  Fully unrolled:
 * on the device every index is a constant and t stays in registers (rng_window_at); the host's compiler may do as it likes. */
__host__ __device__ __forceinline__ void rng_polymul_wide(const uint32_t *a, const uint32_t *b, uint32_t (&t)[2 * RNG_LAG - 1])
{
#pragma unroll
	for (int d = 0; d < 2 * RNG_LAG - 1; d++) t[d] = 0;
#pragma unroll
	for (int i = 0; i < RNG_LAG; i++) {
		const uint32_t h = a[i];
#pragma unroll
		for (int j = 0; j < RNG_LAG; j++) t[i + j] += h * b[j];
	}
#pragma unroll
	for (int d = 2 * RNG_LAG - 2; d >= RNG_LAG; d--) {	/* x^d = x^(d-3) + x^(d-31) */
		t[d - 3] += t[d];
		t[d - RNG_LAG] += t[d];
	}
}

/* window (31 words behind the first draw) of a thread whose first draw lies n draws into the stream, x^n = hi(x) * lo(x)
 * mod (x^31 - x^28 - 1): hi is wave-uniform (scalar loads), lo is stored [31][lo_stride] so that lanes read consecutive words */
__device__ __forceinline__ void rng_window_at(const rng_window &base, const uint32_t *__restrict__ hi,
		const uint32_t *__restrict__ lo_table, size_t lo_stride, size_t lo_index, uint32_t (&w)[RNG_LAG])
{
	uint32_t t[2 * RNG_LAG - 1];
	{
		uint32_t lo[RNG_LAG];
#pragma unroll
		for (int j = 0; j < RNG_LAG; j++) lo[j] = lo_table[j * lo_stride + lo_index];
		rng_polymul_wide(hi, lo, t);
	}
	/* w[e] = sum_j poly[j] * s[e + j] */
#pragma unroll
	for (int e = 0; e < RNG_LAG; e++) {
		uint32_t v = 0;
#pragma unroll
		for (int j = 0; j < RNG_LAG; j++) v += t[j] * base.s[e + j];
		w[e] = v;
	}
}

/* the thread whose chunk starts 256*blockIdx.x + threadIdx.x chunks of RNG_CHUNK draws into the stream: hi = x^(256*CHUNK*block),
 * lo = x^(CHUNK*thread) */
__device__ __forceinline__ void rng_thread_window(const rng_window &base, const uint32_t *__restrict__ jump_hi,
		const uint32_t *__restrict__ jump_lo, uint32_t (&w)[RNG_LAG])
{
	rng_window_at(base, jump_hi + (size_t)blockIdx.x * RNG_LAG, jump_lo, 256, threadIdx.x, w);
}

__global__ __launch_bounds__(256) void k_draw_partition(rng_window base, const uint32_t *__restrict__ jump_hi,
		const uint32_t *__restrict__ jump_lo, size_t n_chunks, uint32_t K, uint32_t magic, uint32_t shift, uint32_t *out)
{
	const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (c >= n_chunks) return;
	uint32_t w[RNG_LAG];
	rng_thread_window(base, jump_hi, jump_lo, w);
	uint32_t *dst = out + c * (RNG_CHUNK / 4);
	for (int round = 0; round < RNG_CHUNK / (4 * RNG_LAG); round++) {
		uint32_t word[RNG_LAG];
#pragma unroll
		for (int d = 0; d < 4 * RNG_LAG; d++) {
			const int e = d % RNG_LAG;
			const uint32_t x = w[e] + w[(e + RNG_LAG - 3) % RNG_LAG];	/* x_{j-31} + x_{j-3} */
			w[e] = x;
			const uint32_t v = x >> 1;
			/* v % K by multiplication: floor(v / K) = (v * magic) >> (31 + ceil(log2 K)), exact for v < 2^31 */
			const uint32_t r = v - (__umulhi(v, magic) >> shift) * K;
			if (d % 4 == 0) word[d / 4] = r;
			else word[d / 4] |= r << (8 * (d % 4));
		}
#pragma unroll
		for (int x = 0; x < RNG_LAG; x++) dst[round * RNG_LAG + x] = word[x];
	}
}

/* parametric_bootstrap_admixture (bootstrap.c:84-124) on the device.  Allele copy j (i, l, n order) takes draws 2j
 * (source cluster: inverse-CDF walk over the individual's eta) and 2j+1 (allele: walk over p[k][l][.]) of the rand()
 * stream, r = rand() / RAND_MAX in double.  The reference's walk `while (k < K && r > sum) sum += eta[k++]; if (k) k--;`
 * stops at the first t with !(r > c_t), c_t = eta[0] + ... + eta[t-1] the left-to-right partial sum (t = K if there is none),
 * and returns t - 1 (0 for t = 0).  r > c is a statement about the integer the generator returned: v / RAND_MAX, rounded,
 * never decreases in v, so r > c  <=>  v >= V(c) with V(c) the smallest v whose quotient exceeds c.  Fitted parameters
 * need not be non-negative (no projection: entries below 0; an individual with no observed copy: NaN), so the partial
 * sums need not rise; the first t with r <= c_t is also the first t with r <= max(c_0, ..., c_t), and a NaN sum stops the
 * walk there and at every later t.  The thresholds are therefore taken of the running maximum, and 2^31 (no draw reaches
 * it) from the first NaN sum on: they never decrease, and t - 1 is the number of thresholds t_1 .. t_{K-1} the draw reaches.
 * k_walk_tables finds every V once per call -- with the same double additions and the same division the reference executes
 * per copy -- and the per-copy work is integer compares against those thresholds: no running sums, no divisions, and none
 * of a copy's loads waits for another.  Every copy is simulated (in the default build the "missing stays missing" count is
 * overwritten before it is used, bootstrap.c:87-96). */
constexpr int SIM_QW = 8, SIM_PW = 4;	/* widths of the padded threshold rows of the FAST form (K <= 8, at most 4 alleles per locus) */

/* smallest v in [0, 2^31] with (double)v / RAND_MAX > c (2^31: no value of rand() does) */
__device__ uint32_t walk_threshold(double c)
{
	const double D = 2147483647.0;
	if (!(c < 2.0)) return 0x80000000u;	/* v / D <= 1 < 2; also +inf (padding) and NaN */
	double g = c * D - 2.0;
	uint32_t v = g > 0.0 ? (uint32_t)g : 0u;	/* c < 2: g < 2^32 */
	if (v > 0x80000000u) v = 0x80000000u;
	while (v > 0u && (double)(v - 1u) / D > c) v--;
	while (v < 0x80000000u && !((double)v / D > c)) v++;
	return v;
}

/* thq[i][j] = V(q[i][0] + ... + q[i][j-1]) (j < K; rows of SIM_QW padded with 2^31 when fast_q); thp[k][c0 + m] =
 * V(p[k][c0] + ... + p[k][c0 + m - 1]), or rows of SIM_PW per (k, l), padded, when fast_p; V of the running maximum of the
 * partial sums, and 2^31 from the first NaN sum on (see above).  The admixture generator sets both flags together (K <= 8 and
 * at most 4 alleles); the mixture generator walks one shared row of any K unpadded and pads the allele rows alone. */
__device__ __forceinline__ uint32_t walk_step(double sum, double &peak, bool &nan_seen)
{
	nan_seen = nan_seen || sum != sum;
	if (sum > peak) peak = sum;
	return nan_seen ? 0x80000000u : walk_threshold(peak);
}

__global__ void k_walk_tables(int n_qrows, int K, int L, int T, const int32_t *__restrict__ toff, const double *__restrict__ q,
			      const double *__restrict__ p, int fast_q, int fast_p, uint32_t *thq, uint32_t *thp)
{
	const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx < (size_t)n_qrows) {
		const double *src = q + idx * K;
		uint32_t *dst = thq + idx * (size_t)(fast_q ? SIM_QW : K);
		double sum = 0.0, peak = 0.0;
		bool nan_seen = false;
		for (int j = 0; j < K; j++) { dst[j] = walk_step(sum, peak, nan_seen); sum += src[j]; }
		if (fast_q) for (int j = K; j < SIM_QW; j++) dst[j] = 0x80000000u;
	}
	if (idx < (size_t)K * L) {
		const int l = (int)(idx % L), k = (int)(idx / L);
		const int c0 = toff[l], M = toff[l + 1] - c0;
		const double *src = p + (size_t)k * T + c0;
		uint32_t *dst = fast_p ? thp + idx * SIM_PW : thp + (size_t)k * T + c0;
		double sum = 0.0, peak = 0.0;
		bool nan_seen = false;
		for (int m = 0; m < M; m++) { dst[m] = walk_step(sum, peak, nan_seen); sum += src[m]; }
		if (fast_p) for (int m = M; m < SIM_PW; m++) dst[m] = 0x80000000u;
	}
}

/* A thread's generator in LDS: word e of all 256 lanes is one conflict-free row of `ring` ([31][256] words), so the state costs
 * no registers and the position may be a run-time value. */
struct rng_ring {
	uint32_t *ring;
	int e = 0;		/* position of x_{j-31} */
	__device__ __forceinline__ rng_ring(uint32_t *ring_) : ring(ring_) {}
	__device__ __forceinline__ void load(const uint32_t (&w)[RNG_LAG])
	{
#pragma unroll
		for (int x = 0; x < RNG_LAG; x++) ring[x * 256 + threadIdx.x] = w[x];
	}
	__device__ __forceinline__ uint32_t next()
	{
		const int e3 = e >= 3 ? e - 3 : e + RNG_LAG - 3;
		const uint32_t x = ring[e * 256 + threadIdx.x] + ring[e3 * 256 + threadIdx.x];	/* x_{j-31} + x_{j-3} */
		ring[e * 256 + threadIdx.x] = x;
		e = e + 1 == RNG_LAG ? 0 : e + 1;
		return x >> 1;		/* rand() */
	}
};

/* largest j in [0, n) with v >= tab[j], 0 if there is none; tab never decreases (k_walk_tables: thresholds of the running
 * maximum of the partial sums), so that is the count of tab[1 .. n-1] that v reaches */
__device__ __forceinline__ int walk_search(const uint32_t *__restrict__ tab, int n, uint32_t v)
{
	int lo = 0;
	while (n > 1) {
		const int half = n >> 1;
		if (v >= tab[lo + half]) lo += half;
		n -= half;
	}
	return lo;
}

/* Thread c owns RNG_CHUNK consecutive draws = RNG_CHUNK/2 copies; its generator window lives in LDS ([31][256]: word e of
 * all lanes is one conflict-free row).  Four copies (one output word) are in flight at a time: eight draws, then the four
 * cluster searches, then the four allele searches, so that the loads of the four overlap. */
template <bool FAST>
__global__ __launch_bounds__(256) void k_simulate_admixture(rng_window base, const uint32_t *__restrict__ jump_hi,
		const uint32_t *__restrict__ jump_lo, size_t n_chunks, int I, int L, int pl, int K, int T,
		const int32_t *__restrict__ toff, const uint32_t *__restrict__ thq, int per_individual, const uint32_t *__restrict__ thp,
		uint32_t *out)
{
	__shared__ uint32_t ring[RNG_LAG * 256];
	const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (c >= n_chunks) return;
	rng_ring rng(ring);
	{
		uint32_t w[RNG_LAG];
		rng_thread_window(base, jump_hi, jump_lo, w);
		rng.load(w);
	}
	constexpr int COPIES = RNG_CHUNK / 2;
	const size_t j0 = c * COPIES;
	const size_t per_i = (size_t)L * pl;
	int i = (int)(j0 / per_i);	/* <= I; copies past the data set's end are clamped to the last individual */
	int l = (int)((j0 % per_i) / pl), a = (int)(j0 % pl);
	uint32_t *dst = out + c * (COPIES / 4);
	const int qrow = FAST ? SIM_QW : K;
	for (int x = 0; x < COPIES / 4; x++) {
		uint32_t v1[4], v2[4];
		int ci[4], cl[4], k[4];
#pragma unroll
		for (int y = 0; y < 4; y++) {
			v1[y] = rng.next();
			v2[y] = rng.next();
			ci[y] = i < I ? i : I - 1;
			cl[y] = l;
			if (++a == pl) {
				a = 0;
				if (++l == L) { l = 0; i++; }
			}
		}
#pragma unroll
		for (int y = 0; y < 4; y++) {
			const uint32_t *tab = thq + (per_individual ? (size_t)ci[y] * qrow : 0);
			if (FAST) {
				const uint4 t0 = *reinterpret_cast<const uint4 *>(tab), t1 = *reinterpret_cast<const uint4 *>(tab + 4);
				k[y] = (v1[y] >= t0.y) + (v1[y] >= t0.z) + (v1[y] >= t0.w) + (v1[y] >= t1.x) + (v1[y] >= t1.y) + (v1[y] >= t1.z) +
				       (v1[y] >= t1.w);		/* t0.x = V(0): k = 0 either way */
			} else {
				k[y] = walk_search(tab, K, v1[y]);
			}
		}
		uint32_t word = 0;
#pragma unroll
		for (int y = 0; y < 4; y++) {
			int m;
			if (FAST) {
				const uint4 t = *reinterpret_cast<const uint4 *>(thp + ((size_t)k[y] * L + cl[y]) * SIM_PW);
				m = (v2[y] >= t.y) + (v2[y] >= t.z) + (v2[y] >= t.w);
			} else {
				const int c0 = toff[cl[y]], M = toff[cl[y] + 1] - c0;
				m = walk_search(thp + (size_t)k[y] * T + c0, M, v2[y]);
			}
			word |= (uint32_t)m << (8 * y);
		}
		dst[x] = word;
	}
}

/* out[j * sj + n * sn] = coefficient j of x^(A*n) mod (x^31 - x^28 - 1), n < count, from pow2[b] = x^(A * 2^b): the jump
 * polynomials of a regular lattice of stream positions, computed once per data-set shape */
__global__ void k_jump_powers(const uint32_t *__restrict__ pow2, unsigned count, size_t sj, size_t sn, uint32_t *out)
{
	const unsigned n = blockIdx.x * blockDim.x + threadIdx.x;
	if (n >= count) return;
	uint32_t acc[RNG_LAG];
	for (int j = 0; j < RNG_LAG; j++) acc[j] = j == 0;
	for (int b = 0; b < 32 && (n >> b); b++) {
		if (!((n >> b) & 1u)) continue;
		uint32_t t[2 * RNG_LAG - 1];	/* rng_polymul_wide's product with run-time indices: rolled loops over arrays in scratch */
		for (int d = 0; d < 2 * RNG_LAG - 1; d++) t[d] = 0;
		for (int i = 0; i < RNG_LAG; i++)
			for (int j = 0; j < RNG_LAG; j++) t[i + j] += acc[i] * pow2[b * RNG_LAG + j];
		for (int d = 2 * RNG_LAG - 2; d >= RNG_LAG; d--) {
			t[d - 3] += t[d];
			t[d - RNG_LAG] += t[d];
		}
		for (int j = 0; j < RNG_LAG; j++) acc[j] = t[j];
	}
	for (int j = 0; j < RNG_LAG; j++) out[j * sj + n * sn] = acc[j];
}

/* The same data set generated tile by tile (FAST form: K <= 8, at most 4 alleles per locus, ploidy <= 8): workgroup = 256
 * individuals x the `tile_loci` loci from blockIdx.x * tile_loci on.  Thread = individual i: its draws for the tile start
 * 2 * (i * L * PL + l0 * PL) into the stream, x^that = jump_i[i] * jump_r[blockIdx.x] (k_jump_powers).  The allele
 * thresholds of the tile's loci are staged in LDS ([locus][k][3]: the 64 lanes are at the same locus and differ in k only), the
 * individual's own cluster thresholds sit in registers, and the copies go straight into the two device layouts (gtS: the
 * thread's 8 loci x PL bytes are one contiguous run, runs of consecutive individuals adjacent; gtA: PL bytes per locus, 8
 * consecutive lanes adjacent) -- no raw [I][L][PL] intermediate and no gather from global memory.  tile_loci % 8 == 0. */
/* What k_simulate_tile and k_simulate_mixture_tile share, the layouts of a generated tile.  sim_tile_begin: the allele thresholds of
 * the tile's nl loci from l0 on into LDS ([locus][k][3]), a barrier, colA = the thread's PL bytes of locus l0 in gtA, MISSING into
 * the rows that pad the last block of 8 individuals; false for a thread that has nothing to draw (called by every thread). */
template <int PL>
__device__ __forceinline__ bool sim_tile_begin(uint32_t *tile, const uint32_t *__restrict__ thp, int I, int L, int K, int l0, int nl, int i,
		uint8_t *__restrict__ gtA, uint8_t *&colA)
{
	for (int idx = threadIdx.x; idx < K * nl; idx += 256) {
		const int k = idx / nl, ll = idx - k * nl;
		const uint4 t = *reinterpret_cast<const uint4 *>(thp + ((size_t)k * L + l0 + ll) * SIM_PW);
		uint32_t *dst = tile + ((size_t)ll * K + k) * 3;
		dst[0] = t.y; dst[1] = t.z; dst[2] = t.w;	/* t.x = V(0): allele 0 either way */
	}
	__syncthreads();
	if (i >= ((I + 7) & ~7)) return false;
	colA = gtA + ((((size_t)(i >> 3) * L + l0) * 8) + (i & 7)) * PL;	/* + ll * 8 * PL per locus */
	if (i >= I) {		/* rows that pad the last block of 8 individuals */
		for (int ll = 0; ll < nl; ll++)
#pragma unroll
			for (int a = 0; a < PL; a++) colA[(size_t)ll * 8 * PL + a] = MCHIP_MISSING;
		return false;
	}
	return true;
}

/* the PL copies of locus ll of the tile (`bytes`, copy a in byte a) to gtA by width, and into locus t of the 8-locus gtS run */
template <int PL>
__device__ __forceinline__ void sim_tile_store_locus(uint8_t *colA, int ll, int t, unsigned long long bytes, unsigned long long (&run)[PL])
{
	uint8_t *dst = colA + (size_t)ll * 8 * PL;
	if (PL == 4) *reinterpret_cast<uint32_t *>(dst) = (uint32_t)bytes;
	else if (PL == 2) *reinterpret_cast<uint16_t *>(dst) = (uint16_t)bytes;
	else if (PL == 8) *reinterpret_cast<unsigned long long *>(dst) = bytes;
	else {
#pragma unroll
		for (int a = 0; a < PL; a++) dst[a] = (uint8_t)(bytes >> (8 * a));
	}
#pragma unroll
	for (int a = 0; a < PL; a++) {
		constexpr unsigned long long ff = 0xFFull;
		const int b = t * PL + a;
		run[b >> 3] = (run[b >> 3] & ~(ff << (8 * (b & 7)))) | (((bytes >> (8 * a)) & ff) << (8 * (b & 7)));
	}
}

/* the run of block `lgroup` of 8 loci to gtS */
template <int PL>
__device__ __forceinline__ void sim_tile_store_run(uint8_t *__restrict__ gtS, int I, int i, int lgroup, const unsigned long long (&run)[PL])
{
	unsigned long long *dstS = reinterpret_cast<unsigned long long *>(gtS + (((size_t)lgroup * I + i) * 8) * PL);
#pragma unroll
	for (int x = 0; x < PL; x++) dstS[x] = run[x];
}

template <int PL>
__global__ __launch_bounds__(256) void k_simulate_tile(rng_window base, const uint32_t *__restrict__ jump_i,
		const uint32_t *__restrict__ jump_r, int I, int L, int K, int tile_loci, const uint32_t *__restrict__ thq,
		int per_individual, const uint32_t *__restrict__ thp, uint8_t *__restrict__ gtA, uint8_t *__restrict__ gtS)
{
	extern __shared__ uint32_t sim_lds[];
	uint32_t *ring = sim_lds, *tile = sim_lds + RNG_LAG * 256;
	const int l0 = blockIdx.x * tile_loci;
	const int nl = L - l0 < tile_loci ? L - l0 : tile_loci;
	const int i = blockIdx.y * 256 + threadIdx.x;
	uint8_t *colA;
	if (!sim_tile_begin<PL>(tile, thp, I, L, K, l0, nl, i, gtA, colA)) return;
	rng_ring rng(ring);
	{
		uint32_t w[RNG_LAG];
		rng_window_at(base, jump_r + (size_t)blockIdx.x * RNG_LAG, jump_i, (size_t)I, (size_t)i, w);
		rng.load(w);
	}
	uint32_t tq[SIM_QW - 1];
	{
		const uint32_t *row = thq + (per_individual ? (size_t)i * SIM_QW : 0);
		const uint4 t0 = *reinterpret_cast<const uint4 *>(row), t1 = *reinterpret_cast<const uint4 *>(row + 4);
		tq[0] = t0.y; tq[1] = t0.z; tq[2] = t0.w; tq[3] = t1.x; tq[4] = t1.y; tq[5] = t1.z; tq[6] = t1.w;
	}
	for (int g = 0; g * 8 < nl; g++) {
		unsigned long long run[PL];	/* the 8 * PL bytes of this individual's gtS group */
#pragma unroll
		for (int x = 0; x < PL; x++) run[x] = ~0ull;
#pragma unroll
		for (int t = 0; t < 8; t++) {
			const int ll = g * 8 + t;
			if (ll < nl) {		/* uniform */
				uint32_t v1[PL], v2[PL];
#pragma unroll
				for (int a = 0; a < PL; a++) { v1[a] = rng.next(); v2[a] = rng.next(); }
				unsigned long long bytes = 0;
#pragma unroll
				for (int a = 0; a < PL; a++) {
					int k = 0;
#pragma unroll
					for (int x = 0; x < SIM_QW - 1; x++) k += v1[a] >= tq[x];
					const uint32_t *th = tile + ((size_t)ll * K + k) * 3;
					const unsigned m = (v2[a] >= th[0]) + (v2[a] >= th[1]) + (v2[a] >= th[2]);
					bytes |= (unsigned long long)m << (8 * a);
				}
				sim_tile_store_locus<PL>(colA, ll, t, bytes, run);
			}
		}
		sim_tile_store_run<PL>(gtS, I, i, l0 / 8 + g, run);
	}
}

/* parametric_bootstrap_mixture (bootstrap.c:132-175) on the device.  Individual i owns draws i * (1 + L*PL) .. of the rand()
 * stream: the first chooses its cluster by the walk over eta, draw 1 + l*PL + a chooses copy (l, a) by the walk over
 * p[k][l][.]; the decisions are the integer compares against k_walk_tables' thresholds described above.
 * k_simulate_mixture_source: thread = individual, its window taken at the individual's first draw (jump_i[i]; jump_r[0] = x^0),
 * one draw, one search of the shared row thq[0..K), the cluster stored as a byte. */
__global__ __launch_bounds__(256) void k_simulate_mixture_source(rng_window base, const uint32_t *__restrict__ jump_i,
		const uint32_t *__restrict__ jump_r, int I, int K, const uint32_t *__restrict__ thq, uint8_t *__restrict__ cluster)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= I) return;
	uint32_t w[RNG_LAG];
	rng_window_at(base, jump_r, jump_i, (size_t)I, (size_t)i, w);
	const uint32_t v = (w[0] + w[RNG_LAG - 3]) >> 1;	/* rand(): x_{j-31} + x_{j-3} */
	cluster[i] = (uint8_t)walk_search(thq, K, v);
}

/* The copies, tile by tile (at most 4 alleles per locus, ploidy <= 8; any K: the cluster is fixed per thread): the geometry of
 * k_simulate_tile with one draw per copy.  `base` stands one draw into the stream, so that jump_i[i] * jump_r[blockIdx.x] =
 * x^(i * (1 + L*PL) + l0 * PL) lands on the thread's first copy draw of the tile.  Allele thresholds of the tile's loci in LDS
 * ([locus][k][3]), copies straight into gtA and gtS, MISSING in the rows that pad the last block of 8 individuals. */
template <int PL>
__global__ __launch_bounds__(256) void k_simulate_mixture_tile(rng_window base, const uint32_t *__restrict__ jump_i,
		const uint32_t *__restrict__ jump_r, int I, int L, int K, int tile_loci, const uint8_t *__restrict__ cluster,
		const uint32_t *__restrict__ thp, uint8_t *__restrict__ gtA, uint8_t *__restrict__ gtS)
{
	extern __shared__ uint32_t sim_lds[];
	uint32_t *ring = sim_lds, *tile = sim_lds + RNG_LAG * 256;
	const int l0 = blockIdx.x * tile_loci;
	const int nl = L - l0 < tile_loci ? L - l0 : tile_loci;
	const int i = blockIdx.y * 256 + threadIdx.x;
	uint8_t *colA;
	if (!sim_tile_begin<PL>(tile, thp, I, L, K, l0, nl, i, gtA, colA)) return;
	rng_ring rng(ring);
	{
		uint32_t w[RNG_LAG];
		rng_window_at(base, jump_r + (size_t)blockIdx.x * RNG_LAG, jump_i, (size_t)I, (size_t)i, w);
		rng.load(w);
	}
	const uint32_t *mine = tile + (size_t)cluster[i] * 3;	/* + ll * K * 3 per locus */
	for (int g = 0; g * 8 < nl; g++) {
		unsigned long long run[PL];	/* the 8 * PL bytes of this individual's gtS group */
#pragma unroll
		for (int x = 0; x < PL; x++) run[x] = ~0ull;
#pragma unroll
		for (int t = 0; t < 8; t++) {
			const int ll = g * 8 + t;
			if (ll < nl) {		/* uniform */
				const uint32_t *th = mine + (size_t)ll * K * 3;
				const uint32_t t1 = th[0], t2 = th[1], t3 = th[2];
				unsigned long long bytes = 0;
#pragma unroll
				for (int a = 0; a < PL; a++) {
					const uint32_t v = rng.next();
					const unsigned m = (v >= t1) + (v >= t2) + (v >= t3);
					bytes |= (unsigned long long)m << (8 * a);
				}
				sim_tile_store_locus<PL>(colA, ll, t, bytes, run);
			}
		}
		sim_tile_store_run<PL>(gtS, I, i, l0 / 8 + g, run);
	}
}

/* Launch of either tile kernel: one workgroup per (tile of loci, 256 individuals, the rows that pad the last block of 8 included);
 * LDS = the ring + the staged thresholds [tile][K][3].  `model` = the kernel's arguments between tile_loci and gtA. */
template <typename Kernel, typename... Model>
static void launch_sim_tile(mchip_context *ctx, Kernel kernel, const rng_window &base, int K, int tile, Model... model)
{
	const unsigned R = (unsigned)((ctx->L + tile - 1) / tile), by = (unsigned)((((ctx->I + 7) & ~7) + 255) / 256);
	const size_t lds = ((size_t)RNG_LAG * 256 + (size_t)tile * K * 3) * sizeof(uint32_t);
	hipLaunchKernelGGL(kernel, dim3(R, by), dim3(256), lds, ctx->stream, base, ctx->lat[0].d_i, ctx->lat[0].d_r, ctx->I, ctx->L, K, tile,
			   model..., ctx->d_gtA, ctx->d_gtS);
}

/* loci per tile: as many as keep the staged thresholds near 16 KiB (three workgroups per compute unit), a multiple of 8
 * (K = 64: 16 loci, 12 KiB; the mixture generator's K > 170: 8 loci all the same) */
static int sim_tile_loci(int K, int L)
{
	int tile = (16384 / (K * 12)) & ~7;
	if (tile < 8) tile = 8;
	if (tile > 512) tile = 512;
	if (tile > ((L + 7) & ~7)) tile = (L + 7) & ~7;
	return tile;
}

/* the generated data set is in stream order in d_raw, or in gtA / gtS already (d_raw == nullptr): launch check, the rest of the
 * layouts, and the stream drained before the caller's temporaries go */
static int sim_install(mchip_context *ctx, const uint8_t *d_raw)
{
	HIPCHK(hipGetLastError());
	const int rc = d_raw ? install_raw(ctx, d_raw) : install_layouts(ctx, 0);
	(void)MCHIP_WAIT(hipStreamSynchronize(ctx->stream));	/* the temporaries go out of scope */
	return rc;
}

/* The general form (more than 4 alleles at some locus, ploidy > 8, MCHIP_SIM_NO_TILE): the same lattice -- workgroup = 256
 * individuals x a chunk of `chunk_loci` loci, thread = individual, `base` one draw into the stream -- with the thresholds read
 * from global memory through walk_search (rows [k][T], or the padded [k][l][SIM_PW] rows when no locus has more than 4 alleles)
 * and the copies stored in raw [I][L][pl] order for install_raw. */
__global__ __launch_bounds__(256) void k_simulate_mixture_general(rng_window base, const uint32_t *__restrict__ jump_i,
		const uint32_t *__restrict__ jump_r, int I, int L, int pl, int T, int chunk_loci, const int32_t *__restrict__ toff,
		const uint8_t *__restrict__ cluster, const uint32_t *__restrict__ thp, int fast_p, uint8_t *__restrict__ raw)
{
	__shared__ uint32_t ring[RNG_LAG * 256];
	const int i = blockIdx.y * 256 + threadIdx.x;
	if (i >= I) return;
	const int l0 = blockIdx.x * chunk_loci;
	const int l1 = L - l0 < chunk_loci ? L : l0 + chunk_loci;
	rng_ring rng(ring);
	{
		uint32_t w[RNG_LAG];
		rng_window_at(base, jump_r + (size_t)blockIdx.x * RNG_LAG, jump_i, (size_t)I, (size_t)i, w);
		rng.load(w);
	}
	const int k = cluster[i];
	uint8_t *dst = raw + ((size_t)i * L + l0) * pl;
	for (int l = l0; l < l1; l++) {
		const int c0 = toff[l], M = toff[l + 1] - c0;
		const uint32_t *tab = fast_p ? thp + ((size_t)k * L + l) * SIM_PW : thp + (size_t)k * T + c0;
		for (int a = 0; a < pl; a++) *dst++ = (uint8_t)walk_search(tab, M, rng.next());
	}
}

/* random_allele_partition + the counts of the first M step (rnd_init.c:349-357,456-482) in one pass, nothing stored per copy.
 * Workgroup = 256 individuals x one locus chunk of the S-side pass (blockIdx.x; its loci taken `tile` at a time); thread =
 * individual i: copy (i, l, b) takes draw i*L*PL + l*PL + b of the stream, so the thread's draws for the chunk are consecutive
 * from x^(L*PL*i) * x^(lchunk*PL*blockIdx.x) on (k_jump_powers).  d[i][k][l][m] = 1 for every (allele m, cluster k) pair
 * some non-missing copy of the individual at the locus was given: the thread drops the repeats among its PL copies, then
 *   S side: one count per pair into its own packed 16-bit counters in LDS (at most lchunk*PL <= 65535), written as doubles
 *           to Spart[chunk][i][.] at the end -- what k_partition_individuals writes;
 *   N side: one LDS atomic per pair into the tile's packed 16-bit counters [column][KP] (at most 256 per workgroup), stored
 *           per tile into this workgroup's slab; k_partition_finish adds the slabs.  Integer counts: the order of the
 *           atomics does not matter, the sums are exact.
 * The genotype comes from gtS (the thread's 8 loci x PL bytes are one contiguous run).  KP = K rounded up to even. */
template <int PL>
__global__ __launch_bounds__(256) void k_partition_tile(rng_window base, const uint32_t *__restrict__ jump_i,
		const uint32_t *__restrict__ jump_r, int I, int L, int K, uint32_t magic, uint32_t shift, int lchunk, int tile,
		const int32_t *__restrict__ toff, const uint8_t *__restrict__ gtS, uint32_t *__restrict__ slabs, size_t slab_words,
		double *__restrict__ Spart)
{
	extern __shared__ uint32_t part_lds[];
	const int KP = (K + 1) & ~1;
	uint32_t *ring = part_lds, *scnt = part_lds + RNG_LAG * 256, *ncnt = scnt + (KP / 2) * 256;
	const int i = blockIdx.y * 256 + threadIdx.x;
	const bool live = i < I;
	const int l_begin = blockIdx.x * lchunk, l_end = L - l_begin < lchunk ? L : l_begin + lchunk;
	rng_ring rng(ring);
	if (live) {
		uint32_t w[RNG_LAG];
		rng_window_at(base, jump_r + (size_t)blockIdx.x * RNG_LAG, jump_i, (size_t)I, (size_t)i, w);
		rng.load(w);
	}
	for (int x = 0; x < KP / 2; x++) scnt[x * 256 + threadIdx.x] = 0;
	auto next = [&]() -> uint32_t {
		const uint32_t v = rng.next();
		return K == 1 ? 0u : v - (__umulhi(v, magic) >> shift) * (uint32_t)K;	/* rand() % K (k_draw_partition) */
	};
	uint32_t *slab = slabs + (size_t)blockIdx.y * slab_words;
	for (int t0 = l_begin; t0 < l_end; t0 += tile) {
		const int t1 = l_end - t0 < tile ? l_end : t0 + tile;
		const int col0 = toff[t0], nwords = (toff[t1] - col0) * (KP / 2);
		for (int x = threadIdx.x; x < nwords; x += 256) ncnt[x] = 0;
		__syncthreads();
		if (live)
			for (int g = t0 >> 3; g * 8 < t1; g++) {
				unsigned long long run[PL];
				{
					const unsigned long long *src = reinterpret_cast<const unsigned long long *>(gtS + (((size_t)g * I + i) * 8) * PL);
#pragma unroll
					for (int x = 0; x < PL; x++) run[x] = src[x];
				}
#pragma unroll
				for (int t = 0; t < 8; t++) {
					const int l = g * 8 + t;
					if (l < t1) {		/* uniform */
						const int cl = toff[l] - col0;
						uint32_t key[PL];
#pragma unroll
						for (int b = 0; b < PL; b++) {
							const int at = t * PL + b;
							const uint32_t mb = (uint32_t)(run[at >> 3] >> (8 * (at & 7))) & 0xFFu;
							const uint32_t kb = next();
							key[b] = mb | (kb << 8);
							bool count = mb != MCHIP_MISSING;
#pragma unroll
							for (int b2 = 0; b2 < b; b2++) count = count && key[b2] != key[b];
							if (count) {
								scnt[(kb >> 1) * 256 + threadIdx.x] += 1u << (16 * (kb & 1u));
								const uint32_t en = (uint32_t)(cl + (int)mb) * (uint32_t)KP + kb;
								atomicAdd(&ncnt[en >> 1], 1u << (16 * (en & 1u)));
							}
						}
					}
				}
			}
		__syncthreads();
		uint32_t *dst = slab + (size_t)col0 * (KP / 2);
		for (int x = threadIdx.x; x < nwords; x += 256) dst[x] = ncnt[x];
		__syncthreads();
	}
	if (live) {
		double *out = Spart + ((size_t)blockIdx.x * I + i) * K;
		for (int k = 0; k < K; k++) out[k] = (double)((scnt[(k >> 1) * 256 + threadIdx.x] >> (16 * (k & 1))) & 0xFFFFu);
	}
}

/* Apart[0][c][k] = sum over the workgroup slabs of k_partition_tile; thread = (c, k) */
__global__ void k_partition_finish(const uint32_t *__restrict__ slabs, size_t slab_words, int n_slabs, int T, int K, double *Apart)
{
	const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= (size_t)T * K) return;
	const int k = (int)(idx % K);
	const size_t c = idx / K;
	const int KP = (K + 1) & ~1;
	const size_t en = c * KP + k;
	unsigned sum = 0;
	for (int b = 0; b < n_slabs; b++) sum += (slabs[(size_t)b * slab_words + (en >> 1)] >> (16 * (en & 1))) & 0xFFFFu;
	Apart[idx] = (double)sum;
}

/* out = (a * b) mod (x^31 - x^28 - 1) over Z/2^32; out may be a or b */
static void rng_polymul(const uint32_t *a, const uint32_t *b, uint32_t *out)
{
	uint32_t t[2 * RNG_LAG - 1];
	rng_polymul_wide(a, b, t);
	memcpy(out, t, RNG_LAG * sizeof(uint32_t));
}

/* tables of x^(lo*CHUNK), lo < 256 (stored [31][256]) and x^(hi*256*CHUNK), hi < n_hi (stored [n_hi][31]) */
static int rng_jump_tables(mchip_context *ctx, size_t n_hi)
{
	if (ctx->d_jump_lo && ctx->n_jump_hi >= n_hi) return MCHIP_OK;
	dfree(ctx->d_jump_hi);
	dfree(ctx->d_jump_lo);
	ctx->n_jump_hi = 0;
	uint32_t step[RNG_LAG] = {0}, sq[RNG_LAG] = {0}, cur[RNG_LAG];
	step[0] = 1;	/* x^0 */
	sq[1] = 1;	/* x^1 */
	for (unsigned e = RNG_CHUNK; e; e >>= 1) {	/* step = x^CHUNK */
		if (e & 1) rng_polymul(step, sq, step);
		rng_polymul(sq, sq, sq);
	}
	std::vector<uint32_t> lo((size_t)RNG_LAG * 256), hi(n_hi * RNG_LAG);
	memset(cur, 0, sizeof cur);
	cur[0] = 1;
	for (int x = 0; x < 256; x++) {
		for (int j = 0; j < RNG_LAG; j++) lo[(size_t)j * 256 + x] = cur[j];
		rng_polymul(cur, step, cur);
	}
	memcpy(step, cur, sizeof step);	/* x^(256*CHUNK) */
	memset(cur, 0, sizeof cur);
	cur[0] = 1;
	for (size_t x = 0; x < n_hi; x++) {
		memcpy(&hi[x * RNG_LAG], cur, sizeof cur);
		rng_polymul(cur, step, cur);
	}
	HIPCHK(hipMalloc((void **)&ctx->d_jump_lo, lo.size() * sizeof(uint32_t)));
	HIPCHK(hipMalloc((void **)&ctx->d_jump_hi, hi.size() * sizeof(uint32_t)));
	HIPCHK(hipMemcpy(ctx->d_jump_lo, lo.data(), lo.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
	HIPCHK(hipMemcpy(ctx->d_jump_hi, hi.data(), hi.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
	ctx->n_jump_hi = n_hi;
	return MCHIP_OK;
}

static int rng_stream_setup(mchip_context *ctx, const uint32_t *window, size_t n_draws, rng_window *base, size_t *n_chunks, size_t *n_blocks)
{
	*n_chunks = (n_draws + RNG_CHUNK - 1) / RNG_CHUNK;
	*n_blocks = (*n_chunks + 255) / 256;
	*base = rng_window_from(window);
	return rng_jump_tables(ctx, *n_blocks);
}

/* x^e mod (x^31 - x^28 - 1) */
static void rng_xpow(uint64_t e, uint32_t *out)
{
	uint32_t acc[RNG_LAG] = {0}, sq[RNG_LAG] = {0};
	acc[0] = 1;
	sq[1] = 1;
	for (; e; e >>= 1) {
		if (e & 1) rng_polymul(acc, sq, acc);
		rng_polymul(sq, sq, sq);
	}
	memcpy(out, acc, sizeof acc);
}

/* d_out[j * sj + n * sn] = coefficient j of x^(A*n), n < count */
static int rng_lattice_table(mchip_context *ctx, uint64_t A, unsigned count, size_t sj, size_t sn, uint32_t *d_out)
{
	uint32_t pw[32 * RNG_LAG];
	rng_xpow(A, pw);
	for (int b = 1; b < 32; b++) rng_polymul(pw + (b - 1) * RNG_LAG, pw + (b - 1) * RNG_LAG, pw + b * RNG_LAG);
	scoped_dev<uint32_t> d_pw;
	HIPCHK(d_pw.alloc(32 * RNG_LAG));
	HIPCHK(hipMemcpyAsync(d_pw, pw, sizeof pw, hipMemcpyHostToDevice, ctx->stream));
	hipLaunchKernelGGL(k_jump_powers, dim3(nblk(count)), dim3(256), 0, ctx->stream, d_pw.p, count, sj, sn, d_out);
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(ctx->stream));
	return MCHIP_OK;
}

/* jump polynomials of a tiled generator (see mchip_context::lat): thread (i, r) starts A*i + B*r draws into the stream */
static int lattice_tables(mchip_context *ctx, int which, uint64_t A, unsigned nA, uint64_t B, unsigned nB)
{
	mchip_context::lattice &t = ctx->lat[which];
	if (t.d_i && t.A == A && t.nA == nA && t.B == B && t.nB == nB) return MCHIP_OK;
	dfree(t.d_i);
	dfree(t.d_r);
	t.nA = 0;
	HIPCHK(hipMalloc((void **)&t.d_i, (size_t)RNG_LAG * nA * sizeof(uint32_t)));
	HIPCHK(hipMalloc((void **)&t.d_r, (size_t)RNG_LAG * nB * sizeof(uint32_t)));
	int rc = rng_lattice_table(ctx, A, nA, (size_t)nA, 1, t.d_i);
	if (!rc) rc = rng_lattice_table(ctx, B, nB, 1, RNG_LAG, t.d_r);
	if (rc) return rc;
	t.A = A; t.nA = nA; t.B = B; t.nB = nB;
	return MCHIP_OK;
}

/* v % K through floor(v / K) = (v * magic) >> (31 + l), l = ceil(log2 K), magic = ceil(2^(31+l) / K) < 2^32: exact for every
 * v < 2^31 (division by an invariant integer); the kernels take the high word, so shift = l - 1.  K >= 2. */
static void mod_k_magic(int K, uint32_t *magic, uint32_t *shift)
{
	uint32_t l = 0;
	while ((1u << l) < (uint32_t)K) l++;
	const uint64_t pw = (uint64_t)1 << (31 + l);
	*magic = (uint32_t)((pw + (uint64_t)K - 1) / (uint64_t)K);
	*shift = l - 1;
}

int draw_mod_stream(mchip_context *ctx, const uint32_t *window, size_t n_draws, int m, uint8_t *d_out)
{
	rng_window base;
	size_t n_chunks, n_blocks;
	const int rc = rng_stream_setup(ctx, window, n_draws, &base, &n_chunks, &n_blocks);
	if (rc) return rc;
	if (m == 1) {
		HIPCHK(hipMemsetAsync(d_out, 0, n_chunks * RNG_CHUNK, ctx->stream));	/* rand() % 1 */
		return MCHIP_OK;
	}
	uint32_t magic, shift;
	mod_k_magic(m, &magic, &shift);
	hipLaunchKernelGGL(k_draw_partition, dim3((unsigned)n_blocks), dim3(256), 0, ctx->stream, base, ctx->d_jump_hi, ctx->d_jump_lo,
			   n_chunks, (uint32_t)m, magic, shift, (uint32_t *)d_out);
	HIPCHK(hipGetLastError());
	return MCHIP_OK;
}

void drop_generators(mchip_context *ctx)
{
	dfree(ctx->d_jump_hi); dfree(ctx->d_jump_lo);
	ctx->n_jump_hi = 0;
	for (int x = 0; x < 2; x++) { dfree(ctx->lat[x].d_i); dfree(ctx->lat[x].d_r); ctx->lat[x].nA = 0; }
	dfree(ctx->d_part_slabs);
	ctx->part_slab_bytes = 0;
	dfree(ctx->d_sim_cluster);
}

extern "C" {

/* the tiled form of the random partition + first M step (k_partition_tile); returns -1 when the shape does not fit it */
static int rand_partition_tiled(mchip_context *ctx, const uint32_t *window, int to)
{
	const int K = ctx->K, KP = (K + 1) & ~1, pl = ctx->ploidy;
	if (pl > 8 || (size_t)ctx->geo.lchunk * pl > 65535 || ctx->knob.part_no_tile) return -1;
	/* N-side counters of a tile: tile * max_M * KP / 2 words, about 16 KiB, a multiple of 8 loci */
	int tile = (int)((16384 / ((size_t)ctx->max_M * KP * 2)) & ~(size_t)7);
	if (tile < 8) tile = 8;
	if (tile > ctx->geo.lchunk) tile = ctx->geo.lchunk;
	const size_t lds = ((size_t)RNG_LAG * 256 + (size_t)(KP / 2) * 256 + (size_t)tile * ctx->max_M * (KP / 2)) * sizeof(uint32_t);
	if (lds > 64 * 1024) return -1;
	int rc;
	const rng_window base = rng_window_from(window);
	if ((rc = lattice_tables(ctx, 1, (uint64_t)ctx->L * pl, (unsigned)ctx->I, (uint64_t)ctx->geo.lchunk * pl, (unsigned)ctx->geo.n_lchunks))) return rc;
	const size_t slab_words = (size_t)ctx->T * (KP / 2), n_slabs = (size_t)(ctx->I + 255) / 256;
	HIPCHK(grow_dev(ctx, &ctx->d_part_slabs, &ctx->part_slab_bytes, n_slabs * slab_words * sizeof(uint32_t)));
	uint32_t magic = 0, shift = 0;
	if (K > 1) mod_k_magic(K, &magic, &shift);
	const uint8_t *gtS = ctx->init_geno_set ? ctx->d_initS : ctx->d_gtS;	/* bootstrap fits: the observed haplotypes (rnd_init.c:471) */
	with_ploidy(pl, [&](auto PL) {
		hipLaunchKernelGGL(k_partition_tile<PL()>, dim3((unsigned)ctx->geo.n_lchunks, nblk((size_t)ctx->I)), dim3(256), lds, ctx->stream, base,
				   ctx->lat[1].d_i, ctx->lat[1].d_r, ctx->I, ctx->L, K, magic, shift, ctx->geo.lchunk, tile, ctx->d_toff, gtS, ctx->d_part_slabs,
				   slab_words, ctx->d_Spart);
	});
	HIPCHK(hipGetLastError());
	hipLaunchKernelGGL(k_partition_finish, dim3(nblk((size_t)ctx->T * K)), dim3(256), 0, ctx->stream, ctx->d_part_slabs, slab_words,
			   (int)n_slabs, ctx->T, K, ctx->d_Apart);
	HIPCHK(hipGetLastError());
	return partition_finalize(ctx, to, 0, 1);
}

int mchip_mstep_from_rand_partition(mchip_context *ctx, const uint32_t *window, int to)
{
	MCHIP_ENTRY();
	int rc = check_partition_call(ctx, window, to);
	if (rc) return rc;
	HIPCHK(hipSetDevice(ctx->device));
	if ((rc = rand_partition_tiled(ctx, window, to)) >= 0) return rc;
	const size_t n = (size_t)ctx->I * ctx->L * ctx->ploidy;
	if ((rc = stream_buffer(ctx))) return rc;
	if ((rc = draw_mod_stream(ctx, window, n, ctx->K, ctx->d_draw))) return rc;
	return partition_mstep(ctx, ctx->d_draw, to);
}

int mchip_simulate_genotypes(mchip_context *ctx, int I, int L, int ploidy, const int32_t *ua, const uint32_t *window,
			     int K, int eta_constrained, const double *q, const double *p)
{
	MCHIP_ENTRY();
	if (!ctx) return MCHIP_ERR_INVALID;
	if (!window || !q || !p || K < 1) return fail(ctx, MCHIP_ERR_INVALID, "simulate_genotypes: null pointer or K < 1%s", nullptr);
	/* a replicate of the same observed data: the observed haplotypes installed by mchip_set_init_genotypes stay in force
	 * (the reference's dat->IL stays in place across parametric_bootstrap calls, bootstrap.c:35-41) */
	int rc = set_shape(ctx, I, L, ploidy, ua, KEEP_INIT);
	if (rc) return rc;
	set_empty_rows(ctx, {});	/* every copy of a generated data set is drawn */
	const size_t n_copies = (size_t)I * L * ploidy;
	rng_window base;
	size_t n_chunks, n_blocks;
	if ((rc = rng_stream_setup(ctx, window, 2 * n_copies, &base, &n_chunks, &n_blocks))) return rc;
	const size_t n_qrows = eta_constrained ? 1 : (size_t)I, nq = n_qrows * K, np = (size_t)K * ctx->T;
	const int fast = K <= SIM_QW && ctx->max_M <= SIM_PW;
	const size_t ncq = n_qrows * (fast ? SIM_QW : K), ncp = fast ? (size_t)K * L * SIM_PW : np;
	scoped_dev<double> d_q, d_p;
	scoped_dev<uint32_t> d_cq, d_cp;
	HIPCHK(d_q.alloc(nq));
	HIPCHK(d_p.alloc(np));
	HIPCHK(d_cq.alloc(ncq));
	HIPCHK(d_cp.alloc(ncp));
	HIPCHK(hipMemcpyAsync(d_q, q, nq * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(hipMemcpyAsync(d_p, p, np * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	{
		const size_t n = n_qrows > (size_t)K * L ? n_qrows : (size_t)K * L;
		hipLaunchKernelGGL(k_walk_tables, dim3(nblk(n)), dim3(256), 0, ctx->stream, (int)n_qrows, K, L, ctx->T, ctx->d_toff, d_q.p, d_p.p,
				   fast, fast, d_cq.p, d_cp.p);
	}
	if (fast && ploidy <= 8 && !ctx->knob.sim_no_tile) {
		const int tile = sim_tile_loci(K, L);
		if ((rc = lattice_tables(ctx, 0, 2ull * (uint64_t)L * ploidy, (unsigned)I, 2ull * (uint64_t)tile * ploidy, (unsigned)((L + tile - 1) / tile))))
			return rc;
		with_ploidy(ploidy, [&](auto PL) {
			launch_sim_tile(ctx, k_simulate_tile<PL()>, base, K, tile, d_cq.p, eta_constrained ? 0 : 1, d_cp.p);
		});
		return sim_install(ctx, nullptr);
	}
	if ((rc = stream_buffer(ctx))) return rc;	/* n_chunks * RNG_CHUNK / 2 <= its size */
	uint8_t *d_raw = ctx->d_draw;
	if (fast)
		hipLaunchKernelGGL(k_simulate_admixture<true>, dim3((unsigned)n_blocks), dim3(256), 0, ctx->stream, base, ctx->d_jump_hi,
				   ctx->d_jump_lo, n_chunks, I, L, ploidy, K, ctx->T, ctx->d_toff, d_cq.p, eta_constrained ? 0 : 1, d_cp.p,
				   (uint32_t *)d_raw);
	else
		hipLaunchKernelGGL(k_simulate_admixture<false>, dim3((unsigned)n_blocks), dim3(256), 0, ctx->stream, base, ctx->d_jump_hi,
				   ctx->d_jump_lo, n_chunks, I, L, ploidy, K, ctx->T, ctx->d_toff, d_cq.p, eta_constrained ? 0 : 1, d_cp.p,
				   (uint32_t *)d_raw);
	return sim_install(ctx, d_raw);
}

/* The mixture model's generator.  Dispatch: tile form (k_simulate_mixture_tile) when no locus has more than SIM_PW alleles and
 * ploidy <= 8, at every K; otherwise, and under MCHIP_SIM_NO_TILE, the general form (k_simulate_mixture_general) in chunks of
 * MIX_GENERAL_CHUNK loci.  Both follow k_simulate_mixture_source, which leaves every individual's cluster in d_sim_cluster.
 * K <= 256: the cluster is a byte.  (As in mchip_simulate_genotypes, a HIPCHK that returns after the asynchronous uploads frees the
 * scoped buffers without waiting for the stream; the runtime's hipFree synchronises, and the call has failed anyway.) */
constexpr int MIX_GENERAL_CHUNK = 64;

int mchip_simulate_genotypes_mixture(mchip_context *ctx, int I, int L, int ploidy, const int32_t *ua, const uint32_t *window,
				     int K, const double *eta, const double *p)
{
	MCHIP_ENTRY();
	if (!ctx) return MCHIP_ERR_INVALID;
	if (!window || !eta || !p || K < 1) return fail(ctx, MCHIP_ERR_INVALID, "simulate_genotypes_mixture: null pointer or K < 1%s", nullptr);
	if (K > 256) return fail(ctx, MCHIP_ERR_INVALID, "simulate_genotypes_mixture: more than 256 clusters%s", nullptr);
	int rc = set_shape(ctx, I, L, ploidy, ua, KEEP_INIT);
	if (rc) return rc;
	set_empty_rows(ctx, {});	/* every copy of a generated data set is drawn */
	/* at the first draw (the first individual's cluster); one draw on (its first copy) */
	const rng_window base = rng_window_from(window), base1 = rng_window_from(base.s + 1);
	const size_t np = (size_t)K * ctx->T;
	const int fast_p = ctx->max_M <= SIM_PW;
	const int tiled = fast_p && ploidy <= 8 && !ctx->knob.sim_no_tile;
	const size_t ncp = fast_p ? (size_t)K * L * SIM_PW : np;
	scoped_dev<double> d_q, d_p;
	scoped_dev<uint32_t> d_cq, d_cp;
	HIPCHK(d_q.alloc((size_t)K));
	HIPCHK(d_p.alloc(np));
	HIPCHK(d_cq.alloc((size_t)K));
	HIPCHK(d_cp.alloc(ncp));
	if (!ctx->d_sim_cluster) HIPCHK(hipMalloc((void **)&ctx->d_sim_cluster, (size_t)I));
	HIPCHK(hipMemcpyAsync(d_q, eta, (size_t)K * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(hipMemcpyAsync(d_p, p, np * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	hipLaunchKernelGGL(k_walk_tables, dim3(nblk((size_t)K * L)), dim3(256), 0, ctx->stream, 1, K, L, ctx->T, ctx->d_toff, d_q.p, d_p.p,
			   0, fast_p, d_cq.p, d_cp.p);
	HIPCHK(hipGetLastError());
	const int chunk = tiled ? sim_tile_loci(K, L) : MIX_GENERAL_CHUNK;
	const unsigned n_chunks = (unsigned)((L + chunk - 1) / chunk);
	if ((rc = lattice_tables(ctx, 0, 1ull + (uint64_t)L * ploidy, (unsigned)I, (uint64_t)chunk * ploidy, n_chunks))) return rc;
	hipLaunchKernelGGL(k_simulate_mixture_source, dim3(nblk((size_t)I)), dim3(256), 0, ctx->stream, base, ctx->lat[0].d_i, ctx->lat[0].d_r, I, K,
			   d_cq.p, ctx->d_sim_cluster);
	HIPCHK(hipGetLastError());
	if (tiled) {
		with_ploidy(ploidy, [&](auto PL) {
			launch_sim_tile(ctx, k_simulate_mixture_tile<PL()>, base1, K, chunk, ctx->d_sim_cluster, d_cp.p);
		});
		return sim_install(ctx, nullptr);
	}
	if ((rc = stream_buffer(ctx))) return rc;
	hipLaunchKernelGGL(k_simulate_mixture_general, dim3(n_chunks, nblk((size_t)I)), dim3(256), 0, ctx->stream, base1, ctx->lat[0].d_i,
			   ctx->lat[0].d_r, I, L, ploidy, ctx->T, chunk, ctx->d_toff, ctx->d_sim_cluster, d_cp.p, fast_p, ctx->d_draw);
	return sim_install(ctx, ctx->d_draw);
}

}	/* extern "C" */
