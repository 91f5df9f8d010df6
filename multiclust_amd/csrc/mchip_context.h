/*
 * mchip_context.h -- the per-context state of libmulticlust_hip.so and what its host-side units call of one another: the units of
 * the core (mchip.hip the context, the install path and the model; mchip_plan.hip geometry and plan; mchip_em.hip the EM step;
 * mchip_accel.hip; mchip_init.hip; mchip_profile.hip) and the units holding a data-set feature's kernels and entry points
 * (mchip_bed.hip, mchip_cv.hip, mchip_divergence.hip, mchip_generators.hip, mchip_impute.hip, mchip_pca.hip, mchip_query.hip, mchip_resample.hip, mchip_residuals.hip, mchip_kinship.hip).
 * Private to those units; not part of the C-ABI, and mchip_kernels_k.hip does not include it.
 */
#ifndef MCHIP_CONTEXT_H
#define MCHIP_CONTEXT_H

#include "mchip_internal.h"
#include "mchip_feature_geometry.h"
#include "mchip_progress.h"

#include <cstddef>
#include <functional>
#include <type_traits>
#include <stdio.h>
#include <string.h>

constexpr int RNG_LAG = 31;
constexpr int RNG_CHUNK = 4 * RNG_LAG * 32;	/* draws (= bytes written) per thread: 32 rounds of 31 packed words */

/* a data set kept beside the installed one, in upload form [I][L][ploidy] (I and ploidy are the installed data set's) */
struct saved_set {
	uint8_t *d_raw = nullptr;	/* null = none saved */
	int L = 0;
	std::vector<int32_t> ua;	/* its uniquealleles */
	std::vector<int> empty;		/* its empty_rows */
};

/* testing / tuning knobs of the environment (README) */
struct mchip_knobs {
	int no_bial, no_counts, force_dense, force_safe, no_graph, no_dual, no_slab_sum, no_col_split, part_no_tile, sim_no_tile;
	int no_fused_finalize, no_pair;
	int kin_two_launches;		/* mchip_kinship_products: its two products a chunk as two launches (the same bits) */
	int per_cu_col, per_cu_ind, geometry_given, no_roundup;
	double slab_frac;
};

/* launch geometry of a model on a data set (mchip_plan.hip: model_geometry) */
struct mchip_geometry {
	int ichunk, n_ichunks, lchunk, n_lchunks, n_llpart, flush_blocks, safe_rcp, sparse;
	int ind_waves;			/* waves per workgroup of the cooperating individual-side kernels (mchip_internal.h) */
	int xcd_rows;			/* their slab rows come in whole groups of eight: one row, one XCD */
};

/* what a data set's shape is to the launch geometry and the plan */
struct mchip_shape { int I, L, T, ploidy, min_M, max_M, count_bits; };

/* the finalisers behind an E step's passes: both in one launch (k_finalize_qp: an M step with individual mixing proportions whose P
 * side takes the tiled form), or k_finalize_q and the P side's, the latter behind k_sum_slabs where the column pass left many slabs */
struct estep_finish { int p_loci; bool slab_sum, fused; };

/* The small results of the device code, one allocation per context (d_scalars): every field has one use and shares storage with
 * no other, so which launch runs before which decides nothing here.  Kernels are handed the record or &rec->field. */
struct mchip_scalars {
	double logL;			/* log likelihood of the last E step (k_stop_check, mchip_last_loglik) */
	double emll;			/* of the second EM iterate of a cycle; of mchip_loglik */
	double ll_point;		/* of the extrapolated point of a cycle; of mchip_loglik_prefetch (with s_cache_slot) */
	double step;			/* step size of a batched cycle (step_size_body -> k_accel_update_slots) */
	/* up to three dot products: their eta parts from [DOT_ETA] on, their p parts from [DOT_P] on; one array, because dots_common
	 * fetches the eight doubles in one copy */
	double dots[8];
	double eta_sums[MCHIP_MAX_K];	/* column sums of S_ik under shared mixing proportions: k_column_sums runs K blocks */
	unsigned long long cells[2];	/* mchip_data_counts: cells with n_ic > 0, non-missing allele copies */
	int bad_input;			/* the layout kernels' "bad input" word (bad_flag) */
};
static_assert(std::is_standard_layout<mchip_scalars>::value && std::is_trivially_copyable<mchip_scalars>::value, "copied with hipMemcpy");
static_assert(sizeof(mchip_scalars::eta_sums) == MCHIP_MAX_K * sizeof(double), "k_column_sums writes one sum per cluster");
static_assert(offsetof(mchip_scalars, cells) % alignof(unsigned long long) == 0 && offsetof(mchip_scalars, bad_input) % alignof(int) == 0,
	      "the kernels update the counts as 64-bit words and the bad-input word as a 32-bit one");

enum { DOT_ETA = 0, DOT_P = 4 };

/* what a batched accelerated cycle decides on the device (d_cyc) */
struct mchip_cycle_flags {
	int no_update;			/* the reference would leave this cycle without an update (step_size_body) */
	int accepted;			/* the extrapolated point was accepted: Spart holds its S-side sums for the next cycle's first E step */
};

/* The block partials of the dot products in d_redpart: up to three sums of at most DOT_MAX_BLOCKS partials for the eta part,
 * then as many for the p part.  A block of k_dots / k_dots_slots covers 4096 elements, or more once the cap is reached. */
constexpr int DOT_MAX_BLOCKS = 512, DOT_MAX_SUMS = 3;
constexpr size_t DOT_PARTIALS = (size_t)2 * DOT_MAX_SUMS * DOT_MAX_BLOCKS;
static inline int dot_blocks(size_t n) { const size_t g = (n + 4095) / 4096; return g > DOT_MAX_BLOCKS ? DOT_MAX_BLOCKS : (int)g; }
static inline double *dot_part_eta(double *redpart) { return redpart; }
static inline double *dot_part_p(double *redpart) { return redpart + (size_t)DOT_MAX_SUMS * DOT_MAX_BLOCKS; }

struct mchip_context {
	int device;
	hipStream_t stream;
	char err[512];
	int n_cu;
	/* data set */
	int I, L, ploidy, T, max_M, min_M;
	std::vector<int32_t> h_ua;	/* host copy of uniquealleles: a data set of the same shape reuses every buffer */
	int parked_K;			/* model buffers kept allocated for this K (and the signature below) while no model is set */
	int sig_admixture, sig_constrained, sig_projection, sig_nsec;
	double sig_eta_lb, sig_p_lb;
	int init_geno_set;		/* d_initA / d_initS hold the observed haplotypes (mchip_set_init_genotypes) */
	int32_t *d_ua, *d_toff, *d_col_locus;
	uint8_t *d_col_allele;
	uint8_t *d_gtA, *d_gtS, *d_gtC;
	int count_bits, has_missing;
	int first_empty;	/* first individual without a single observed copy, or -1 */
	std::vector<int> empty_rows;	/* all of them: their mixing proportions are 0 / 0 in the reference (em_alg.c:685-690) */
	int empty_rows_nan[3];	/* per slot: the slot's rows of such individuals stand for the reference's 0 / 0 (an M step wrote the slot, or
				 * something computed from such a slot did, or NaN rows were uploaded): mchip_get_q reports them as NaN */
	unsigned long long nnz_cells, n_copies;	/* cells with n_ic > 0, non-missing allele copies (mchip_data_counts) */
	int counts_valid;
	size_t geno_bytes_A, geno_bytes_S;
	uint8_t *d_asA, *d_asS;		/* hard-partition scratch, allocated on first use */
	uint8_t *d_initA, *d_initS;	/* genotype the hard-partition M step reads when it is not the data set itself (bootstrap) */
	uint8_t *d_draw;		/* device-drawn partition in stream order [I][L][ploidy], padded to whole chunks */
	/* K-fold cross-validation (mchip_cv.hip): state of the data set, dropped with it */
	uint8_t *d_cv_fold;		/* fold of every genotype [I][L], padded to whole generator chunks + CV_PAD; null = no folds */
	int cv_n_folds;
	saved_set cv_full;		/* the full data set, saved by the first hold-out */
	int cv_fold;			/* fold held out of the installed data set, -1 = none */
	double *d_cv_part;		/* the score's partial sums, one per workgroup */
	size_t cv_part_cap;
	unsigned long long *d_cv_out;	/* [0] the score's sum (a double), [1] copies, [2] floored copies */
	/* selections of loci (mchip_resample.hip): the base they are gathered from, saved by the first one and dropped by every other
	 * call that installs a data set */
	saved_set rs_base;
	/* Rand-EM candidates (mchip_init_from_allele_centers), kept from one candidate to the next and grown when needed: the
	 * rand() % K values of a candidate's span of the stream, its center alleles [L][K], its per-locus draw offsets */
	uint8_t *d_cand_span, *d_cand_centers;
	unsigned long long *d_cand_off;
	size_t cand_span_bytes, cand_loci, cand_center_bytes;
	uint32_t *d_jump_hi, *d_jump_lo;	/* jump polynomials of the rand() stream (mchip_mstep_from_rand_partition) */
	size_t n_jump_hi;
	/* jump polynomials of the tiled generators (0: bootstrap data set, 1: random partition): x^(A*i), i < nA, stored [31][nA]
	 * (one per individual) and x^(B*r), r < nB, stored [nB][31] (one per locus tile); kept while A, nA, B, nB stay the same */
	struct lattice { uint32_t *d_i, *d_r; uint64_t A, B; unsigned nA, nB; } lat[2];
	uint32_t *d_part_slabs;		/* tiled random partition: packed 16-bit N-side counts per block of 256 individuals */
	size_t part_slab_bytes;
	/* mixture model on generated data: the cluster of every individual of the data set (mchip_simulate_genotypes_mixture), and the
	 * workspaces of mchip_init_from_individual_centers (partial distances [chunk][K][I]; counts [T][K], n_k, centers, assignment) */
	uint8_t *d_sim_cluster;
	uint32_t *d_cen_part, *d_cen_work;
	size_t cen_part_bytes, cen_work_bytes;
	/* model */
	int K, admixture, constrained, do_projection, nsec, nq, qstride;
	double eta_lb, p_lb;
	const mchip_ktable *kt;
	double *d_p[3], *d_q[3];
	double *d_up[MCHIP_MAX_SECANTS], *d_vp[MCHIP_MAX_SECANTS], *d_uq[MCHIP_MAX_SECANTS], *d_vq[MCHIP_MAX_SECANTS];
	double *d_sik;			/* [I][K] expected counts / vik */
	double *d_stage;		/* K*T staging for the [K][T] <-> [T][K] transposes */
	double *d_logp;			/* mixture model: log P table [T][K] */
	/* workspaces */
	mchip_geometry geo;
	/* read when a context is created and again with every data set and every model -- never on a launch path */
	mchip_knobs knob;
	double *d_Apart, *d_Spart, *d_llpart;
	mchip_scalars *d_scalars;
	double *d_llpart2;		/* partial log likelihoods of the second parameter set of a dual individual pass */
	double *d_redpart;		/* block partials of the dot products: DOT_PARTIALS doubles (dot_part_eta, dot_part_p) */
	uint8_t *d_flags;		/* michelot "fixed" flags for loci with more than 64 alleles */
	double *h_pinned;		/* sizeof(mchip_scalars) bytes: room for any fetch of its doubles (fetch_scalars) */
	mchip_run_state *d_run;		/* batched-run state (mchip_em_run) */
	hipGraphExec_t step_graph[3];	/* one captured {EM step + stop check} per slot; rebuilt when the model changes */
	hipGraphExec_t cycle_graph[3][5];	/* one captured accelerated cycle per (start slot, scheme) */
	mchip_cycle_flags *d_cyc;	/* batched accelerated runs */
	int have_ll;
	int ll_parts;			/* partial log likelihoods the last E step left in d_llpart */
	int s_cache_slot;		/* slot whose S-side sums + logL are held in Spart / d_scalars->ll_point (mchip_loglik_prefetch), or -1 */
	/* profiling */
	int profiling;
	hipEvent_t ev_begin, ev_end;
	std::vector<hipEvent_t> ev_pool;
	std::vector<int> ev_kind;	/* kernel kind of pair p = events 2p, 2p+1 */
	size_t ev_used;
	/* profiled paired E steps (k_estep_pair; mchip_profile.hip: k_pair_spans): two clock readings per block of the latest such launch, and
	 * one span per launch since mchip_profile_begin, in allocations of a fixed number of spans */
	unsigned long long *d_pair_marks;
	size_t pair_marks_cap;		/* blocks d_pair_marks has room for */
	std::vector<mchip_pair_span *> pair_spans;
	size_t pair_used;
};

static int fail(mchip_context *ctx, int code, const char *fmt, const char *detail)
{
	if (ctx) snprintf(ctx->err, sizeof ctx->err, fmt, detail ? detail : "");
	return code;
}

#define HIPCHK(call)                                                                                  \
	do {                                                                                          \
		hipError_t e_ = MCHIP_WAIT(call);                                                     \
		if (e_ != hipSuccess) {                                                               \
			snprintf(ctx->err, sizeof ctx->err, "%s failed: %s (%s:%d)", #call,           \
				 hipGetErrorString(e_), __FILE__, __LINE__);                          \
			return MCHIP_ERR_HIP;                                                         \
		}                                                                                     \
	} while (0)

template <typename Tp> static void dfree(Tp *&p)
{
	if (p) (void)MCHIP_WAIT(hipFree(p));
	p = nullptr;
}

/* temporary device allocation released on every exit path of the function that owns it */
template <typename Tp> struct scoped_dev {
	Tp *p = nullptr;
	scoped_dev() = default;
	scoped_dev(const scoped_dev &) = delete;
	scoped_dev &operator=(const scoped_dev &) = delete;
	~scoped_dev() { if (p) (void)MCHIP_WAIT(hipFree(p)); }
	hipError_t alloc(size_t count) { return hipMalloc((void **)&p, count * sizeof(Tp)); }
	operator Tp *() const { return p; }
};

/* a buffer kept in the context from one call to the next, grown when a call needs more: nothing happens while it is large enough
 * (a hipFree waits for the whole device, i.e. for every other stream's fits); otherwise the stream is drained, the buffer freed
 * and one of want_bytes allocated.  On failure the buffer is gone and *have_bytes is 0. */
template <typename Tp> static hipError_t grow_dev(mchip_context *ctx, Tp **p, size_t *have_bytes, size_t want_bytes)
{
	if (*have_bytes >= want_bytes) return hipSuccess;
	if (*p) { (void)MCHIP_WAIT(hipStreamSynchronize(ctx->stream)); (void)MCHIP_WAIT(hipFree(*p)); *p = nullptr; *have_bytes = 0; }
	const hipError_t e = hipMalloc((void **)p, want_bytes);
	if (e == hipSuccess) *have_bytes = want_bytes;
	return e;
}

/* f(std::integral_constant<int, PL>) for the kernels instantiated per ploidy 1..8 (the callers have checked pl <= 8) */
template <typename F> static void with_ploidy(int pl, F &&f)
{
	switch (pl) {
	case 1: f(std::integral_constant<int, 1>()); break;
	case 2: f(std::integral_constant<int, 2>()); break;
	case 3: f(std::integral_constant<int, 3>()); break;
	case 4: f(std::integral_constant<int, 4>()); break;
	case 5: f(std::integral_constant<int, 5>()); break;
	case 6: f(std::integral_constant<int, 6>()); break;
	case 7: f(std::integral_constant<int, 7>()); break;
	default: f(std::integral_constant<int, 8>()); break;
	}
}

static inline unsigned nblk(size_t n, unsigned b = 256) { return (unsigned)((n + b - 1) / b); }
/* for the kernels with a grid-stride loop: at most cap_blocks blocks; 0 = the layout kernels' 2^30 work-items per launch */
static inline unsigned nblk_capped(size_t n, unsigned b = 256, size_t cap_blocks = 0)
{
	const size_t blocks = (n + b - 1) / b, cap = cap_blocks ? cap_blocks : ((size_t)1 << 30) / b;
	return (unsigned)(blocks < cap ? blocks : cap);
}

/* the "bad input" word of the layout kernels lives in the context's scalars, so that an initialisation allocates and frees
 * nothing (hipFree waits for the whole device, i.e. for every other stream's fits) */
static int *bad_flag(mchip_context *ctx) { return &ctx->d_scalars->bad_input; }

/* ---- PLINK 1 packed records on the device: what the units that read them share (mchip_bed.hip, mchip_pca.hip) ---- */
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

/* a tile of BT_L records x BT_I individuals into LDS: the 64 bytes from byte i0 / 4 of the records l0 ... l0 + BT_L - 1 as 16 dwords
 * each, BT_ROW dwords apart; 0 behind the record's last byte and for the records behind the last.  All 256 lanes; the caller syncs. */
__device__ __forceinline__ void bed_stage_tile(uint32_t *tile, const uint8_t *__restrict__ bed, size_t rb, int L, int l0, int i0)
{
	const size_t b0 = (size_t)(i0 / 4);	/* first staged byte of every record */
	for (int x = threadIdx.x; x < BT_L * 16; x += 256) {
		const int ll = x / 16, w = x % 16, l = l0 + ll;
		const size_t off = b0 + 4 * (size_t)w;
		tile[ll * BT_ROW + w] = (l < L && off < rb) ? bed_word(bed, (size_t)l * rb + off) : 0u;
	}
}

/* the sum of an integer over the 64 lanes of a wave, in every lane */
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
	return v;
}

/* what every entry point asks of its records, and how they go up: n_bytes of whole records and BED_PAD zero bytes behind them in a
 * buffer of d_bed's own.  d_bed.p stays null when the buffer does not fit; the return value is the first failure's. */
static bool bed_shape_ok(int I, int L, const uint8_t *bed, size_t record_bytes) { return I > 0 && L > 0 && bed && record_bytes >= ((size_t)I + 3) / 4; }
static hipError_t bed_upload(mchip_context *ctx, scoped_dev<uint8_t> &d_bed, const uint8_t *records, size_t n_bytes)
{
	hipError_t e = d_bed.alloc(n_bytes + BED_PAD);
	if (e == hipSuccess) e = hipMemcpyAsync(d_bed.p, records, n_bytes, hipMemcpyHostToDevice, ctx->stream);
	if (e == hipSuccess) e = hipMemsetAsync(d_bed.p + n_bytes, 0, BED_PAD, ctx->stream);
	return e;
}

/* ---- what the units call of one another, never exported from the library; first mchip.hip's ---- */
#pragma GCC visibility push(hidden)

/* the testing / tuning knobs as the environment has them now */
void read_knobs(mchip_knobs *knob);
/* raw [I][L][pl] -> gtA, gtS, validated against ua or, without one, `limit`; flags land in *bad; nonzero: too large for the kernel */
int launch_relayout(hipStream_t stream, const uint8_t *raw, int I, int L, int pl, const int32_t *ua, int limit, uint8_t *gtA, uint8_t *gtS, int *bad);
/* the model's K*T doubles from host order [K][T] to device order [T][K] (to_tk) or back */
void launch_transpose(mchip_context *ctx, const double *src, double *dst, bool to_tk);
int check_slot(mchip_context *ctx, int slot);
void free_model(mchip_context *ctx);
/* free_data and set_shape drop both saved sets with the data set that goes, unless told to keep the base of the selections */
enum { KEEP_INIT = 1, KEEP_RS_BASE = 2 };
void free_data(mchip_context *ctx, int keep = 0);
/* shape of a data set: tables derived from uniquealleles, genotype buffers allocated but not filled; no model afterwards.
 * KEEP_INIT: the observed haplotypes of mchip_set_init_genotypes stay in force when the shape is the one held. */
int set_shape(mchip_context *ctx, int I, int L, int ploidy, const int32_t *ua, int keep = 0);
/* gtA / gtS are in place: flags and the packed per-column allele counts of the column pass */
int install_layouts(mchip_context *ctx, int has_missing);

/* the only writer of empty_rows, first_empty and empty_rows_nan; the second form lists the individuals with seen[i] == 0 */
void set_empty_rows(mchip_context *ctx, std::vector<int> rows);
void set_empty_rows_unseen(mchip_context *ctx, const std::vector<uint8_t> &seen);
/* The installed data set -> `set`, in upload form, with its L, uniquealleles and empty rows; synchronises the stream.  On any
 * failure the buffer is freed and the set stays empty. */
int save_installed(mchip_context *ctx, saved_set &set);
void drop_saved(saved_set &set);
/* A saved set of the installed shape -> the kernels' layouts, with its empty rows. */
int install_saved(mchip_context *ctx, const saved_set &set);
/* A data set made on the device -> the kernels' layouts.  fill(d_out, d_seen) launches the kernel that writes the upload form
 * [I][L][ploidy] of the installed shape to d_out and sets d_seen[i] (zeroed here) = 1 for every individual that keeps an observed
 * copy. */
int install_derived(mchip_context *ctx, const std::function<void(uint8_t *d_out, uint8_t *d_seen)> &fill);
/* one byte per allele copy in stream order, padded to whole generator chunks (ctx->d_draw), allocated on first use */
int stream_buffer(mchip_context *ctx);
/* genotype held on the device as [I][L][ploidy] bytes -> the kernels' layouts (validated), packed counts */
int install_raw(mchip_context *ctx, const uint8_t *d_raw);

/* mchip_plan.hip: host arithmetic alone */
/* bits per packed allele count of the column pass's second genotype layout (gtC), 0 = none */
int count_bits_for(int ploidy, const mchip_knobs &kn);
mchip_shape shape_of(const mchip_context *ctx);
/* a function of the shape, the model, the knobs and the device's CU count alone: it touches neither the device nor a context */
mchip_geometry model_geometry(const mchip_shape &sh, int K, int admixture, int do_projection, double p_lb, const mchip_knobs &kn, int n_cu);
/* the arguments of a pass over the installed data set that reads parameter slot `slot` */
mchip_pass_args pass_args(mchip_context *ctx, int slot);
/* the plan of these arguments, less what the knobs switch off */
mchip_plan plan_for(const mchip_ktable *kt, const mchip_pass_args &a, const mchip_knobs &kn);
estep_finish finish_for(const mchip_plan &p, int K, int max_M, bool indiv, int do_mstep, const mchip_knobs &kn);
/* loci per block of k_finalize_p_tile for this data set and K, or 0 where a locus can outgrow the tile (k_finalize_p then) */
int finalize_p_loci(int K, int max_M);
/* partial log likelihoods k_mix_finalize leaves; whether the projection of P keeps its "fixed" flags in d_flags (above 64 alleles) */
int mix_ll_parts(int I);
bool needs_byte_flags(int max_M);

/* mchip_em.hip */
/* out[0 .. count) = the `count` doubles of d_scalars from `field` on, after a wait for the stream; a null out: nothing happens */
int fetch_scalars(mchip_context *ctx, const double *field, int count, double *out);
/* an E step on slot `from`, with do_mstep the M step into slot `to`; defer_ll: the caller's stop_check adds the partial log
 * likelihoods up; run_mixture is the mixture model's (mode 1: logL_mixture alone), *ll the field of d_scalars that receives it */
int run_estep(mchip_context *ctx, int from, int to, int do_mstep, const int *stop = nullptr, const int *skip_ind = nullptr, bool defer_ll = false);
int run_mixture(mchip_context *ctx, int from, int to, int do_mstep, int mode, const int *stop = nullptr, double *ll = nullptr, bool defer_ll = false);
/* one pass that takes the log likelihood, between the marks of a profiled run; ll given: the partial sums' sum goes there */
typedef void (*ll_pass_fn)(const mchip_pass_args &a, const mchip_plan &p, hipStream_t s);
void ll_pass(mchip_context *ctx, int kind, ll_pass_fn launch, const mchip_pass_args &a, const mchip_plan &p, double *ll, const int *stop = nullptr);
/* the stop rule of the batched loops on the E step that has just run */
void stop_check(mchip_context *ctx);
/* whether *exec holds a graph to launch: unless it does already, what enqueue() puts on the stream is captured into it */
bool captured(mchip_context *ctx, hipGraphExec_t *exec, const std::function<int()> &enqueue);
/* projection of slot `to` where the model projects */
int project_slot(mchip_context *ctx, int to, const int *stop = nullptr);
/* shared eta: eta[to] = normalise(sum_i S_ik + add), projected where the model projects and `project` says so */
int finalize_shared_eta(mchip_context *ctx, int to, const int *stop = nullptr, double add = 0.0, int project = 1);
/* P[to] in place from n_slabs slabs of Apart by k_finalize_p itself, unweighted, with the byte flags */
void launch_finalize_p_untiled(mchip_context *ctx, int n_slabs, int to, double add_lb, int do_projection);
/* out[0] = in[0] + ... + in[n - 1] in k_reduce_sum's fixed order, one workgroup */
void launch_reduce_sum(mchip_context *ctx, const double *in, int n, double *out);
/* out[r] = in[r][0] + ... + in[r][n - 1] for the n_rows rows of in, each as launch_reduce_sum adds it, in one launch */
void launch_reduce_rows(mchip_context *ctx, const double *in, int n_rows, int n, double *out);

/* mchip_init.hip */
/* the hard partition: argument checks of its entry points; relayout of a partition held in stream order + M step into slot `to`;
 * normalisation of counts already in Spart and n_aslabs slabs of Apart */
int check_partition_call(mchip_context *ctx, const void *arg, int to);
int partition_mstep(mchip_context *ctx, const uint8_t *d_raw, int to, int counts = 0);
int partition_finalize(mchip_context *ctx, int to, int counts, int n_aslabs);

/* mchip_profile.hip */
/* an event on the stream in front of (start) or behind a pass of kernel kind `kind`; nothing unless the context is profiling */
void prof_mark(mchip_context *ctx, int kind, bool start);
/* room for the next profiled paired launch: its blocks' clock readings (*marks) and its span, which launch_pair_spans fills */
int pair_profile_slot(mchip_context *ctx, size_t n_blocks, unsigned long long **marks);
void launch_pair_spans(mchip_context *ctx, const unsigned long long *marks, const mchip_plan &plan);

/* what an entry point that reads a fitted slot asks first: a data set, a model, a slot; admixture_message (NULL: either model
 * will do) refuses the mixture model in the unit's own words */
static inline int require_fit(mchip_context *ctx, int slot, const char *admixture_message)
{
	if (!ctx->T) return fail(ctx, MCHIP_ERR_STATE, "no genotypes set%s", nullptr);
	const int rc = check_slot(ctx, slot);
	if (rc) return rc;
	if (admixture_message && !ctx->admixture) return fail(ctx, MCHIP_ERR_UNSUPPORTED, "%s", admixture_message);
	return MCHIP_OK;
}
/* a kernel launched with dynamic LDS sized against a budget below 64 KiB: its static LDS still fits beside it */
template <typename Kern> static int check_lds(mchip_context *ctx, Kern kernel, size_t dynamic_bytes, const char *message)
{
	hipFuncAttributes attr;
	HIPCHK(hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(kernel)));
	if (attr.sharedSizeBytes + dynamic_bytes > 64 * 1024) return fail(ctx, MCHIP_ERR_STATE, "%s", message);
	return MCHIP_OK;
}

/* mchip_generators.hip */
/* rand() % m for the n_draws draws that follow `window`, one byte each, to d_out: whole chunks of RNG_CHUNK bytes are written */
int draw_mod_stream(mchip_context *ctx, const uint32_t *window, size_t n_draws, int m, uint8_t *d_out);
/* the jump tables of the rand() stream, the tiled partition's slabs and the generated individuals' clusters go with the data set */
void drop_generators(mchip_context *ctx);

/* mchip_cv.hip: folds, the saved full data set and a hold-out in force belong to the data set that goes */
void drop_cv(mchip_context *ctx);

#pragma GCC visibility pop

#endif
