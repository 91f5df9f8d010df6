/* kernels_k/common.h -- K, the reciprocals, the genotype group and the compile-time geometry every pass family of
 * mchip_kernels_k.hip shares */
#ifndef MCHIP_KERNELS_K_COMMON_H
#define MCHIP_KERNELS_K_COMMON_H

#include "mchip_internal.h"

#ifndef MCHIP_K
#error "compile with -DMCHIP_K=<K>"
#endif

namespace {

constexpr int K = MCHIP_K;

/* 1/t to full double precision for t in (0, 1]: v_rcp_f64 is good to ~2^-25 (measured 2.1e8 ulp,
 * scripts/micro/fp64_micro.hip); one second-order step r0 (1 + e + e^2), e = 1 - t r0, leaves e^3 ~ 1e-22 plus
 * rounding (measured <= 1 ulp), for 3 FMAs instead of the 4 of two Newton steps.  No scaling / fix-up: t is a
 * convex combination of probabilities >= the lower bound, never denormal or huge. */
__device__ __forceinline__ double rcp_full(double t)
{
	const double r = __builtin_amdgcn_rcp(t);
	const double e = __builtin_fma(-t, r, 1.0);
	const double p = __builtin_fma(e, e, e);
	return __builtin_fma(r, p, r);
}

/* Four reciprocals from one: 1/(t0 t1 t2 t3) by rcp_full, then back-multiplication (9 multiplies + 1 reciprocal
 * instead of 4 reciprocals; v_rcp_f64 issues at a quarter of the FMA rate).  Each t is in [p_lb/K, 1], so the
 * product of four stays far from underflow; every result carries <= 2.5 ulp. */
__device__ __forceinline__ void rcp4(const double (&t)[4], double (&rc)[4])
{
	const double p01 = t[0] * t[1], p23 = t[2] * t[3];
	const double rp = rcp_full(p01 * p23);
	const double r01 = rp * p23, r23 = rp * p01;
	rc[0] = r01 * t[1];
	rc[1] = r01 * t[0];
	rc[2] = r23 * t[3];
	rc[3] = r23 * t[2];
}

__device__ __forceinline__ void rcp_group(const double (&t)[4], double (&rc)[4]) { rcp4(t, rc); }
__device__ __forceinline__ void rcp_group(const double (&t)[2], double (&rc)[2])
{
	const double rp = rcp_full(t[0] * t[1]);
	rc[0] = rp * t[1];
	rc[1] = rp * t[0];
}
__device__ __forceinline__ void rcp_group(const double (&t)[1], double (&rc)[1]) { rc[0] = rcp_full(t[0]); }

/* genotype bytes of sub-entry j (0..7) of an 8-entry group; PL = 2 fast path keeps the group in a uint4 */
template <int PL> struct geno_group;

template <> struct geno_group<2> {
	uint4 g;
	__device__ __forceinline__ void load(const uint8_t *base, size_t group, int) { g = *reinterpret_cast<const uint4 *>(base + group * 16); }
	__device__ __forceinline__ unsigned field(int j) const
	{
		unsigned w = (j < 2) ? g.x : (j < 4) ? g.y : (j < 6) ? g.z : g.w;
		return (w >> ((j & 1) * 16)) & 0xFFFFu;
	}
	/* number of copies of entry j equal to allele m */
	__device__ __forceinline__ int count(int j, unsigned m, int) const
	{
		unsigned w = field(j);
		return (int)((w & 0xFFu) == m) + (int)((w >> 8) == m);
	}
	__device__ __forceinline__ unsigned copy(int j, int a, int) const { return (field(j) >> (8 * a)) & 0xFFu; }
	/* the loaded word is here from now on (an empty statement that reads it: hipcc puts its s_waitcnt in front of it).  Before
	 * a loop whose body starts with loads of its own: the in-order counter would otherwise make the body's first use of this
	 * group wait for those younger loads as well, every trip */
	__device__ __forceinline__ void arrive() const { asm volatile("" :: "v"(g.x), "v"(g.y), "v"(g.z), "v"(g.w)); }
	/* entries 4h..4h+3 moved to positions 0..3 (h wave-uniform) */
	__device__ __forceinline__ geno_group<2> half(int h) const
	{
		geno_group<2> r;
		r.g.x = h ? g.z : g.x;
		r.g.y = h ? g.w : g.y;
		r.g.z = 0xFFFFFFFFu;
		r.g.w = 0xFFFFFFFFu;
		return r;
	}
};

template <> struct geno_group<4> {	/* tetraploid: 8 entries x 4 bytes = two 16-byte loads */
	uint4 g0, g1;
	__device__ __forceinline__ void load(const uint8_t *base, size_t group, int)
	{
		const uint4 *p = reinterpret_cast<const uint4 *>(base + group * 32);
		g0 = p[0];
		g1 = p[1];
	}
	__device__ __forceinline__ unsigned field(int j) const
	{
		return (j == 0) ? g0.x : (j == 1) ? g0.y : (j == 2) ? g0.z : (j == 3) ? g0.w
		     : (j == 4) ? g1.x : (j == 5) ? g1.y : (j == 6) ? g1.z : g1.w;
	}
	__device__ __forceinline__ int count(int j, unsigned m, int) const
	{
		const unsigned w = field(j);
		return (int)((w & 0xFFu) == m) + (int)(((w >> 8) & 0xFFu) == m) + (int)(((w >> 16) & 0xFFu) == m) + (int)((w >> 24) == m);
	}
	__device__ __forceinline__ unsigned copy(int j, int a, int) const { return (field(j) >> (8 * a)) & 0xFFu; }
	__device__ __forceinline__ void arrive() const
	{
		asm volatile("" :: "v"(g0.x), "v"(g0.y), "v"(g0.z), "v"(g0.w), "v"(g1.x), "v"(g1.y), "v"(g1.z), "v"(g1.w));
	}
	__device__ __forceinline__ geno_group<4> half(int h) const
	{
		geno_group<4> r;
		r.g0 = h ? g1 : g0;
		r.g1 = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
		return r;
	}
};

template <> struct geno_group<0> {	/* any ploidy: byte loads */
	const uint8_t *p;
	__device__ __forceinline__ void load(const uint8_t *base, size_t group, int pl) { p = base + group * 8 * (size_t)pl; stride_pl = pl; }
	__device__ __forceinline__ int count(int j, unsigned m, int pl) const
	{
		int n = 0;
		for (int a = 0; a < pl; a++) n += (int)(p[j * pl + a] == m);
		return n;
	}
	__device__ __forceinline__ unsigned copy(int j, int a, int pl) const { return p[j * pl + a]; }
	__device__ __forceinline__ void arrive() const {}	/* (bytes are loaded where they are used) */
	__device__ __forceinline__ geno_group<0> half(int h) const
	{
		geno_group<0> r;
		r.p = p + h * 4 * stride_pl;
		r.stride_pl = stride_pl;
		return r;
	}
	int stride_pl;
};

/* ---------------------------------------------------------------- compile-time geometry: what more than one family, or a
 * family and its launcher, reads */
/* k_column_counts_split (column.h): CSPLIT adjacent lanes = one allele column, lane part s holds k in [s CKS, (s+1) CKS) */
constexpr int CSPLIT = mchip_col_split(K);
constexpr int CKS = (K + CSPLIT - 1) / CSPLIT;		/* k per lane part */
constexpr int CKSE = (CKS + 1) & ~1;			/* rounded up to whole 16-byte reads (the padding multiplies p = 0) */
/* LDS doubles per (individual, part): the parts of a row must not start on the same banks (64 banks x 4 bytes; a 16-byte read
 * covers 4): K = 60 with a stride of 32 doubles = 256 bytes put both parts on banks 0-3 and cost 25 % */
constexpr int cqs_stride(int n) { return ((2 * n) % 64 < 4 || (2 * n) % 64 > 60) ? n + 2 : n; }
constexpr int CQS = cqs_stride(CKSE + 2);

/* lanes per workgroup of the individual-side passes */
constexpr int QBLOCK = mchip_qblock(K);

/* LDS row stride in doubles (mchip_internal.h) and the lane split of the sparse individual pass: SPLIT lanes per individual,
 * lane part s holds k in [s * KSP, (s + 1) * KSP) (KS values, KSP = KS rounded up to even; slots past K hold zeros) */
constexpr int KP = mchip_kp(K);
constexpr int SPLIT = mchip_ind_split(K);
constexpr int KS = (K + SPLIT - 1) / SPLIT;
constexpr int KSP = SPLIT == 1 ? K : ((KS + 1) & ~1);	/* doubles a lane works on */
constexpr int KGP = SPLIT == 1 ? KP / 2 : KSP / 2;	/* 16-byte LDS reads per gathered row part */
constexpr int PSTR = mchip_ind_pstride(K);		/* LDS doubles from one lane part of a row to the next (KSP, or padded: bank conflicts) */
/* where cluster k of a staged row sits in LDS */
__device__ __forceinline__ constexpr int lds_k(int k) { return SPLIT == 1 ? k : (k / KSP) * PSTR + (k % KSP); }
static_assert(SPLIT * PSTR <= KP || SPLIT == 1, "row stride holds every lane's range");

/* Keeps a running product of t values away from underflow without a log in the loop: below 1e-100 its binary
 * exponent moves into an integer (v_frexp_exp_i32_f64 / v_frexp_mant_f64); log(product) = ex*ln2 + log(prod). */
__device__ __forceinline__ void rescale(double &prod, int &ex)
{
	if (prod < 1e-100) {
		ex += __builtin_amdgcn_frexp_exp(prod);
		prod = __builtin_amdgcn_frexp_mant(prod);
	}
}

/* (the cooperating forms: k_individual_sparse_w and k_individual_bial) */
__device__ __forceinline__ double wave_total(double v)
{
	/* fixed tree over the 64 lanes; lane 0 ends with the total */
	for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
	return v;
}

}  // namespace

#endif
