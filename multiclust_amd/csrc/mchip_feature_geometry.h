/*
 * mchip_feature_geometry.h -- launch geometry of a lane-per-individual pass over blocks of 8 loci (k_cv_score, k_impute,
 * k_resid_tile, k_kin_tile).  Plain C++, no HIP types: tests/feature_geometry_driver.cpp compiles it alone and tests/feature_geometry.py
 * restates it.
 */
#ifndef MCHIP_FEATURE_GEOMETRY_H
#define MCHIP_FEATURE_GEOMETRY_H

#include <stddef.h>

constexpr int LANE_PASS_LBLOCK = 8;	/* loci per gtS group and per staged block */

struct lane_pass_geometry {
	int threads;		/* lanes per workgroup: 256, 128, ... down to the smallest the caller allows */
	int stage;		/* the P rows of a block of 8 loci are staged in LDS beside the q rows */
	size_t lds;		/* dynamic LDS: q rows, the reduction space, the P tile where staged */
	int n_itiles;		/* workgroups along the individuals */
	int lchunk, n_lchunks;	/* loci per workgroup (whole blocks of 8) and workgroups along the loci */
};

/* The q rows are (K | 1) doubles each (lds_pitch) and a block's P tile 8 max_M rows of as many.  threads: the most lanes whose q
 * rows leave room for the tile inside lds_budget beside red_bytes of reduction space; when no workgroup size from 256 down to
 * min_threads does, the most lanes that fit alone, the rows read from memory (64 lanes at K = 64: 33 KB).  The loci are cut into
 * enough chunks to fill n_cu compute units a few times over. */
static inline lane_pass_geometry lane_pass_geometry_of(int I, int L, int K, int max_M, int n_cu, size_t red_bytes, int min_threads,
							size_t lds_budget)
{
	lane_pass_geometry g;
	const size_t row = (size_t)(K | 1) * sizeof(double);
	const size_t ptile = (size_t)LANE_PASS_LBLOCK * (size_t)max_M * row;
	g.threads = 0;
	for (int t = 256; t >= min_threads && !g.threads; t >>= 1)
		if ((size_t)t * row + red_bytes + ptile <= lds_budget) g.threads = t;
	g.stage = g.threads ? 1 : 0;
	for (int t = 256; t >= min_threads && !g.threads; t >>= 1)
		if ((size_t)t * row + red_bytes <= lds_budget) g.threads = t;
	g.lds = (size_t)g.threads * row + red_bytes + (g.stage ? ptile : 0);
	g.n_itiles = (I + g.threads - 1) / g.threads;
	const int lblocks = (L + LANE_PASS_LBLOCK - 1) / LANE_PASS_LBLOCK;
	int want = (16 * (n_cu > 0 ? n_cu : 256) + g.n_itiles - 1) / g.n_itiles;
	if (want > lblocks) want = lblocks;
	if (want > 65535) want = 65535;
	if (want < 1) want = 1;
	g.lchunk = ((lblocks + want - 1) / want) * LANE_PASS_LBLOCK;
	g.n_lchunks = (L + g.lchunk - 1) / g.lchunk;
	return g;
}

/* ---- the LD band of packed records (k_ld_band, mchip_bed.hip; tests/ld_util.py restates the constants) ----
 * A workgroup owns LD_TILE first variants x LD_DCHUNK offsets and a run of whole stages of LD_STAGE 64-bit words (32 individuals
 * each).  The individuals are cut into n_split runs only while that takes the launch towards target_blocks workgroups: the sums
 * are integers, so the cut shows in no bit of the result. */
constexpr int LD_TILE = 64;	/* first variants per workgroup */
constexpr int LD_DCHUNK = 32;	/* offsets per workgroup: a lane owns one first variant and LD_DCHUNK / 4 offsets */
constexpr int LD_STAGE = 4;	/* 64-bit words of every staged record's planes in LDS at a time: 128 individuals */

struct ld_band_geometry {
	int n_tiles, n_dchunks;		/* workgroups along the first variants and along the offsets */
	int n_split, stages_per_split;	/* workgroups along the individuals, and the stages each of them walks */
};

static inline ld_band_geometry ld_band_geometry_of(int I, int n_first, int window, long long target_blocks)
{
	ld_band_geometry g;
	g.n_tiles = (n_first + LD_TILE - 1) / LD_TILE;
	g.n_dchunks = (window + LD_DCHUNK - 1) / LD_DCHUNK;
	const long long base = (long long)g.n_tiles * g.n_dchunks;
	const int n_stages = ((I + 31) / 32 + LD_STAGE - 1) / LD_STAGE;
	long long want = base > 0 ? (target_blocks + base - 1) / base : 1;
	if (want > n_stages) want = n_stages;
	if (want > 65535) want = 65535;
	if (want < 1) want = 1;
	g.stages_per_split = (int)((n_stages + want - 1) / want);
	g.n_split = (n_stages + g.stages_per_split - 1) / g.stages_per_split;
	return g;
}

/* ---- KING-robust kinship between individuals of packed records (k_king_pairs, mchip_bed.hip; tests/king_util.py restates the
 * constants) ----
 * A workgroup owns KING_TILE row individuals x KING_TILE column individuals and a run of whole stages of KING_STAGE 64-bit words (64
 * variants each) of their bit planes.  The variants are cut into n_split runs only while that takes the launch towards
 * target_blocks workgroups: the counts are integers, so the cut shows in no bit of the result. */
constexpr int KING_TILE = 64;	/* row and column individuals per workgroup: a lane owns KING_TILE / 16 of each */
constexpr int KING_STAGE = 4;	/* 64-bit words of every staged individual's planes in LDS at a time: 256 variants */

struct king_geometry {
	int n_rtiles, n_ctiles;		/* workgroups along the rows of the slab and along all the individuals */
	int n_split, stages_per_split;	/* workgroups along the variants, and the stages each of them walks */
};

static inline king_geometry king_geometry_of(int I, int n_rows, int L, long long target_blocks)
{
	king_geometry g;
	g.n_rtiles = (n_rows + KING_TILE - 1) / KING_TILE;
	g.n_ctiles = (I + KING_TILE - 1) / KING_TILE;
	const long long base = (long long)g.n_rtiles * g.n_ctiles;
	const int n_stages = (int)((((long long)L + 63) / 64 + KING_STAGE - 1) / KING_STAGE);
	long long want = base > 0 ? (target_blocks + base - 1) / base : 1;
	if (want > n_stages) want = n_stages;
	if (want > 65535) want = 65535;
	if (want < 1) want = 1;
	g.stages_per_split = (int)((n_stages + want - 1) / want);
	g.n_split = (n_stages + g.stages_per_split - 1) / g.stages_per_split;
	return g;
}

/* ---- genotype counts of packed records along both axes (k_qc_variants, k_qc_individuals, mchip_bed.hip; tests/qc_util.py restates
 * the constants) ----
 * Variant pass: a workgroup owns QC_VARIANTS variants, a wave each, and a run of whole steps of QC_STEP 64-bit words (32 individuals
 * each) of their records.  Individual pass: a workgroup owns QC_ITILE individuals and a run of whole 64-bit words of variants (64
 * each), one word staged at a time.  Either run is cut into several only while that takes the launch towards target_blocks
 * workgroups: the counts are integers, so the cut shows in no bit of the result. */
constexpr int QC_VARIANTS = 4;	/* variants per workgroup of the variant pass: one wave each */
constexpr int QC_STEP = 64;	/* 64-bit words a wave reads of its record at a time: 2048 individuals */
constexpr int QC_ITILE = 256;	/* individuals per workgroup of the individual pass: a lane each */

struct qc_geometry {
	int n_vgroups;			/* variant pass: workgroups along the variants */
	int v_split, steps_per_split;	/*   workgroups along the individuals, and the steps each of them walks */
	int n_itiles;			/* individual pass: workgroups along the individuals */
	int i_split, words_per_split;	/*   workgroups along the variants, and the words each of them walks */
};

static inline void qc_cut(long long base, long long n_units, long long target_blocks, int *n_split, int *per_split)
{
	long long want = base > 0 ? (target_blocks + base - 1) / base : 1;
	if (want > n_units) want = n_units;
	if (want > 65535) want = 65535;
	if (want < 1) want = 1;
	*per_split = (int)((n_units + want - 1) / want);
	*n_split = (int)((n_units + *per_split - 1) / *per_split);
}

static inline qc_geometry qc_geometry_of(int I, int L, long long target_blocks)
{
	qc_geometry g;
	g.n_vgroups = (int)(((long long)L + QC_VARIANTS - 1) / QC_VARIANTS);
	g.n_itiles = (int)(((long long)I + QC_ITILE - 1) / QC_ITILE);
	qc_cut(g.n_vgroups, (((long long)I + 31) / 32 + QC_STEP - 1) / QC_STEP, target_blocks, &g.v_split, &g.steps_per_split);
	qc_cut(g.n_itiles, ((long long)L + 63) / 64, target_blocks, &g.i_split, &g.words_per_split);
	return g;
}

/* ---- principal components of packed records (k_pca_project, k_pca_expand, k_pca_fold, mchip_pca.hip; tests/pca_util.py restates the
 * constants) ----
 * Projection W = Z^T X: a workgroup owns PCA_VARIANTS variants and walks all the individuals, nothing is cut.  Expansion Y = Z W / L':
 * a workgroup owns PCA_ITILE individuals and one slab of PCA_LSLAB variants; the slabs' partial sums are added in index order.  The
 * sums are floating point, so unlike the cuts above this one is a CONSTANT of the shape: no target_blocks enters, and no launch knob
 * can show in any bit of Y. */
constexpr int PCA_VARIANTS = 64;	/* variants per workgroup of the projection: a wave per 16 */
constexpr int PCA_ITILE = 64;		/* individuals per workgroup of the expansion: a wave per 16 */
constexpr int PCA_LSLAB = 4096;		/* variants per slab of the expansion */

struct pca_geometry {
	int n_vgroups;		/* projection: workgroups along the variants */
	int n_itiles, Ipad;	/* expansion: workgroups along the individuals, and the rows of a slab's partial sums */
	int n_slabs;		/*   workgroups along the variants = slabs of partial sums */
};

static inline pca_geometry pca_geometry_of(int I, int L)
{
	pca_geometry g;
	g.n_vgroups = (int)(((long long)L + PCA_VARIANTS - 1) / PCA_VARIANTS);
	g.n_itiles = (int)(((long long)I + PCA_ITILE - 1) / PCA_ITILE);
	g.Ipad = g.n_itiles * PCA_ITILE;
	g.n_slabs = (int)(((long long)L + PCA_LSLAB - 1) / PCA_LSLAB);
	return g;
}

#endif
