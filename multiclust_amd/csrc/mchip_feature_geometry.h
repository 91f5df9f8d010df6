/*
 * mchip_feature_geometry.h -- launch geometry of a lane-per-individual pass over blocks of 8 loci (k_cv_score, k_impute,
 * k_resid_tile).  Plain C++, no HIP types: tests/feature_geometry_driver.cpp compiles it alone and tests/feature_geometry.py
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

#endif
