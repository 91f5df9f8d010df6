/*
 * mchip_kernels_k.hip -- the K-specialised gfx950 kernels of the admixture EM hot path.
 * Compiled once per K (hipcc -DMCHIP_K=<K>), see Makefile; each object exports mchip_ktable_<K>.
 *
 * Fused E+M without materialising d_iklm (reference em_alg.c:291-486 + 592-754):
 *   per non-empty cell (i, c=(l,m)), n = ILM[i][l][m]:
 *       t = sum_k q_ik P_kc ; r = n / t ; logL += n log t
 *       S_ik = q_ik * sum_c P_kc r_ic        (= sum_{l,m} d_iklm, em_alg.c:650-682)
 *       N_kc = P_kc * sum_i q_ik r_ic        (= sum_i d_iklm,      em_alg.c:706-731)
 * The two marginals reduce over opposite axes, so the genotype matrix is streamed by two passes whose
 * reductions are both thread-private (no cross-lane traffic, no atomics, bitwise reproducible):
 *   column pass     (lane = allele column c, loop over individuals): N-side sum_i q_ik r_ic, and logL;
 *                    q_i is wave-uniform -> scalar loads, P_kc and the accumulators live in VGPRs.
 *   individual pass (lane = individual i, loop over loci/alleles):   S-side sum_c P_kc r_ic;
 *                    P_.c is wave-uniform -> scalar loads, q_ik and the accumulators live in VGPRs.
 * All arithmetic is IEEE double (v_fma_f64); n log t is accumulated as log of a running product of t
 * (one v_log-free multiply per allele copy, one log per flush), see DESIGN.md.
 *
 * The kernels are in kernels_k/, one header per pass family, included here in the order they are defined; this file is what is
 * chosen and launched: the grids, the plan, the launchers and the table.
 */
#include "kernels_k/common.h"
#include "kernels_k/column.h"
#include "kernels_k/individual.h"
#include "kernels_k/sparse.h"
#include "kernels_k/sparse_w.h"
#include "kernels_k/pair.h"
#include "kernels_k/mixture.h"
#include "kernels_k/partition.h"
#include "kernels_k/finalize_q.h"

namespace {

/* ---------------------------------------------------------------- grids (coop_rows, coop_grid and the dynamic LDS sizes stand
 * beside their kernels in sparse_w.h and sparse.h) */
inline dim3 column_grid(const mchip_pass_args &a) { return dim3((a.T + MCHIP_BLOCK - 1) / MCHIP_BLOCK, a.n_ichunks); }
/* packed-count column pass (cooperating waves): 64 columns per workgroup, one slab per workgroup row */
inline dim3 counts_grid(const mchip_pass_args &a) { return dim3((a.T + 63) / 64, mchip_col_slabs(a)); }
inline dim3 indiv_grid(const mchip_pass_args &a) { return dim3((a.I + QBLOCK - 1) / QBLOCK, a.n_lchunks); }
inline dim3 sparse_grid(const mchip_pass_args &a) { return dim3((a.I + QBLOCK / SPLIT - 1) / (QBLOCK / SPLIT), a.n_lchunks); }

/* ---------------------------------------------------------------- the plan (mchip_internal.h): every choice of an instance */
/* the sparse individual pass of these arguments: S-side sums and logL (accum) or logL alone */
mchip_instance sparse_instance(const mchip_pass_args &a, bool accum)
{
	mchip_instance k = {};
	const bool safe = a.flush_blocks < 1;
	k.accum = accum;
	/* measured (profiles/r02_biallelic_variant.txt): the stand-alone log-likelihood pass gains 6-21 % from K = 6 up (it is
	 * LDS-bound in the general kernel), the S-side pass only from K = 10 (it is FP64-bound, and the dense-over-two-alleles
	 * form costs more instructions per locus: +8-19 % below that) */
	const bool bial_pays = SPLIT == 1 && (accum ? (K >= 10) : (K >= 6));	/* (its grid and partials are one lane per individual) */
	if (bial_pays && a.biallelic && a.ploidy == 2 && !safe) {
		k.kernel = MCHIP_K_INDIVIDUAL_BIAL;
		k.nomiss = !a.has_missing;
		return k;
	}
	k.kernel = SPLIT == 1 ? MCHIP_K_INDIVIDUAL_SPARSE_W : MCHIP_K_INDIVIDUAL_SPARSE;
	k.pl = (a.ploidy == 2 || a.ploidy == 4) ? a.ploidy : 0;
	k.safe = safe || k.pl == 0;
	k.nomiss = !a.has_missing && !k.safe;	/* idle lanes of the last block recompute individual I-1 and are dropped at the end */
	return k;
}
void plan(const mchip_pass_args &a, mchip_plan *p)
{
	*p = mchip_plan();
	const int pl2 = a.ploidy == 2 ? 2 : 0;		/* the dense kernels are specialised for diploids only */
	const bool dense_safe = pl2 == 0 || a.flush_blocks < 1;
	/* a.sparse: the column pass only accumulates the N-side sums; S-side sums and logL come from the sparse
	 * individual pass.  Otherwise (loci with more alleles than the LDS tile is sized for) the dense pair is used:
	 * the column pass also produces logL and the individual pass loops over every allele of every locus. */
	p->col.accum = true;
	if (a.sparse && a.count_bits) {
		const bool split = CSPLIT > 1 && !a.no_col_split;
		p->col.kernel = split ? MCHIP_K_COLUMN_COUNTS_SPLIT : MCHIP_K_COLUMN_COUNTS;
		p->col.bits = a.count_bits;
		p->col.safe = a.safe_rcp != 0;
		p->col_slabs = split ? a.n_ichunks : mchip_col_slabs(a);
	} else {
		p->col.kernel = MCHIP_K_COLUMN_PASS;
		p->col.pl = pl2;
		p->col.ll = !a.sparse;
		p->col.safe = !a.sparse && dense_safe;
		p->col_slabs = a.n_ichunks;
	}
	if (a.sparse) {
		p->sside = sparse_instance(a, true);
		p->ll = sparse_instance(a, false);
		p->ind_slabs = SPLIT == 1 ? mchip_ind_slabs(a) : a.n_lchunks;
		p->ll_parts = SPLIT == 1 ? ((a.I + 63) / 64) * mchip_ind_slabs(a) : ((a.I + QBLOCK / SPLIT - 1) / (QBLOCK / SPLIT)) * a.n_lchunks;
	} else {
		p->sside.kernel = MCHIP_K_INDIVIDUAL_PASS;
		p->sside.accum = true;
		p->sside.pl = pl2;
		p->ll.kernel = MCHIP_K_COLUMN_PASS;
		p->ll.pl = pl2;
		p->ll.ll = true;
		p->ll.safe = dense_safe;
		p->ind_slabs = a.n_lchunks;
		p->ll_parts = ((a.T + MCHIP_BLOCK - 1) / MCHIP_BLOCK) * a.n_ichunks;	/* dense pair: the column pass takes the log likelihood */
	}
	/* mixture model */
	p->mix_gather.kernel = MCHIP_K_MIX_GATHER;
	p->mix_gather.pl = pl2;
	p->mix_gather.staged = a.sparse != 0;
	p->mix_col.accum = true;
	if (a.count_bits) {
		p->mix_col.kernel = MCHIP_K_COLUMN_COUNTS;
		p->mix_col.bits = a.count_bits;
		p->mix_col.mix = true;
		p->mix_col_slabs = mchip_col_slabs(a);
	} else {
		p->mix_col.kernel = MCHIP_K_MIX_COLUMN;
		p->mix_col.pl = pl2;
		p->mix_col_slabs = a.n_ichunks;
	}
	/* the dual pass exists where both of its halves would run the sparse kernel with shared reciprocals (so that its results are
	 * theirs bit for bit) and the second set's registers still fit */
	const bool diploid_w = p->sside.kernel == MCHIP_K_INDIVIDUAL_SPARSE_W && p->sside.pl == 2;
	if (K <= 12 && diploid_w && !p->sside.safe && p->ll.kernel == MCHIP_K_INDIVIDUAL_SPARSE_W && coop_lds_bytes(a, 2) <= 64 * 1024) {
		p->dual = 1;
		p->dual_pass = p->sside;
		p->dual_pass.dual = true;
	}
	/* the paired E step exists where col is k_column_counts<2, false, SAFE> and sside k_individual_sparse_w<2, true, SAFE, NOMISS>
	 * with four waves and the same SAFE (so that its results are theirs bit for bit), at the K where both bodies fit a 256-thread
	 * workgroup's registers */
	if (K <= 12 && SPLIT == 1 && CSPLIT == 1 && p->col.kernel == MCHIP_K_COLUMN_COUNTS && p->col.bits == 2 && diploid_w &&
	    a.ind_waves * 64 == MCHIP_BLOCK && p->col.safe == p->sside.safe) {
		const dim3 cg = counts_grid(a);
		const unsigned n_col = cg.x * cg.y, n_ind = coop_rows(a).x;
		mchip_pair_runs r;
		r.col_runs = (n_col + MCHIP_PAIR_RUN - 1) / MCHIP_PAIR_RUN;
		r.ind_runs = (n_ind + MCHIP_PAIR_RUN - 1) / MCHIP_PAIR_RUN;
		/* (mchip_pair_is_ind's 32-bit products) */
		if (r.col_runs && r.ind_runs && (unsigned long long)(r.col_runs + r.ind_runs) * r.ind_runs < (1ull << 32)) {
			p->pair = 1;
			p->pair_pass = p->sside;
			p->pair_pass.kernel = MCHIP_K_ESTEP_PAIR;
			p->pair_pass.bits = 2;
			p->pair_runs = r;
			p->pair_blocks = (r.col_runs + r.ind_runs) * MCHIP_PAIR_RUN;
		}
	}
}

/* ---------------------------------------------------------------- launchers of the passes: what the plan names, nothing else.
 * The case labels list the instances that exist; the `if constexpr` guards keep those from being compiled at a K where no plan
 * names them. */
constexpr int tkey(int n, bool x, bool y = false) { return n * 4 + (x ? 2 : 0) + (y ? 1 : 0); }

void launch_column(const mchip_pass_args &a, const mchip_instance &k, hipStream_t s)
{
	const dim3 block(MCHIP_BLOCK);
	auto go = [&](auto kernel, dim3 grid, dim3 blk, size_t lds) { hipLaunchKernelGGL(kernel, grid, blk, lds, s, a); };
	switch (k.kernel) {
	case MCHIP_K_COLUMN_COUNTS_SPLIT:
		if constexpr (CSPLIT > 1) {
			const dim3 grid((a.T + MCHIP_BLOCK / CSPLIT - 1) / (MCHIP_BLOCK / CSPLIT), a.n_ichunks);
			switch (tkey(k.bits, k.safe)) {
			case tkey(2, true): go(k_column_counts_split<2, true>, grid, block, 0); break;
			case tkey(2, false): go(k_column_counts_split<2, false>, grid, block, 0); break;
			case tkey(4, true): go(k_column_counts_split<4, true>, grid, block, 0); break;
			case tkey(4, false): go(k_column_counts_split<4, false>, grid, block, 0); break;
			}
		}
		break;
	case MCHIP_K_COLUMN_COUNTS:
		switch (tkey(k.bits, k.mix, k.safe)) {
		case tkey(2, false, true): go(k_column_counts<2, false, true>, counts_grid(a), block, 0); break;
		case tkey(4, false, true): go(k_column_counts<4, false, true>, counts_grid(a), block, 0); break;
		case tkey(2, false, false): go(k_column_counts<2, false>, counts_grid(a), block, 0); break;
		case tkey(4, false, false): go(k_column_counts<4, false>, counts_grid(a), block, 0); break;
		case tkey(2, true, false): go(k_column_counts<2, true>, counts_grid(a), block, 0); break;
		case tkey(4, true, false): go(k_column_counts<4, true>, counts_grid(a), block, 0); break;
		}
		break;
	case MCHIP_K_COLUMN_PASS:	/* <pl, accum, safe, ll> */
		switch (tkey(k.pl + (k.accum ? 1 : 0), k.safe, k.ll)) {
		case tkey(2 + 1, false, false): go(k_column_pass<2, true, false, false>, column_grid(a), block, 0); break;
		case tkey(0 + 1, false, false): go(k_column_pass<0, true, false, false>, column_grid(a), block, 0); break;
		case tkey(2 + 1, false, true): go(k_column_pass<2, true, false, true>, column_grid(a), block, 0); break;
		case tkey(2 + 1, true, true): go(k_column_pass<2, true, true, true>, column_grid(a), block, 0); break;
		case tkey(0 + 1, true, true): go(k_column_pass<0, true, true, true>, column_grid(a), block, 0); break;
		case tkey(2, false, true): go(k_column_pass<2, false, false, true>, column_grid(a), block, 0); break;
		case tkey(2, true, true): go(k_column_pass<2, false, true, true>, column_grid(a), block, 0); break;
		case tkey(0, true, true): go(k_column_pass<0, false, true, true>, column_grid(a), block, 0); break;
		}
		break;
	case MCHIP_K_MIX_COLUMN:
		if (k.pl == 2) hipLaunchKernelGGL((k_mix_column<2>), column_grid(a), block, 0, s, a);
		else hipLaunchKernelGGL((k_mix_column<0>), column_grid(a), block, 0, s, a);
		break;
	}
}
/* (the (SAFE, NOMISS) pairs of the sparse kernels: shared reciprocals without and with missing data, one reciprocal per cell) */
template <bool ACCUM> void launch_individual(const mchip_pass_args &a, const mchip_instance &k, hipStream_t s)
{
	auto go = [&](auto kernel, dim3 grid, dim3 blk, size_t lds) { hipLaunchKernelGGL(kernel, grid, blk, lds, s, a); };
	switch (k.kernel) {
	case MCHIP_K_INDIVIDUAL_PASS:
		if (k.pl == 2) hipLaunchKernelGGL((k_individual_pass<2>), indiv_grid(a), dim3(QBLOCK), 0, s, a);
		else hipLaunchKernelGGL((k_individual_pass<0>), indiv_grid(a), dim3(QBLOCK), 0, s, a);
		break;
	case MCHIP_K_INDIVIDUAL_BIAL:
		if constexpr (SPLIT == 1) {
			const dim3 grid = coop_grid(a), block(64 * a.ind_waves);
			if (k.nomiss) hipLaunchKernelGGL((k_individual_bial<ACCUM, true>), grid, block, 0, s, a);
			else hipLaunchKernelGGL((k_individual_bial<ACCUM, false>), grid, block, 0, s, a);
		}
		break;
	case MCHIP_K_INDIVIDUAL_SPARSE_W:
		if constexpr (SPLIT == 1) {
			const dim3 rows = coop_rows(a), block(64 * a.ind_waves);
			const size_t cl = coop_lds_bytes(a, 1);
			switch (tkey(k.pl, k.safe, k.nomiss)) {
			case tkey(2, false, true): go(k_individual_sparse_w<2, ACCUM, false, true>, rows, block, cl); break;
			case tkey(2, false, false): go(k_individual_sparse_w<2, ACCUM, false, false>, rows, block, cl); break;
			case tkey(2, true, false): go(k_individual_sparse_w<2, ACCUM, true, false>, rows, block, cl); break;
			case tkey(4, false, true): go(k_individual_sparse_w<4, ACCUM, false, true>, rows, block, cl); break;
			case tkey(4, false, false): go(k_individual_sparse_w<4, ACCUM, false, false>, rows, block, cl); break;
			case tkey(4, true, false): go(k_individual_sparse_w<4, ACCUM, true, false>, rows, block, cl); break;
			case tkey(0, true, false): go(k_individual_sparse_w<0, ACCUM, true, false>, rows, block, cl); break;
			}
		}
		break;
	case MCHIP_K_INDIVIDUAL_SPARSE:
		if constexpr (SPLIT != 1) {
			const dim3 grid = sparse_grid(a), block(QBLOCK);
			const size_t lds = sparse_lds_bytes(a);
			switch (tkey(k.pl, k.safe, k.nomiss)) {
			case tkey(2, false, true): go(k_individual_sparse<2, ACCUM, false, true>, grid, block, lds); break;
			case tkey(2, false, false): go(k_individual_sparse<2, ACCUM, false, false>, grid, block, lds); break;
			case tkey(2, true, false): go(k_individual_sparse<2, ACCUM, true, false>, grid, block, lds); break;
			case tkey(4, false, true): go(k_individual_sparse<4, ACCUM, false, true>, grid, block, lds); break;
			case tkey(4, false, false): go(k_individual_sparse<4, ACCUM, false, false>, grid, block, lds); break;
			case tkey(4, true, false): go(k_individual_sparse<4, ACCUM, true, false>, grid, block, lds); break;
			case tkey(0, true, false): go(k_individual_sparse<0, ACCUM, true, false>, grid, block, lds); break;
			}
		}
		break;
	}
}
void launch_accum_p(const mchip_pass_args &a, const mchip_plan &p, hipStream_t s) { launch_column(a, p.col, s); }
void launch_mix_column(const mchip_pass_args &a, const mchip_plan &p, hipStream_t s) { launch_column(a, p.mix_col, s); }
void launch_accum_q(const mchip_pass_args &a, const mchip_plan &p, hipStream_t s) { launch_individual<true>(a, p.sside, s); }
void launch_loglik(const mchip_pass_args &a, const mchip_plan &p, hipStream_t s)
{
	if (p.ll.kernel == MCHIP_K_COLUMN_PASS) launch_column(a, p.ll, s);
	else launch_individual<false>(a, p.ll, s);
}
void launch_accum_q_dual(const mchip_pass_args &a, const mchip_plan &p, hipStream_t s)
{
	if constexpr (K <= 12) {
		const size_t lds = coop_lds_bytes(a, 2);
		if (p.dual_pass.nomiss) hipLaunchKernelGGL((k_individual_sparse_w<2, true, false, true, true>), coop_rows(a), dim3(64 * a.ind_waves), lds, s, a);
		else hipLaunchKernelGGL((k_individual_sparse_w<2, true, false, false, true>), coop_rows(a), dim3(64 * a.ind_waves), lds, s, a);
	}
}
void launch_estep_pair(const mchip_pass_args &a, const mchip_plan &p, unsigned long long *marks, hipStream_t s)
{
	if constexpr (K <= 12 && SPLIT == 1 && CSPLIT == 1) {
		const mchip_pair_runs r = p.pair_runs;
		const dim3 grid(p.pair_blocks), block(MCHIP_BLOCK);
		const size_t ind_lds = coop_lds_bytes(a, 1), col_lds = (size_t)K * 64 * sizeof(double);
		const size_t lds = ind_lds > col_lds ? ind_lds : col_lds;
		if (p.pair_pass.safe) hipLaunchKernelGGL((k_estep_pair<2, 2, true, false>), grid, block, lds, s, a, r, marks);
		else if (p.pair_pass.nomiss) hipLaunchKernelGGL((k_estep_pair<2, 2, false, true>), grid, block, lds, s, a, r, marks);
		else hipLaunchKernelGGL((k_estep_pair<2, 2, false, false>), grid, block, lds, s, a, r, marks);
	}
}
void launch_mix_gather(const mchip_pass_args &a, const mchip_plan &p, hipStream_t s)
{
	const mchip_instance &k = p.mix_gather;
	const size_t lds = 2 * (size_t)a.tile_cols * KP * sizeof(double);
	switch (tkey(k.pl, k.staged)) {
	case tkey(2, true): hipLaunchKernelGGL((k_mix_gather<2, true>), indiv_grid(a), dim3(QBLOCK), lds, s, a); break;
	case tkey(0, true): hipLaunchKernelGGL((k_mix_gather<0, true>), indiv_grid(a), dim3(QBLOCK), lds, s, a); break;
	case tkey(2, false): hipLaunchKernelGGL((k_mix_gather<2, false>), indiv_grid(a), dim3(QBLOCK), 0, s, a); break;
	case tkey(0, false): hipLaunchKernelGGL((k_mix_gather<0, false>), indiv_grid(a), dim3(QBLOCK), 0, s, a); break;
	}
}
void launch_mix_finalize(int I, int n_lchunks, const double *Vpart, const double *eta, double *vik, double *llpart, int mode, const int *stop, hipStream_t s)
{
	hipLaunchKernelGGL(k_mix_finalize, dim3((I + MCHIP_BLOCK - 1) / MCHIP_BLOCK), dim3(MCHIP_BLOCK), 0, s, I, n_lchunks, Vpart, eta, vik, llpart, mode, stop);
}
void launch_part_p(const mchip_pass_args &a, hipStream_t s)
{
	if (a.ploidy == 2) hipLaunchKernelGGL((k_partition_columns<2>), column_grid(a), dim3(MCHIP_BLOCK), 0, s, a);
	else if (a.ploidy == 4) hipLaunchKernelGGL((k_partition_columns<4>), column_grid(a), dim3(MCHIP_BLOCK), 0, s, a);
	else hipLaunchKernelGGL((k_partition_columns<0>), column_grid(a), dim3(MCHIP_BLOCK), 0, s, a);
}
void launch_part_q(const mchip_pass_args &a, hipStream_t s)
{
	if (a.ploidy == 2) hipLaunchKernelGGL((k_partition_individuals<2>), indiv_grid(a), dim3(QBLOCK), 0, s, a);
	else if (a.ploidy == 4) hipLaunchKernelGGL((k_partition_individuals<4>), indiv_grid(a), dim3(QBLOCK), 0, s, a);
	else hipLaunchKernelGGL((k_partition_individuals<0>), indiv_grid(a), dim3(QBLOCK), 0, s, a);
}
void launch_finalize_q(int I, int, int n_lchunks, const double *Spart, const double *Qfrom, int qstride_from,
		       double *Qto, double *sik, int do_mstep, int weighted, int do_projection, double lb, const int *stop, hipStream_t s,
		       double add)
{
	hipLaunchKernelGGL(k_finalize_q, dim3((I + FQ_IND - 1) / FQ_IND), dim3(MCHIP_BLOCK), 0, s,
			   I, n_lchunks, Spart, Qfrom, qstride_from, Qto, sik, do_mstep, weighted, do_projection, lb, stop, add);
}
void launch_finalize_qp(int I, int n_lchunks, const double *Spart, const double *Qfrom, int qstride_from, double *Qto, double *sik,
			int do_projection_q, double lb_q, const mchip_finalize_p_args &p, const int *stop, hipStream_t s)
{
	const int q_blocks = (I + FQ_IND - 1) / FQ_IND, p_blocks = (p.L + p.loci_per_block - 1) / p.loci_per_block;
	hipLaunchKernelGGL(k_finalize_qp, dim3(q_blocks + p_blocks), dim3(MCHIP_BLOCK), 0, s,
			   q_blocks, I, n_lchunks, Spart, Qfrom, qstride_from, Qto, sik, do_projection_q, lb_q, p, stop);
}
void launch_project_q(int nrows, int, double *Q, double lb, const int *stop, hipStream_t s)
{
	hipLaunchKernelGGL(k_project_q, dim3((nrows + MCHIP_BLOCK - 1) / MCHIP_BLOCK), dim3(MCHIP_BLOCK), 0, s, nrows, Q, lb, stop);
}

}  // namespace

#define MCHIP_CAT2(a, b) a##b
#define MCHIP_CAT(a, b) MCHIP_CAT2(a, b)
/* a function, not a const global: hipcc would try to emit a const table of host pointers on the device side */
const mchip_ktable *MCHIP_CAT(mchip_ktable_get_, MCHIP_K)()
{
	static mchip_ktable t = {
		plan, launch_accum_p, launch_loglik, launch_accum_q, launch_part_p, launch_part_q, launch_finalize_q, launch_project_q,
		launch_mix_gather, launch_mix_finalize, launch_mix_column, launch_accum_q_dual, launch_finalize_qp, launch_estep_pair,
	};
	return &t;
}
