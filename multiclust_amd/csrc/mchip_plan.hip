/*
 * mchip_plan.hip -- the launch geometry of a model on a data set, the arguments of its passes and the plan of their kernel
 * instances, with mchip_describe_plan, which prints them.  Host arithmetic alone: this unit launches no kernel.
 */
#include "mchip_context.h"
#include "mchip_finalize.h"

#include <math.h>
#include <string>

/* bits per packed allele count of the column pass's second genotype layout (gtC), 0 = none */
int count_bits_for(int ploidy, const mchip_knobs &kn)
{
	if (kn.no_counts) return 0;
	return ploidy <= 3 ? 2 : (ploidy <= 15 ? 4 : 0);
}

/* Launch geometry of a model on a data set: a function of the shape, the model, the knobs and the device's CU count alone (it
 * touches neither the device nor a context: mchip_describe_plan runs it on a machine without a GPU). */
mchip_geometry model_geometry(const mchip_shape &sh, int K, int admixture, int do_projection, double p_lb, const mchip_knobs &kn, int n_cu)
{
	mchip_geometry g = {};
	/* launch geometry.  Both passes are FP64-issue-bound and every workgroup does the same amount of work, so
	 * the grid's last partial "round" of workgroups runs at low occupancy: measured at config 3, 8 workgroups
	 * per CU cost 6.9 ms per EM step, 64 per CU 5.4 ms (profiles/r01_geometry_sweep.txt).  More chunks mean
	 * more partial-sum slabs (Apart/Spart are written and re-read once per step), so the chunk count is capped
	 * where the slab bytes reach ~30 % of the genotype bytes the pass streams (config 2: 0.188 -> 0.179 ms per step against 15 %;
	 * config 3 reaches its 64 workgroups per CU before either cap).  The column pass stops at 15 % once the grid fills the
	 * device twice over: its slabs are K*T doubles each and k_finalize_p reads them all (config 5: 28 -> 15 slabs, 1.61 ->
	 * 1.56 ms per step; scripts/diag/geom.sh).  Chunk sizes are multiples of 8. */
	const int per_cu_col = kn.per_cu_col, per_cu_ind = kn.per_cu_ind;	/* tuning knobs (default 64) */
	int target = per_cu_col * n_cu;
	const int col_tiles = (sh.T + MCHIP_BLOCK - 1) / MCHIP_BLOCK;
	const int iblocks = (sh.I + 7) / 8, lblocks = (sh.L + 7) / 8;
	const double slab_frac = kn.slab_frac;	/* tuning knob (default 0.3) */
	/* column pass: slab bytes per chunk 8*K*T, genotype bytes per chunk ichunk*L*ploidy */
	int min_ichunk = (int)ceil(8.0 * K * sh.T / (slab_frac * sh.L * sh.ploidy));
	int want = (target + col_tiles - 1) / col_tiles;
	int cap = sh.I / (min_ichunk > 0 ? min_ichunk : 1);
	{
		const int cap_lo = cap / 2;						/* half the slab budget */
		const int fill = (2 * 8 * n_cu + col_tiles - 1) / col_tiles;	/* two rounds of 8 resident workgroups per CU */
		const int soft = cap_lo > (fill < cap ? fill : cap) ? cap_lo : (fill < cap ? fill : cap);
		if (!kn.geometry_given && want > soft) want = soft;
	}
	if (want > cap) want = cap;
	if (want < 1) want = 1;
	if (want > iblocks) want = iblocks;
	if (sh.count_bits && !kn.no_roundup) {	/* the packed-count column pass puts MCHIP_COL_WAVES chunks into a workgroup: whole workgroups where the caps allow */
		const int up = ((want + MCHIP_COL_WAVES - 1) / MCHIP_COL_WAVES) * MCHIP_COL_WAVES;
		if (up <= cap && up <= iblocks) want = up;
	}
	{
		const int gran = sh.count_bits ? 128 / sh.count_bits : 8;	/* individuals per packed word */
		const int per = (sh.I + want - 1) / want;
		g.ichunk = ((per + gran - 1) / gran) * gran;
	}
	g.n_ichunks = (sh.I + g.ichunk - 1) / g.ichunk;
	/* individual pass: slab bytes per chunk 8*K*I, genotype bytes per chunk lchunk*I*ploidy */
	/* (the sparse pass gives an individual mchip_ind_split(K) lanes; the dense and mixture kernels one, and do not use n_ll_ind) */
	const int ind_per_block = mchip_qblock(K) / (admixture ? mchip_ind_split(K) : 1);
	const int ind_tiles = (sh.I + ind_per_block - 1) / ind_per_block;
	int min_lchunk = (int)ceil(8.0 * K / (slab_frac * sh.ploidy));
	target = per_cu_ind * n_cu;
	want = (target + ind_tiles - 1) / ind_tiles;
	cap = sh.L / (min_lchunk > 0 ? min_lchunk : 1);
	if (want > cap) want = cap;
	if (want < 1) want = 1;
	if (want > lblocks) want = lblocks;
	{	/* the sparse individual pass stages two tiles of 8 loci of P rows in LDS: use it while they fit 64 KiB */
		const size_t kp = (size_t)mchip_kp(K);
		const size_t lds = (2 * 8 * (size_t)sh.max_M * kp + mchip_qblock(K)) * sizeof(double);
		g.sparse = (sh.max_M <= MCHIP_SPARSE_MAX_M) && lds <= 65536 && !kn.force_dense;
	}
	/* cooperating waves (mchip_internal.h): chunks are still what ONE WAVE takes; a workgroup of the sparse individual-side kernels
	 * is ind_waves of them, so a whole number of workgroups wants a multiple of that many chunks where the caps allow it */
	const bool ind_coop = admixture && g.sparse && mchip_ind_split(K) == 1;
	g.ind_waves = ind_coop ? mchip_ind_waves(K, 8 * sh.max_M) : 1;
	if (ind_coop) {
		/* ... and a multiple of eight slab rows where possible: the sparse kernel then keeps a row on one XCD (coop_rows() in
		 * kernels_k/sparse_w.h), and eight XCDs with 52 rows between them would have 7 and 6 each */
		const int w8 = 8 * g.ind_waves, w1 = g.ind_waves;
		const int up8 = ((want + w8 - 1) / w8) * w8, up1 = ((want + w1 - 1) / w1) * w1;
		if (up8 <= cap && up8 <= lblocks) want = up8;
		else if (up1 <= cap && up1 <= lblocks) want = up1;
	}
	g.lchunk = ((lblocks + want - 1) / want) * 8;
	g.n_lchunks = (sh.L + g.lchunk - 1) / g.lchunk;
	g.xcd_rows = (ind_coop && ((g.n_lchunks + g.ind_waves - 1) / g.ind_waves) % 8 == 0) ? 1 : 0;
	{	/* partial log likelihoods any pass can leave: one per workgroup; no individual-side kernel has fewer than 64 individuals
		 * per workgroup, no column-side one fewer than 64 columns */
		const int by_col = ((sh.T + 63) / 64) * g.n_ichunks, by_ind = ((sh.I + 63) / 64) * g.n_lchunks;
		g.n_llpart = by_col > by_ind ? by_col : by_ind;
	}
	/* log-product check interval: with every parameter >= its lower bound, t = sum_k q_k p_k >= p_lb / K, so
	 * floor(200 / -log10(t_min)) multiplications keep a product that starts above 1e-100 above 1e-300
	 * (DESIGN.md section 4).  A block of 8 loci (or individuals) multiplies 8*ploidy times. */
	{
		const double tmin = p_lb / K;
		int blocks = 0;
		if (do_projection && tmin > 0 && tmin < 1) {
			const double mults = floor(200.0 / -log10(tmin));
			/* the sparse tetraploid pass checks twice per block (every 4 loci = 16 multiplications) */
			blocks = (int)(mults / (sh.ploidy == 4 ? 16.0 : 8.0 * sh.ploidy));
			if (blocks > 1 << 16) blocks = 1 << 16;
		}
		g.flush_blocks = blocks;
		/* Supported lower bounds (--bound): any value >= 0.  The fast kernels share one reciprocal among the four cells of a
		 * column-pass step (1 / (t0 t1 t2 t3)) and between the two copies of a locus, which needs every t > 0 and
		 * t^4 >= DBL_MIN: guaranteed when projection is on and p_lb >= 1e-75 (t >= p_lb).  Otherwise -- projection off
		 * (--projection: an unobserved allele column, e.g. the phantom slot of a locus with missing data or an allele a
		 * bootstrap replicate lacks, has P = 0 for every k, so t = 0 in its zero-count cells) or a smaller bound -- the
		 * kernels take one reciprocal per non-empty cell and zero-count cells contribute exactly 0, as in em_alg.c:338-342.
		 * A non-empty cell with t = 0 is NaN here as it is in the reference (n * 0 / 0). */
		g.safe_rcp = (!do_projection || !(p_lb >= 1e-75)) ? 1 : 0;
		if (kn.force_safe) g.safe_rcp = 1;
		if (g.safe_rcp) g.flush_blocks = 0;
	}
	return g;
}

/* the pass arguments that shape, geometry and knobs give: everything the plan reads, no buffer */
static mchip_pass_args shape_args(const mchip_shape &sh, const mchip_geometry &g, const mchip_knobs &kn, int K, int qstride, int has_missing)
{
	mchip_pass_args a;
	memset(&a, 0, sizeof a);
	a.I = sh.I; a.L = sh.L; a.T = sh.T; a.ploidy = sh.ploidy; a.K = K;
	a.count_bits = sh.count_bits; a.has_missing = has_missing;
	a.qstride = qstride;
	a.ichunk = g.ichunk; a.n_ichunks = g.n_ichunks;
	a.flush_blocks = g.flush_blocks;
	a.safe_rcp = g.safe_rcp;
	a.lchunk = g.lchunk; a.n_lchunks = g.n_lchunks;
	a.sparse = g.sparse; a.tile_cols = 8 * sh.max_M;
	a.biallelic = (sh.min_M == 2 && sh.max_M == 2 && !kn.no_bial) ? 1 : 0;
	a.ind_waves = g.ind_waves;
	a.xcd_rows = g.xcd_rows;
	a.no_col_split = kn.no_col_split;
	return a;
}

mchip_shape shape_of(const mchip_context *ctx)
{
	return mchip_shape{ ctx->I, ctx->L, ctx->T, ctx->ploidy, ctx->min_M, ctx->max_M, ctx->count_bits };
}

mchip_pass_args pass_args(mchip_context *ctx, int slot)
{
	mchip_pass_args a = shape_args(shape_of(ctx), ctx->geo, ctx->knob, ctx->K, ctx->qstride, ctx->has_missing);
	a.gtA = ctx->d_gtA; a.gtS = ctx->d_gtS; a.gtC = ctx->d_gtC;
	a.ua = ctx->d_ua; a.toff = ctx->d_toff; a.col_locus = ctx->d_col_locus; a.col_allele = ctx->d_col_allele;
	a.P = ctx->d_p[slot]; a.Q = ctx->d_q[slot];
	a.Apart = ctx->d_Apart; a.llpart = ctx->d_llpart; a.Spart = ctx->d_Spart;
	a.asA = ctx->d_asA; a.asS = ctx->d_asS;
	return a;
}

/* partial log likelihoods k_mix_finalize leaves: one per workgroup */
int mix_ll_parts(int I) { return (I + MCHIP_BLOCK - 1) / MCHIP_BLOCK; }
/* the projection of P keeps its "fixed" flags in registers up to 64 alleles per locus, above that in d_flags */
bool needs_byte_flags(int max_M) { return max_M > 64; }

/* the plan of these arguments, less what the knobs switch off */
mchip_plan plan_for(const mchip_ktable *kt, const mchip_pass_args &a, const mchip_knobs &kn)
{
	mchip_plan p;
	kt->plan(a, &p);
	if (kn.no_pair) p.pair = 0;
	if (kn.no_dual) p.dual = 0;
	return p;
}

/* loci per block of k_finalize_p_tile for this data set and K, or 0 where a locus can outgrow the tile (k_finalize_p then) */
int finalize_p_loci(int K, int max_M)
{
	if (max_M > 64 || max_M < 1) return 0;
	const int n = FP_TILE / (max_M * K);
	return n >= 4 ? n : 0;
}

estep_finish finish_for(const mchip_plan &p, int K, int max_M, bool indiv, int do_mstep, const mchip_knobs &kn)
{
	estep_finish f;
	f.p_loci = finalize_p_loci(K, max_M);
	f.slab_sum = p.col_slabs > 8 && !kn.no_slab_sum;
	f.fused = do_mstep && indiv && f.p_loci && !f.slab_sum && !kn.no_fused_finalize;
	return f;
}

extern "C" {

/* How an instance is spelled: its kernel's name and, in the order of the kernel's template arguments, the fields of mchip_instance
 * that are those arguments (p pl, b bits, A accum, S safe, N nomiss, L ll, M mix, D dual, G staged). */
static const struct { const char *name, *args; } kernel_names[MCHIP_K_KINDS] = {
	{ "", "" },
	{ "k_column_pass", "pASL" },
	{ "k_column_counts", "bMS" },
	{ "k_column_counts_split", "bS" },
	{ "k_individual_pass", "p" },
	{ "k_individual_sparse", "pASND" },
	{ "k_individual_sparse_w", "pASND" },
	{ "k_individual_bial", "AN" },
	{ "k_estep_pair", "bpSN" },
	{ "k_mix_gather", "pG" },
	{ "k_mix_column", "p" },
};
static std::string instance_name(const mchip_instance &k)
{
	std::string out = kernel_names[k.kernel].name;
	for (const char *c = kernel_names[k.kernel].args; *c; c++) {
		const bool flag = *c == 'A' ? k.accum : *c == 'S' ? k.safe : *c == 'N' ? k.nomiss : *c == 'L' ? k.ll : *c == 'M' ? k.mix : *c == 'D' ? k.dual : k.staged;
		out += c == kernel_names[k.kernel].args ? "<" : ",";
		out += *c == 'p' ? std::to_string(k.pl) : *c == 'b' ? std::to_string(k.bits) : flag ? "true" : "false";
	}
	return out + ">";
}

int mchip_describe_plan(const mchip_plan_query *q, char *buf, int buf_len)
{
	if (!q || !buf || buf_len < 1) return MCHIP_ERR_INVALID;
	if (q->K < 1 || q->I < 1 || q->L < 1 || q->T < 1 || q->ploidy < 1 || q->ploidy > 64 || q->min_alleles > q->max_alleles ||
	    q->max_alleles < 1 || q->max_alleles > 255 || q->n_cu < 1)
		return MCHIP_ERR_INVALID;
	if (q->K > MCHIP_MAX_K) return MCHIP_ERR_UNSUPPORTED;
	mchip_knobs kn;
	read_knobs(&kn);
	const int K = q->K, indiv = q->admixture && !q->eta_constrained;
	const mchip_shape sh = { q->I, q->L, q->T, q->ploidy, q->min_alleles, q->max_alleles, count_bits_for(q->ploidy, kn) };
	const mchip_geometry g = model_geometry(sh, K, q->admixture, q->do_projection, q->p_lb, kn, q->n_cu);
	const mchip_pass_args a = shape_args(sh, g, kn, K, indiv ? K : 0, q->has_missing);
	const mchip_plan p = plan_for(mchip_get_ktable(K), a, kn);
	const estep_finish fin = finish_for(p, K, sh.max_M, indiv, 1, kn);
	std::vector<std::string> lines;
	auto launch = [&](const std::string &name) {
		for (const std::string &l : lines) if (l == name) return;
		lines.push_back(name);
	};
	auto fact = [&](const char *key, long v) { lines.push_back(std::string(key) + "=" + std::to_string(v)); };
	const char *finalize_p = fin.p_loci ? "k_finalize_p_tile" : "k_finalize_p";	/* (launch_finalize_p) */
	if (!q->admixture) {	/* run_mixture, with and without the M step, whatever the calls */
		launch(instance_name(p.mix_gather));
		launch("k_mix_finalize");
		launch(instance_name(p.mix_col));
		launch(finalize_p);
	} else {
		if (q->accel_cycle && p.col.ll) return MCHIP_ERR_UNSUPPORTED;	/* (mchip_accel_run: the dense pair runs cycle by cycle) */
		/* run_estep with the M step: the passes, then the finalisers */
		if (p.pair) launch(instance_name(p.pair_pass));	/* (one launch that runs the bodies of the two below) */
		launch(instance_name(p.col));
		launch(instance_name(p.sside));
		if (fin.fused) launch("k_finalize_qp");
		else {
			launch("k_finalize_q");
			if (fin.slab_sum) launch("k_sum_slabs");
			launch(finalize_p);
		}
		if (q->accel_cycle) {	/* accel_cycle_enqueue: log L of the second EM iterate and of the extrapolated point */
			if (p.dual) launch(instance_name(p.dual_pass));
			else { launch(instance_name(p.ll)); launch(instance_name(p.sside)); }
		} else {
			launch(instance_name(p.ll));						/* mchip_loglik */
			if (p.col.ll) launch(instance_name(p.ll));				/* mchip_e_step: run_estep without the M step */
			launch(instance_name(p.sside));
			launch("k_finalize_q");
			launch(instance_name(p.col.ll ? p.ll : p.sside));			/* mchip_loglik_prefetch */
		}
	}
	fact("n_ichunks", g.n_ichunks); fact("lchunk", g.lchunk); fact("n_lchunks", g.n_lchunks);
	fact("ind_waves", g.ind_waves); fact("xcd_rows", g.xcd_rows); fact("sparse", g.sparse);
	fact("col_slabs", q->admixture ? p.col_slabs : p.mix_col_slabs);
	fact("ind_slabs", p.ind_slabs);
	fact("ll_parts", q->admixture ? p.ll_parts : mix_ll_parts(q->I));
	fact("pair", q->admixture ? p.pair : 0); fact("dual", q->admixture ? p.dual : 0);
	fact("shared_eta", !indiv); fact("byte_flags", needs_byte_flags(sh.max_M));
	std::string out;
	for (const std::string &l : lines) out += l + "\n";
	if (out.size() >= (size_t)buf_len) return MCHIP_ERR_INVALID;
	memcpy(buf, out.c_str(), out.size() + 1);
	return MCHIP_OK;
}

}	/* extern "C" */
