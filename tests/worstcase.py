"""Worst-case parameters for the streaming EM passes, and a long-double reference of one EM step.

The rest of the suite draws Q and P from Dirichlet(1): every t = sum_k q_k p_k a kernel sees there is 0.1 to 0.5, and the two
numerical contracts of DESIGN.md section 4.2 are never near their limits:

  * the running-product log likelihood is looked at every `flush_blocks` units of 16 multiplications, an interval the host
    sizes (model_geometry, mchip_plan.hip) so that a product that starts above 1e-100 stays above 1e-300;
  * shared reciprocals (rcp4, rcp_group, the pair and the tetraploid four of the individual side, k_individual_bial's
    rcp_full(t0 t1)) are allowed down to a bound of 1e-75.

This module builds the inputs that are: bounds at the edge of each `flush_blocks` value (`edge_bound`), allele columns whose
P is the bound for every k ("tiny": t = lb whatever Q is, Q summing to 1) or the value `med` that takes the product to just
above 1e-100 in one look's worth of multiplications ("medium"), rows and columns of homozygotes that line these up against the
look grid, and heterozygotes that put one t at the bound beside one of order 1 under a shared reciprocal.  `reference_step`
restates one EM step in numpy.longdouble; it shares no code with oracle/ (only the projection, applied to the rounded result).

What legal parameters can reach: the host sizes the interval for t >= lb / K, but every t is >= lb (the q_k sum to 1), so the
largest fall between two looks is n (-log10 lb) decades, n = 16 flush_blocks, from just above 1e-100: 1e-300 at K = 1 and
16 b log10(1.001 K) decades less at K > 1 (`deepest_log10`).  A look that comes half as often lets two looks' worth of tiny
factors follow a product that stands just above 1e-100: 100 + 2 n (-log10 lb) > 324 decades at every edge bound, so 0.

The pattern of a worst row, in blocks of one look's worth of loci (`unit`): A B C D, repeating.  C and D are tiny.  A B has
to end between 1e-100 and 1e-97.4 with no look of either interval having rescaled the product on the way, so that C is
the deepest fall with the right interval and C D underflow with a doubled one.  From a product of exactly 1 (the row
begins with B, or with an A of missing copies, slots of exactly 1, where the case has missing copies) B is all medium and
ends at 1.001^n 1e-100: the start of the deepest legal fall.  Anywhere else the product in front of A B is the mantissa a
rescale left, in [0.5, 1): n medium factors would end below 1e-100 and be rescaled.  There A B is made of ordinary
copies (the likelier of alleles 2 and 3, t >= 0.49; missing copies in A where the case has them), which from its end
backwards become medium ones while the sum stays above -99.7 decades (`build`).
What is covered (`row_shifts`): the first four rows start at A, B, C and D exactly (the row that starts at B reaches the
deepest legal product; B ends at an even look in the rows that start at A and C, which is what a doubled interval
needs); the others are shifted by 5, 10, ... loci, which with 27 worst rows is every residue modulo `unit` (at most 24)
against the look grid, and 27 of the 4 `unit` against the period.  L is 7 `unit` + 2 where that exceeds 130, so that
every shift holds a whole B C D.  The 1e-8 control keeps the plain pattern, medium for one look and tiny for three (A is
tiny, B all medium, no missing copies in a worst row): with the full pattern a doubled interval would show there too
(100 + 2 16 8 = 356 decades); the control records that two looks' worth of tiny factors alone (256) cannot.
The biallelic family has the pattern in P, so all its worst rows share two alignments: B C D A A B C D from locus 0 (the
first B exact, the second ending at an even look) and, after three random loci, A B C D again, misaligned by three loci;
L is 12 `unit` + 3 where that exceeds 130.  Its ordinary copies are 1 - lb at a tiny locus and 1 - med at a medium one.
The worst columns of the dense family (every 4th locus) carry one pattern per column with the same shifts, over
I = 7 `unit` + 3 individuals where that exceeds 131; a column sees slots of 1 wherever its allele is absent.

All cases run with one chunk per axis (WHOLE_AXIS).  A chunk restarts the product, and the blocks above are laid against
the look grid of a chunk that begins at locus (individual) 0; cut anywhere else, A B no longer ends at a look and the
case loses its teeth without failing.  More than one chunk, and the default launch geometry, are what
test_gpu_kernel_matrix.py and test_gpu_parity.py run."""
import math

import numpy as np

import oracle_bind as ob

MISSING = 0xFF
I_DEFAULT, L_DEFAULT = 131, 130
K_VALUES = (1, 2, 5, 6, 10, 12, 13, 20, 21, 27, 28, 36, 37, 48, 49, 64)
K_SHARED = (8, 28, 64)
FAMILIES = ("dip", "bial", "tet", "dense", "shared")
BOUNDS = ("edge1", "edge2", "edge3", "1e-75", "1e-8")
# whole-axis chunks: a chunk restarts the product, and at small K the default geometry cuts 130 loci into chunks of two looks
# (model_geometry: min_lchunk = ceil(8 K / (slab_frac ploidy)) > L leaves one chunk; likewise min_ichunk > I)
WHOLE_AXIS = {"MCHIP_SLAB_FRAC": "0.001"}
WORST_ROW_EVERY, WORST_COL_EVERY, VERTEX_EVERY = 5, 4, 5       # worst rows 0, 5, ...; vertex rows 2, 7, ...


# ------------------------------------------------------------------------------------------------------------ the host's sizing
def host_flush_blocks(K, p_lb, ploidy=2, projection=True):
    """model_geometry (mchip_plan.hip), the block behind "log-product check interval":
        tmin = p_lb / K;  mults = floor(200.0 / -log10(tmin));  blocks = (int)(mults / (ploidy == 4 ? 16.0 : 8.0 * ploidy));
        safe_rcp = !do_projection || !(p_lb >= 1e-75);  if (safe_rcp) flush_blocks = 0
    Returns (safe_rcp, flush_blocks)."""
    safe = (not projection) or not (p_lb >= 1e-75)
    tmin = p_lb / K
    blocks = 0
    if projection and 0 < tmin < 1:
        mults = math.floor(200.0 / -math.log10(tmin))
        blocks = min(int(mults / (16.0 if ploidy == 4 else 8.0 * ploidy)), 1 << 16)
    return safe, (0 if safe else blocks)


def edge_bound(K, b, unit=16):
    """the smallest p_lb (to 0.1 %) for which model_geometry yields flush_blocks == b on diploid and tetraploid data, where a
    unit is 16 multiplications: K 10^(-200 / (unit b)) 1.001"""
    lb = K * 10.0 ** (-200.0 / (unit * b)) * 1.001
    for ploidy in (2, 4):
        assert host_flush_blocks(K, lb, ploidy) == (False, b), (K, b, lb)
        assert host_flush_blocks(K, lb / 1.003, ploidy) == (False, b - 1), (K, b, lb)
    return lb


def medium(n):
    """n factors of it leave a product of 1 about 1.6 % above 1e-100: one look finds it not yet to be rescaled"""
    return 10.0 ** (-100.0 / n) * 1.001


def deepest_log10(lb, n):
    """log10 of the smallest product legal parameters reach with the right interval: n factors of lb from just above 1e-100"""
    return -100.0 + n * math.log10(lb)


# ------------------------------------------------------------------------------------------------------------------- the cases
def make_case(family, K, bound, missing):
    ploidy = 4 if family == "tet" else 2
    if bound.startswith("edge"):
        lb = edge_bound(K, int(bound[4:]))
    else:
        lb = float(bound)
    safe, blocks = host_flush_blocks(K, lb, ploidy)
    b = max(blocks, 1)                    # 1e-75: no interval (the individual side looks after every copy); the pattern of b = 1
    n = 16 * b
    med = medium(n)
    assert med >= lb, (K, bound, med, lb)
    knobs = dict(WHOLE_AXIS)
    if family == "dense":
        knobs["MCHIP_FORCE_DENSE"] = "1"
    unit = n // ploidy                      # loci (for a column: individuals) of one look's worth of homozygotes
    L = max(L_DEFAULT, 12 * unit + 3 if family == "bial" else 7 * unit + 2)
    I = max(I_DEFAULT, 7 * (n // 2) + 3 if family == "dense" else 0)
    return dict(family=family, K=K, bound=bound, lb=lb, missing=0.01 if missing else 0.0, ploidy=ploidy, I=I, L=L,
                model="admix_c" if family == "shared" else "admix", knobs=knobs, flush_blocks=blocks, safe_rcp=safe,
                n=n, med=med, seed=7919 * K + 101 * FAMILIES.index(family) + 13 * BOUNDS.index(bound) + int(missing))


def all_cases():
    out = []
    for family in FAMILIES:
        for K in (K_SHARED if family == "shared" else K_VALUES):
            for bound in BOUNDS:
                for missing in (False, True):
                    out.append(make_case(family, K, bound, missing))
    return out


def case_id(c):
    return "%s-K%d-%s-%s" % (c["family"], c["K"], c["bound"], "miss" if c["missing"] else "nomiss")


def is_edge(c):
    return c["bound"].startswith("edge")


def worst_rows(c):
    return list(range(0, c["I"], WORST_ROW_EVERY))


def worst_cols(c):
    """loci whose genotypes carry the pattern over individuals: the dense family, whose column pass carries the log likelihood"""
    return list(range(3, c["L"], WORST_COL_EVERY)) if c["family"] == "dense" else []


def reaches_1e280(c):
    """whether the deepest legal product of an edge case is below 1e-280: where 16 b log10(1.001 K) < 20"""
    d = deepest_log10(c["lb"], c["n"])
    assert abs(d + 280.0) > 0.2, (case_id(c), d)        # nothing sits on the edge
    return d < -280.0


A, B, C, D = 0, 1, 2, 3


def block(pos, unit):
    """which block of the period A B C D a position falls in, and whether it is the block's last position"""
    pos %= 4 * unit
    return pos // unit, pos % unit == unit - 1


def row_shifts(count, unit):
    """where in the period each worst row (or column) starts: at A, B, C, D exactly, then 5, 10, ... positions in"""
    return [0, unit, 2 * unit, 3 * unit] + [5 * m for m in range(1, count - 3)]


def bounded_simplex(x, lb):
    """rows clipped to the bound and the others renormalised, until nothing is below it: entries ON the bound, sum 1"""
    x = np.array(x, dtype=np.float64)
    fixed = np.zeros(x.shape, dtype=bool)
    for _ in range(x.shape[-1] + 1):
        fixed |= x < lb
        free = np.where(fixed, 0.0, x)
        scale = (1.0 - lb * fixed.sum(axis=-1, keepdims=True)) / np.maximum(free.sum(axis=-1, keepdims=True), 1e-300)
        x = np.where(fixed, lb, free * scale)
        if not (x < lb).any():
            break
    assert (x >= lb).all() and np.allclose(x.sum(axis=-1), 1.0, rtol=0, atol=1e-14)
    return x


def build(c):
    """(ua, geno, q0, p0) of a case; q0 is (I, K), or (K,) for shared mixing proportions"""
    K, I, L, pl, lb, med = c["K"], c["I"], c["L"], c["ploidy"], c["lb"], c["med"]
    rs = np.random.default_rng(c["seed"])
    bial = c["family"] == "bial"
    M = 2 if bial else 4
    ua = np.full(L, M, dtype=np.int32)
    unit = (c["n"] // pl)                       # loci (or, for a column, individuals) per look: n / ploidy homozygotes
    rows = worst_rows(c)

    # ---- P: (K, T), T = M L
    p = np.empty((K, L, M))
    if bial:
        # the pattern lives in P: B C D A A B C D from locus 0, three random loci, then A B C D again from an odd locus
        role = np.full(L, -1)
        layout = [B, C, D, A, A, B, C, D]
        for l in range(L):
            if l < 8 * unit:
                role[l] = layout[l // unit]
            elif 8 * unit + 3 <= l < 12 * unit + 3:
                role[l] = (l - (8 * unit + 3)) // unit
        kind = np.where(role == B, 1, np.where(role >= 0, 0, -1))       # P of the locus: 1 medium, 0 tiny, -1 random
        p[:, :, 1] = lb + (1.0 - 2.0 * lb) * rs.random((K, L))
        p[:, kind == 1, 1] = med
        p[:, kind == 0, 1] = 1.0 - lb
        p[:, :, 0] = 1.0 - p[:, :, 1]
        p[:, kind == 0, 0] = lb
    else:
        p[:, :, 0] = lb
        p[:, :, 1] = med
        rest = 1.0 - lb - med
        split = rs.random((K, L))
        p[:, :, 2] = lb + (rest - 2.0 * lb) * split
        p[:, :, 3] = rest - p[:, :, 2]
    assert (p >= lb).all()
    p0 = np.ascontiguousarray(p.reshape(K, L * M))

    # ---- Q
    q = bounded_simplex(rs.dirichlet(np.ones(K), size=I), lb)
    for i in range(2, I, VERTEX_EVERY):         # rows at a vertex: most of the row exactly on the bound
        q[i] = lb
        q[i, i % K] = 1.0 - (K - 1) * lb
    q0 = np.ascontiguousarray(bounded_simplex(rs.dirichlet(np.ones(K)), lb) if c["model"] == "admix_c" else q)

    # ---- genotypes: uniform over the alleles (heterozygotes tiny / ordinary), 1 % missing, then the worst rows and columns
    geno = rs.integers(0, M, size=(I, L, pl)).astype(np.uint8)
    if c["missing"]:
        geno[rs.random(geno.shape) < c["missing"]] = MISSING
    qf = full_q(q0, I)
    plain = c["bound"] == "1e-8"                # the control: B C D D, nothing left unrescaled at 1e-100 in front of two looks
    lmed = math.log10(med)
    for i, shift in zip(rows, row_shifts(len(rows), unit)):
        span = []                               # the loci of the A B in hand
        for l in range(L + 1):
            if l == L:
                blk = -1
            elif bial:
                blk = role[l]
                if blk < 0:
                    geno[i, l, :] = rs.integers(0, 2, size=pl)
            else:
                blk, _ = block(l + shift, unit)
            if blk in (A, B) and not plain:
                span.append(l)
                continue
            if blk >= 0:
                geno[i, l, :] = 1 if blk == B else 0
            if not span:
                continue
            # A B ends here.  In front of it stands a product of exactly 1 (the row begins) or the mantissa a rescale left,
            # in [0.5, 1); behind it C and D.  It has to end between 1e-100 and 1e-97.4 without a look of either interval
            # having rescaled it on the way: all its copies are ordinary ones (the likelier of alleles 2 and 3; missing in A
            # where the case has missing copies), and from its end backwards they become medium while the sum stays above
            # -99.7 decades.  From an exact 1, B is all medium: 1.001^n 1e-100, the start of the deepest legal fall.
            exact = span[0] == 0 and (bool(c["missing"]) or (role[0] if bial else block(shift, unit)[0]) == B)
            ordinary, cost = {}, 0.0
            for m in span:
                in_a = (role[m] if bial else block(m + shift, unit)[0]) == A
                if in_a and c["missing"]:
                    geno[i, m, :] = MISSING
                    continue
                if bial:
                    al = 1 if in_a else 0       # 1 - lb at a tiny locus, 1 - med at a medium one
                    conv = not in_a
                else:
                    al, conv = 2 + int(qf[i] @ p[:, m, 3] > qf[i] @ p[:, m, 2]), True
                geno[i, m, :] = al
                t = math.log10(float(qf[i] @ p[:, m, al]))
                cost += pl * t
                if conv:
                    ordinary[m] = t
            for m in reversed(span):
                if m not in ordinary:
                    continue
                for a in reversed(range(pl)):
                    if exact and (role[m] if bial else block(m + shift, unit)[0]) == B:
                        geno[i, m, a] = 1
                    elif not exact and cost - ordinary[m] + lmed >= -99.7:
                        geno[i, m, a] = 1
                        cost += lmed - ordinary[m]
            span = []
    # worst columns (written last: in the dense family the column side carries the log likelihood).  A column sees only the
    # copies of its own allele, slots of 1 otherwise, so the tiny allele's product is brought to just above 1e-100 by the
    # head of the tiny run itself: the last `lead` copies of block B are tiny ones, in front of the look that ends B, and
    # C and D follow.  Individuals of block A are homozygous for an ordinary allele, the others of B for the medium one.
    lead = 0 if plain else int(100.0 / -math.log10(lb))
    cols = worst_cols(c)
    for l, shift in zip(cols, row_shifts(len(cols), unit)):
        for i in range(I):
            blk, _ = block(i + shift, unit)
            left = 2 * (unit - (i + shift) % unit) if blk == B else 0      # copies from this individual to the end of B
            geno[i, l, :] = 2 + (i + l) % 2 if blk == A else 1 if blk == B else 0
            if blk == B and left <= lead:
                geno[i, l, :] = 0
            elif blk == B and left == lead + 1:
                geno[i, l, 0] = 0               # one more copy of the tiny allele in front of the run: a heterozygote
    return ua, np.ascontiguousarray(geno), q0, p0


# -------------------------------------------------------------------------------------------------------- the product rule's input
def counts(ua, geno):
    """n_ic, (I, T)"""
    I, L, pl = geno.shape
    toff = np.concatenate(([0], np.cumsum(ua)))[:-1]
    n = np.zeros((I, int(ua.sum())), dtype=np.int64)
    ii, ll = np.meshgrid(np.arange(I), np.arange(L), indexing="ij")
    for a in range(pl):
        g = geno[:, :, a]
        ok = g != MISSING
        np.add.at(n, (ii[ok], (toff[ll] + g)[ok]), 1)
    return n


def full_q(q, I):
    return np.broadcast_to(q, (I, q.shape[-1])) if q.ndim == 1 else q


def row_slots(c, ua, geno, q, p, i):
    """what the individual-side passes multiply for individual i, in order: one slot per copy, 1.0 for a missing one"""
    toff = np.concatenate(([0], np.cumsum(ua)))[:-1]
    qi = full_q(q, geno.shape[0])[i]
    out = []
    for l in range(geno.shape[1]):
        for a in range(geno.shape[2]):
            g = geno[i, l, a]
            out.append(1.0 if g == MISSING else float(qi @ p[:, toff[l] + g]))
    return out


def col_slots(c, ua, geno, q, p, l, m):
    """what the dense column pass multiplies for allele column (l, m): `ploidy` slots per individual, t for each copy of m"""
    toff = np.concatenate(([0], np.cumsum(ua)))[:-1]
    qf = full_q(q, geno.shape[0])
    out = []
    for i in range(geno.shape[0]):
        nc = int((geno[i, l, :] == m).sum())
        t = float(qf[i] @ p[:, toff[l] + m])
        out += [t] * nc + [1.0] * (geno.shape[2] - nc)
    return out


def simulate_product(slots, interval):
    """The kernels' rule in double precision: multiply, look every `interval` slots, move the exponent out below 1e-100 (rescale()
    of kernels_k/common.h: frexp), one log at the end.  Returns (log of the product, smallest product seen)."""
    prod, ex, low = 1.0, 0, 1.0
    for s, t in enumerate(slots, 1):
        prod *= t
        low = min(low, prod)
        if s % interval == 0 and prod < 1e-100:
            mant, e = math.frexp(prod)
            prod, ex = mant, ex + e
    return (ex * math.log(2.0) + math.log(prod)) if prod > 0.0 else -math.inf, low


# ------------------------------------------------------------------------------------------------------------ the reference
def reference_step(ua, geno, q, p, lb, model="admix"):
    """One EM step in numpy.longdouble: logL = sum n log t, S_ik = q_ik sum_c n_ic p_kc / t_ic, A_kc = p_kc sum_i n_ic q_ik / t_ic,
    Q1 and P1 the normalised sums rounded to double and projected onto the bounded simplex.  Returns (logL, Q1, P1, S)."""
    ld = np.longdouble
    assert np.finfo(ld).eps < 2.0 ** -60, "this platform's long double is no wider than double"
    I, L, _ = geno.shape
    K = p.shape[0]
    n = counts(ua, geno).astype(ld)
    Q = np.array(full_q(np.asarray(q), I), dtype=ld)
    P = np.asarray(p).astype(ld)
    t = Q @ P                                                   # (I, T)
    logL = (n * np.log(t)).sum()
    r = n / t
    S = Q * (r @ P.T)                                           # (I, K)
    A = P * (Q.T @ r)                                           # (K, T)
    if model == "admix_c":
        eta = S.sum(axis=0)
        q1 = ob.michelot((eta / eta.sum()).astype(np.float64), lb)
    else:
        q1 = (S / S.sum(axis=1, keepdims=True)).astype(np.float64)
        for i in range(I):
            q1[i] = ob.michelot(q1[i], lb)
    p1 = np.empty(p.shape, dtype=np.float64)
    off = 0
    for l in range(L):
        M = int(ua[l])
        blockA = A[:, off:off + M]
        norm = (blockA / blockA.sum(axis=1, keepdims=True)).astype(np.float64)
        for k in range(K):
            p1[k, off:off + M] = ob.michelot(norm[k], lb)
        off += M
    return float(logL), q1, p1, S.astype(np.float64)


def oracle_step(c, ua, geno, q, p):
    """the suite's oracle, fused order: (logL, Q1, P1, S)"""
    con = int(c["model"] == "admix_c")
    opt = ob.make_options(admixture=1, eta_constrained=con, do_projection=1, lower_bound=c["lb"], fused=1, abs_error=0.0)
    mod = ob.Model(ob.Data(c["I"], c["L"], c["ploidy"], ua, geno), opt, c["K"])
    mod.q(0)[...] = q
    mod.p(0)[...] = p
    mod.em_step()
    return mod.logL, mod.q(mod.pindex).copy(), mod.p(mod.pindex).copy(), mod.sik().copy()


def ratios(got, want):
    """largest |difference| / tolerance of (logL, Q1, P1, S) at the suite's step-1 tolerances
    (tests/test_gpu_parity.py: test_em_steps_vs_oracle_paths)"""
    def arr(a, b, rtol, atol):
        return float((np.abs(a - b) / (atol + rtol * np.abs(b))).max())
    return (abs(got[0] - want[0]) / max(1e-8, 1e-12 * abs(want[0])), arr(got[1], want[1], 1e-11, 1e-15),
            arr(got[2], want[2], 1e-11, 1e-15), arr(got[3], want[3], 1e-11, 1e-12))
