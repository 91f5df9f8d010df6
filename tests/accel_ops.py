"""Inputs, references and checkers for the acceleration vector ops (secants, step-size dot products, extrapolation, Michelot
projection): tests/test_accel_ops_cpu.py holds them to exact arithmetic and to mutants, tests/test_gpu_accel_ops.py holds the
HIP kernels to them.  Nothing here needs a GPU; a `ctx` argument is a multiclust_amd.Context.

Everything is staged through the C-ABI without an EM step: the base slot takes arbitrary finite values, the secant buffers
arbitrary u and v, so the genotypes only fix I, L and the allele counts.

Row families of the projection tests (`FAMILIES`; row i of Q, and block number l * K + k of P, is family `i % 7`; a family that
cannot be built at a row length falls back to (c), and `labels` of the case says what every row is):

  a  already on the simplex
  b  all entries positive, the sum far from 1 (1e-3, 0.3, 7, 1e3 in turn)
  c  about half the entries far negative
  d  a geometric cascade -1e6 r^-k (k = 0 .. n-1; r = 2, 1.5, 3, 1.25 in turn) in permuted order: no entry exceeds 1e6 in size,
     a few entries are fixed per round, so the loop runs for many rounds
  e  one large positive entry, the others negative: all but one entry end fixed
  f  (length >= 3, bound >= 1e-12) an exact tie: the first shift is s1 = j 2^-52 exactly (the row's serial sum is tuned to
     1 + n j 2^-52 through one entry), entry B = lb + s1 exactly, so B - s1 == lb: not below the bound, not fixed, while another
     entry is fixed in the same round and the next round's shift takes B below.  These rows come in through the base slot with
     zero secants (the update then reproduces the base exactly), because the tie needs every bit of the row
  g  (length > 32) every entry of index >= 32 far negative (fixed in round 1), a cascade below index 32 that goes on for rounds
"""
import math
from fractions import Fraction

import numpy as np

import oracle_bind as ob

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the dot-product reference needs a long double wider than double"
EPS = 2.0 ** -53                      # unit roundoff of double
FAMILIES = "abcdefg"
MODELS = {"admix": (1, 0), "admix_c": (1, 1), "mix": (0, 0)}      # (admixture, eta_constrained) of mchip_set_model
# (u_index, v_index) of mchip_multisecant_update: 0, 1, 4 and 9 terms as mc_qn_accelerated_update orders them (q = 1; q = 2 with
# delta_index 1; q = 3 with delta_index 2), and one that repeats an index out of that order
MULTI_PATTERNS = [(0, []), (0, [0]), (1, [1, 1, 0, 0]), (0, [2, 2, 2, 0, 0, 0, 1, 1, 1]), (2, [2, 0, 2, 2])]


# ------------------------------------------------------------------------------------------------------------------ shapes
def make_shape(K, I, ua, model="admix", ploidy=2):
    ua = np.asarray(ua, dtype=np.int32)
    return dict(K=K, I=I, ua=ua, T=int(ua.sum()), model=model, ploidy=ploidy, nq=I * K if model == "admix" else K)


def ua_for(T, M=64):
    """allele counts of T columns in loci of M alleles (and one shorter locus for the rest)"""
    return np.array([M] * (T // M) + ([T % M] if T % M else []), dtype=np.int32)


def draw_genotypes(shape, seed=0):
    """every copy observed (so no individual is without data), except at a locus with no allele at all"""
    rng = np.random.default_rng(seed)
    ua, I, pl = shape["ua"], shape["I"], shape["ploidy"]
    g = (rng.random((I, len(ua), pl)) * ua[None, :, None]).astype(np.uint8)
    g[:, ua == 0, :] = 0xFF
    return g


def dots_shapes():
    """The smallest sizes that reach each edge of the dot-product kernels, n = I * K and n = K * T alike: 1; 255 (one partly filled
    block); 4096 and 4097 (grid 1 -> 2); just above 256 * 4096 (more than 256 partials: a second term per thread of
    block_ordered_sum); just above 2 097 152 (the 512-block cap, an uneven grid-stride tail) -- the last two once on the P side
    (K = 64, 16 449 / 32 833 allele columns, 5 individuals) and once on the Q side (16 449 / 32 833 individuals, 8 biallelic loci)."""
    return [make_shape(1, 1, [1]), make_shape(15, 17, [8, 9]), make_shape(16, 256, ua_for(256)), make_shape(17, 241, ua_for(241)),
            make_shape(64, 5, ua_for(16449)), make_shape(64, 5, ua_for(32833)),
            make_shape(64, 16449, [2] * 8), make_shape(64, 32833, [2] * 8)]


def p_side_shapes(K, I=9):
    """the P side's paths: loci of 1, 2, 8 alleles (michelot_small), 9, 32, 33, 64 (michelot_strided with the bit mask; 33 and 64
    set bits of index >= 32) and one without an allele column, twice each so that every family meets every length -- and the same
    with 65 and 100 alleles added (byte flags for those two; the flag array then exists for every locus)"""
    return [make_shape(K, I, [1, 2, 8, 9, 32, 33, 64, 0] * 2), make_shape(K, I, [1, 2, 8, 9, 32, 33, 64, 65, 100, 0] * 2)]


def shape_id(s):
    return "%s-K%d-I%d-T%d" % (s["model"], s["K"], s["I"], s["T"])


def install(ctx, shape, do_projection, lb, n_secants=3):
    ctx.set_genotypes(shape["ua"], draw_genotypes(shape))
    adm, con = MODELS[shape["model"]]
    ctx.set_model(shape["K"], admixture=adm, eta_constrained=con, do_projection=do_projection, lower_bound=lb, n_secants=n_secants)


def qshape(shape):
    return (shape["I"], shape["K"]) if shape["model"] == "admix" else (shape["K"],)


# ------------------------------------------------------------------------------------------------------------------ element-wise
def random_pair(shape, rng, scale=1.0):
    """(q, p) in boundary order, every element distinct and random, mixed signs, magnitudes over six decades"""
    def draw(sh):
        return scale * rng.standard_normal(sh) * np.exp(rng.uniform(-7, 7, sh))
    return draw(qshape(shape)), draw((shape["K"], shape["T"]))


def random_state(shape, seed):
    rng = np.random.default_rng(seed)
    return dict(x=[random_pair(shape, rng) for _ in range(3)], u=[random_pair(shape, rng) for _ in range(3)],
                v=[random_pair(shape, rng) for _ in range(3)])


def stage(ctx, st, slots=(0, 1, 2)):
    for sl in slots:
        ctx.set_q(sl, st["x"][sl][0])
        ctx.set_p(sl, st["x"][sl][1])
    for j in range(3):
        ctx.set_secant(0, j, st["u"][j][1], st["u"][j][0])
        ctx.set_secant(1, j, st["v"][j][1], st["v"][j][0])


def ref_accel(x0, u, v, s, qn_form):
    """k_accel_update's expression, every product and sum rounded, in the reference's order"""
    if qn_form:
        return (x0 + u) + s * v
    return (x0 - (2 * s) * u) + (s * s) * (v - u)


def ref_multisecant(base, u, vs, v_index, ca, cb):
    out = base + u
    for t, j in enumerate(v_index):
        out = out + (vs[j] * ca[t]) * cb[t]
    return out


def fma_accel(x0, u, v, s, qn_form):
    """MUTANT: the same with the multiply-adds fused (one rounding), emulated in long double"""
    def fma(a, b, c):
        return (LD(a) * np.asarray(b, LD) + np.asarray(c, LD)).astype(np.float64)
    if qn_form:
        return fma(s, v, x0 + u)
    return fma(s * s, v - u, fma(-(2 * s), u, x0))


def check_bits(got, want, what):
    """bit for bit, or AssertionError naming the first element that differs"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape and got.dtype == np.float64, (what, got.shape, want.shape)
    if got.tobytes() == want.tobytes():
        return
    bad = np.flatnonzero(got.ravel().view(np.uint64) != want.ravel().view(np.uint64))
    i = np.unravel_index(bad[0], got.shape)
    raise AssertionError("%s: %d of %d elements differ in bits; first at %r: got %r, want %r"
                         % (what, bad.size, got.size, tuple(int(x) for x in i), got[i], want[i]))


# ------------------------------------------------------------------------------------------------------------------ projection
def michelot_restated(x, lb, mask_bits=1 << 30, max_rounds=None, le=False):
    """simplex.c:109-143 in Python floats (IEEE double, the kernels' order of operations), counting: returns (projected row,
    rounds, per round the indices fixed in it, per round the free indices that landed exactly on the bound).
    MUTANTS: mask_bits=32 keeps the fixed set in a 32-bit mask (index j aliases j % 32, as a 32-bit shift does), max_rounds=1
    stops after the first round, le=True fixes an entry that is <= the bound."""
    x = [float(v) for v in x]
    n, fixed, rounds, fixed_in, ties = len(x), 0, 0, [], []
    while n:
        csum = 0.0
        for v in x:
            csum += v
        shift = (csum - 1.0) / n
        rounds += 1
        now, tie, done = [], [], True
        for j in range(len(x)):
            if (fixed >> (j % mask_bits)) & 1:
                continue
            v = x[j] - shift
            if v == lb:
                tie.append(j)
            if v < lb or (le and v == lb):
                v = lb
                fixed |= 1 << (j % mask_bits)
                n -= 1
                done = False
                now.append(j)
            x[j] = v
        fixed_in.append(now)
        ties.append(tie)
        if done or (max_rounds and rounds >= max_rounds):
            break
    return np.array(x), rounds, fixed_in, ties


def exact_projection(x, lb):
    """the point of {y >= lb, sum y = 1} nearest to x, in exact rational arithmetic (sort-based), as Fractions"""
    xs, lbf, n = [Fraction(float(v)) for v in x], Fraction(float(lb)), len(x)
    assert 1 - n * lbf >= 0
    order = sorted(xs, reverse=True)
    top, tau = Fraction(0), None
    best = None
    for k in range(1, n + 1):
        top += order[k - 1]
        tau = (top - (1 - (n - k) * lbf)) / k
        if order[k - 1] - tau > lbf:
            best = tau                      # the largest k whose k-th largest entry stays above the bound
    if best is None:
        best = order[0] - (1 - (n - 1) * lbf)
    return [max(v - best, lbf) for v in xs]


def _serial_sum(row):
    s = 0.0
    for v in row:
        s += v
    return s


_TIES = {}


def tie_row(n, lb, variant):
    """family (f), or None where it cannot be built (module docstring)"""
    key = (n, lb, variant)
    if key in _TIES:
        return _TIES[key]
    row = None
    if n >= 3 and lb >= 1e-12:
        rng = np.random.default_rng(1000 * n + variant)
        for _ in range(50):
            s1 = float(rng.integers(1 << 18, 1 << 21)) * 2.0 ** -52
            b = lb + s1
            if b - s1 != lb or b - lb != s1:
                continue
            ia, ib, ic = (int(v) for v in rng.permutation(n)[:3])
            r = rng.integers(1, 1 << 20, n).astype(np.float64) * 2.0 ** -22 / n          # coarse dyadic values, about 1/8 in sum
            r[ia], r[ib], r[ic] = -float(rng.integers(1 << 10, 1 << 20)) * 2.0 ** -21, b, 0.0
            target = 1.0 + n * s1
            r = [float(v) for v in r]
            lo, hi = int(np.float64(0.25).view(np.int64)), int(np.float64(4.0).view(np.int64))      # positive doubles order as their bits
            while lo < hi:
                mid = (lo + hi) // 2
                r[ic] = float(np.int64(mid).view(np.float64))
                if _serial_sum(r) < target:
                    lo = mid + 1
                else:
                    hi = mid
            r[ic] = float(np.int64(lo).view(np.float64))
            if _serial_sum(r) != target:
                continue
            _, rounds, fixed_in, ties = michelot_restated(r, lb)
            if ties[0] == [ib] and ia in fixed_in[0] and ib not in fixed_in[0] and rounds >= 2 and ib in fixed_in[1]:
                row = np.array(r)
                break
    _TIES[key] = row
    return row


def cascade(n, rng, variant=0, top=1e6):
    """-top r^-k, k = 0 .. n-1, in permuted order (r = 2, 1.5, 3, 1.25 in turn), each within 10 % below that"""
    r = (2.0, 1.5, 3.0, 1.25)[variant % 4]
    return -top * r ** -rng.permutation(n).astype(np.float64) * rng.uniform(0.9, 1.0, n)


def family_row(fam, n, lb, rng, variant):
    """(target row of length n, the family it really is)"""
    if fam == "f":
        t = tie_row(n, lb, variant % 4)
        if t is not None:
            return t, "f"
    if fam == "g" and n > 32:
        row = np.empty(n)
        row[:32] = cascade(32, rng, variant, top=1e2)
        row[32:] = -1e4 * rng.uniform(1.0, 2.0, n - 32)
        return row, "g"
    if fam == "a":
        return rng.dirichlet(np.ones(n)) * (1 - n * lb) + lb, "a"
    if fam == "b":
        return (rng.dirichlet(np.ones(n)) + 1e-6) * (1e-3, 0.3, 7.0, 1e3)[variant % 4], "b"
    if fam == "d" and n >= 2:
        return cascade(n, rng, variant), "d"
    if fam == "e":
        row = -rng.uniform(0.1, 10.0, n)
        row[rng.integers(n)] = rng.uniform(2.0, 9.0)
        return row, "e"
    row = rng.uniform(0.0, 1.0, n)
    neg = rng.random(n) < 0.5
    row[neg] = -rng.uniform(1.0, 100.0, int(neg.sum()))
    return row, "c"


def target_rows(nrows, n, lb, seed):
    rng = np.random.default_rng(seed)
    rows, labels = np.empty((nrows, n)), []
    for i in range(nrows):
        rows[i], lab = family_row(FAMILIES[i % 7], n, lb, rng, i // 7)
        labels.append(lab)
    return rows, labels


def targets(shape, lb, seed):
    """(Q target [I][K] or [K], P target [K][T], labels of the Q rows, labels of the P blocks in (locus, k) order)"""
    K = shape["K"]
    if shape["model"] == "admix":
        yq, lq = target_rows(shape["I"], K, lb, seed)
    else:
        rows, lab = target_rows(7, K, lb, seed)
        pick = seed % 7                       # one row only: the family changes with the seed
        yq, lq = rows[pick], [lab[pick]]
    yp, lp, off, b = np.empty((K, shape["T"])), [], 0, 0
    rng = np.random.default_rng(seed + 1)
    for M in shape["ua"]:
        for k in range(K):
            if M:
                yp[k, off:off + M], lab = family_row(FAMILIES[b % 7], int(M), lb, rng, b // 7)
                lp.append(lab)
            else:
                lp.append("-")
            b += 1
        off += M
    return yq, yp, lq, lp


def _tie_mask_q(shape, labels):
    m = np.zeros(qshape(shape), dtype=bool)
    if shape["model"] == "admix":
        m[[i for i, lab in enumerate(labels) if lab == "f"]] = True
    elif labels[0] == "f":
        m[:] = True
    return m


def _tie_mask_p(shape, labels):
    K, m, off, b = shape["K"], np.zeros((shape["K"], shape["T"]), dtype=bool), 0, 0
    for M in shape["ua"]:
        for k in range(K):
            if labels[b] == "f":
                m[k, off:off + M] = True
            b += 1
        off += M
    return m


def projection_case(shape, lb, form, s, seed, pattern=None):
    """Base, secants and update whose unprojected result falls in the row families.  form: "squarem" / "qn" (mchip_accel_update
    with secant pair 1 and step s) or "multi" (mchip_multisecant_update with `pattern` of MULTI_PATTERNS)."""
    rng = np.random.default_rng(seed + 7)
    yq, yp, lq, lp = targets(shape, lb, seed)
    c = dict(shape=shape, lb=lb, form=form, s=s, labels_q=lq, labels_p=lp, u=[None] * 3, v=[None] * 3)
    if form == "multi":
        c["u_index"], c["v_index"] = pattern
        nt = len(c["v_index"])
        c["ca"], c["cb"] = rng.standard_normal(nt) * 3, rng.standard_normal(nt) * 0.3
    sides = []
    for y, tie in ((yq, _tie_mask_q(shape, lq)), (yp, _tie_mask_p(shape, lp))):
        x0 = np.where(tie, y, rng.uniform(0.01, 1.0, y.shape))
        us = [np.where(tie, 0.0, 0.1 * rng.standard_normal(y.shape)) for _ in range(3)]
        vs = [np.where(tie, 0.0, 0.1 * rng.standard_normal(y.shape)) for _ in range(3)]
        if form == "squarem":
            vs[1] = np.where(tie, 0.0, us[1] + ((y - x0) + (2 * s) * us[1]) / (s * s))
        elif form == "qn":
            vs[1] = np.where(tie, 0.0, ((y - x0) - us[1]) / s)
        else:
            tail = np.zeros(y.shape)
            for t, j in enumerate(c["v_index"]):
                tail = tail + (vs[j] * c["ca"][t]) * c["cb"][t]
            us[c["u_index"]] = np.where(tie, 0.0, (y - x0) - tail)
        sides.append((x0, us, vs))
    c["x0"] = (sides[0][0], sides[1][0])
    for j in range(3):
        c["u"][j] = (sides[0][1][j], sides[1][1][j])
        c["v"][j] = (sides[0][2][j], sides[1][2][j])
    return c


def unprojected(c):
    """numpy's value of the update, (q, p)"""
    out = []
    for side in (0, 1):
        if c["form"] == "multi":
            out.append(ref_multisecant(c["x0"][side], c["u"][c["u_index"]][side], [v[side] for v in c["v"]], c["v_index"], c["ca"], c["cb"]))
        else:
            out.append(ref_accel(c["x0"][side], c["u"][1][side], c["v"][1][side], c["s"], c["form"] == "qn"))
    return tuple(out)


def project_q(shape, q, lb, michelot=ob.michelot):
    if shape["model"] != "admix":
        return michelot(q, lb)
    return np.array([michelot(row, lb) for row in q])


def project_p(shape, p, lb, michelot=ob.michelot):
    out, off = np.array(p, dtype=np.float64), 0
    for M in shape["ua"]:
        if M:
            for k in range(shape["K"]):
                out[k, off:off + M] = michelot(p[k, off:off + M], lb)
        off += M
    return out


def projected(c, michelot=ob.michelot):
    xq, xp = unprojected(c)
    return project_q(c["shape"], xq, c["lb"], michelot), project_p(c["shape"], xp, c["lb"], michelot)


def run_case(ctx, c, to=2, base=0):
    """stage the case and run its update on the device: (Q, P) of slot `to`"""
    ctx.set_q(base, c["x0"][0])
    ctx.set_p(base, c["x0"][1])
    for j in range(3):
        ctx.set_secant(0, j, c["u"][j][1], c["u"][j][0])
        ctx.set_secant(1, j, c["v"][j][1], c["v"][j][0])
    if c["form"] == "multi":
        ctx.multisecant_update(to, base, c["u_index"], c["v_index"], c["ca"], c["cb"])
    else:
        ctx.accel_update(to, base, 1, c["s"], int(c["form"] == "qn"))
    return ctx.get_q(to), ctx.get_p(to)


def check_projection(got_q, got_p, c, what):
    want_q, want_p = projected(c)
    check_bits(got_q, want_q, what + " Q")
    check_bits(got_p, want_p, what + " P")


# ------------------------------------------------------------------------------------------------------------------ dot products
def kernel_depth(n):
    """Depth D of the device's summation of n products (k_dots, k_reduce_dots, the host's last addition): g = min(512,
    ceil(n / 4096)) blocks of 256 threads; a thread's grid-stride chain has ceil(n / (256 g)) terms, the block tree 8 levels,
    block_ordered_sum's per-thread chain over the g partials ceil(g / 256) terms and its tree 8 levels, and the host adds the
    eta part and the p part."""
    g = min(512, -(-n // 4096))
    return -(-n // (256 * g)) + 8 + -(-g // 256) + 8 + 1


def grid_of(n):
    return min(512, -(-n // 4096))


def dots_operands(shape, family, seed):
    """three independent secant pairs: (u[j], v[j]) as (q, p).  Families: "unit" |u|, |v| in [0.5, 2] with random signs -- one
    of the two in [0.5, 0.75] and the other in [1.25, 2], so that |v - u| >= 0.5 as well and every single term of every sum is at
    least 0.25; "tiny" the same times 1e-9 (secants near convergence); "wide" magnitudes 10^U(-12, 0)."""
    rng = np.random.default_rng(seed)

    def draw(sh):
        if family == "wide":
            return 10.0 ** rng.uniform(-12, 0, sh) * rng.choice([-1.0, 1.0], sh), 10.0 ** rng.uniform(-12, 0, sh) * rng.choice([-1.0, 1.0], sh)
        small, large, swap = rng.uniform(0.5, 0.75, sh), rng.uniform(1.25, 2.0, sh), rng.random(sh) < 0.5
        a, b = np.where(swap, large, small), np.where(swap, small, large)
        f = 1e-9 if family == "tiny" else 1.0
        return a * f * rng.choice([-1.0, 1.0], sh), b * f * rng.choice([-1.0, 1.0], sh)
    u, v = [], []
    for _ in range(3):
        (uq, vq), (up, vp) = draw(qshape(shape)), draw((shape["K"], shape["T"]))
        u.append((uq, up))
        v.append((vq, vp))
    return u, v


def _ld(a):
    return np.ascontiguousarray(a, dtype=np.float64).ravel().astype(LD)


def _dot(a, b):
    """(sum a_i b_i, sum |a_i| |b_i|, min |a_i| |b_i|) in long double, pairwise (numpy's sum): the first is within 2^-58 of the
    second of the exact value, against a bound that is never below 22 * 2^-53 of it"""
    t = a * b
    return t.sum(), np.abs(t).sum(), np.abs(t).min()


def step_terms(u, v):
    """the factor pairs (a, b) of the three sums of mchip_step_dots, per side, with v - u exact"""
    out = []
    for side in (0, 1):
        uu, vv = _ld(u[side]), _ld(v[side])
        d = vv - uu
        out.append([(uu, uu), (uu, d), (d, d)])
    return out


def secant_terms(u1, u2, v2):
    out = []
    for side in (0, 1):
        a = _ld(u1[side])
        out.append([(a, _ld(u2[side])), (a, _ld(v2[side]))])
    return out


def dots_reference(terms):
    """per sum: (exact value, [sum |a||b| of the eta part, of the p part], smallest single |a||b|)"""
    out = []
    for x in range(len(terms[0])):
        parts = [_dot(*terms[side][x]) for side in (0, 1)]
        out.append((parts[0][0] + parts[1][0], [parts[0][1], parts[1][1]], min(parts[0][2], parts[1][2])))
    return out


def dots_bound(scales, depth_q, depth_p):
    """(D + 3) eps sum |a_i||b_i|, each part with its own depth: 3 = the product and the two roundings of v - u"""
    return float(((depth_q + 3) * scales[0] + (depth_p + 3) * scales[1]) * EPS)


def dots_ratio(got, ref, shape):
    """|got - exact| / bound at the kernels' depth, per sum"""
    nq, KT = shape["nq"], shape["K"] * shape["T"]
    return [float(abs(LD(g) - e) / dots_bound(sc, kernel_depth(nq), kernel_depth(KT))) for g, (e, sc, _) in zip(got, ref)]


def check_dots(got, ref, shape, what):
    """prints one WORST line, raises when a sum is outside its bound; returns the largest ratio"""
    r = dots_ratio(got, ref, shape)
    print("WORST %s %s %s" % (shape_id(shape), what, " ".join("%.3g" % x for x in r)))
    assert all(np.isfinite(got)) and max(r) <= 1.0, "%s %s: error / bound %r (got %r)" % (shape_id(shape), what, r, list(got))
    return max(r)


def emulate_device_dots(terms, drop=None, acc=np.float64, swap_parts=False):
    """numpy model of k_dots + k_reduce_dots + the host's addition: products in double, per block the elements of its grid-stride
    trips, partials laid out [sum][block] in a 3 * 512 buffer per part.  (Summation inside a block is numpy's, not the
    kernel's tree: the model is for mutants, not for bits.)  MUTANTS: drop = "last" / "block" / "trip" leaves out the last
    element / the last 256 elements / one whole grid-stride trip of the p part; acc = float32 accumulates in single;
    swap_parts reads the eta partials with the p part's stride and count and the other way round."""
    nout = len(terms[0])
    bufs, grids = [], []
    for side in (0, 1):
        n = terms[side][0][0].size
        g = grid_of(n)
        buf = np.zeros(3 * 512)
        for x in range(nout):
            a, b = terms[side][x]
            t = (a.astype(np.float64) * b.astype(np.float64))
            if side == 1 and drop == "last":
                t = t[:-1]
            elif side == 1 and drop == "block":
                t = t[:-256]
            elif side == 1 and drop == "trip":
                trips = -(-n // (256 * g))
                keep = np.arange(n) // (256 * g) != trips // 2
                t = np.where(keep, t, 0.0)
            blk = (np.arange(t.size) // 256) % g
            order = np.argsort(blk, kind="stable")
            starts = np.searchsorted(blk[order], np.arange(g))
            if t.size:
                buf[x * g:(x + 1) * g] = np.add.reduceat(t[order].astype(acc), np.minimum(starts, t.size - 1), dtype=acc) * (starts < t.size)
        bufs.append(buf)
        grids.append(g)
    if swap_parts:
        grids = grids[::-1]
    return [float(bufs[0][x * grids[0]:(x + 1) * grids[0]].sum() + bufs[1][x * grids[1]:(x + 1) * grids[1]].sum()) for x in range(nout)]


def exact_dot_fsum(a, b):
    """sum a_i b_i correctly rounded: Dekker's exact products (Veltkamp split) and math.fsum -- the check of the long-double sums"""
    a, b = np.ascontiguousarray(a, dtype=np.float64).ravel(), np.ascontiguousarray(b, dtype=np.float64).ravel()
    p = a * b

    def split(x):
        c = 134217729.0 * x
        hi = c - (c - x)
        return hi, x - hi
    ah, al = split(a)
    bh, bl = split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return math.fsum(list(p) + list(e))
