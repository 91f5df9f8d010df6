"""Quality control of packed PLINK records (TEST INFRASTRUCTURE): the definition of include/multiclust_hip.h (mchip_bed_qc) restated
-- the counts with numpy comparisons, the Hardy-Weinberg exact test with Python integers and floats in the operation order of the
header (float(int) and int/int-free float arithmetic of CPython are IEEE round-to-nearest, hence the same bits as the device's
conversions, multiplies and divides) and once more as exact rationals --, the rules of --mind, --geno, --maf and --hwe
(multiclust_amd/host/mc_qc.c) restated as they are worded, the launch geometry restated, the files the command line writes, a fileset
with planted bad samples and variants, and the mutants that the cases of the tests have to tell from the real thing.  Filesets are
written by bedfiles.py.

Run as a program it prints the digest of the device's counts and p values of a GEOMETRY case: tests/test_gpu_qc.py starts it in fresh
processes under different launch geometries."""
import hashlib
from fractions import Fraction
from math import factorial

import numpy as np

import bedfiles
from ld_util import codes_of, repack, same_bits      # noqa: F401  (the tests take them from here)

# restated from multiclust_amd/csrc/mchip_feature_geometry.h
QC_VARIANTS = 4         # variants per workgroup of the variant pass
QC_STEP = 64            # 64-bit words (32 individuals each) a wave reads of its record at a time
QC_ITILE = 256          # individuals per workgroup of the individual pass
STEP_INDIVIDUALS = 32 * QC_STEP

KEPT, GENO, MAF, HWE = 0, 1, 2, 3
WHY = ("kept", "geno", "maf", "hwe")

COUNT_MUTANTS = ("padding bits counted", "keep mask ignored", "codes 0 and 3 swapped in one plane")
HWE_MUTANTS = ("walk started at mid + 2", "walk started at mid - 2", "second walk sums all weights")
RULE_MUTANTS = ("<= for < and >= for >",)
MUTANTS = COUNT_MUTANTS + HWE_MUTANTS + RULE_MUTANTS


# ---- the counts ----
def counts(bed, I, keep=None, mutant=None):
    """packed records [L][record_bytes] -> (ind_counts [I][4], var_counts [L][4]) uint32: ind over all variants, var over the
    individuals with keep != 0 (None: all)"""
    bed = np.asarray(bed, dtype=np.uint8)
    codes = codes_of(bed, I)                                        # [L][I]
    ind = np.stack([(codes == c).sum(axis=0) for c in range(4)], axis=1).astype(np.uint32)
    k = np.ones(I, dtype=bool) if keep is None or mutant == "keep mask ignored" else np.asarray(keep).astype(bool)
    vcodes = codes[:, k]
    if mutant == "padding bits counted":
        n_all = 4 * bed.shape[1]
        vcodes = np.concatenate([vcodes, codes_of(bed, n_all)[:, I:]], axis=1)
    var = np.stack([(vcodes == c).sum(axis=1) for c in range(4)], axis=1).astype(np.uint32)
    if mutant == "codes 0 and 3 swapped in one plane":              # both bits set taken for neither
        var = var[:, [3, 1, 2, 0]]
    return ind, var


# ---- the exact test ----
def hwe_mid(n0, n2, n3):
    N = n0 + n2 + n3
    r = 2 * min(n0, n3) + n2
    mid = (r * (2 * N - r)) // (2 * N)
    if (mid ^ r) & 1:
        mid += 1
    return N, r, mid


def hwe_walk(N, r, mid):
    """(h, w) in visiting order: mid, then downwards, then upwards; one multiply then one divide a step"""
    h, a = mid, (r - mid) // 2
    b = N - h - a
    w = 1.0
    yield h, w
    while h >= 2:
        w = (w * float(h * (h - 1))) / float(4 * (a + 1) * (b + 1))
        h, a, b = h - 2, a + 1, b + 1
        yield h, w
    h, a = mid, (r - mid) // 2
    b = N - h - a
    w = 1.0
    while h <= r - 2:
        w = (w * float(4 * a * b)) / float((h + 2) * (h + 1))
        h, a, b = h + 2, a - 1, b - 1
        yield h, w


def hwe_p(n0, n2, n3, mutant=None, tie_factor=True):
    """the definition in float64, the operation order of the header"""
    n0, n2, n3 = int(n0), int(n2), int(n3)
    if n0 + n2 + n3 == 0:
        return 1.0
    N, r, mid = hwe_mid(n0, n2, n3)
    if mutant == "walk started at mid + 2" and mid + 2 <= r:
        mid += 2
    if mutant == "walk started at mid - 2" and mid >= 2:
        mid -= 2
    S, w_obs = 0.0, 0.0
    for h, w in hwe_walk(N, r, mid):
        S += w
        if h == n2:
            w_obs = w
    bound = w_obs * 1.0000001 if tie_factor else w_obs
    T = 0.0
    for h, w in hwe_walk(N, r, mid):
        if w <= bound or mutant == "second walk sums all weights":
            T += w
    p = T / S
    return 1.0 if p > 1.0 else p


def hwe_p_of(var_counts, mutant=None):
    return np.array([hwe_p(c[0], c[2], c[3], mutant) for c in np.asarray(var_counts).tolist()], dtype=np.float64).reshape(-1)


def hwe_exact(n0, n2, n3):
    """(p as a Fraction, near_tie): the multinomial weights N! / (a! h! b!) 2^h of every heterozygote count h of the table's margins,
    p = the share of those not above the observed one; near_tie: some weight unequal to the observed one lies within 1e-6 relative of
    it (the tie factor of the definition legitimately merges such weights)"""
    N = n0 + n2 + n3
    if N == 0:
        return Fraction(1), False
    r = 2 * min(n0, n3) + n2
    fN = factorial(N)
    weights = {}
    for h in range(r % 2, r + 1, 2):
        a = (r - h) // 2
        b = N - h - a
        weights[h] = Fraction(fN * 2 ** h, factorial(a) * factorial(h) * factorial(b))
    obs = weights[n2]
    near = any(w != obs and abs(w - obs) * 1000000 <= obs for w in weights.values())
    return sum(w for w in weights.values() if w <= obs) / sum(weights.values()), near


def hwe_steps(n0, n2, n3):
    """weights of the table's walk: r // 2 + 1"""
    return (2 * min(n0, n3) + n2) // 2 + 1


# ---- the rules ----
def missing_rate(num, den):
    return float(int(num)) / float(int(den)) if den else 0.0


def maf_of(c):
    n0, n2, n3 = int(c[0]), int(c[2]), int(c[3])
    N = n0 + n2 + n3
    return float(min(2 * n0 + n2, 2 * n3 + n2)) / float(2 * N) if N else 0.0


def decide(bed, I, mind=None, geno=None, maf=None, hwe=None, mutant=None):
    """the four rules in PLINK 1.9's order on packed records: dict(ind, ind_keep, var, p, reason)"""
    L = bed.shape[0]
    strict = mutant != "<= for < and >= for >"
    gt = (lambda x, t: x > t) if strict else (lambda x, t: x >= t)
    lt = (lambda x, t: x < t) if strict else (lambda x, t: x <= t)
    ind, _ = counts(bed, I, mutant=mutant if mutant in COUNT_MUTANTS else None)
    keep = np.ones(I, dtype=bool)
    if mind is not None:
        keep = np.array([not gt(missing_rate(ind[i, 1], L), mind) for i in range(I)])
    _, var = counts(bed, I, keep, mutant=mutant if mutant in COUNT_MUTANTS else None)
    p = hwe_p_of(var, mutant if mutant in HWE_MUTANTS else None)
    reason = np.zeros(L, dtype=np.uint8)
    for l in range(L):
        c = var[l]
        if geno is not None and gt(missing_rate(c[1], int(c.sum())), geno):
            reason[l] = GENO
        elif maf is not None and lt(maf_of(c), maf):
            reason[l] = MAF
        elif hwe is not None and lt(p[l], hwe):
            reason[l] = HWE
    return dict(ind=ind, ind_keep=keep, var=var, p=p, reason=reason)


def compose(first, second):
    """the map of a filter that ran on what `first` left: places in the fileset"""
    return [first[x] for x in second] if first is not None else list(second)


# ---- the files of the command line ----
def line_text(d, mind=None, geno=None, maf=None, hwe=None):
    out = "Quality control:"
    if mind is not None:
        out += " kept %d of %d individuals (missing rate > %g)" % (d["ind_keep"].sum(), len(d["ind_keep"]), mind)
    if geno is not None or maf is not None or hwe is not None:
        parts = []
        if geno is not None:
            parts.append("%d missing rate > %g" % ((d["reason"] == GENO).sum(), geno))
        if maf is not None:
            parts.append("%d MAF < %g" % ((d["reason"] == MAF).sum(), maf))
        if hwe is not None:
            parts.append("%d HWE p < %g" % ((d["reason"] == HWE).sum(), hwe))
        out += "%s kept %d of %d variants (%s)" % ("," if mind is not None else "", (d["reason"] == KEPT).sum(), len(d["reason"]), ", ".join(parts))
    return out + "\n"


def var_table_text(d, ids):
    out = ["ID\tN_HOM1\tN_MISS\tN_HET\tN_HOM2\tF_MISS\tMAF\tHWE_P\tQC\n"]
    for l, c in enumerate(d["var"]):
        out.append("%s\t%d\t%d\t%d\t%d\t%.6g\t%.6g\t%.6g\t%s\n" % (ids[l], c[0], c[1], c[2], c[3], missing_rate(c[1], int(c.sum())), maf_of(c),
                                                               d["p"][l], WHY[d["reason"][l]]))
    return "".join(out)


def ind_table_text(d, fids, iids, L):
    out = ["FID\tIID\tF_MISS\tHET\tQC\n"]
    for i, c in enumerate(d["ind"]):
        typed = int(c[0]) + int(c[2]) + int(c[3])
        het = "%.6g" % (float(int(c[2])) / float(typed)) if typed else "nan"
        out.append("%s\t%s\t%.6g\t%s\t%s\n" % (fids[i], iids[i], missing_rate(c[1], L), het, "kept" if d["ind_keep"][i] else "mind"))
    return "".join(out)


# ---- cases ----
def draw_codes(I, L, seed, missing=0.0):
    """[I][L] codes, Hardy-Weinberg at frequencies that reach down to rare"""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.0, 0.6, size=L) ** 2
    a2 = (rng.random((I, L)) < f) * 1 + (rng.random((I, L)) < f) * 1
    codes = np.array([bedfiles.HOM1, bedfiles.HET, bedfiles.HOM2], dtype=np.uint8)[a2]
    codes[rng.random((I, L)) < missing] = bedfiles.MISS
    return codes


def plant(codes, seed=0):
    """where the shape has room, in place: an all-missing, a monomorphic and an all-heterozygous variant and a fully missing individual"""
    I, L = codes.shape
    rng = np.random.default_rng(seed + 17)
    if L >= 4:
        for l, c in zip(rng.permutation(L)[:3], (bedfiles.MISS, bedfiles.HOM2, bedfiles.HET)):
            codes[:, l] = c
    if I >= 3:
        codes[int(rng.integers(I)), :] = bedfiles.MISS
    return codes


def case(I, L, seed, missing=0.1, extra=0):
    """(packed records with garbage in every bit that carries no individual, codes [I][L])"""
    codes = plant(draw_codes(I, L, seed, missing), seed)
    return repack(codes, seed, extra), codes


def keep_masks(I, seed=0):
    """empty, full, alternating, a single individual, and a drawn one"""
    one = np.zeros(I, dtype=np.uint8)
    one[(7 * I) // 11] = 1
    return dict(none=None, empty=np.zeros(I, dtype=np.uint8), full=np.full(I, 255, dtype=np.uint8), alternating=(np.arange(I) % 2).astype(np.uint8),
                single=one, drawn=(np.random.default_rng(seed).random(I) < 0.7).astype(np.uint8) * 3)


def tables_from_codes(n0, n2, n3):
    """records of one variant with these counts: [1][ceil(N/4)]"""
    codes = np.array([bedfiles.HOM1] * n0 + [bedfiles.HET] * n2 + [bedfiles.HOM2] * n3, dtype=np.uint8).reshape(-1, 1)
    return bedfiles.pack(codes, padding=1), codes.shape[0]


# tables at N about 2000 whose walk passes through subnormals to zero, r = 0 and r = 1, n2 = mid, and ordinary ones
HWE_TABLES = [(1000, 0, 1000), (0, 2000, 0), (1000, 2, 1001), (900, 200, 900), (5, 0, 0), (0, 0, 7), (6, 1, 0), (0, 1, 9), (0, 1, 0),
              (40, 42, 11), (50, 50, 12), (25, 50, 25), (3, 0, 3), (1, 2, 1), (700, 600, 700), (1999, 1, 0), (10, 1980, 10)]


CLI = dict(I=60, L=400, seed=21, mind=0.1, geno=0.05, maf=0.03, hwe=1e-4, prune_t=0.5, prune_window=20, king_t=0.125, boundary=200)


def cli_case():
    """(codes [60][400], fids, iids, chrom) of the command-line tests: two populations, three bad samples (one of them all missing),
    rare and monomorphic variants, all-missing and badly typed variants, variants far out of Hardy-Weinberg proportions (all
    heterozygous; no heterozygote at frequency about one half), two duplicated individuals for --king-cutoff (55 are left: not a multiple of 4), and a run of identical
    variants 196 ... 203 across the boundary of two chromosomes for --prune: read with places in the thinned data set instead of places
    in the fileset, the chromosomes would put 200 with 196 and remove it.  Family ids are placed so that the kept individuals' locales
    are numbered anew"""
    I, L = CLI["I"], CLI["L"]
    rng = np.random.default_rng(CLI["seed"])
    anc = rng.uniform(0.15, 0.85, size=L)
    pop = (np.arange(I) >= I // 2).astype(int)
    f = np.stack([np.clip(anc + 0.1, 0, 1), np.clip(anc - 0.1, 0, 1)])[pop]         # [I][L]
    a2 = (rng.random((I, L)) < f) * 1 + (rng.random((I, L)) < f) * 1
    codes = np.array([bedfiles.HOM1, bedfiles.HET, bedfiles.HOM2], dtype=np.uint8)[a2]
    codes[rng.random((I, L)) < 0.01] = bedfiles.MISS
    for l in range(197, 204):
        codes[:, l] = codes[:, 196]
    order = rng.permutation(np.setdiff1d(np.arange(L), np.arange(190, 210)))
    rare, mono, allmiss, poorly, allhet, nohet = (order[a:b] for a, b in ((0, 25), (25, 35), (35, 41), (41, 55), (55, 59), (59, 63)))
    for l in rare:
        codes[:, l] = bedfiles.HOM1
        codes[rng.permutation(I)[:2], l] = bedfiles.HET
    codes[:, mono] = bedfiles.HOM2
    codes[:, allmiss] = bedfiles.MISS
    for l in poorly:
        codes[rng.permutation(I)[:9], l] = bedfiles.MISS
    codes[:, allhet] = bedfiles.HET
    for l in nohet:
        codes[:, l] = np.where(rng.random(I) < 0.5, bedfiles.HOM1, bedfiles.HOM2)
    codes[33, :] = codes[12, :]
    codes[50, :] = codes[45, :]
    codes[0, :] = bedfiles.MISS
    codes[17, rng.random(L) < 0.6] = bedfiles.MISS
    codes[41, rng.random(L) < 0.2] = bedfiles.MISS
    fids = ["fam%d" % (i % 3) for i in range(I)]
    fids[0], fids[1], fids[2], fids[17] = "fam9", "fam1", "fam0", "fam8"                 # fam9 and fam8 leave with their only member
    iids = ["ind%d" % i for i in range(I)]
    return codes, fids, iids, ["1" if l < CLI["boundary"] else "2" for l in range(L)]


def pipeline(codes, chrom, mind=None, geno=None, maf=None, hwe=None, prune=False, king=False):
    """what pre_fit() does, with the restatements of the three filters: dict(qc = decide's, rows, cols = the places in the fileset
    of the individuals and variants left, seen = what --prune and --king-cutoff saw, phi, cnt = the kinships --king-cutoff saw)"""
    import king_util
    import ld_util
    I, L = codes.shape
    qc = decide(bedfiles.pack(codes), I, mind, geno, maf, hwe)
    rows, cols = np.flatnonzero(qc["ind_keep"]), np.flatnonzero(qc["reason"] == KEPT)
    out = dict(qc=qc, seen={})
    if prune and len(rows) and len(cols):
        sub = codes[np.ix_(rows, cols)]
        w = CLI["prune_window"]
        vkeep = ld_util.greedy(ld_util.band(bedfiles.pack(sub), len(rows), w), w, CLI["prune_t"], [chrom[l] for l in cols])
        out["seen"]["prune"] = len(cols)
        cols = cols[vkeep]
    if king and len(rows) and len(cols):
        out["phi"], out["cnt"] = king_util.kinship(codes[np.ix_(rows, cols)])
        out["rows_seen"] = rows
        out["seen"]["king"] = len(rows)
        rows = rows[king_util.greedy(king_util.related(out["phi"], CLI["king_t"]))]
    out.update(rows=rows, cols=cols)
    return out


# ---- the launch geometry ----
def qc_cut(base, n_units, target):
    want = max(1, min(-(-target // base) if base > 0 else 1, n_units, 65535))
    per = -(-n_units // want)
    return -(-n_units // per), per


def qc_geometry(I, L, target_blocks):
    """qc_geometry_of (multiclust_amd/csrc/mchip_feature_geometry.h) restated: (n_vgroups, v_split, steps_per_split, n_itiles, i_split,
    words_per_split); tests/test_qc_cpu.py holds it to the header"""
    n_vg, n_it = -(-L // QC_VARIANTS), -(-I // QC_ITILE)
    v = qc_cut(n_vg, -(-(-(-I // 32)) // QC_STEP), target_blocks)
    i = qc_cut(n_it, -(-L // 64), target_blocks)
    return (n_vg,) + v + (n_it,) + i


def blocks_per_cu(env):
    """the knob as mchip.hip reads it: MCHIP_BLOCKS_PER_CU_IND, else MCHIP_BLOCKS_PER_CU, else 64"""
    return int(env.get("MCHIP_BLOCKS_PER_CU_IND") or env.get("MCHIP_BLOCKS_PER_CU") or 64)


# the cases of the launch-geometry test, on the 256 compute units of an MI355X.  6149 individuals are 4 steps of a record and 25
# tiles; 37 are one of each.  "steps", 600 variants = 150 groups and 10 words: knob 1 cuts the records into 2 runs of 2 steps, knob 64
# into 4 of one; the individual pass walks one word a workgroup.  "whole", 1100 variants = 275 groups and 18 words: under knob 1 one
# workgroup walks all 4 steps of its records, and the individual pass 9 runs of 2 words.  "words", 32833 variants = 514 words against
# one tile: knob 1 gives 172 runs of 3 words, the last of 1; knob 64 one word a workgroup.
GEOMETRY = dict(steps=dict(I=6149, L=600), whole=dict(I=6149, L=1100), words=dict(I=37, L=32833))


def geometry_case(name):
    """(packed records, keep bytes) of a GEOMETRY case"""
    g = GEOMETRY[name]
    bed, _ = case(g["I"], g["L"], seed=1000 + g["L"], missing=0.1, extra=3)
    return bed, keep_masks(g["I"], g["L"])["drawn"]


def digest(ic, vc, hp):
    return hashlib.sha256(np.ascontiguousarray(ic, dtype=np.uint32).tobytes() + np.ascontiguousarray(vc, dtype=np.uint32).tobytes() +
                          np.ascontiguousarray(hp, dtype=np.float64).tobytes()).hexdigest()


def reference(bed, I, keep=None):
    """(ind_counts, var_counts, hwe_p) of the definition"""
    ind, var = counts(bed, I, keep)
    return ind, var, hwe_p_of(var)


if __name__ == "__main__":
    # qc_util.py <case>: the digest of the device's result, and the geometry the launch had: the last five of qc_geometry, and n_cu
    import os
    import sys
    from multiclust_amd import hip
    name = sys.argv[1]
    g = GEOMETRY[name]
    ctx = hip.Context(0)
    bed, keep = geometry_case(name)
    print(digest(*ctx.bed_qc(g["I"], bed, ind_keep=keep)))
    n_cu = ctx.device_info()[1]
    geo = qc_geometry(g["I"], g["L"], blocks_per_cu(os.environ) * (n_cu if n_cu > 0 else 256))
    print("%d %d %d %d %d" % (geo[1], geo[2], geo[4], geo[5], n_cu))
    ctx.close()
