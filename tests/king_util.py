"""KING-robust kinship between the individuals of packed PLINK records (TEST INFRASTRUCTURE): the definition of phi in
include/multiclust_hip.h (mchip_bed_king) restated with numpy boolean planes and Python integers -- phi = num / (4 m) is CPython's
int true division, correctly rounded, hence the same bits as the device's one division --, the greedy rule of --king-cutoff
(multiclust_amd/host/mc_king.c) restated as it is worded, a generator of planted pedigrees, and the mutants of both that the cases of
the tests have to tell from the real thing.  Filesets are written by bedfiles.py.

Run as a program it prints the digest of the device's kinships and counts of fixed_case(): tests/test_gpu_king.py starts it in fresh
processes under different launch geometries."""
import hashlib

import numpy as np

import bedfiles
from bits import canonical_bytes
from ld_util import codes_of, repack, same_bits      # noqa: F401  (the tests take them from here)

# restated from multiclust_amd/csrc/mchip_feature_geometry.h and mchip_bed.hip
TILE = 64               # row and column individuals per workgroup
STAGE_VARIANTS = 256    # variants of every staged individual's planes in LDS at a time: KING_STAGE = 4 words of 64
PLANE_INDIVIDUALS = 256  # individuals per workgroup of the transposing kernel
SLAB = 1024             # MC_KING_SLAB (multiclust_amd/host/mc_cli.h)

MUTANTS = ("max for min", "h without 'j typed'", "IBS0 in one orientation", "missing counted as homozygous")


def counts(codes, mutant=None):
    """codes [I][L] -> (n, hh, op, h), each [I][I] int64: variants typed in both, both heterozygous, opposite homozygotes, and
    h[i][j] = variants at which i is heterozygous and j is typed"""
    c = np.asarray(codes)
    V = (c != bedfiles.MISS)
    H = (c == bedfiles.HET)
    A = (c == bedfiles.HOM1)
    B = (c == bedfiles.HOM2)
    if mutant == "missing counted as homozygous":
        A = A | ~V
        V = np.ones_like(V)
    V, H, A, B = (x.astype(np.int64) for x in (V, H, A, B))
    n = V @ V.T
    hh = H @ H.T
    op = A @ B.T if mutant == "IBS0 in one orientation" else A @ B.T + B @ A.T
    h = H @ np.ones_like(V).T if mutant == "h without 'j typed'" else H @ V.T
    return n, hh, op, h


def phi_of(hh, op, hij, hji, mutant=None):
    """one pair, Python integers: NaN exactly when m = 0, else the correctly rounded num / (4 m)"""
    hh, op, hij, hji = int(hh), int(op), int(hij), int(hji)
    m = max(hij, hji) if mutant == "max for min" else min(hij, hji)
    if m == 0:
        return float("nan")
    return (2 * hh - 4 * op - hij - hji + 2 * m) / (4 * m)


def kinship(codes, i0=0, n_rows=None, mutant=None):
    """(phi [n_rows][I] float64, counts [n_rows][I][4] uint32) as mchip_bed_king defines them"""
    I = np.asarray(codes).shape[0]
    n_rows = I - i0 if n_rows is None else n_rows
    n, hh, op, h = counts(codes, mutant)
    phi = np.empty((n_rows, I))
    for a in range(n_rows):
        i = i0 + a
        phi[a] = [phi_of(hh[i, j], op[i, j], h[i, j], h[j, i], mutant) for j in range(I)]
    rows = slice(i0, i0 + n_rows)
    return phi, np.stack([n[rows], hh[rows], op[rows], h[rows]], axis=2).astype(np.uint32)


def related(phi, t):
    """the relatedness graph of a whole matrix phi [I][I]: phi > t off the diagonal (NaN compares false)"""
    with np.errstate(invalid="ignore"):
        rel = phi > t
    np.fill_diagonal(rel, False)
    return rel


def greedy(rel, tie="highest"):
    """keep [I] of the rule: while some pair of remaining individuals is related, the remaining individual with the most remaining
    related partners goes; of equals the one with the highest index"""
    rel = np.asarray(rel, dtype=bool)
    keep = np.ones(rel.shape[0], dtype=bool)
    while True:
        deg = (rel & keep[None, :]).sum(axis=1) * keep
        if deg.max() == 0:
            return keep
        worst = np.flatnonzero(deg == deg.max())
        keep[worst[-1] if tie == "highest" else worst[0]] = False


def kin0_text(codes, fids, iids, t):
    """<stem>.king.kin0 of these individuals at threshold t"""
    phi, cnt = kinship(codes)
    I = phi.shape[0]
    rel = related(phi, t)
    out = ["FID1\tIID1\tFID2\tIID2\tN_SNP\tHETHET\tIBS0\tKINSHIP\n"]
    for i in range(I):
        for j in range(i + 1, I):
            if rel[i, j]:
                n, hh, op = (int(x) for x in cnt[i, j, :3])
                out.append("%s\t%s\t%s\t%s\t%d\t%.6f\t%.6f\t%.6f\n" % (fids[i], iids[i], fids[j], iids[j], n, hh / n, op / n, phi[i, j]))
    return "".join(out)


def draw_codes(I, L, seed, missing=0.0):
    """[I][L] codes of unrelated individuals, Hardy-Weinberg"""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.1, 0.9, size=L)
    a2 = (rng.random((I, L)) < f) * 1 + (rng.random((I, L)) < f) * 1
    codes = np.array([bedfiles.HOM1, bedfiles.HET, bedfiles.HOM2], dtype=np.uint8)[a2]
    codes[rng.random((I, L)) < missing] = bedfiles.MISS
    return codes


def plant(codes, seed=0):
    """special individuals where the shape has room, in place: one all missing, one without a heterozygous call, a duplicate of
    another; returns their positions"""
    I, L = codes.shape
    where = {}
    if I >= 6:
        pos = np.random.default_rng(seed + 31).permutation(I)[:4]
        where = dict(zip(("missing", "nohet", "dup", "dup_of"), (int(p) for p in pos)))
        codes[where["missing"], :] = bedfiles.MISS
        row = codes[where["nohet"]]
        row[row == bedfiles.HET] = bedfiles.HOM2
        codes[where["dup"], :] = codes[where["dup_of"], :]
    return where


# ---- planted pedigrees: founders of two populations, a duplicate, parent-child, sibs ----
def pedigree(seed, L, missing=0.05, fst=0.15):
    """(codes [24][L], first-degree-or-closer pairs as a set of (i, j) with i < j, population of every individual); the individuals
    are shuffled so that relatives stand anywhere in the file"""
    rng = np.random.default_rng(seed)
    anc = rng.uniform(0.1, 0.9, size=L)
    # Balding-Nichols frequencies of the two populations
    freq = [rng.beta(anc * (1 - fst) / fst, (1 - anc) * (1 - fst) / fst) for _ in range(2)]
    hap = {}                                        # individual -> [2][L] haplotypes
    pop = {}

    def founder(x, p):
        hap[x] = (rng.random((2, L)) < freq[p]).astype(np.uint8)
        pop[x] = p

    def child(x, mother, father):
        pick_m, pick_f = rng.integers(0, 2, size=L), rng.integers(0, 2, size=L)
        hap[x] = np.stack([hap[mother][pick_m, np.arange(L)], hap[father][pick_f, np.arange(L)]])
        pop[x] = pop[mother]

    for x in range(0, 11):
        founder(x, 0)
    for x in range(11, 17):
        founder(x, 1)
    hap[17], pop[17] = hap[2].copy(), pop[2]        # a duplicate
    child(18, 0, 1)
    child(19, 0, 1)                                 # a trio with two sibs
    child(20, 11, 12)                               # parents and one child
    child(21, 13, 14)
    child(22, 13, 14)
    child(23, 13, 14)                               # three sibs
    pairs = {(2, 17), (0, 18), (1, 18), (0, 19), (1, 19), (18, 19), (11, 20), (12, 20)}
    pairs |= {(p, c) for p in (13, 14) for c in (21, 22, 23)} | {(21, 22), (21, 23), (22, 23)}
    n = len(hap)
    dosage = np.stack([hap[x].sum(axis=0) for x in range(n)])
    codes = np.array([bedfiles.HOM1, bedfiles.HET, bedfiles.HOM2], dtype=np.uint8)[dosage]
    codes[rng.random(codes.shape) < missing] = bedfiles.MISS
    order = rng.permutation(n)                      # file position x holds individual order[x]
    place = np.argsort(order)
    planted = {tuple(sorted((int(place[a]), int(place[b])))) for a, b in pairs}
    return codes[order], planted, [pop[int(x)] for x in order]


CLI = dict(seed=11, L=900, t=0.125, I=24)


def cli_case():
    """(codes [24][900], planted pairs, fids, iids) of the command-line tests; four family ids that do not follow the pedigree, placed
    so that the kept individuals' locales have to be numbered anew: the first fam1 of the file is removed and a fam2 stands before
    the next, and both fam3 are removed (tests/test_king_cpu.py asserts that the numbering changes)"""
    codes, planted, pop = pedigree(CLI["seed"], CLI["L"])
    I = codes.shape[0]
    fids = ["fam%d" % (i % 3) for i in range(I)]
    for i, f in {0: 0, 1: 0, 2: 0, 3: 1, 4: 2, 7: 3, 11: 3}.items():
        fids[i] = "fam%d" % f
    iids = ["ind%d" % i for i in range(I)]
    return codes, planted, fids, iids


def digest(phi, cnt):
    return hashlib.sha256(canonical_bytes(phi) + np.ascontiguousarray(cnt, dtype=np.uint32).tobytes()).hexdigest()


FIXED = dict(I=130, L=1100)


def fixed_case():
    """packed records with garbage in every bit that carries no individual, and their codes [I][L]"""
    codes = draw_codes(FIXED["I"], FIXED["L"], seed=77, missing=0.1)
    plant(codes, seed=77)
    return repack(codes, 77, 3), codes


def king_geometry(I, n_rows, L, target_blocks):
    """king_geometry_of (multiclust_amd/csrc/mchip_feature_geometry.h) restated: (n_rtiles, n_ctiles, n_split, stages_per_split);
    tests/test_king_cpu.py holds it to the header"""
    n_rt, n_ct = -(-n_rows // TILE), -(-I // TILE)
    base = n_rt * n_ct
    n_stages = -(-(-(-L // 64)) // (STAGE_VARIANTS // 64))
    want = max(1, min(-(-target_blocks // base) if base > 0 else 1, n_stages, 65535))
    per = -(-n_stages // want)
    return n_rt, n_ct, -(-n_stages // per), per


def blocks_per_cu(env):
    """the knob as mchip.hip reads it: MCHIP_BLOCKS_PER_CU_IND, else MCHIP_BLOCKS_PER_CU, else 64"""
    return int(env.get("MCHIP_BLOCKS_PER_CU_IND") or env.get("MCHIP_BLOCKS_PER_CU") or 64)


# the cases of the launch-geometry test: 18 words of variants = 5 stages, the last of 2 words.  On the 256 compute units of an
# MI355X, MCHIP_BLOCKS_PER_CU = 1 asks for 256 workgroups: "fixed" (3 x 3 tiles) is cut into 5 runs of one stage under every knob;
# "runs" (11 x 11 = 121 tiles) into 3 runs of 2, 2 and 1 stages; "whole" (17 x 17 = 289 tiles) is not cut: one run of 5 stages
GEOMETRY = dict(fixed=dict(I=FIXED["I"], L=FIXED["L"]), runs=dict(I=641, L=1100), whole=dict(I=1025, L=1100))


def geometry_case(name):
    """(packed records with garbage in every bit that carries no individual, codes [I][L])"""
    if name == "fixed":
        return fixed_case()
    g = GEOMETRY[name]
    codes = draw_codes(g["I"], g["L"], seed=900 + g["I"], missing=0.1)
    plant(codes, seed=g["I"])
    return repack(codes, g["I"], 3), codes


if __name__ == "__main__":
    # king_util.py <case>: the digest of the device's result, and the geometry the launch had: n_split stages_per_split n_cu
    import os
    import sys
    from multiclust_amd import hip
    name = sys.argv[1] if len(sys.argv) > 1 else "fixed"
    g = GEOMETRY[name]
    ctx = hip.Context(0)
    bed, _ = geometry_case(name)
    print(digest(*ctx.bed_king(g["I"], bed)))
    n_cu = ctx.device_info()[1]
    geo = king_geometry(g["I"], g["I"], g["L"], blocks_per_cu(os.environ) * (n_cu if n_cu > 0 else 256))
    print("%d %d %d" % (geo[2], geo[3], n_cu))
    ctx.close()
