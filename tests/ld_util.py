"""Linkage disequilibrium between the variants of packed PLINK records (TEST INFRASTRUCTURE): the definition of r2 in
include/multiclust_hip.h (mchip_bed_ld_band) restated with Python integers and numpy.float64, the forward greedy rule of --prune
(multiclust_amd/host/mc_ld.c) restated as it is worded -- a variant looks back at the kept variants before it --, and a generator of
records with real LD.  Filesets are written by bedfiles.py.

Run as a program it prints the digest of the device's band of fixed_case(): tests/test_gpu_ld.py starts it in fresh processes under
different launch geometries."""
import hashlib

import numpy as np

import bedfiles
from bits import canonical_bytes, same_bits, ulp_distance      # noqa: F401  (the tests take the last two from here)

# restated from multiclust_amd/csrc/mchip_feature_geometry.h
TILE = 64        # first variants per workgroup
DCHUNK = 32      # offsets per workgroup
STAGE_INDIVIDUALS = 128
MAX_WINDOW = 4096

DOSAGE = np.array([0, -1, 1, 2], dtype=np.int64)    # of the codes 0, 1 (missing), 2, 3


def codes_of(bed, I):
    """[L][record_bytes] packed records -> [L][I] codes; padding bits and bytes behind ceil(I/4) carry no individual"""
    bed = np.asarray(bed, dtype=np.uint8)
    L = bed.shape[0]
    four = np.stack([(bed >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(L, -1)
    return four[:, :I]


def sums(cx, cy):
    """n, Sx, Sy, Sxx, Syy, Sxy of two variants' codes over the individuals missing at neither, as Python integers"""
    n = Sx = Sy = Sxx = Syy = Sxy = 0
    for a, b in zip(cx, cy):
        x, y = int(DOSAGE[a]), int(DOSAGE[b])
        if x < 0 or y < 0:
            continue
        n += 1; Sx += x; Sy += y; Sxx += x * x; Syy += y * y; Sxy += x * y
    return n, Sx, Sy, Sxx, Syy, Sxy


def cvv(n, Sx, Sy, Sxx, Syy, Sxy):
    return n * Sxy - Sx * Sy, n * Sxx - Sx * Sx, n * Syy - Sy * Sy


def r2_of_sums(n, Sx, Sy, Sxx, Syy, Sxy):
    """two products and one division in float64; NaN exactly when a variance is 0"""
    C, Vx, Vy = cvv(n, Sx, Sy, Sxx, Syy, Sxy)
    if Vx == 0 or Vy == 0:
        return np.float64("nan")
    c = np.float64(C)
    return (c * c) / (np.float64(Vx) * np.float64(Vy))


def r2_pair(cx, cy):
    return r2_of_sums(*sums(cx, cy))


def band(bed, I, window, l0=0, n_first=None):
    """r2[n_first][window] as mchip_bed_ld_band defines it: row l - l0, column d - 1 = r2(l, l + d), NaN where l + d >= L.  int64 sums
    per offset (exact: every product stays below 2^62 for I < 2^29), the same float64 expression as r2_of_sums."""
    codes = codes_of(bed, I)
    L = codes.shape[0]
    n_first = L - l0 if n_first is None else n_first
    x = DOSAGE[codes]                                   # [L][I], -1 missing
    ok = x >= 0
    x = np.where(ok, x, 0)
    out = np.full((n_first, window), np.nan)
    for d in range(1, min(window, L - 1 - l0) + 1):
        m = min(n_first, L - d - l0)                    # rows with a second variant
        if m <= 0:
            break
        a, b = slice(l0, l0 + m), slice(l0 + d, l0 + d + m)
        both = ok[a] & ok[b]
        xa, xb = x[a] * both, x[b] * both
        n = both.sum(axis=1, dtype=np.int64)
        Sx, Sy = xa.sum(axis=1), xb.sum(axis=1)
        Sxx, Syy, Sxy = (xa * xa).sum(axis=1), (xb * xb).sum(axis=1), (xa * xb).sum(axis=1)
        C, Vx, Vy = n * Sxy - Sx * Sy, n * Sxx - Sx * Sx, n * Syy - Sy * Sy
        with np.errstate(divide="ignore", invalid="ignore"):
            c = C.astype(np.float64)
            r = (c * c) / (Vx.astype(np.float64) * Vy.astype(np.float64))
        r[(Vx == 0) | (Vy == 0)] = np.nan
        out[:m, d - 1] = r
    return out


def greedy(r2, window, t, chrom=None):
    """keep[l] of the forward greedy rule on the whole band r2[L][>= window]: in file order, l is removed when some kept l' with
    l - window <= l' < l on the same chromosome has r2(l', l) > t (NaN compares false)"""
    L = r2.shape[0]
    keep = np.ones(L, dtype=bool)
    for l in range(L):
        for lp in range(max(0, l - window), l):
            if keep[lp] and (chrom is None or chrom[lp] == chrom[l]) and r2[lp, l - lp - 1] > t:
                keep[l] = False
                break
    return keep


def draw_records(I, L, seed, copy=0.6, flip=0.08, missing=0.0, extra_bytes=0, garbage=True):
    """(bed [L][ceil(I/4) + extra_bytes], codes [I][L]): Hardy-Weinberg variants; with probability `copy` a variant is its
    predecessor with `flip` of the calls drawn again (LD blocks); `missing` of the calls missing; garbage: random padding bits in the
    last byte of a record and random bytes behind it"""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.1, 0.9, size=L)
    fresh = ((rng.random((I, L)) < f) * 1 + (rng.random((I, L)) < f) * 1)
    a2 = fresh.copy()
    for l in range(1, L):
        if rng.random() < copy:
            again = rng.random(I) < flip
            a2[:, l] = np.where(again, fresh[:, l], a2[:, l - 1])
    codes = np.array([bedfiles.HOM1, bedfiles.HET, bedfiles.HOM2], dtype=np.uint8)[a2]
    codes[rng.random((I, L)) < missing] = bedfiles.MISS
    return repack(codes, seed, extra_bytes, garbage), codes


def repack(codes, seed=0, extra_bytes=0, garbage=True):
    """[I][L] codes -> records, with garbage in everything that carries no individual"""
    I, L = codes.shape
    rng = np.random.default_rng(seed + 977)
    bed = bedfiles.pack(codes)
    if garbage and I % 4:
        pad = (rng.integers(0, 256, size=L, dtype=np.uint8) << (2 * (I % 4))).astype(np.uint8)
        bed[:, -1] |= pad
    if extra_bytes:
        tail = rng.integers(0, 256, size=(L, extra_bytes), dtype=np.uint8) if garbage else np.zeros((L, extra_bytes), dtype=np.uint8)
        bed = np.concatenate([bed, tail], axis=1)
    return np.ascontiguousarray(bed)


def plant(codes, seed=0):
    """special variants where the shape has room, in place: one all missing, one monomorphic, one all heterozygous, and a pair of
    duplicates next to each other (r2 = 1 exactly when polymorphic); returns their positions"""
    I, L = codes.shape
    rng = np.random.default_rng(seed + 31)
    where = {}
    if L >= 8:
        pos = rng.permutation(np.arange(0, L - 1, 2))[:4]
        where = dict(zip(("missing", "mono", "het", "dup"), (int(p) for p in pos)))
        codes[:, where["missing"]] = bedfiles.MISS
        codes[:, where["mono"]] = bedfiles.HOM2
        codes[:, where["het"]] = bedfiles.HET
        codes[:, where["dup"] + 1] = codes[:, where["dup"]]
    return where


def digest(r2):
    return hashlib.sha256(canonical_bytes(r2)).hexdigest()


FIXED = dict(I=1001, L=300, window=305)


def fixed_case():
    bed, codes = draw_records(FIXED["I"], FIXED["L"], seed=77, missing=0.1, extra_bytes=3)
    return bed


CLI = dict(I=200, L=600, t=0.5, window=20, split=330)


def cli_case():
    """(codes [I][L], chrom [L]) of the command-line tests: LD blocks, 5 % missing calls, the special variants planted, two
    chromosomes with a run of duplicates across their boundary"""
    bed, codes = draw_records(CLI["I"], CLI["L"], seed=4242, copy=0.7, flip=0.05, missing=0.05)
    plant(codes, seed=4242)
    s = CLI["split"]
    for l in range(s - 2, s + 3):
        codes[:, l] = codes[:, s - 3]
    # the window's two ends: a stretch of unlinked variants with a copy of its first one W behind it (removed) and a copy of its
    # second one W + 1 behind that (kept)
    W, at = CLI["window"], 100
    rng = np.random.default_rng(99)
    fresh = (rng.random((CLI["I"], W + 3)) < 0.5) * 1 + (rng.random((CLI["I"], W + 3)) < 0.5) * 1
    codes[:, at:at + W + 3] = np.array([bedfiles.HOM1, bedfiles.HET, bedfiles.HOM2], dtype=np.uint8)[fresh]
    codes[:, at + W] = codes[:, at]
    codes[:, at + W + 2] = codes[:, at + 1]
    chrom = ["1"] * s + ["2"] * (CLI["L"] - s)
    return codes, chrom


def write_bim(prefix, chrom, ids=None, pos=None):
    """prefix.bim with these chromosomes, ids (snp<l>) and base-pair positions (l + 1)"""
    with open(prefix + ".bim", "w") as f:
        for l, c in enumerate(chrom):
            f.write("%s\t%s\t0\t%d\tA\tC\n" % (c, ids[l] if ids else "snp%d" % l, pos[l] if pos is not None else l + 1))


if __name__ == "__main__":
    from multiclust_amd import hip
    ctx = hip.Context(0)
    bed = fixed_case()
    print(digest(ctx.bed_ld_band(FIXED["I"], bed, window=FIXED["window"])))
    ctx.close()
