"""PLINK 1 filesets for the tests (TEST INFRASTRUCTURE): a code matrix drawn with numpy, written as .bed/.bim/.fam and as the
equivalent STRUCTURE file that defines what the fileset means (multiclust_amd/host/mc_cli.h, mc_read_bed).

Codes are the values of the two bits of a .bed genotype, low bit first: 0 homozygous A1, 1 missing, 2 heterozygous,
3 homozygous A2."""
import numpy as np

HOM1, MISS, HET, HOM2 = 0, 1, 2, 3
# the two lines of the equivalent STRUCTURE file per code
FIRST = {HOM1: "1", MISS: "-9", HET: "1", HOM2: "2"}
SECOND = {HOM1: "1", MISS: "-9", HET: "2", HOM2: "2"}


def draw_codes(I, L, missing=0.0, seed=0, plant=True):
    """[I][L] codes: per locus an A2 frequency, Hardy-Weinberg genotypes, `missing` of the calls missing.  plant: where the shape
    has room, loci with A1 only, A2 only, heterozygotes only and no call at all, and an individual without a single call."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.05, 0.95, size=L)
    a = (rng.random((I, L)) < f) * 1 + (rng.random((I, L)) < f) * 1          # copies of A2
    codes = np.array([HOM1, HET, HOM2], dtype=np.uint8)[a]
    codes[rng.random((I, L)) < missing] = MISS
    if plant:
        for l, c in zip(rng.permutation(L)[:4], (HOM1, HOM2, HET, MISS)):
            codes[:, l] = c
        if I > 1:
            codes[int(rng.integers(I)), :] = MISS
    return codes


def pack(codes, padding=0):
    """[I][L] codes -> [L][ceil(I/4)] bytes: sample j of a record in byte j/4, bits 2(j%4) and 2(j%4)+1; `padding` fills the
    bits of the last byte that carry no sample"""
    I, L = codes.shape
    rb = (I + 3) // 4
    full = np.full((L, rb * 4), padding & 3, dtype=np.uint8)
    full[:, :I] = codes.T
    q = full.reshape(L, rb, 4)
    return (q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).astype(np.uint8)


def default_ids(I, n_fid=3):
    return ["fam%d" % (i * 7 % n_fid) for i in range(I)], ["ind%d" % i for i in range(I)]


def write_fileset(prefix, codes, padding=0, fids=None, iids=None, magic=b"\x6c\x1b\x01"):
    """prefix.bed / .bim / .fam; returns the packed records"""
    I, L = codes.shape
    if fids is None:
        fids, iids = default_ids(I)
    bed = pack(codes, padding)
    with open(prefix + ".bed", "wb") as f:
        f.write(magic)
        f.write(bed.tobytes())
    with open(prefix + ".bim", "w") as f:
        for l in range(L):
            f.write("1\tsnp%d\t0\t%d\tA\tC\n" % (l, l + 1))
    with open(prefix + ".fam", "w") as f:
        for i in range(I):
            f.write("%s %s 0 0 0 -9\n" % (fids[i], iids[i]))
    return bed


def write_equivalent_stru(path, codes, fids=None, iids=None):
    """the STRUCTURE file the fileset stands for: a header of L locus names, then per individual two lines `IID FID a_1 .. a_L`"""
    I, L = codes.shape
    if fids is None:
        fids, iids = default_ids(I)
    first = np.array([FIRST[c] for c in range(4)])[codes]
    second = np.array([SECOND[c] for c in range(4)])[codes]
    with open(path, "w") as f:
        f.write(" ".join("snp%d" % l for l in range(L)) + "\n")
        for i in range(I):
            f.write("%s %s %s\n" % (iids[i], fids[i], " ".join(first[i])))
            f.write("%s %s %s\n" % (iids[i], fids[i], " ".join(second[i])))
