"""PLINK .bed input on the host (multiclust_amd/host/mc_bed.c), without a GPU: a fileset means what the STRUCTURE reader yields
on its equivalent STRUCTURE file, so mc_read_bed + mc_bed_decode are compared with mc_read_structure on that file -- every
field, exactly; then one fileset decoded by hand, the failures and their exit statuses, and the command line's refusals."""
import os
import subprocess

import numpy as np
import pytest

import bedfiles as bf
from cli_util import BIN
from multiclust_amd import host

SHAPE_I = (1, 3, 4, 5, 8, 9, 63, 65, 257)
SHAPE_L = (1, 7, 8, 9, 63, 65, 300)
FIELDS = ("I", "L", "ploidy", "M", "T", "missing_data", "interleaved", "numpops", "names", "pops", "i_p", "L_alleles")


def assert_same_data_set(bed, stru):
    for k in FIELDS:
        assert bed[k] == stru[k], k
    for k in ("ua", "toff", "locale", "geno"):
        assert bed[k].dtype == stru[k].dtype and np.array_equal(bed[k], stru[k]), k
    assert np.array_equal(bed["ua_decoded"], stru["ua"])       # the decoder's own allele counts
    assert bed["geno_is_null"]                                  # the reader itself built no genotype


def both_readers(tmp_path, codes, padding=0):
    prefix, stru = str(tmp_path / "set"), str(tmp_path / "equivalent.stru")
    packed = bf.write_fileset(prefix, codes, padding=padding)
    bf.write_equivalent_stru(stru, codes)
    rc_b, b = host.read_bed(prefix)
    rc_s, s = host.read_structure(stru)
    assert rc_b == 0 and rc_s == 0
    assert np.array_equal(b["bed"], packed)
    return b, s


@pytest.mark.parametrize("missing", [0.0, 0.03, 0.5])
@pytest.mark.parametrize("L", SHAPE_L)
@pytest.mark.parametrize("I", SHAPE_I)
def test_decoder_matches_reader_on_equivalent_file(I, L, missing, tmp_path):
    codes = bf.draw_codes(I, L, missing=missing, seed=1000 * I + L)
    b, s = both_readers(tmp_path, codes)
    assert_same_data_set(b, s)


@pytest.mark.parametrize("I,L,padding", [(5, 9, 3), (9, 65, 1), (63, 8, 2), (257, 7, 3), (1, 7, 3)])
def test_padding_bits_carry_no_sample(I, L, padding, tmp_path):
    """garbage in the bits behind the last sample of a record: with padding = 0 they would read as homozygous A1, with 2 or 3
    as carriers of A2, with 1 as missing calls -- none of which may reach the allele lists (the planted A1-only, A2-only and
    all-missing loci would change their counts)"""
    codes = bf.draw_codes(I, L, missing=0.03, seed=77 + I)
    b, s = both_readers(tmp_path, codes, padding=padding)
    assert_same_data_set(b, s)
    clean = bf.pack(codes, 0)
    assert I % 4 == 0 or not np.array_equal(clean, b["bed"])    # the garbage is really there


def test_planted_loci_follow_the_reader(tmp_path):
    """what the reader gives for the special loci, spelled out: A1 only -> one allele, index 0; A2 only -> one allele, index 0;
    heterozygotes only -> two alleles; no observed call -> no allele column and no missing_data from that locus"""
    I = 6
    codes = np.empty((I, 6), dtype=np.uint8)
    codes[:, 0] = bf.HOM1
    codes[:, 1] = bf.HOM2
    codes[:, 2] = bf.HET
    codes[:, 3] = bf.MISS
    codes[:, 4] = [bf.HOM2, bf.MISS, bf.HOM2, bf.HOM2, bf.MISS, bf.HOM2]      # A2 and missing: phantom slot
    codes[:, 5] = [bf.HOM1, bf.HET, bf.HOM2, bf.HOM1, bf.HET, bf.HOM2]
    b, s = both_readers(tmp_path, codes)
    assert_same_data_set(b, s)
    assert b["ua"].tolist() == [1, 1, 2, 0, 2, 2] and b["L_alleles"] == [[1], [2], [1, 2], [], [2], [1, 2]]
    assert b["missing_data"] == 1 and b["M"] == 2 and b["T"] == 8
    only_allmiss = np.full((I, 2), bf.MISS, dtype=np.uint8)
    only_allmiss[:, 1] = bf.HOM1
    b, s = both_readers(tmp_path, only_allmiss)
    assert_same_data_set(b, s)
    assert b["missing_data"] == 0 and b["ua"].tolist() == [0, 1]


def test_hand_decoded_fileset(tmp_path):
    """5 individuals, 3 variants, two bytes per record:
    variant 0: codes 0 2 3 1 | 0 + padding 111111 -> 0x78 0xfc: A1, A2 and a missing call: three allele slots
    variant 1: codes 3 3 1 3 | 3                   -> 0xdf 0x03: A2 only (index 0) and a missing call: two slots
    variant 2: codes 1 1 1 1 | 1                   -> 0x55 0x01: no observed call: no slot"""
    prefix = str(tmp_path / "hand")
    open(prefix + ".bed", "wb").write(bytes.fromhex("6c1b01" "78fc" "df03" "5501"))
    open(prefix + ".bim", "w").write("".join("1 rs%d 0 %d G T\n" % (l, 100 + l) for l in range(3)))
    open(prefix + ".fam", "w").write("north a1 0 0 1 -9\nsouth a2 0 0 2 -9\nnorth a3 0 0 1 -9\n\neast a4 0 0 0 -9\nsouth a5 0 0 2 -9\n")
    rc, b = host.read_bed(prefix)
    assert rc == 0
    F = 0xFF
    expected = np.array([[[0, 0], [0, 0], [F, F]],
                         [[0, 1], [0, 0], [F, F]],
                         [[1, 1], [F, F], [F, F]],
                         [[F, F], [0, 0], [F, F]],
                         [[0, 0], [0, 0], [F, F]]], dtype=np.uint8)
    assert np.array_equal(b["geno"], expected)
    assert b["ua"].tolist() == [3, 2, 0] and b["ua_decoded"].tolist() == [3, 2, 0] and b["toff"].tolist() == [0, 3, 5, 5]
    assert (b["I"], b["L"], b["ploidy"], b["M"], b["T"], b["missing_data"], b["interleaved"]) == (5, 3, 2, 3, 5, 1, 0)
    assert b["L_alleles"] == [[1, 2], [2], []]
    assert b["names"] == ["a1", "a2", "a3", "a4", "a5"] and b["pops"] == ["north", "south", "east"]
    assert b["locale"].tolist() == [0, 1, 0, 2, 1] and b["i_p"] == [2, 2, 1] and b["numpops"] == 3


def test_decode_accepts_a_row_pitch(tmp_path):
    """records further apart than ceil(I/4) bytes (the C-ABI takes any pitch): the bytes between them are not samples"""
    codes = bf.draw_codes(9, 20, missing=0.1, seed=3)
    packed = bf.pack(codes)
    wide = np.full((20, packed.shape[1] + 3), 0xAA, dtype=np.uint8)
    wide[:, :packed.shape[1]] = packed
    ua0, g0 = host.bed_decode(9, packed)
    ua1, g1 = host.bed_decode(9, wide)
    assert np.array_equal(ua0, ua1) and np.array_equal(g0, g1)


def fileset(tmp_path, I=10, L=6):
    codes = bf.draw_codes(I, L, missing=0.1, seed=5)
    prefix = str(tmp_path / "f")
    bf.write_fileset(prefix, codes)
    return prefix, codes


def test_failures_leave_with_the_reference_statuses(tmp_path):
    prefix, codes = fileset(tmp_path)
    good = open(prefix + ".bed", "rb").read()
    assert host.read_bed(prefix)[0] == 0

    def status_with(bed_bytes):
        open(prefix + ".bed", "wb").write(bed_bytes)
        rc, out = host.read_bed(prefix)
        assert out is None or rc == 0
        return rc

    assert status_with(b"\x6c\x1c\x01" + good[3:]) == 7          # wrong magic
    assert status_with(b"\x6d\x1b\x01" + good[3:]) == 7
    assert status_with(b"\x6c\x1b\x00" + good[3:]) == 7          # sample-major mode
    assert status_with(good[:-1]) == 7                           # truncated
    assert status_with(good + b"\x00") == 7                      # overlong
    assert status_with(good[:2]) == 7                            # not even a header
    assert status_with(good) == 0
    fam = open(prefix + ".fam").read()
    open(prefix + ".fam", "w").write(fam + "famX extra 0 0 0 -9\nfamX extra2 0 0 0 -9\nfamX extra3 0 0 0 -9\n")   # 13 individuals: 4 bytes per record
    assert host.read_bed(prefix)[0] == 7                         # .fam line count against the size
    open(prefix + ".fam", "w").write(fam)
    bim = open(prefix + ".bim").read()
    open(prefix + ".bim", "w").write(bim + "1 more 0 99 A C\n")
    assert host.read_bed(prefix)[0] == 7                         # .bim line count against the size
    os.remove(prefix + ".bim")
    assert host.read_bed(prefix)[0] == 5                         # a file that cannot be opened
    open(prefix + ".bim", "w").write(bim)
    os.remove(prefix + ".fam")
    assert host.read_bed(prefix)[0] == 5
    open(prefix + ".fam", "w").write(fam)
    os.remove(prefix + ".bed")
    assert host.read_bed(prefix)[0] == 5


@pytest.mark.parametrize("extra", [["-f", "other.stru"], ["-R"], ["-p", "4"]])
def test_command_line_refuses_bed_with_structure_only_flags(extra, tmp_path):
    prefix, codes = fileset(tmp_path)
    res = subprocess.run([BIN, "--bed", prefix, "-a", "-k", "2"] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         timeout=60, cwd=str(tmp_path))
    assert res.returncode == 11, (res.returncode, res.stderr[-500:])
    assert "--bed" in res.stderr


def test_command_line_statuses_of_a_bad_fileset(tmp_path):
    """the reader's statuses reach the shell; all of this happens before a GPU is needed"""
    prefix, codes = fileset(tmp_path)
    os.remove(prefix + ".bim")
    res = subprocess.run([BIN, "--bed", prefix, "-a", "-k", "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert res.returncode == 5, res.stderr[-500:]
    res = subprocess.run([BIN, "--bed"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert res.returncode == 10
    res = subprocess.run([BIN, "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert "--bed <prefix>" in res.stdout


def test_struct_mirrors_cover_the_new_trailing_fields():
    """the C structs grew at the end; the ctypes mirrors must be as long as what the C side reads"""
    import ctypes as C
    assert host.McData._fields_[-3:] == [("bed", C.c_void_p), ("bed_record_bytes", C.c_size_t), ("lazy", C.c_void_p)]
    assert [n for n, _ in host.CliData._fields_[-3:]] == ["bed", "bed_record_bytes", "lazy"]
    assert host.CliOptions._fields_[-1][0] == "bed_prefix"
