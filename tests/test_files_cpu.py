"""The file plumbing of the host side (multiclust_amd/host/mc_files.h) as a program of its own (tests/files_host_driver.c, plain and
under AddressSanitizer + UBSan), where the feature tests do not look: the result path at every form of -d and in a buffer it does not
fit, the line a failed open leaves, the lines of a text that hold anything but white space -- what the readers count and what the
kept-lines copy writes -- and the two writers of a filter at the ends of their maps.  Every expectation is restated here in Python
from the wording of mc_cli.h; nothing is read back from the code under test."""
import os

import pytest

import host_driver

BLANK = b" \t\r"


# (mc_files.h comes with mc_cli.h; the program's output is taken as bytes and decoded here)
driver = host_driver.plain_and_sanitized("files_host", ["tests/files_host_driver.c"], werror=True, timeout=60, text=False,
                                         result=lambda res: (res.stdout.decode(), res.stderr.decode()))


# ---- the result path ----
SUFFIXES = (".admix.K=3.first.txt", ".second", "_third_and_longer_12.popq")     # what the driver's three calls put behind the stem


def stem_of(o, d, name):
    """-o, else -d, a '/' unless -d is empty or ends in '/' or '\\', and the file part"""
    if o is not None:
        return o
    return d + ("/" if d and d[-1] not in "/\\" else "") + name


@pytest.mark.parametrize("o,d,stem", [("out/stem", "ignored", "out/stem"), (None, "./", "./data.stru"), (None, "dir", "dir/data.stru"),
                                      (None, "dir/", "dir/data.stru"), (None, "dir\\", "dir\\data.stru"), (None, "", "data.stru")])
def test_result_path_of_every_form_of_the_directory(driver, tmp_path, o, d, stem):
    assert stem_of(o, d, "data.stru") == stem
    out, _ = driver("path", 4400, "-" if o is None else o, d, "data.stru", cwd=tmp_path)
    assert out.split("\n") == [str(len(stem))] + [stem + s for s in SUFFIXES] + [""]


@pytest.mark.parametrize("n", [1, 2, 9, 13, 14, 15, 20, 33, 34])
def test_result_path_is_cut_to_its_buffer_and_never_overruns_it(driver, tmp_path, n):
    """a buffer of n bytes holds n - 1 of the path: shorter than the stem (13 bytes), exactly it, one more, and one short of and
    exactly the first suffix's end; the sanitized build's buffer is n bytes on the heap"""
    stem = stem_of(None, "dir", "data.stru")
    assert len(stem) == 13 and len(stem + SUFFIXES[0]) == 33
    out, _ = driver("path", n, "-", "dir", "data.stru", cwd=tmp_path)
    kept = min(len(stem), n - 1)
    assert out.split("\n") == [str(kept)] + [(stem[:kept] + s)[:n - 1] for s in SUFFIXES] + [""]


# ---- opening ----
def test_open_in_a_directory_that_does_not_exist_says_who_asked(driver, tmp_path):
    path = os.path.join("no_such_dir", "stem.prune.in")
    for origin in ("mc_ld.c", "some_caller.c"):
        out, err = driver("open", origin, path, cwd=tmp_path)
        assert out == "NULL\n"
        assert err == "ERROR [%s::open_out]: could not open file '%s'\n" % (origin, path)
    out, err = driver("open", "mc_ld.c", "made", cwd=tmp_path)
    assert out == "open\n" and err == "" and (tmp_path / "made").read_text() == "written\n"


def test_slurp_reads_every_byte_and_reports_a_file_it_cannot_open(driver, tmp_path):
    (tmp_path / "bytes").write_bytes(b"a b\r\n\x00c\n")
    assert driver("slurp", "mc_bed.c", "bytes", cwd=tmp_path) == ("0 8\n", "")
    (tmp_path / "empty").write_bytes(b"")
    assert driver("slurp", "mc_bed.c", "empty", cwd=tmp_path) == ("0 0\n", "")
    out, err = driver("slurp", "mc_impute.c", "absent", cwd=tmp_path)
    assert out == "5 0\n" and err == "ERROR [mc_impute.c::slurp]: could not open file 'absent'\n"


# ---- the lines of a text ----
def lines_of(text):
    """(line, first, end, stop) of every line that holds anything but white space, as mc_cli.h words mc_lines"""
    out, at = [], 0
    while at < len(text):
        nl = text.find(b"\n", at)
        end = len(text) if nl < 0 else nl
        stop = end if nl < 0 else end + 1
        first = at
        while first < end and text[first] in BLANK:
            first += 1
        if first < end:
            out.append((at, first, end, stop))
        at = stop
    return out


TEXTS = {
    "empty": b"",
    "one line without a newline": b"1 rs1 0 100 A G",
    "only white space": b" \t\r\n\n   \n\t",
    "blank lines between": b"\n1 a\n\n \t \n2 b\n\r\n\n3 c\n\n",
    "crlf": b"f1 i1 0 0 1 -9\r\nf1 i2 0 0 2 -9\r\n\r\nf2 i3 0 0 1 -9\r\n",
    "last line without a newline": b"1 a\n2 b\n  3 c",
    "one token": b"chr1\n  chr2  \nchr3",
    "indented, tabs": b"\t1\trs1\n \t 2\trs2\t\n",
}
# what each case must yield: the data lines without their ends
EXPECTED_LINES = {
    "empty": [],
    "one line without a newline": [b"1 rs1 0 100 A G"],
    "only white space": [],
    "blank lines between": [b"1 a", b"2 b", b"3 c"],
    "crlf": [b"f1 i1 0 0 1 -9\r", b"f1 i2 0 0 2 -9\r", b"f2 i3 0 0 1 -9\r"],
    "last line without a newline": [b"1 a", b"2 b", b"  3 c"],
    "one token": [b"chr1", b"  chr2  ", b"chr3"],
    "indented, tabs": [b"\t1\trs1", b" \t 2\trs2\t"],
}


@pytest.mark.parametrize("case", sorted(TEXTS))
def test_line_iterator_and_the_copy_of_every_line(driver, tmp_path, case):
    """the count, each line's bytes without its end (what a reader tokenises) and with it (what the copy writes), and the copy of all of
    them: the text without its blank lines"""
    text = TEXTS[case]
    want = lines_of(text)
    assert [text[a:c] for a, _, c, _ in want] == EXPECTED_LINES[case]          # (the restatement, against the cases written out)
    assert all(text[c:d] in (b"\n", b"") and text[b] not in BLANK for _, b, c, d in want)
    (tmp_path / "text").write_bytes(text)
    out, _ = driver("lines", "text", cwd=tmp_path)
    got = out.split("\n")
    assert got[-1] == "" and int(got[0]) == len(want) == len(got) - 2
    assert [tuple(int(x) for x in ln.split()) for ln in got[1:-1]] == want
    out, err = driver("copy", "text", "all", *range(len(want)), cwd=tmp_path)
    assert (out, err) == ("0\n", "")
    assert (tmp_path / "all").read_bytes() == b"".join(text[a:d] for a, _, _, d in want)


# ---- the kept-lines copy and the lists ----
MAPS = ("all", "first", "last", "none")


def map_of(kind, n):
    return {"all": list(range(n)), "first": [0], "last": [n - 1], "none": []}[kind]


@pytest.mark.parametrize("kind", MAPS)
@pytest.mark.parametrize("case", ["blank lines between", "crlf", "last line without a newline"])
def test_kept_lines_copy_counts_lines_as_the_readers_do(driver, tmp_path, case, kind):
    """entry v of the map is the v-th line that holds anything: blank lines neither count nor are copied, a kept line goes out with its
    own end (a last line without a newline stays without one)"""
    text = TEXTS[case]
    want = lines_of(text)
    kept = map_of(kind, len(want))
    (tmp_path / "text").write_bytes(text)
    assert driver("copy", "text", "kept", *kept, cwd=tmp_path) == ("0\n", "")
    assert (tmp_path / "kept").read_bytes() == b"".join(text[want[v][0]:want[v][3]] for v in kept)


def test_kept_lines_copy_reports_a_source_it_cannot_open(driver, tmp_path):
    out, err = driver("copy", "absent", "kept", 0, cwd=tmp_path)
    assert out == "5\n" and err == "ERROR [files_host_driver.c::slurp]: could not open file 'absent'\n"
    assert not (tmp_path / "kept").exists()


@pytest.mark.parametrize("kind", MAPS)
@pytest.mark.parametrize("n_file", [1, 5])
def test_lists_of_the_kept_and_the_removed(driver, tmp_path, n_file, kind):
    """<stem>.kept.in holds the entries of the map and <stem>.kept.out the others, each in file order: everything kept leaves .out
    empty, nothing kept leaves .in empty, and both files exist either way"""
    kept = map_of(kind, n_file)
    assert driver("lists", "stem", n_file, *kept, cwd=tmp_path) == ("0\n", "")
    assert (tmp_path / "stem.kept.in").read_text() == "".join("e%d\n" % v for v in range(n_file) if v in kept)
    assert (tmp_path / "stem.kept.out").read_text() == "".join("e%d\n" % v for v in range(n_file) if v not in kept)


def test_lists_in_a_directory_that_does_not_exist(driver, tmp_path):
    out, err = driver("lists", os.path.join("no_such_dir", "stem"), 3, 1, cwd=tmp_path)
    assert out == "5\n" and err == "ERROR [files_host_driver.c::open_out]: could not open file '%s'\n" % os.path.join("no_such_dir", "stem.kept.in")
