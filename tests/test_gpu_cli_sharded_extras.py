"""-m gpu: the sharded path's copy of the bookkeeping (--streams 2: two workers on one GPU) together with -A, --cv, --se and -b.
Every unit of a sharded run starts at the serial stream's position and the kernels are bitwise reproducible, so the same command
with and without --streams 2 prints the same lines (elapsed time masked) and writes the same files, byte for byte."""
import os
import re

import pytest

from cli_util import ROOT, run_fresh

pytestmark = pytest.mark.gpu
DATA = os.path.join(ROOT, "tests", "golden", "data", "multi.stru")
CV_LINE = re.compile(r"^CV error \(K=(\d+), ")
SE_LINE = re.compile(r"^Bootstrap SE \(K=(\d+), ")
COMMON = ["-f", DATA, "-a", "-s", "3", "-r", "7"]


def individuals():
    with open(DATA) as f:
        return (sum(1 for ln in f if ln.strip()) - 1) // 2      # one header line, two lines per diploid individual


def run(args, d):
    return run_fresh(COMMON + args, d)[:2]


def partition_file(tmp_path):
    path = tmp_path / "partition.txt"
    path.write_text(" ".join(str(i % 3 + 1) for i in range(individuals())) + "\n")
    return str(path)


CASES = {
    "partition": (["-k", "3", "-n", "3"], True),                   # three units over two workers: one worker fits two
    "cv": (["-1", "1", "-2", "2", "-n", "2", "--cv", "3"], False),
    "cv_se": (["-1", "1", "-2", "2", "-n", "2", "--cv", "3", "--se", "5"], False),
    "bootstrap_partition": (["-k", "3", "-n", "2", "-b", "2"], True),   # the H0 estimate, and bootstrap fits that are not partitioned
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_two_streams_reproduce_the_serial_run(case, tmp_path):
    args, with_partition = CASES[case]
    if with_partition:
        args = args + ["-A", partition_file(tmp_path)]
    serial, files_serial = run(args, tmp_path / "serial")
    sharded, files_sharded = run(args + ["--streams", "2"], tmp_path / "sharded")
    assert sharded == serial
    assert sorted(files_sharded) == sorted(files_serial) and len(files_serial) >= 5
    for f in files_serial:
        assert files_sharded[f] == files_serial[f], f
    if with_partition:
        assert not any(" ND " in ln for ln in serial if ln.startswith(DATA))   # the summary lines carry the index
    if "--cv" in args:
        assert [CV_LINE.match(ln).group(1) for ln in serial if CV_LINE.match(ln)] == ["1", "2"]
    if "--se" in args:
        for n, ln in enumerate(serial):                           # per K the CV line comes first, the SE line right behind it
            if CV_LINE.match(ln):
                assert SE_LINE.match(serial[n + 1]).group(1) == CV_LINE.match(ln).group(1), serial[n:n + 2]
        assert sum(1 for ln in serial if SE_LINE.match(ln)) == 2
