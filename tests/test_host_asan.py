"""The plain-C host side under AddressSanitizer + UBSan (CPU build): reader on every fixture (including the error
paths), writers, partition, rand() jump-ahead, the threaded partition draw and the bookkeeping."""
import os

from cli_util import DATA
import host_driver


def test_host_c_code_is_sanitizer_clean(tmp_path):
    exe = host_driver.build(tmp_path, "asan_host", ["tests/asan_host_driver.c"] + ["multiclust_amd/host/" + f for f in (
        "mc_reader.c", "mc_writer.c", "mc_fit.c", "mc_em.c", "mc_init.c", "mc_watchdog.c")], libs=("-lm", "-lpthread"))
    args = []
    for fn, p in (("multi.stru", 2), ("missing.stru", 2), ("tetra.stru", 4), ("multi_interleaved.stru", 2),
                  ("c1_tiny.stru", 2), ("multi.stru", 3), ("missing99.stru", 2)):
        args += [os.path.join(DATA, fn), str(p)]
    res = host_driver.run(exe, args, cwd=tmp_path)
    assert "ok 1" in res.stdout
    assert "of a partition with itself 1.000000" in res.stdout and "WATCHDOG [mc_watchdog.c]" in res.stdout
