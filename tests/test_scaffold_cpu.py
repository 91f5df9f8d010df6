"""The shared test helpers fail when they should (no GPU): a helper that swallowed a failure would weaken every test that uses it.
tests/host_driver.py on programs that exit with a status, overflow an int and leak; tests/cli_util.py on the program's usage exit,
on the files a run leaves, on the memo of runs and on the reader of the written fit."""
import re
import subprocess

import numpy as np
import pytest

import cli_util
import host_driver

EXITS_2 = "int main(void) {\n    return 2;\n}\n"
OVERFLOWS = "#include <limits.h>\n#include <stdio.h>\nint main(int argc, char **argv) {\n    (void)argv;\n    printf(\"%d\\n\", INT_MAX + argc);\n    return 0;\n}\n"
LEAKS = ("#include <stdlib.h>\n#include <string.h>\nint main(int argc, char **argv) {\n    (void)argv;\n    char *p = malloc(100 + argc);\n"
         "    memset(p, 1, 100);\n    p = 0;\n    return p != 0;\n}\n")


def program(tmp_path, name, text, **kw):
    (tmp_path / (name + ".c")).write_text(text)
    return host_driver.build(tmp_path, name, [str(tmp_path / (name + ".c"))], **kw)


def test_a_non_zero_exit_fails(tmp_path):
    exe = program(tmp_path, "exits", EXITS_2, sanitize=False)
    with pytest.raises(AssertionError, match=r"exits'?, \[\], 2,"):
        host_driver.run(exe)


def test_a_sanitizer_report_fails_and_the_plain_build_passes(tmp_path):
    with pytest.raises(AssertionError, match="runtime error: signed integer overflow"):
        host_driver.run(program(tmp_path, "overflows_san", OVERFLOWS))
    res = host_driver.run(program(tmp_path, "overflows", OVERFLOWS, sanitize=False), quiet_stderr=True)
    assert re.match(r"^-?\d+\n$", res.stdout)


def test_a_leak_fails(tmp_path):
    with pytest.raises(AssertionError, match="LeakSanitizer: detected memory leaks"):
        host_driver.run(program(tmp_path, "leaks_san", LEAKS))
    host_driver.run(program(tmp_path, "leaks", LEAKS, sanitize=False), quiet_stderr=True)


def test_quiet_stderr_fails_on_any_text(tmp_path):
    exe = program(tmp_path, "talks", "#include <stdio.h>\nint main(void) {\n    fputs(\"note\\n\", stderr);\n    return 0;\n}\n", sanitize=False)
    assert host_driver.run(exe).stderr == "note\n"
    with pytest.raises(AssertionError, match="note"):
        host_driver.run(exe, quiet_stderr=True)


def test_run_cli_asserts_on_the_status(tmp_path):
    with pytest.raises(AssertionError, match="expected 0"):
        cli_util.run_cli(["-h"], tmp_path, expect=0)
    lines, files, res = cli_util.run_cli(["-h"], tmp_path, expect=1)        # the usage exit
    assert res.returncode == 1 and files == {} and any("--bed" in ln for ln in lines) and lines == cli_util.normalise(res.stdout)
    cli_util.option_is_there("--bed")
    with pytest.raises(AssertionError, match="--no-such-option"):
        cli_util.option_is_there("--no-such-option")


def test_run_cli_returns_exactly_the_files_that_appeared(tmp_path, monkeypatch):
    (tmp_path / "before.txt").write_text("already here\n")

    def writes_two(cmd, cwd, timeout):
        assert cmd == [cli_util.BIN, "-x", "1"] and timeout == 300
        for name in ("stem.b", "stem.a"):
            open(cwd + "/" + name, "w").write(name + "\n")
        open(cwd + "/before.txt", "a").write("more\n")
        return subprocess.CompletedProcess(cmd, 0, "took 01:02:03\nKinship: x\n", "")
    monkeypatch.setattr(cli_util.procutil, "run_program", writes_two)
    lines, files, res = cli_util.run_cli(["-x", "1"], tmp_path)
    assert lines == ["took HH:MM:SS", "Kinship: x", ""] and list(files) == ["stem.a", "stem.b"] and files["stem.a"] == b"stem.a\n"
    others, own, files = cli_util.run_cli(["-x", "1"], tmp_path, own="Kinship")
    assert others == ["took HH:MM:SS", ""] and own == ["Kinship: x"] and files == {}      # (the second run made nothing new)
    others, own, _ = cli_util.run_cli(["-x", "1"], tmp_path, own=re.compile(r"^Kinship: (\w)$"))
    assert others == ["took HH:MM:SS", ""] and [m.groups() for m in own] == [("x",)]


def test_runs_launches_once_per_distinct_command_line(tmp_path):
    launched = []

    def launch(args, d, own=None):
        launched.append((args, str(d), own))
        return ["line %d" % len(launched)], [], {}
    dirs = iter(tmp_path / ("out%d" % n) for n in range(9))
    runs = cli_util.Runs(lambda: next(dirs), own="Own", launch=launch)
    first = runs(["-a", "-k", "3"])
    assert runs(["-a", "-k", "3"]) is first and runs(("-a", "-k", "3")) is first
    second = runs(["-a", "-k", "3", "--fst"])
    assert second is not first and runs(["-a", "-k", "3", "--fst"]) is second
    assert launched == [(["-a", "-k", "3"], str(tmp_path / "out0"), "Own"), (["-a", "-k", "3", "--fst"], str(tmp_path / "out1"), "Own")]
    assert cli_util.Runs(lambda: next(dirs), launch=launch)(["-a", "-k", "3"]) is not first       # the memo is the instance's


def fit_files(q_name, q_text, p_rows):
    return {"stem.admix.K=2.pklm.txt": ("k\tl\tm\tp\n" + "".join("%d\t%d\t%d\t%s\n" % r for r in p_rows)).encode(),
            "stem.admix.K=2." + q_name: q_text.encode(), "stem.admix.K=2.other.txt": b"unread\n"}


def test_written_fit_reads_both_forms_and_misses_no_cell():
    ua = np.array([2, 0, 3], dtype=np.int32)                      # columns 0-1 of locus 0, none of locus 1, 2-4 of locus 2
    cells = [(k, l, m, "0.%d%d%d000" % (k + 1, l, m)) for k in range(2) for l, M in enumerate(ua) for m in range(M)]
    want_P = np.array([[0.100, 0.101, 0.120, 0.121, 0.122], [0.200, 0.201, 0.220, 0.221, 0.222]])
    etaik = "i\tk\teta\n0\t0\t0.250000\n0\t1\t0.750000\n2\t0\t1.000000\n2\t1\t0.000000\n"
    q, P = cli_util.written_fit(fit_files("etaik.txt", etaik, cells), ua, 3, 2)
    assert np.array_equal(P, want_P) and q.shape == (3, 2)
    assert np.array_equal(q[[0, 2]], [[0.25, 0.75], [1.0, 0.0]]) and np.isnan(q[1]).all()      # an individual without a row stays NaN
    q, P = cli_util.written_fit(fit_files("etak.txt", "k\teta\n0\t0.400000\n1\t0.600000\n", cells), ua, 3, 2)
    assert np.array_equal(P, want_P) and np.array_equal(q, [0.4, 0.6])
    with pytest.raises(AssertionError, match="a cell of P is absent"):
        cli_util.written_fit(fit_files("etaik.txt", etaik, cells[:-1]), ua, 3, 2)
    with pytest.raises(AssertionError):
        cli_util.written_fit(fit_files("etak.txt", "k\teta\n0\t1.000000\n", cells), ua, 3, 2)      # one proportion for two clusters
