"""Host code as stand-alone programs: a driver with a main() of its own and the units under test, compiled plain or under
AddressSanitizer + UBSan, and run directly.  The one copy of the build line, of the environment and of the three assertions every
such test makes: status 0, no sanitizer report, and (where asked) nothing on stderr at all.  Nothing is preloaded into anything.

pytest does not rewrite the asserts of a helper module, so each carries its evidence in its message."""
import os
import shutil
import subprocess

import pytest

from cli_util import ROOT

HOST = os.path.join(ROOT, "multiclust_amd", "host")
CSRC = os.path.join(ROOT, "multiclust_amd", "csrc")
SANITIZED = ("-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer")
PLAIN = ("-O2",)
ENV = dict(ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")


def build(tmp, name, sources, sanitize=True, cxx=False, warnings=("-Wall", "-Wextra"), werror=False, include=None, libs=("-lm",)):
    """compile `sources` (paths below the repository's root) into tmp/name; a C program sees include/ and the host units' directory,
    a C++ program the device units' directory.  Skips where the compiler is absent; a failed compilation is an error."""
    compiler = "g++" if cxx else "gcc"
    if shutil.which(compiler) is None:
        pytest.skip("needs " + compiler)
    if include is None:
        include = (CSRC,) if cxx else (os.path.join(ROOT, "include"), HOST)
    exe = os.path.join(str(tmp), name)
    cmd = [compiler, "-std=c++17" if cxx else "-std=gnu11"] + list(warnings) + (["-Werror"] if werror else [])
    cmd += list(SANITIZED if sanitize else PLAIN) + ["-I" + d for d in include] + ["-o", exe]
    subprocess.run(cmd + [os.path.join(ROOT, s) for s in sources] + list(libs), check=True)
    return exe


def run(exe, args=(), cwd=None, stdin=None, timeout=120, quiet_stderr=False, text=True):
    """run the program once; AssertionError unless it ends with status 0 and without a sanitizer's report"""
    args = [str(a) for a in args]
    res = subprocess.run([exe] + args, cwd=None if cwd is None else str(cwd), input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=text, env=dict(os.environ, **ENV), timeout=timeout)
    err = res.stderr if text else res.stderr.decode(errors="replace")
    assert res.returncode == 0, (exe, args, res.returncode, err[-2000:])
    assert "AddressSanitizer" not in err and "runtime error" not in err, (exe, args, res.returncode, err[-2000:])
    if quiet_stderr:
        assert not err, (exe, args, res.returncode, err[-2000:])
    return res


def plain_and_sanitized(name, sources, result=None, timeout=120, text=True, **kw):
    """a module-scoped fixture `run(*args, cwd)` over the program built twice, ids "plain" and "sanitized"; what a call returns is
    result(res), by default the completed process itself"""
    @pytest.fixture(scope="module", params=[False, True], ids=["plain", "sanitized"])
    def driver(request, tmp_path_factory):
        exe = build(tmp_path_factory.mktemp(name + "_driver"), name + ("_san" if request.param else ""), sources, sanitize=request.param, **kw)

        def call(*args, cwd):
            res = run(exe, args, cwd=cwd, timeout=timeout, text=text)
            return res if result is None else result(res)
        return call
    return driver
