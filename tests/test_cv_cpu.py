"""--cv on the command line where no GPU is needed: what it cannot be combined with is a usage error (the status and the form of
the other bad arguments, the option named on stderr), and a plain -c still means shared mixing proportions."""
import os
import subprocess

import pytest

from cli_util import BIN, ROOT

MULTI = os.path.join(ROOT, "tests", "golden", "data", "multi.stru")
INVALID_CMD_ARGUMENT = 10

CASES = [
    (["-a", "--cv", "1"], "--cv"),
    (["-a", "--cv", "65"], "--cv"),
    (["--cv", "5"], "--cv"),                              # without -a
    (["-a", "--cv", "5", "-b", "3"], "--cv"),
    (["-a", "--cv", "5", "--gpus", "2"], "--cv"),
    (["-a", "--cv", "5", "-w", "n", "2"], "--cv"),
    (["-a", "--cv", "5", "-M"], "--cv"),
    (["-a", "--cv", "5", "--cv-floor", "0"], "--cv-floor"),
    (["-a", "--cv", "5", "--cv-floor", "1.5"], "--cv-floor"),
]


def run(args, cwd):
    return subprocess.run([BIN, "-f", MULTI, "-k", "2"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, cwd=cwd)


@pytest.mark.parametrize("args,option", CASES)
def test_usage_errors(args, option, tmp_path):
    res = run(args, str(tmp_path))
    assert res.returncode == INVALID_CMD_ARGUMENT, (args, res.returncode, res.stderr[-500:])
    assert "ERROR [mc_main.c::parse_options]" in res.stderr and option in res.stderr and "try -h" in res.stderr
    assert res.stdout == "" and not os.listdir(str(tmp_path))


def test_plain_c_still_means_shared_mixing_proportions(tmp_path):
    """-c beside -b is accepted by the parser (a --cv would not be): the run gets as far as the device, or through it"""
    res = run(["-a", "-c", "-b", "1", "-n", "1", "-T", "2"], str(tmp_path))
    assert res.returncode != INVALID_CMD_ARGUMENT and "parse_options" not in res.stderr, res.stderr[-500:]
    # and --c is the same option, not a prefix of --cv
    res = run(["--c", "--cv", "1", "-a"], str(tmp_path))
    assert res.returncode == INVALID_CMD_ARGUMENT and "--cv" in res.stderr


def test_usage_lists_the_option(tmp_path):
    res = subprocess.run([BIN, "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, cwd=str(tmp_path))
    assert res.returncode == 1 and "--cv <F>" in res.stdout and "--cv-floor" in res.stdout
