"""--se on the command line where no GPU is needed: what it cannot be combined with is a usage error (the status and the form of
the --cv checks, the option named on stderr), a block longer than the data is refused once the data is read, -h lists both
options, and -s <n> beside --streams still parses."""
import os
import subprocess

import pytest

from cli_util import BIN, ROOT

MULTI = os.path.join(ROOT, "tests", "golden", "data", "multi.stru")
INVALID_CMD_ARGUMENT = 10
INVALID_USER_SETUP = 11

CASES = [
    (["-a", "--se", "1"], "--se"),
    (["-a", "--se", "10001"], "--se"),
    (["-a", "--se"], "--se"),
    (["-a", "--se", "5", "-b", "3"], "--se"),
    (["--se", "5", "-b", "3"], "--se"),                    # the mixture model is allowed; the bootstrap beside it is not
    (["-a", "--se", "5", "--gpus", "2"], "--se"),
    (["-a", "--se", "5", "-w", "n", "2"], "--se"),
    (["-a", "--se", "5", "-M"], "--se"),
    (["-a", "--se", "5", "--se-block", "0"], "--se-block"),
    (["-a", "--se", "5", "--se-block", "x"], "--se-block"),
]


def run(args, cwd):
    return subprocess.run([BIN, "-f", MULTI, "-k", "2"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, cwd=cwd)


@pytest.mark.parametrize("args,option", CASES)
def test_usage_errors(args, option, tmp_path):
    res = run(args, str(tmp_path))
    assert res.returncode == INVALID_CMD_ARGUMENT, (args, res.returncode, res.stderr[-500:])
    assert "ERROR [mc_main.c::parse_options]" in res.stderr and option in res.stderr and "try -h" in res.stderr
    assert res.stdout == "" and not os.listdir(str(tmp_path))


def test_block_longer_than_the_data(tmp_path):
    """known only once the file is read: the reference's status for a set-up the data does not allow, before any device is opened"""
    res = run(["-a", "--se", "5", "--se-block", "1000000"], str(tmp_path))
    assert res.returncode == INVALID_USER_SETUP, (res.returncode, res.stderr[-500:])
    assert "--se-block" in res.stderr and res.stdout == "" and not os.listdir(str(tmp_path))


def test_usage_lists_the_options(tmp_path):
    res = subprocess.run([BIN, "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, cwd=str(tmp_path))
    assert res.returncode == 1 and "--se <B>" in res.stdout and "--se-block <n>" in res.stdout and "--cv <F>" in res.stdout


def test_s_and_streams_still_parse(tmp_path):
    """-s 3 is the acceleration scheme and --streams its own option: with a bad --se behind them the parser gets that far and names
    --se; a bad -s or --streams is still named as itself; --simulate is still refused as itself"""
    res = run(["-a", "-s", "3", "--streams", "2", "--se", "1"], str(tmp_path))
    assert res.returncode == INVALID_CMD_ARGUMENT and "'1'" in res.stderr and "--se " in res.stderr and "--streams" not in res.stderr
    res = run(["-a", "-s", "7"], str(tmp_path))
    assert res.returncode == INVALID_CMD_ARGUMENT and "-s (argument '7')" in res.stderr
    res = run(["-a", "--streams", "17"], str(tmp_path))
    assert res.returncode == INVALID_CMD_ARGUMENT and "--streams (argument '17')" in res.stderr
    res = run(["-a", "--simulate"], str(tmp_path))
    assert res.returncode == INVALID_CMD_ARGUMENT and "--simulate is not supported" in res.stderr
    # accepted by the parser: the run gets as far as the device, or through it
    res = run(["-a", "-s", "3", "--streams", "2", "--se", "2", "-n", "1", "-T", "2"], str(tmp_path))
    assert res.returncode != INVALID_CMD_ARGUMENT and "parse_options" not in res.stderr, res.stderr[-500:]
