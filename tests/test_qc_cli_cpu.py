"""The command line of --mind, --geno, --maf and --hwe where it needs no GPU: parse_options runs before any file or device is opened,
so what it refuses, and that the four options are matched in full and leave -m, -g, -h and --missing their meaning, shows here.  (An
emptied data set ends the run behind the device: tests/test_gpu_qc_cli.py, and tests/test_qc_cpu.py through the driver.)"""
import subprocess

import pytest

from cli_util import BIN

RANGE = {"--mind": "the missing rate of --mind must lie in [0, 1)", "--geno": "the missing rate of --geno must lie in [0, 1)",
         "--maf": "the minor-allele frequency of --maf must lie in (0, 0.5]", "--hwe": "the p value of --hwe must lie in (0, 1)"}
BAD = {"--mind": ["-0.1", "1", "nan"], "--geno": ["-0.1", "1", "2", "nan"], "--maf": ["0", "-0.01", "0.51", "nan"], "--hwe": ["0", "1", "-1e-6", "nan"]}
GOOD = {"--mind": ["0", "0.1", "0.999"], "--geno": ["0", "0.05"], "--maf": ["0.01", "0.5"], "--hwe": ["1e-6", "0.999"]}


def program(args, cwd):
    return subprocess.run([BIN, "-a", "-k", "2"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, cwd=str(cwd))


@pytest.mark.parametrize("option", sorted(RANGE))
def test_refused_setups(option, tmp_path):
    res = program(["-f", "x.stru", option, GOOD[option][0]], tmp_path)
    assert res.returncode == 10, (res.returncode, res.stderr[-500:])       # MC_EXIT_INVALID_CMD_ARGUMENT: the usual refuse()
    assert "ERROR [mc_main.c::parse_options]: %s needs a PLINK fileset (--bed) (argument '%s')" % (option, option) in res.stderr and res.stdout == ""
    for t in BAD[option]:
        res = program(["--bed", "x", option, t], tmp_path)
        assert res.returncode == 10, (option, t, res.returncode, res.stderr[-500:])
        assert "ERROR [mc_main.c::parse_options]: %s (argument '%s')" % (RANGE[option], option) in res.stderr and res.stdout == ""
    res = program(["--bed", "x", option], tmp_path)                          # no threshold
    assert res.returncode == 10 and res.stdout == ""


@pytest.mark.parametrize("option", sorted(RANGE))
def test_accepted_thresholds_reach_the_reader(option, tmp_path):
    for t in GOOD[option]:
        res = program(["--bed", "none", option, t], tmp_path)
        assert res.returncode == 5 and "parse_options" not in res.stderr, (option, t, res.stderr[-500:])       # the fileset does not exist


def test_the_options_are_matched_in_full_and_the_short_ones_keep_their_meaning(tmp_path):
    res = program(["--bed", "none", "--mi", "-7", "-m", "3", "-g", "2", "--missing", "-5"], tmp_path)
    assert res.returncode == 5 and "parse_options" not in res.stderr              # --missing, the candidates, the back-tracking
    res = program(["--bed", "none", "--ma", "x"], tmp_path)
    assert res.returncode == 10 and "-m" in res.stderr and "--maf" not in res.stderr        # -m wants a number of candidates
    res = program(["--bed", "none", "--gen", "x"], tmp_path)
    assert res.returncode == 10 and "-g" in res.stderr and "--geno" not in res.stderr
    res = program(["--hw", "0.1"], tmp_path)
    assert res.returncode == 1 and res.stdout.startswith("Usage:")                 # anything else that begins with h is the help
    for o in RANGE:
        assert o + " <t>" in res.stdout
