"""No GPU: what the command line refuses of --pca, --pca-iter and --pca-tol before anything is read (multiclust_amd/host/mc_cli_options.c),
and what the usage text says about the option."""

from cli_util import BIN
from procutil import run_program

INVALID_CMD_ARGUMENT = 10


def refused(args, why):
    res = run_program([BIN] + args, timeout=60)
    assert res.returncode == INVALID_CMD_ARGUMENT and why in res.stderr and res.stdout == "", (args, res.returncode, res.stderr)


def test_usage_names_the_option_its_matrix_and_what_it_is_not():
    res = run_program([BIN, "-h"], timeout=60)
    text = " ".join(res.stdout.split())
    assert res.returncode == 1
    for words in ("--pca <n>", "--pca-iter <m>", "--pca-tol <t>", "flashpca", "--pca approx", "NOT PLINK 1.9's pairwise-complete GRM",
                  "not smartpca's normalisation", "noise bulk of the spectrum converge slowly and mean nothing", "<stem>.eigenvec"):
        assert words in text, words


def test_refusals():
    refused(["-f", "data.stru", "-a", "-k", "2", "--pca", "3"], "--pca needs a PLINK fileset (--bed)")
    for n in ("0", "49", "-1"):
        refused(["--bed", "data", "-a", "-k", "2", "--pca", n], "the number of components of --pca must lie in 1 ... 48")
    for t in ("0", "1", "-0.5", "2"):
        refused(["--bed", "data", "-a", "-k", "2", "--pca", "3", "--pca-tol", t], "the tolerance of --pca-tol must lie in (0, 1)")
    for args in (["--pca"], ["--pca", "three"], ["--pca", "3", "--pca-iter", "0"], ["--pca", "3", "--pca-iter"], ["--pca", "3", "--pca-tol"]):
        res = run_program([BIN, "--bed", "data", "-a", "-k", "2"] + args, timeout=60)
        assert res.returncode == INVALID_CMD_ARGUMENT and res.stdout == "", args
