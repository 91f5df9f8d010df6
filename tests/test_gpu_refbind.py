"""-m gpu: INTEGRATION.md's binding EXECUTED.  oracle/_ref/multiclust_ref_hip is the reference's own program -- its main(),
option parser, STRUCTURE reader, maximize_likelihood() bookkeeping, stdout lines and output-file writers, compiled unmodified
from /root/reference in the build container -- linked WITHOUT its EM layer (em_alg.c, accel_em.c, log_likelihood.c, simplex.c,
rnd_init.c) and with oracle/glue/ref_bind.c + ref_glue.c in its place, i.e. on libmulticlust_host.so / libmulticlust_hip.so.
The five symbols the driver then lacks (initialize_model, em, converged, aic, bic) are the drop-in boundary on the reference's
side.  The binary travels with the tree (the sources do not); here it runs the command lines of the reference's own goldens
(tests/golden/cli_*: what the unmodified reference printed and wrote for the same arguments).

Left out: the goldens on data with missing values (the reference's reader leaves the phantom allele slot uninitialised and
the program aborts in free() depending on the length of its path strings, oracle/make_fixtures.py) and -P/-Q starting values:
the reference-side driver code that fails there is not ours to fix.  -b has no committed golden; the second test runs the bound
program beside the unmodified one (oracle/_ref/multiclust_ref, which travels too) on bootstrap command lines: the replicates
come from the reference's own parametric_bootstrap() in both, drawn from the one rand() stream that the bound program lends to
the device for its initialisations in between.  Skipped where the binaries are absent."""
import os

import pytest

from cli_util import CLOCK, ROOT
from procutil import run_program

import test_gpu_cli as cli

pytestmark = pytest.mark.gpu
BOUND = os.path.join(ROOT, "oracle", "_ref", "multiclust_ref_hip")


@pytest.mark.skipif(not os.access(BOUND, os.X_OK), reason="oracle/_ref/multiclust_ref_hip not built (needs /root/reference at build time)")
@pytest.mark.parametrize("case,atol", [
    ("multi_admix_k4", 2e-6),               # -n 3: three initialisations drawn in turn from the program's libc rand() stream
    ("multi_mix_k3", 2e-6),                 # mixture model: vik for the writers
    ("multi_admix_c_k3", 2e-6),             # -c
    ("tetra_admix_k3", 2e-6),
    ("multi_admix_k4_i1000", 2e-6),
    ("multi_admix_k4_i1000_T5", 2e-6),
    ("multi_admix_k4_i1000_T5_s3", 2e-6),
])
def test_reference_program_on_the_hip_path_reproduces_its_own_goldens(case, atol, tmp_path, monkeypatch):
    monkeypatch.setattr(cli, "BIN", BOUND)
    cli.test_cli_matches_reference_binary(case, atol, tmp_path)


REFBIN = os.path.join(ROOT, "oracle", "_ref", "multiclust_ref")


@pytest.mark.skipif(not (os.access(BOUND, os.X_OK) and os.access(REFBIN, os.X_OK)), reason="oracle/_ref binaries not built")
@pytest.mark.parametrize("args", [
    "-a -k 3 -n 2 -b 3 -r 9",                    # H0 and HA on the observed data, three replicates, two initialisations each
    "-a -k 4 -n 1 -b 2 -r 4 -s 3 -T 30",
    "-k 3 -n 2 -b 2 -r 4",                       # mixture model
    "-p 4 -a -k 3 -n 1 -b 2 -r 11 tetra",
])
def test_bound_program_beside_the_unmodified_one_on_bootstrap_runs(args, tmp_path):
    import subprocess
    args = args.split()
    stru = os.path.join(cli.GOLD, "data", "tetra.stru" if args[-1] == "tetra" else "multi.stru")
    args = [a for a in args if a != "tetra"]
    lines = {}
    for name, exe in (("ref", REFBIN), ("bound", BOUND)):
        d = tmp_path / name
        d.mkdir()
        res = run_program([exe, "-f", stru, "-d", os.path.join(str(d), "")] + args, cwd=str(d), timeout=600)
        assert res.returncode == 0, (name, res.stderr[-2000:])
        lines[name] = CLOCK.sub("HH:MM:SS", res.stdout).strip().split("\n")
    assert len(lines["ref"]) == len(lines["bound"])
    exact = "-s" not in args
    for r, g in zip(lines["ref"], lines["bound"]):
        assert cli.NUM.sub("#", r) == cli.NUM.sub("#", g), (r, g)
        toks = cli.NUM.findall(r)
        for tok, x, y in zip(toks, [float(t) for t in toks], [float(t) for t in cli.NUM.findall(g)]):
            if "." not in tok and "e" not in tok and abs(x) < 1e6:
                if exact:
                    assert x == y, (r, g)                     # iteration counts, initialisations, K
            else:
                assert abs(x - y) <= max(2e-5, 1e-6 * abs(x)) + (0 if exact else 5e-2), (r, g)
    assert any(l.startswith("p-value to reject H0") for l in lines["bound"])

