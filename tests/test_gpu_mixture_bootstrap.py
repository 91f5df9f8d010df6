"""-m gpu: bootstrap replicates of the mixture model that never exist on the host.

  * mc_fit_replicate for the mixture model (it answered MCHIP_ERR_UNSUPPORTED = 6): replicate b generated on the device at its
    place in the rand() stream (mc_replicate_starts), initialised on the device, fitted -- against the serial route in the same
    process: host generator -> upload -> MC_HOST_INIT initialisation -> mc_em, consuming one stream from replicate 0 on.  Same
    data bytes, same initial bits, same kernels: logL_H0, logL_HA, ts and n_iter are compared with ==.
  * the command line without -a: `-b` prints the same text with replicates generated and initialised on the device, drawn and
    initialised on the host (MC_HOST_BOOTSTRAP + MC_HOST_INIT), and handed to workers as whole replicates (MC_FORCE_SHARDED,
    one device), where the run's only exchange is the replicates' table; and, where the reference program is built, the lines
    agree with it."""
import ctypes as C
import os

import numpy as np
import pytest

from cli_util import BIN, CLOCK
import test_gpu_cli as cli
from multiclust_amd import host
from procutil import run_program
from synth import make_dataset, random_params
from test_generators_cpu import needs_ref
from test_gpu_cli_differential import REFBIN, compare_bookkeeping_lines, run_both

pytestmark = pytest.mark.gpu
MP = C.POINTER(host.McModel)


def serial_replicates(lib, opt, ua, geno, base, n_rep, K0, K1, n_init, eta, p, monkeypatch):
    """what the serial program does from `base` on: [(logL_H0, logL_HA, ts, n_iter)] per replicate"""
    I, L, ploidy = geno.shape
    obs = host.McData(I, L, ploidy, ua.ctypes.data, geno.ctypes.data)
    rng = host.McRng.from_buffer_copy(base)
    out = []
    for b in range(n_rep):
        sim = np.empty_like(geno)
        lib.mc_bootstrap_genotypes(C.byref(opt), C.byref(obs), K0, eta.ctypes.data, p.ctypes.data, C.byref(rng), sim.ctypes.data)
        dat = host.McData(I, L, ploidy, ua.ctypes.data, sim.ctypes.data, geno.ctypes.data)
        best, n_iter = [], 0
        for K in (K0, K1):
            mp = MP()
            assert lib.mc_model_create(C.byref(mp), C.byref(opt), C.byref(dat), K, 0) == 0
            top = -np.inf
            for _ in range(1 if K == 1 else n_init):
                keep = mp.contents.delta_index
                lib.mc_reset_model_state(mp)
                mp.contents.delta_index = keep
                monkeypatch.setenv("MC_HOST_INIT", "1")
                assert lib.mc_initialize_model(C.byref(opt), C.byref(dat), mp, C.byref(rng)) == 0
                monkeypatch.delenv("MC_HOST_INIT")
                lib.mc_em(C.byref(opt), C.byref(dat), mp)
                assert mp.contents.fatal == 0
                n_iter += mp.contents.n_iter
                top = max(top, mp.contents.logL)
            lib.mc_model_free(mp)
            best.append(top)
        out.append((best[0], best[1], best[1] - best[0], n_iter))
    return out


@pytest.mark.parametrize("I,L,ploidy,maxal,K0,K1,n_init", [(120, 90, 2, 3, 2, 3, 2), (77, 60, 4, 4, 1, 2, 3), (64, 40, 9, 6, 3, 4, 1)],
                         ids=["K2-3", "K1-2", "K3-4-ploidy9"])
def test_fit_replicate_of_the_mixture_model_equals_the_serial_route(monkeypatch, I, L, ploidy, maxal, K0, K1, n_init):
    monkeypatch.delenv("MC_HOST_INIT", raising=False)
    lib = host.load()
    ua, geno = make_dataset(I, L, max(K1, 2), ploidy=ploidy, max_alleles=maxal, seed=I + L, missing=0.03)
    ua, geno = np.ascontiguousarray(ua, dtype=np.int32), np.ascontiguousarray(geno)
    opt = host.McOptions()
    lib.mc_make_options(C.byref(opt))
    opt.admixture, opt.verbosity, opt.max_iter = 0, 1, 40
    dat = host.McData(I, L, ploidy, ua.ctypes.data, geno.ctypes.data)
    assert lib.mc_synchronize(C.byref(opt), C.byref(dat)) == 0
    q, p = random_params(I, ua, K0, seed=5, lower_bound=opt.lower_bound)
    eta = np.ascontiguousarray(q[0] / q[0].sum())
    base = host.McRng()
    lib.mc_srand(C.byref(base), 4242)
    for _ in range(17):
        lib.mc_rand(C.byref(base))
    want = serial_replicates(lib, opt, ua, geno, base, 3, K0, K1, n_init, eta, p, monkeypatch)
    for b in (2, 0, 1):                 # any order: a replicate's place in the stream does not depend on the others' fits
        r = host.McReplicateResult()
        rc = lib.mc_fit_replicate(C.byref(opt), C.byref(dat), 0, C.byref(base), b, K0, K1, n_init, K0, eta.ctypes.data, p.ctypes.data,
                                  C.byref(r), None)
        assert rc == 0, rc
        assert r.fatal == 0 and r.replicate == b
        assert (r.logL_H0, r.logL_HA, r.ts, r.n_iter) == want[b], (b, (r.logL_H0, r.logL_HA, r.ts, r.n_iter), want[b])
    # kept models (what bench.py and the command line do): the same replicates again, buffers re-used
    models = (MP * 2)()
    for b in (0, 1, 2):
        r = host.McReplicateResult()
        assert lib.mc_fit_replicate(C.byref(opt), C.byref(dat), 0, C.byref(base), b, K0, K1, n_init, K0, eta.ctypes.data, p.ctypes.data,
                                    C.byref(r), models) == 0
        assert (r.logL_H0, r.logL_HA, r.ts, r.n_iter) == want[b], b
    for m in models:
        if m:
            lib.mc_model_free(m)
    # the host form of the initialisation cannot read a replicate that exists on the device only
    monkeypatch.setenv("MC_HOST_INIT", "1")
    r = host.McReplicateResult()
    assert lib.mc_fit_replicate(C.byref(opt), C.byref(dat), 0, C.byref(base), 0, K0, K1, n_init, K0, eta.ctypes.data, p.ctypes.data,
                                C.byref(r), None) == 6


ARGS = ["-k", "3", "-n", "2", "-b", "3", "-r", "9"]


def test_cli_mixture_bootstrap_device_host_and_sharded_agree(tmp_path, monkeypatch):
    stru = os.path.join(cli.GOLD, "data", "multi.stru")
    cmd = [BIN, "-f", stru] + ARGS + ["-d", str(tmp_path)]
    outs = []
    for mode in ("device", "host", "sharded"):
        for k in ("MC_HOST_BOOTSTRAP", "MC_HOST_INIT", "MC_FORCE_SHARDED", "MC_TRACE_EXCHANGE"):
            monkeypatch.delenv(k, raising=False)
        extra = []
        if mode == "host":
            monkeypatch.setenv("MC_HOST_BOOTSTRAP", "1")
            monkeypatch.setenv("MC_HOST_INIT", "1")
        if mode == "sharded":
            monkeypatch.setenv("MC_FORCE_SHARDED", "1")
            monkeypatch.setenv("MC_TRACE_EXCHANGE", "1")
            extra = ["--gpus", "1"]
        res = run_program(cmd + extra, timeout=600)
        assert res.returncode == 0, res.stderr
        if mode == "sharded":
            # the two fits of the observed data are not sharded for the mixture model: the replicates' table is the one exchange
            trace = [l for l in res.stderr.split("\n") if l.startswith("exchange: RCCL")]
            assert len(trace) == 1, res.stderr
            assert "bootstrap test statistics" in trace[0] and "6 doubles" in trace[0] and "all-reduce #1" in trace[0]
        assert res.stdout.count("Bootstrap dataset") == 3 and "p-value to reject H0: K=2" in res.stdout
        text = CLOCK.sub("HH:MM:SS", res.stdout)
        outs.append(text[text.index("Bootstrap dataset 1"):])
    assert outs[0] == outs[1], outs
    assert outs[0] == outs[2], outs


@needs_ref
def test_cli_mixture_bootstrap_lines_agree_with_the_reference_program(tmp_path, monkeypatch):
    assert os.access(REFBIN, os.X_OK), "oracle/_ref/ holds ref_time but not multiclust_ref: one recipe builds both"
    for k in ("MC_HOST_BOOTSTRAP", "MC_HOST_INIT", "MC_FORCE_SHARDED"):
        monkeypatch.delenv(k, raising=False)
    stru = os.path.join(cli.GOLD, "data", "multi.stru")
    (ref_lines, _), (got_lines, _) = run_both(tmp_path, ARGS + ["-d", "./"], stru)
    compare_bookkeeping_lines(ref_lines, got_lines, stru, False)
