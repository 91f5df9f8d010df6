"""-m gpu: models with shared mixing proportions (the mixture model; admixture with eta_constrained) at the numbers of clusters
at which the K column sums of an M step (k_column_sums -> mchip_scalars::eta_sums) once shared their storage with the other small
device results: K = 8 and 9 (the first K whose sums reached the dot products' words), 56 and 57 (either side of the end of the
64 doubles the context used to hold them in) and 64 (MCHIP_MAX_K).  Whole fits, batched on the device and call by call, end on
the same bits; a fetch of one field of the record leaves the others as they were."""
import ctypes as C

import numpy as np
import pytest

from multiclust_amd import hip, host
from synth import make_dataset, random_params

pytestmark = pytest.mark.gpu

I, L, MAX_ITER = 70, 40, 12
KS = [8, 9, 56, 57, 64]
MODELS = {"mixture": dict(admixture=0, eta_constrained=0), "admixture_shared": dict(admixture=1, eta_constrained=1)}
# seeds of the data set and of the initial parameters per K: a call-by-call loop from them does not end fatal
SEEDS = {8: (11, 5), 9: (12, 5), 56: (13, 5), 57: (14, 5), 64: (15, 5)}


def start(K, model, scheme):
    ua, geno = make_dataset(I, L, K, ploidy=2, max_alleles=3, seed=SEEDS[K][0], missing=0.03)
    fit = host.Fit(ua, geno, K, accel_scheme=scheme, verbosity=1, max_iter=MAX_ITER, **MODELS[model])
    q0, p0 = random_params(I, ua, K, seed=SEEDS[K][1], lower_bound=fit.opt.lower_bound)
    fit.set_params(q0.mean(axis=0), p0)
    return fit


@pytest.mark.parametrize("scheme", [0, 3])
@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("K", KS)
def test_batched_fit_equals_call_by_call(K, model, scheme, monkeypatch):
    out = []
    for batched in (True, False):
        if batched:
            monkeypatch.delenv("MC_NO_BATCH", raising=False)
        else:
            monkeypatch.setenv("MC_NO_BATCH", "1")
        fit = start(K, model, scheme)
        fit.em()
        m = fit.mod
        out.append(((m.n_iter, m.converged, m.iter_stop, m.fatal, m.logL), fit.get_q(m.pindex), fit.get_p(m.pindex), fit.expected_counts()))
        fit.close()
    a, b = out
    print("K=%d %s scheme %d: batched %r, call by call %r" % (K, model, scheme, a[0], b[0]))
    assert b[0][3] == 0, "the call-by-call loop ended fatal: these seeds do not serve"
    assert a[0] == b[0], (a[0], b[0])
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("K", KS)
def test_fetching_one_scalar_leaves_the_dot_products_alone(K, model):
    """mchip_step_dots of the secant pair of two EM steps (each with its K column sums), then mchip_loglik -- another field, fetched
    through the same pinned buffer -- then mchip_step_dots again: the same three doubles."""
    fit = start(K, model, 3)
    lib, ctx = hip.load(), C.c_void_p(fit.mod.dev)
    ll = C.c_double()
    assert lib.mchip_em_step(ctx, 0, 1, C.byref(ll)) == 0 and lib.mchip_em_step(ctx, 1, 2, C.byref(ll)) == 0
    assert np.isfinite(ll.value)
    assert lib.mchip_secant(ctx, 0, 0, 1, 0) == 0 and lib.mchip_secant(ctx, 1, 0, 2, 1) == 0
    first, again = (C.c_double * 3)(), (C.c_double * 3)()
    assert lib.mchip_step_dots(ctx, 0, first) == 0
    assert lib.mchip_loglik(ctx, 2, C.byref(ll)) == 0 and np.isfinite(ll.value)
    assert lib.mchip_step_dots(ctx, 0, again) == 0
    assert np.all(np.isfinite(list(first))) and list(first) == list(again), (list(first), list(again))
    fit.close()
