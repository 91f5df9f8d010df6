"""The Python dispatch rule of tests/test_gpu_kernel_matrix.py against the library's own kernel selection, without a GPU.

mchip_describe_plan runs the library's launch geometry (model_geometry, mchip_plan.hip) and the plan of the K's translation unit
(plan(), mchip_kernels_k.hip) for a query and prints the kernel instances and the geometry facts.  For every case of the GPU
matrix and every configuration of its coverage grid, at every K:

  * the kernel names the library gives are the kernel names of `reach`;
  * the pseudo-cells of `reach` (slab counts above eight, XCD rows, byte flags, shared eta) agree with the library's facts;
  * `geometry` agrees with the library's facts.

So an edit to plan(), to the geometry or to the Python rule that leaves the other behind fails here, and the coverage proof of
test_the_case_list_covers_every_reachable_cell is a proof about what the library launches."""
import pytest

from multiclust_amd import hip
from test_gpu_kernel_matrix import (CASES, DUAL, KNOBS, MAX_K, N_CU, PSEUDO, case_dict, case_ua, count_bits, geometry, grid_configs,
                                    plan_query, reach)

UNSUPPORTED = 6             # MCHIP_ERR_UNSUPPORTED
# key of geometry() -> key of the library
GEOMETRY = {"n_ichunks": "n_ichunks", "lchunk": "lchunk", "n_lchunks": "n_lchunks", "sparse": "sparse", "waves": "ind_waves",
            "xcd_rows": "xcd_rows"}


class Knobs:
    """the case's own knobs in the environment, and no other; touched only when they change"""

    def __init__(self, monkeypatch):
        self.mp, self.now = monkeypatch, None

    def use(self, knobs):
        if knobs == self.now:
            return
        for k in KNOBS:
            self.mp.delenv(k, raising=False)
        for k, v in knobs.items():
            self.mp.setenv(k, v)
        self.now = dict(knobs)


def check(c):
    want = reach(c)
    rc, kernels, facts = hip.describe_plan(**plan_query(c))
    if not want:                                  # a batched cycle on the dense pair: unsupported in the library as in the rule
        assert rc == UNSUPPORTED, (rc, c)
        return
    assert rc == 0, (rc, c)
    assert kernels == want - set(PSEUDO), (sorted(kernels ^ (want - set(PSEUDO))), c)
    for cell, says in PSEUDO.items():
        assert (cell in want) == bool(says(facts)), (cell, facts, c)
    ua = c["ua"]
    g = geometry(c["K"], c["I"], c["L"], int(ua.sum()), c["ploidy"], int(ua.max()), c["model"] != "mix",
                 count_bits(c["ploidy"], c["knobs"]), c["knobs"])
    assert {lib: int(g[py]) for py, lib in GEOMETRY.items()} == {lib: facts[lib] for lib in GEOMETRY.values()}, (g, facts, c)
    assert bool(facts["pair"]) == any(x.startswith("k_estep_pair<") for x in kernels), (facts, kernels)
    if c.get("accel"):
        assert bool(facts["dual"]) == any(x.endswith(",true>") and x.startswith("k_individual_sparse_w<") for x in kernels)


@pytest.mark.parametrize("K", range(1, MAX_K + 1))
def test_the_dispatch_rule_is_the_librarys(monkeypatch, K):
    knobs = Knobs(monkeypatch)
    n = 0
    for c in CASES + DUAL:
        if c["K"] == K:
            knobs.use(c["knobs"])
            check(case_dict(c, case_ua(c)[0]))
            n += 1
    for c in grid_configs(K):
        knobs.use(c["knobs"])
        check(c)
        n += 1
    assert n > 2000


def test_describe_plan_is_bound_and_rejects_bad_queries():
    assert "mchip_describe_plan" in hip.ABI_SYMBOLS
    good = dict(K=3, I=65, L=45, T=100, ploidy=2, min_alleles=2, max_alleles=3, has_missing=0, admixture=1, eta_constrained=0,
                do_projection=1, p_lb=1e-8, n_cu=N_CU, accel_cycle=0)
    assert hip.describe_plan(**good)[0] == 0
    assert hip.describe_plan(**dict(good, K=0))[0] == 1
    assert hip.describe_plan(**dict(good, n_cu=0))[0] == 1
    assert hip.describe_plan(**dict(good, K=MAX_K + 1))[0] == UNSUPPORTED
