"""The geometry of the lane-per-individual passes (k_cv_score, k_impute, k_resid_tile): the C++ rule
(multiclust_amd/csrc/mchip_feature_geometry.h), compiled alone into a program of its own under AddressSanitizer + UBSan, against
its Python restatement (tests/feature_geometry.py) that the GPU tests place their cases with."""

import pytest

import feature_geometry as fg
import host_driver

SHAPES = [(257, 9, 256), (1, 1, 0), (10000, 100000, 256), (63, 33001, 304)]      # (I, L, compute units; 0 = unknown)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = host_driver.build(tmp_path_factory.mktemp("geometry"), "feature_geometry_driver", ["tests/feature_geometry_driver.cpp"], cxx=True,
                            werror=True)

    def run(I, L, n_cu, red, smallest, budget):
        res = host_driver.run(exe, (I, L, n_cu, red, smallest, budget), quiet_stderr=True)
        rows = [tuple(int(x) for x in line.split()) for line in res.stdout.splitlines()]
        assert [r[:2] for r in rows] == [(K, M) for K in range(1, 65) for M in range(1, 256)]
        return {r[:2]: r[2:] for r in rows}
    return run


@pytest.mark.parametrize("name", ["CV", "IMPUTE", "RESID"])
def test_the_restatement_is_the_rule(name, driver):
    c = getattr(fg, name)
    first = None
    for n, (I, L, n_cu) in enumerate(SHAPES):
        got = driver(I, L, n_cu, c["red"], c["smallest"], c["budget"])
        for (K, max_M), (threads, stage, lds, n_itiles, lchunk, n_lchunks) in got.items():
            if n == 0:                                           # (lanes, staging and LDS do not depend on the shape)
                assert (threads, stage) == fg.geometry(K, max_M, **c), (name, K, max_M)
                assert lds == fg.lds_bytes(K, max_M, **c) and lds <= c["budget"], (name, K, max_M, lds)
            else:
                assert (threads, stage, lds) == first[(K, max_M)][:3]
            # the grid covers the data set: whole blocks of 8 loci per chunk, no chunk without a locus, a grid dimension
            assert n_itiles == -(-I // threads) and lchunk % 8 == 0 and lchunk >= 8
            assert (n_lchunks - 1) * lchunk < L <= n_lchunks * lchunk and n_lchunks <= 65535, (name, K, max_M, I, L)
        if n == 0:
            first = got


def test_every_edge_sits_where_the_gpu_tests_mean_it_to(driver):
    c = fg.IMPUTE
    got = driver(257, 9, 256, c["red"], c["smallest"], c["budget"])
    for (K, alleles), want in fg.EDGES.items():
        assert got[(K, alleles + 1)][:2] == want == fg.geometry(K, alleles + 1), (K, alleles)
    # cv's budget is 448 bytes larger: the same lanes and staging everywhere but at (46, 4), which still fits 128 lanes
    c = fg.CV
    got = driver(257, 9, 256, c["red"], c["smallest"], c["budget"])
    for (K, alleles), want in fg.EDGES.items():
        assert got[(K, alleles + 1)][:2] == ((128, 1) if (K, alleles) == (46, 4) else want), (K, alleles)
