"""The geometry of a lane-per-individual pass (multiclust_amd/csrc/mchip_feature_geometry.h: lane_pass_geometry_of) restated:
a workgroup has 256, 128 or 64 lanes -- the most whose q rows (K | 1 doubles each) fit into the LDS budget beside the reduction
space and the staged P rows of a block of 8 loci (8 max_M (K | 1) doubles) -- and when not even the smallest workgroup leaves room
for the P rows, they are read from memory.  tests/test_feature_geometry_cpu.py holds this against the C++."""

CV = dict(red=2048, smallest=64, budget=64 * 1024 - 64)          # k_cv_score
IMPUTE = dict(red=2048, smallest=64, budget=64 * 1024 - 512)     # k_impute
RESID = dict(red=0, smallest=64, budget=64 * 1024 - 512)         # k_resid_tile (RES_TILE lanes at least)

# either side of every edge of impute's geometry (cv's, with 448 bytes more, differs at (46, 4) alone: 128 lanes): (K, alleles) ->
# (lanes, staged); max_M = alleles + 1.  With max_M = 3
# (two alleles and the phantom slot) K = 27 | 28 is the edge between 256 and 128 lanes and K = 51 | 52 the one between 128 and 64;
# with max_M = 5 they are K = 25 | 26 and 45 | 46; at K = 64 the rows are staged up to max_M = 7 and read from memory from 8 on.
EDGES = {(27, 2): (256, 1), (28, 2): (128, 1), (51, 2): (128, 1), (52, 2): (64, 1), (25, 4): (256, 1), (26, 4): (128, 1),
         (45, 4): (128, 1), (46, 4): (64, 1), (64, 6): (64, 1), (64, 7): (64, 0), (64, 35): (64, 0)}


def geometry(K, max_M, red=2048, smallest=64, budget=64 * 1024 - 512):
    """(lanes per workgroup, P rows staged); the defaults are impute's constants"""
    ks = K | 1
    tile = 8 * max_M * ks * 8
    sizes = [t for t in (256, 128, 64, 32, 16, 8, 4, 2, 1) if t >= smallest]
    for t in sizes:
        if t * ks * 8 + red + tile <= budget:
            return t, 1
    for t in sizes:
        if t * ks * 8 + red <= budget:
            return t, 0
    raise AssertionError


def lds_bytes(K, max_M, red=2048, smallest=64, budget=64 * 1024 - 512):
    t, staged = geometry(K, max_M, red, smallest, budget)
    return t * (K | 1) * 8 + red + (8 * max_M * (K | 1) * 8 if staged else 0)
