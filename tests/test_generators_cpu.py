"""CPU tests of the generators that consume the reference's rand() stream, on the inputs where they are most likely to go wrong.

  * the window helper (tests/rand_window.py) against libc's own rand() (stood on the window through setstate) and against the
    oracle's generator, at stream positions 0, 1 000 and 10^6;
  * the host bootstrap generator (mc_em.c: mc_bootstrap_genotypes) against the reference's unmodified parametric_bootstrap()
    run live through `oracle/_ref/ref_time --bootstrap`, byte for byte, on every parameter family of PARAMETER FAMILIES below
    (negative entries, zeros, NaN rows, a NaN inside a p row, rows that do not sum to 1, exact ties with the draw) and with
    draws 0, 1, RAND_MAX - 1 and RAND_MAX placed at the first, a middle and the last copy: per-individual and shared eta and
    the mixture model.  tests/test_gpu_generators.py ties the device to the host on the same families, so the chain reference
    = host = device holds on adversarial inputs, not only on the natural ones of the golden fixtures;
  * the device's integer form of the inverse-CDF walk (k_walk_tables: thresholds of the running maximum of the partial sums),
    restated, against the reference's walk on rows with negative entries, zeros and NaN;
  * mod_k_magic (mchip_generators.hip), restated: the multiply-shift remainder the partition kernels take is exact for every K <= 64."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cli_util import ROOT
import oracle_bind as ob
import rand_window as rw
from multiclust_amd import host
from synth import random_params
from test_bootstrap_cpu import counts_of, walk_threshold

REF_TIME = os.path.join(ROOT, "oracle", "_ref", "ref_time")
D = 2147483647.0
RAND_MAX = rw.RAND_MAX


# ------------------------------------------------------------------------------------------------------------ the window helper
def libc_rand_from_window(window, n):
    """n draws of libc's own rand() stood on `window` (initstate on a buffer of its own, then a TYPE_3 state with rear = 0:
    header 3, the oldest word at front = 3); the caller's libc state is put back afterwards"""
    libc = C.CDLL(None)
    libc.initstate.restype = libc.setstate.restype = C.c_void_p
    libc.initstate.argtypes = [C.c_uint, C.c_void_p, C.c_size_t]
    libc.setstate.argtypes = [C.c_void_p]
    dummy, state = (C.c_int32 * 32)(), (C.c_int32 * 32)()
    old = libc.initstate(1, dummy, 128)
    state[0] = 3
    for t in range(31):
        state[1 + (3 + t) % 31] = C.c_int32(int(window[t])).value
    libc.setstate(state)
    out = [libc.rand() for _ in range(n)]
    libc.setstate(old)
    return out


def host_rng(window):
    """mc_rng standing on the window (r[f] the oldest word, r[b] = x_{j-3})"""
    g = host.McRng()
    for t in range(31):
        g.r[t] = C.c_int32(int(window[t])).value
    g.f, g.b = 0, 28
    return g


def window_words_at(seed, pos):
    """the 32-bit words x_pos .. x_{pos+30} of srand(seed)'s stream (mc_rng_jump: no loop over pos draws)"""
    lib = host.load()
    g = host.McRng()
    lib.mc_srand(C.byref(g), seed)
    lib.mc_rng_jump(C.byref(g), pos)
    x = [int(g.r[(g.f + t) % 31]) & 0xFFFFFFFF for t in range(31)]
    for t in range(31):
        x.append((x[t] + x[t + 28]) & 0xFFFFFFFF)
    return x[31:]


@pytest.mark.parametrize("pos", [0, 1000, 10 ** 6])
def test_window_helper_reproduces_the_seeded_stream(pos):
    """The 31 words at draw `pos` of srand(seed)'s stream, stepped back by the helper, give srand(seed)'s own window: the
    helper's stream is glibc_rand(seed, n), checked against the oracle and against libc's rand()."""
    seed = 20250117 + pos
    words = window_words_at(seed, pos)
    w = rw.window_placing([x >> 1 for x in words], pos, low_bits=[x & 1 for x in words])
    want, _ = ob.glibc_window(seed)
    assert np.array_equal(w, want)
    n = 3000
    seq = ob.glibc_rand(seed, n)
    assert rw.draws(w, n).tolist() == seq
    assert libc_rand_from_window(w, n) == seq


@pytest.mark.parametrize("pos", [0, 1, 1000, 10 ** 6])
def test_window_helper_places_chosen_draws(pos):
    """Draws 0, 1, RAND_MAX - 1 and RAND_MAX (and 27 more) come out of libc's rand(), the oracle's and the host's generators at
    exactly the chosen position."""
    chosen = [0, 1, RAND_MAX - 1, RAND_MAX] + [int(v) for v in np.random.default_rng(pos).integers(0, RAND_MAX + 1, 27)]
    for low in (0, 1):
        w = rw.window_placing(chosen, pos, low_bits=low)
        lib = host.load()
        g = host_rng(w)
        lib.mc_rng_jump(C.byref(g), pos)
        assert [lib.mc_rand(C.byref(g)) for _ in range(31)] == chosen
        if pos <= 1000:
            assert rw.draws(w, pos + 31)[pos:].tolist() == chosen
            assert libc_rand_from_window(w, pos + 31)[pos:] == chosen
            rng = ob.Rng()
            rng.r[:] = host_rng(w).r[:]
            rng.f, rng.b = 0, 28
            assert [ob.lib.mco_rand(C.byref(rng)) for _ in range(pos + 31)][pos:] == chosen


# -------------------------------------------------------------------------------------------------------- PARAMETER FAMILIES
FAMILIES = ("natural", "zeros", "negative", "unnormalised", "nan_q", "nan_p", "tie", "tie-ulp", "tie+ulp")
EDGE_DRAWS = (0, 1, RAND_MAX - 1, RAND_MAX)
# tie families: the draws the placed copies receive (cluster draws alternate TIE_Q, allele draws TIE_P) equal a partial sum of
# the row exactly (v / RAND_MAX == c_t, "tie"), or the partial sum is one ulp below / above it
TIE_Q = (0x2468ACE1, 0x5A5A5A5A)
TIE_P = (0x3C3C3C3C, 0x6ED6ED6E)


def _addend(a, target):
    """b with float64(a + b) == target"""
    b = target - a
    for _ in range(8):
        s = a + b
        if s == target:
            return b
        b = np.nextafter(b, np.inf if s < target else -np.inf)
    raise AssertionError("no addend")


def _tie_row(n, draws, shift):
    """a row of n entries whose partial sums c_1, c_2 are draws[0] / RAND_MAX, draws[1] / RAND_MAX (shifted by an ulp)"""
    cs = [np.float64(v) / D for v in draws]
    if shift:
        cs = [np.nextafter(c, np.inf * shift) for c in cs]
    row = np.empty(n)
    row[0] = cs[0] if n > 1 else 1.0
    if n > 2:
        row[1] = _addend(cs[0], cs[1])
        row[2:] = (1.0 - cs[1]) / (n - 2)
    elif n == 2:
        row[1] = 1.0 - cs[0]
    return row


def family_params(family, I, ua, K, shared, seed):
    """(q, p) of one family: q [I][K] or [K] (shared eta / mixture), p [K][T]"""
    rs = np.random.default_rng(seed)
    lb = 1e-8
    q, p = random_params(I, ua, K, seed=seed, lower_bound=lb)
    q[::3, 0] = lb                                      # entries at the lower bound, as fitted models have
    q /= q.sum(axis=1, keepdims=True)
    p[:, ::5] = lb
    toff = np.concatenate([[0], np.cumsum(ua)])
    prow = [(k, int(toff[l]), int(ua[l])) for k in range(K) for l in range(len(ua))]
    if family == "zeros":
        for i in range(I):
            q[i, [0, K - 1, int(rs.integers(0, K))][i % 3]] = 0.0
            if i % 4 == 0:
                q[i, :K // 2] = 0.0
        for x, (k, c0, M) in enumerate(prow):
            p[k, c0 + [0, M - 1, int(rs.integers(0, M))][x % 3]] = 0.0
    elif family == "negative":
        def neg(row, x):
            n = len(row)
            if n < 2:
                return
            at = [0, n // 2, n - 1][x % 3]           # first, middle, last: a first entry below 0 takes the partial sums below 0
            v = -rs.uniform(0.01, 0.4)
            rest = [j for j in range(n) if j != at]
            row[rest] *= (1.0 - v) / row[rest].sum()
            row[at] = v
        for i in range(I):
            neg(q[i], i)
        for x, (k, c0, M) in enumerate(prow):
            neg(p[k, c0:c0 + M], x)
    elif family == "unnormalised":
        scale = np.array([0.9, 1.1, 0.5, 1.5])
        q *= scale[np.arange(I) % 4][:, None]
        for x, (k, c0, M) in enumerate(prow):
            p[k, c0:c0 + M] *= scale[x % 4]
    elif family == "nan_q":
        q[::5] = np.nan                                 # get_q of an individual with no observed copy
        q[0] = np.nan
    elif family == "nan_p":
        for x, (k, c0, M) in enumerate(prow):
            if x % 3 == 0:
                p[k, c0 + [0, M - 1, M // 2][(x // 3) % 3]] = np.nan
    elif family.startswith("tie"):
        shift = {"tie": 0, "tie-ulp": -1, "tie+ulp": 1}[family]
        q[:] = _tie_row(K, TIE_Q, shift)
        for k, c0, M in prow:
            p[k, c0:c0 + M] = _tie_row(M, TIE_P, shift)
    else:
        assert family == "natural"
    if shared:
        q = np.ascontiguousarray(q[0])
    return np.ascontiguousarray(q), np.ascontiguousarray(p)


def placed_draws(family, pos):
    """the 31 draws placed at draw `pos`: copy j takes draws 2j (cluster) and 2j + 1 (allele) in the admixture model"""
    if family.startswith("tie"):
        return [(TIE_Q if j % 2 == 0 else TIE_P)[(j // 2) % 2] for j in range(pos, pos + 31)]
    return [EDGE_DRAWS[(j // 2 + j) % 4] for j in range(pos, pos + 31)]       # each of the four as cluster and as allele draw


def placement_windows(family, n_draws, positions, seed):
    """(name, window): the stream of srand(seed), and one stream per named draw position with placed_draws there"""
    out = [("seed", ob.glibc_window(seed)[0])]
    for name, pos in positions:
        pos = min(max(pos, 0), n_draws - 31)
        out.append((name, rw.window_placing(placed_draws(family, pos), pos, fill_seed=seed)))
    return out


# ------------------------------------------------------------------------------------------------------- generators, both sides
def host_bootstrap(I, L, ploidy, ua, K, q, p, window, admixture=1, constrained=0):
    """mc_bootstrap_genotypes from the window: (genotype bytes [I][L][ploidy], next rand(), next rand() after a jump by
    mc_bootstrap_draws)"""
    lib = host.load()
    opt = host.McOptions()
    lib.mc_make_options(C.byref(opt))
    opt.admixture, opt.eta_constrained = admixture, constrained
    ua32 = np.ascontiguousarray(ua, dtype=np.int32)
    geno = np.zeros((I, L, ploidy), dtype=np.uint8)
    dat = host.McData(I, L, ploidy, ua32.ctypes.data, geno.ctypes.data)
    rng = host_rng(window)
    sim = np.empty((I, L, ploidy), dtype=np.uint8)
    lib.mc_bootstrap_genotypes(C.byref(opt), C.byref(dat), K, q.ctypes.data, p.ctypes.data, C.byref(rng), sim.ctypes.data)
    jumped = host_rng(window)
    lib.mc_rng_jump(C.byref(jumped), lib.mc_bootstrap_draws(C.byref(opt), C.byref(dat)))
    return sim, lib.mc_rand(C.byref(rng)), lib.mc_rand(C.byref(jumped))


def reference_bootstrap(d, I, L, ploidy, ua, K, q, p, window, admixture=1, constrained=0):
    """the reference's parametric_bootstrap() through `ref_time --bootstrap`: (allele counts [I][T], next rand())"""
    os.makedirs(d, exist_ok=True)
    np.ascontiguousarray(ua, dtype=np.int32).tofile(d + "/ua.i32")
    np.zeros((I, L, ploidy), dtype=np.uint8).tofile(d + "/geno.u8")
    q.tofile(d + "/q_mle.f64")
    p.tofile(d + "/p_mle.f64")
    np.ascontiguousarray(window, dtype=np.uint32).tofile(d + "/window.u32")
    model = (["-a"] if admixture else []) + (["-c"] if constrained else [])
    res = subprocess.run([REF_TIME, "--bootstrap", d, str(I), str(L), str(ploidy), str(K), "-", "--", "-f", "x"] + model + ["-k", str(K)],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    return np.fromfile(d + "/bs_ilm.u8", dtype=np.uint8).reshape(I, -1), int(res.stdout)


def ref_time_bootstraps():
    """whether oracle/_ref/ref_time has its --bootstrap mode: a binary built from an older oracle/ref_time.c (an _ref/ that came
    with the tree where the reference's sources are not at hand to rebuild it) answers with the usage line without it"""
    if not os.access(REF_TIME, os.X_OK):
        return False
    res = subprocess.run([REF_TIME, "--bootstrap"], capture_output=True, text=True, timeout=60)
    return res.returncode == 2 and "[--bootstrap]" in res.stderr


REF_BOOTSTRAP = ref_time_bootstraps()
needs_ref = pytest.mark.skipif(not REF_BOOTSTRAP, reason="oracle/_ref/ref_time without its --bootstrap mode (rebuild: make -C oracle)")


@needs_ref
def test_reference_bootstrap_mode_reproduces_the_golden_data_set(tmp_path):
    """`ref_time --bootstrap` with a seed, and with the seed's window installed in libc's rand(): the golden fixture the harness
    wrote (tests/golden/*/bs_ilm.u8) and the same next draw"""
    from golden_util import Golden
    from test_bootstrap_cpu import golden_bootstrap
    g = Golden("multi_admix_k4")
    q, p = np.ascontiguousarray(g.q("bs")), np.ascontiguousarray(g.p("bs"))
    seed = g.m["bootstrap_seed"]
    window, _ = ob.glibc_window(seed)
    counts, nxt = reference_bootstrap(str(tmp_path), g.I, g.L, g.ploidy, g.ua, g.K, q, p, window)
    assert np.array_equal(counts, golden_bootstrap(g)) and nxt == g.m["rand_after_bootstrap"]
    d = str(tmp_path)
    res = subprocess.run([REF_TIME, "--bootstrap", d, str(g.I), str(g.L), str(g.ploidy), str(g.K), str(seed), "--", "-f", "x", "-a",
                          "-k", str(g.K)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and int(res.stdout) == g.m["rand_after_bootstrap"]
    assert np.array_equal(np.fromfile(d + "/bs_ilm.u8", dtype=np.uint8).reshape(g.I, -1), golden_bootstrap(g))


@needs_ref
@pytest.mark.parametrize("model", ["individual", "shared", "mixture"])
@pytest.mark.parametrize("family", FAMILIES)
def test_host_bootstrap_equals_reference_on_every_family(tmp_path, family, model):
    I, L, ploidy, K = 37, 23, 3, 5
    ua = np.array([2, 3, 4, 5, 7] * 4 + [2, 3, 2], dtype=np.int32)
    admixture, constrained = int(model != "mixture"), int(model == "shared")
    q, p = family_params(family, I, ua, K, shared=model != "individual", seed=len(family) + 3 * admixture + constrained)
    n = I * L * ploidy
    n_draws = 2 * n if admixture else I + n
    positions = [("first copy", 0), ("middle", n_draws // 2 - 16), ("last copy", n_draws - 31)]
    for name, window in placement_windows(family, n_draws, positions, seed=77 + I):
        sim, nxt, nxt_jump = host_bootstrap(I, L, ploidy, ua, K, q, p, window, admixture, constrained)
        ref, ref_next = reference_bootstrap(str(tmp_path / name.replace(" ", "_")), I, L, ploidy, ua, K, q, p, window, admixture,
                                            constrained)
        assert np.array_equal(counts_of(sim, ua), ref), (family, model, name)
        assert nxt == ref_next == nxt_jump, (family, model, name)


# ------------------------------------------------------------------------------------------------- the walk, restated
def reference_walk(w, r):
    j, s = 0, 0.0
    while j < len(w) and r > s:
        s += w[j]
        j += 1
    return j - 1 if j else 0


def fixed_thresholds(w):
    """k_walk_tables: V of the running maximum of the left-to-right partial sums, 2^31 from the first NaN sum on"""
    out, s, peak, nan = [], 0.0, 0.0, False
    for x in w:
        nan = nan or s != s
        peak = max(peak, s) if s == s else peak
        out.append(1 << 31 if nan else walk_threshold(peak))
        s += x
    return out


def search(tab, v):
    """walk_search (mchip_generators.hip), restated"""
    lo, n = 0, len(tab)
    while n > 1:
        half = n >> 1
        if v >= tab[lo + half]:
            lo += half
        n -= half
    return lo


def test_running_maximum_thresholds_decide_what_the_walk_decides():
    """Both integer forms the device takes (the count of thresholds reached, the binary search) on the fixed thresholds equal
    the reference's walk for rows with negative entries, zeros and NaN, at random draws and both sides of every threshold."""
    rs = np.random.default_rng(31)
    for trial in range(600):
        n = int(rs.integers(1, 10))
        w = rs.dirichlet(np.full(n, 0.5))
        kind = trial % 4
        if kind == 0:
            w[rs.integers(0, n)] = -rs.uniform(0, 0.5)
        elif kind == 1:
            w[rs.random(n) < 0.4] = 0.0
            w[rs.integers(0, n)] = -rs.uniform(0, 0.3)
        elif kind == 2:
            w[rs.integers(0, n)] = np.nan
            if n > 2:
                w[rs.integers(0, n)] = -0.1
        else:
            w *= rs.choice([0.7, 1.3])
        thr = fixed_thresholds(w)
        assert all(a <= b for a, b in zip(thr, thr[1:]))
        probes = {0, 1, RAND_MAX - 1, RAND_MAX} | {int(v) for v in rs.integers(0, 1 << 31, 30)}
        for t in thr:
            probes.update(v for v in (t - 1, t, t + 1) if 0 <= v <= RAND_MAX)
        for v in probes:
            want = reference_walk(w, np.float64(v) / D)
            assert sum(v >= t for t in thr[1:]) == want, (w, v)
            assert search(thr, v) == want, (w, v)


def test_issue_rows_walk_as_the_reference_does():
    """the two rows the plain partial-sum thresholds got wrong (count form and binary search)"""
    for w, r, want in (([0.3, 0.3, -0.2, 0.6], 0.45, 1), ([0.29, -0.17, 0.62, 0.17], 0.131, 0)):
        v = next(v for v in range(int(r * D) - 2, int(r * D) + 3) if np.float64(v) / D >= r)
        assert reference_walk(w, np.float64(v) / D) == want
        thr = fixed_thresholds(w)
        assert sum(v >= t for t in thr[1:]) == want and search(thr, v) == want


# ------------------------------------------------------------------------------------------------- mod_k_magic, restated
def mod_k_magic(K):
    l = (K - 1).bit_length()                            # ceil(log2 K)
    magic = -(-(1 << (31 + l)) // K)
    return magic, l - 1


@pytest.mark.parametrize("K", range(2, 65))
def test_mod_k_magic_is_exact(K):
    magic, shift = mod_k_magic(K)
    l = shift + 1
    assert magic < 1 << 32
    assert (magic * K - (1 << (31 + l))) * RAND_MAX < 1 << (31 + l)        # the division bound: exact for every v < 2^31
    m = RAND_MAX // K
    for v in {0, K - 1, K, m * K - 1, m * K, RAND_MAX - 1, RAND_MAX}:
        assert v - (((v * magic) >> 32) >> shift) * K == v % K, (K, v)      # __umulhi(v, magic) >> shift


@pytest.mark.parametrize("family,expect", [("tie", (0, 1)), ("tie-ulp", (1, 2)), ("tie+ulp", (0, 1))])
def test_tie_rows_sit_on_the_placed_draws(family, expect):
    """the tie families do what their names say: the placed draws v give r = v / RAND_MAX equal to a partial sum of the row
    (the walk stops there), or one ulp above it (it passes)"""
    ua = np.array([2, 3, 4], dtype=np.int32)
    q, p = family_params(family, 3, ua, 4, shared=True, seed=1)
    assert tuple(reference_walk(q, np.float64(v) / D) for v in TIE_Q) == expect
    assert tuple(reference_walk(p[0, 2:5], np.float64(v) / D) for v in TIE_P) == expect
    assert placed_draws(family, 0)[:4] == [TIE_Q[0], TIE_P[0], TIE_Q[1], TIE_P[1]]
