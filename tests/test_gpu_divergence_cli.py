"""-m gpu: --fst on the command line.  Nothing but its own line and its two files depends on it -- STRUCTURE and PLINK input, the
three model forms, --streams 2, together with --cv and --fill --; the line and the files say what tests/divergence_util.py computes
from the Q and P files written beside them, to the digits those carry; with --query the weights leave the query individuals out;
K = 1 has no pairs; and on clustered data the two clusters that were drawn furthest apart have the largest F_ST.

Each run of the program is made once per module and shared by the tests that read it.

To the printed digits: etaik / etak and pklm carry six decimals, so every q and p read back is within eps = 5.1e-7 of the number the
program used.  With c = T / L1 columns per locus that moves a weight by eps at most, pbar by (K + 1) eps, H_a by c eps, D_ab by
2 c eps, HT_l by M_l (K + 1) eps and V_l by M_l K eps + 2 (K + 2) eps A_l (A_l = sum_m sum_k w_k |p - pbar|: divergence_util), and
a quotient n / d by (dn d + n dd) / d^2; second-order terms are covered by a factor 1.5.  The program's own figures carry ten
(files) or six (stdout) decimals."""
import re

import numpy as np
import pytest

import bedfiles as bf
from cli_util import clustered_codes, fit_inputs, Runs, written_fit
import divergence_util as du
from multiclust_amd import host

pytestmark = pytest.mark.gpu
NUM = r"(-?\d+\.\d+|nan|-nan)"
FST_LINE = re.compile(r"^Divergence \(K=(\d+)\): (?:pairwise Fst mean " + NUM + " min " + NUM + " max " + NUM +
                      r" over (\d+) pairs|(no pairs)); among clusters " + NUM + r" \[(\d+) loci\]$")
I, L, CLUSTERS = 72, 400, 3
ARGS = ["-s", "3", "-n", "2", "-r", "7", "-k", "3"]
EPS = 5.1e-7


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    inputs = fit_inputs(tmp_path_factory, "fst_in", clustered_codes(I, L, CLUSTERS))
    return dict(inputs, runs=Runs(lambda: tmp_path_factory.mktemp("fst_out"), own="Divergence"))


def run(inputs, args, bed=False):
    """one run of the program per distinct command line: (other stdout lines, the groups of the Divergence lines, files)"""
    others, own, files = inputs["runs"]((["--bed", inputs["bed"]] if bed else ["-f", inputs["stru"]]) + list(args))
    return others, [FST_LINE.match(ln) for ln in own], files


FORMS = {"admix": ["-a"], "shared": ["-a", "-c"], "mix": []}


@pytest.mark.parametrize("name,extra,bed", [
    ("admix", [], False), ("admix", [], True), ("shared", [], False), ("mix", [], False), ("admix", ["--streams", "2"], False),
    ("admix", ["--cv", "2", "--fill"], False), ("mix", ["--se", "2"], False)])
def test_nothing_else_changes(name, extra, bed, inputs):
    args = FORMS[name] + ARGS + extra
    lines0, fst0, files0 = run(inputs, args, bed)
    lines1, fst1, files1 = run(inputs, args + ["--fst"], bed)
    assert fst0 == [] and len(fst1) == 1 and fst1[0] is not None and lines0 == lines1
    mdl = "mix" if name == "mix" else "admix"
    own = ["stem.%s.K=3.fst.txt" % mdl, "stem.%s.K=3.fst.loci.txt" % mdl]
    assert sorted(files1) == sorted(list(files0) + own) and len(files0) >= 5
    for f in files0:
        assert files0[f] == files1[f], f
    if extra:                                                    # ... and --fst says what it says without the other analyses
        _, fst2, files2 = run(inputs, FORMS[name] + ARGS + ["--fst"], bed)
        assert fst2[0].groups() == fst1[0].groups() and all(files2[f] == files1[f] for f in own)


def own_files(files, mdl, K=3):
    """(weights [K], H [K], D [K][K], F [K][K], per locus: columns, HT, F) as --fst wrote them"""
    text = files["stem.%s.K=%d.fst.txt" % (mdl, K)].decode().split("\n")
    assert text[0] == "k\tweight\tH" and text[K + 1] == "" and text[K + 2] == "D" and text[2 * K + 3] == "" and text[2 * K + 4] == "Fst"
    head = np.array([[float(x) for x in ln.split("\t")] for ln in text[1:K + 1]])
    assert head[:, 0].tolist() == list(range(K))
    D = np.array([[float(x) for x in ln.split("\t")] for ln in text[K + 3:2 * K + 3]])
    F = np.array([[float(x) for x in ln.split("\t")] for ln in text[2 * K + 5:3 * K + 5]])
    assert D.shape == F.shape == (K, K) and text[3 * K + 5:] == [""]
    loci = files["stem.%s.K=%d.fst.loci.txt" % (mdl, K)].decode().split("\n")
    assert loci[0] == "l\tcolumns\tHT\tFst" and loci[-1] == ""
    rows = [ln.split("\t") for ln in loci[1:-1]]
    assert [int(r[0]) for r in rows] == list(range(len(rows)))
    return head[:, 1], head[:, 2], D, F, np.array([int(r[1]) for r in rows]), np.array([float(r[2]) for r in rows]), np.array([float(r[3]) for r in rows])


def quotient_tol(n, d, dn, dd):
    return 1.5 * (dn * np.abs(d) + np.abs(n) * dd) / (d * d)


def agree_with_the_written_fit(inputs, name, args, query_rows=()):
    mdl = "mix" if name == "mix" else "admix"
    ua = inputs["ua"]
    _, fst, files = run(inputs, args)
    K, T, L1 = 3, int(ua.sum()), int((ua > 0).sum())
    assert T > 2 * L1 and (ua == 0).sum() == 1                   # phantom columns and a locus without a column are in play
    q, P = written_fit(files, ua, I, 3, mdl)
    if q.ndim == 2:
        assert np.flatnonzero(np.isnan(q).any(axis=1)).tolist() == list(query_rows)
    w = du.weights_from_q(q, K)
    ref = du.reference(ua, P, w, exact_pbar=True)
    wf, H, D, F, cols, HT, Fl = own_files(files, mdl)
    c, p10, p6 = T / L1, 5.1e-11, 5.1e-7
    assert np.array_equal(cols, ua) and (np.abs(wf - w) <= EPS + p10).all() and abs(wf.sum() - 1) <= K * p10 + 1e-15
    dH, dD = c * EPS, 2 * c * EPS
    assert (np.abs(H - ref["H"]) <= 1.5 * dH + p10).all() and (np.abs(D - ref["D"]) <= 1.5 * dD + p10).all()
    den = ref["D"] + (ref["H"][:, None] + ref["H"][None, :]) / 2
    dF = quotient_tol(ref["D"], den, dD, dD + dH)
    assert (np.abs(F - ref["F"]) <= dF + p10).all() and np.array_equal(F, F.T) and not np.diag(F).any()
    # per locus
    M = ua.astype(np.float64)
    dHT, dV = M * (K + 1) * EPS, M * K * EPS + 2 * (K + 2) * EPS * ref["locus_abs"]
    assert (np.abs(HT - ref["locus_ht"]) <= 1.5 * dHT + p10).all()
    assert np.isnan(Fl[ua == 0]).all() and not np.isnan(Fl[HT > 0]).any()
    sure = (ua > 0) & (ref["locus_ht"] >= 100 * dHT)             # (a locus near fixation everywhere: six decimals do not carry its F_l)
    assert sure.sum() >= 0.75 * L1
    dFl = quotient_tol(ref["locus_v"][sure], ref["locus_ht"][sure], dV[sure], dHT[sure])
    assert (np.abs(Fl[sure] - ref["locus_f"][sure]) <= dFl + p10).all()
    # the line: the summary of the matrix in the file, the ratio of the sums, the number of loci with a column
    g = fst[0].groups()
    pairs = F[np.triu_indices(K, 1)]
    assert g[0] == "3" and g[4] == "3" and g[5] is None and int(g[7]) == L1
    assert abs(float(g[1]) - pairs.mean()) <= p6 and abs(float(g[2]) - pairs.min()) <= p6 and abs(float(g[3]) - pairs.max()) <= p6
    dall = quotient_tol(ref["sum_v"], ref["sum_ht"], dV.sum(), dHT.sum())
    assert abs(float(g[6]) - ref["f_all"]) <= dall + p6
    return w, F, q


@pytest.mark.parametrize("name", ["admix", "shared", "mix"])
def test_line_and_files_agree_with_the_written_fit(name, inputs):
    agree_with_the_written_fit(inputs, name, FORMS[name] + ARGS + ["--fst"])


def test_with_query_individuals_the_weights_leave_them_out(inputs):
    rows = [i for i in range(I) if i % 9 == 4]
    w, _, q = agree_with_the_written_fit(inputs, "admix", ["-a"] + ARGS + ["--query", inputs["query"], "--fst"], query_rows=rows)
    _, fst, files = run(inputs, ["-a"] + ARGS + ["--query", inputs["query"], "--fst"])
    assert "stem.admix.K=3.query.txt" in files
    # the panel alone: the mean over all rows of the same file with the query rows given any proportions at all would differ
    filled = np.where(np.isnan(q), 1.0, q)
    assert np.abs(filled.mean(axis=0) - w).max() > 100 * EPS


def test_the_line_equals_the_library_on_the_same_fit(inputs):
    _, fst, _ = run(inputs, ["-a"] + ARGS + ["--fst"])
    rc, d = host.read_structure(inputs["stru"])
    assert rc == 0
    fit = host.Fit(d["ua"], d["geno"], 3, admixture=1, accel_scheme=3, seed=7)
    try:
        ll = [fit.fit_unit(7, u).logL for u in (0, 1)]
        fit.fit_unit(7, 0 if ll[0] >= ll[1] else 1)
        r = fit.divergence()
    finally:
        fit.close()
    assert fst[0].groups() == ("3", "%.6f" % r["f_mean"], "%.6f" % r["f_min"], "%.6f" % r["f_max"], "%d" % r["n_pairs"], None,
                               "%.6f" % r["f_all"], "%d" % r["n_loci"])


def test_one_cluster_has_no_pairs(inputs):
    _, fst, files = run(inputs, ["-a", "-s", "3", "-n", "2", "-r", "7", "-1", "1", "-2", "2", "--fst"])
    assert [m.group(1) for m in fst] == ["1", "2"]
    assert fst[0].group(6) == "no pairs" and fst[0].group(2) is None and float(fst[0].group(7)) == 0.0
    assert fst[1].group(5) == "1" and fst[1].group(2) == fst[1].group(3) == fst[1].group(4)
    text = files["stem.admix.K=1.fst.txt"].decode().split("\n")
    assert text[1].split("\t")[:2] == ["0", "1.0000000000"] and text[4] == "0.0000000000" and text[7] == "0.0000000000"
    assert "stem.admix.K=2.fst.loci.txt" in files


def test_the_clusters_drawn_furthest_apart_have_the_largest_fst(inputs):
    """the condition, from the inputs alone: between the groups the data were drawn in, one pair's F_ST (Hudson, from the observed
    allele frequencies of the groups) exceeds the other two by 0.02.  A fit that recovers the groups -- checked below: every fitted
    cluster is the most probable one of the individuals of one group of its own -- has those observed frequencies for its P but for
    the admixture it leaves in Q, so its F_ST follow the groups' far more closely than that margin"""
    c = clustered_codes(I, L, CLUSTERS)
    obs = (c != bf.MISS)
    z = np.arange(I) % CLUSTERS
    a2 = np.select([c == bf.HOM1, c == bf.HET, c == bf.HOM2], [0, 1, 2], 0)
    keep = obs.any(axis=0)
    f = np.array([a2[z == g].sum(axis=0)[keep] / (2.0 * obs[z == g].sum(axis=0)[keep]) for g in range(CLUSTERS)])
    Pg = np.stack([1 - f, f], axis=2).reshape(CLUSTERS, -1)
    want = du.reference(np.full(keep.sum(), 2), Pg, np.full(CLUSTERS, 1.0 / CLUSTERS))["F"].astype(np.float64)
    order = sorted(((want[a, b], (a, b)) for a in range(CLUSTERS) for b in range(a + 1, CLUSTERS)), reverse=True)
    assert order[0][0] >= order[1][0] + 0.02, order
    _, fst, files = run(inputs, ["-a"] + ARGS + ["--fst"])
    _, _, _, F, _, _, _ = own_files(files, "admix")
    q, _ = written_fit(files, inputs["ua"], I, 3)
    group_of = [int(np.bincount(z[q.argmax(axis=1) == k], minlength=CLUSTERS).argmax()) for k in range(CLUSTERS)]
    assert sorted(group_of) == list(range(CLUSTERS))
    got = max(((F[a, b], tuple(sorted((group_of[a], group_of[b])))) for a in range(CLUSTERS) for b in range(a + 1, CLUSTERS)))
    print("groups:", order, "fitted:", F[np.triu_indices(CLUSTERS, 1)], group_of)
    assert got[1] == order[0][1]
