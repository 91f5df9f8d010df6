"""-m gpu: --kinship on the command line, on a written fileset of the pedigree with admixed founders (tests/kin_util.py: 47
individuals, 1 500 variants, 5 % of the calls missing).  The option prints its line and writes its two files; they are, byte for byte,
what tests/kin_util.py's restatement of the host's rules makes of the device's sums for the same fit, and to the digits of the written
Q and P what it makes of those; every planted pair is among the reported ones; and nothing but the line and the two files depends on
the option -- PLINK and STRUCTURE input, together with --resid --fst, --query and --streams 2.

Each run of the program is made once per module and shared by the tests that read it.

To the printed digits: etaik and pklm carry six decimals, so every q and p read back is within eps = 5.1e-7 of the number the
program used.  That moves t by dt = (K + 1) eps at most, a residual by a dt and G_ij by a dt (|r_i|_1 + |r_j|_1); v = t (1 - t) by dt
and w = a sqrt(v) by dw = a min(dt / (2 sqrt(v)), sqrt(dt)); V_ij by sum_c (dw_i w_j + w_i dw_j + dw_i dw_j); phi = G / V by
(dG + |phi| dV) / V, second-order terms covered by a factor 1.5.  The program's own figures carry six decimals."""

import numpy as np
import pytest

from cli_util import fit_inputs, Runs, table, written_fit
import kin_util as ku
import resid_util as ru
from multiclust_amd import hip, host

pytestmark = pytest.mark.gpu
PED = dict(seed=1, L=1500, founders=40)
K, T_CUT = 2, 0.0884
ARGS = ["-a", "-s", "3", "-n", "2", "-r", "7", "-k", "2"]
OWN = ["stem.admix.K=2.kin.ind.txt", "stem.admix.K=2.kin0"]
EPS, P6 = 5.1e-7, 5.1e-7


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    ped = ku.pedigree(**PED)
    I = ped["codes"].shape[0]
    assert 24 <= I <= 50
    return dict(fit_inputs(tmp_path_factory, "kin_in", ped["codes"]), ped=ped, I=I,
                runs=Runs(lambda: tmp_path_factory.mktemp("kin_out"), own="Kinship"))


def run(inputs, args, bed=True):
    """one run of the program per distinct command line: (other stdout lines, the Kinship lines, files)"""
    return inputs["runs"]((["--bed", inputs["bed"]] if bed else ["-f", inputs["stru"]]) + list(args))


KIN = ["--kinship", "%g" % T_CUT]


@pytest.mark.parametrize("extra,bed", [([], True), (["--resid", "--fst"], True), (["--query", None], True), (["--streams", "2"], True),
                                       ([], False)])
def test_nothing_else_changes(extra, bed, inputs):
    extra = [inputs["query"] if x is None else x for x in extra]
    lines0, own0, files0 = run(inputs, ARGS + extra, bed)
    lines1, own1, files1 = run(inputs, ARGS + extra + KIN, bed)
    assert own0 == [] and len(own1) == 1 and own1[0].startswith("Kinship (K=2): ") and lines0 == lines1
    assert sorted(files1) == sorted(list(files0) + OWN) and len(files0) >= 5
    for f in files0:
        assert files0[f] == files1[f], f
    if extra == ["--streams", "2"] or not bed or "--resid" in extra:  # ... and --kinship says what it says alone, from either input
        _, own2, files2 = run(inputs, ARGS + KIN)
        assert own2 == own1 and all(files2[f] == files1[f] for f in OWN)


def same_fit_sums(inputs):
    """the sums of the device for the fit the program made: the same two initialisations through the library, the better one kept"""
    fit = host.Fit(inputs["ua"], inputs["geno"], K, admixture=1, accel_scheme=3, seed=7)
    try:
        ll = [fit.fit_unit(7, u).logL for u in (0, 1)]
        fit.fit_unit(7, 0 if ll[0] >= ll[1] else 1)
        q, p = fit.get_q(fit.mod.pindex), fit.get_p(fit.mod.pindex)
    finally:
        fit.close()
    return device_sums(inputs, q, p) + (q, p)


def device_sums(inputs, q, p, geno=None):
    c = hip.Context(0)
    try:
        c.set_genotypes(inputs["ua"], inputs["geno"] if geno is None else geno)
        c.set_model(K)
        c.set_q(0, q)
        c.set_p(0, p)
        return c.kinship_products(0)
    finally:
        c.close()


def test_line_and_files_are_the_restatement_of_the_device_sums(inputs):
    _, own, files = run(inputs, ARGS + KIN)
    G, V, q, p = same_fit_sums(inputs)
    want = ku.report(G, V, 2, T_CUT, K)
    assert own == [want["line"]]
    assert files[OWN[1]].decode() == want["kin0"] and files[OWN[0]].decode() == want["ind"]
    # every planted pair is reported, the duplicate as one
    got = {(i, j): d for i, j, _, _, _, d in want["pairs"]}
    ped = inputs["ped"]
    assert ped["planted"] <= set(got) and all(got[pair] == 0 for pair in ped["dup"])
    dup, first, other = ku.margins(want["phi"], ped)
    print("device fit: duplicate %.4f, smallest first degree %.4f, largest other pair %.4f; %s" % (dup, first, other, want["line"]))
    assert min(dup, first) > other
    ku.check(G, V, ku.reference(inputs["ua"], inputs["geno"], q, p))


def agree_with_the_written_fit(inputs, args, query_rows=()):
    ua, geno, I = inputs["ua"], inputs["geno"].copy(), inputs["I"]
    _, own, files = run(inputs, args)
    q, P = written_fit(files, ua, I, K)
    assert np.flatnonzero(np.isnan(q).any(axis=1)).tolist() == list(query_rows)
    q[list(query_rows)] = 1.0 / K                                 # hidden from the fit: no observed copy on the device, any finite row serves
    geno[list(query_rows)] = ru.MISSING
    G, V = device_sums(inputs, q, P, geno)
    ref = ku.reference(ua, geno, q, P)
    ku.check(G, V, ref)
    want = ku.report(G, V, 2, T_CUT, K)
    # how far six decimals of q and p move phi
    dt = (K + 1) * EPS
    a = ref["a"][:, ru.col_locus(ua)].astype(np.float64)
    r1 = np.abs(ref["r"].astype(np.float64)).sum(axis=1)
    w, v = ref["w"].astype(np.float64), ref["v"].astype(np.float64)
    dG = (a.max() * dt) * (r1[:, None] + r1[None, :])
    with np.errstate(divide="ignore", invalid="ignore"):
        dw = a * np.minimum(np.where(v > 0, dt / (2 * np.sqrt(np.where(v > 0, v, 1))), np.inf), np.sqrt(dt))
    dV = dw @ w.T + w @ dw.T + dw @ dw.T
    phi = want["phi"]
    with np.errstate(divide="ignore", invalid="ignore"):
        tol = 1.5 * (dG + np.abs(phi) * dV) / V + P6
    rows = table(files[OWN[1]])
    seen = {}
    for i, j, x, g, vv, d in rows:
        i, j, x = int(i), int(j), float(x)
        seen[(i, j)] = x
        assert i < j and x > T_CUT - P6 and abs(x - phi[i, j]) <= tol[i, j], (i, j, x, phi[i, j], tol[i, j])
        assert abs(float(g) - G[i, j]) <= 1.5 * dG[i, j] + P6 and abs(float(vv) - V[i, j]) <= 1.5 * dV[i, j] + P6
        assert int(d) == ku.degree(x) or min(abs(x - c) for c in ku.CUTS) <= P6
    err = max(abs(x - phi[p]) for p, x in seen.items())
    print("%d pairs, largest |phi - restatement| %.3g, largest tolerance among them %.3g" % (len(seen), err, max(tol[p] for p in seen)))
    for i, j, x, *_ in want["pairs"]:                             # what the restatement reports and the program does not lies at the threshold
        assert (i, j) in seen or x - T_CUT <= tol[i, j]
    ind = table(files[OWN[0]])
    assert [int(r[0]) for r in ind] == list(range(I))
    for r in ind:
        i = int(r[0])
        if i in query_rows:
            assert r[1:] == ["NaN", "NaN", "0", "NaN", "-1"]
            continue
        assert abs(float(r[1]) - phi[i, i]) <= tol[i, i] and abs(float(r[2]) - (2 * phi[i, i] - 1)) <= 2 * tol[i, i]
        assert int(r[5]) not in query_rows and abs(float(r[4]) - phi[i, int(r[5])]) <= tol[i, int(r[5])]
        assert abs(float(r[4]) - want["ind_max"][i]) <= np.nanmax(tol[i][np.isfinite(tol[i])])
    assert all(i not in query_rows and j not in query_rows for i, j in seen)
    return want, own


def test_files_agree_with_the_written_fit(inputs):
    want, own = agree_with_the_written_fit(inputs, ARGS + KIN)
    assert " mean over %d pairs " % (inputs["I"] * (inputs["I"] - 1) // 2) in own[0]


def test_with_query_individuals_their_rows_are_nan(inputs):
    rows = [i for i in range(inputs["I"]) if i % 9 == 4]
    want, own = agree_with_the_written_fit(inputs, ARGS + ["--query", inputs["query"]] + KIN, query_rows=rows)
    n = inputs["I"] - len(rows)
    assert " mean over %d pairs " % (n * (n - 1) // 2) in own[0]
