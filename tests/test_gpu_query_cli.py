"""-m gpu: --query on the command line.  The query individuals are hidden from every fit -- nothing but the query fit's own line
and file depends on their genotypes -- the line and the file are mc_query_fit's on the same fit, and pure individuals of a
clustered data set are put into their own cluster."""
import os
import re

import numpy as np
import pytest

import bedfiles as bf
from cli_util import run_fresh
import cv_util as cu
import query_util as qu
from multiclust_amd import host

pytestmark = pytest.mark.gpu
QUERY_LINE = re.compile(r"^Query fit \(K=(\d+)\): (\d+) individuals, (\d+) converged, (\d+) failed, at most (\d+) iterations, "
                        r"log likelihood (\S+)$")
STANDARD = ["stem.admix.K=%d.out.txt", "stem.admix.K=%d.etaik.txt", "stem.admix.K=%d.pklm.txt", "stem_admix_indivq_%d.indivq",
            "stem_admix_popq_%d.popq"]

I, L, CLUSTERS = 72, 400, 3
QUERY = (np.arange(I) // 3) % 6 == 0            # 12 individuals, four of every cluster (cluster of i = i % 3)
ARGS = ["-a", "-s", "3", "-n", "2", "-r", "7"]


def codes_of(geno):
    """diploid biallelic allele indices [I][L][2] -> .bed codes [I][L] (0xFF in both copies: missing)"""
    n = geno.astype(np.int64).sum(axis=2)
    codes = np.array([bf.HOM1, bf.HET, bf.HOM2], dtype=np.uint8)[np.minimum(n, 2)]
    codes[(geno == 0xFF).all(axis=2)] = bf.MISS
    return codes


def datasets():
    """two code matrices that differ in the query individuals' genotypes only and have the same allele tables: panel individual
    3 is heterozygous at every locus, so a panel individual carries every allele of every locus; the query genotypes of the
    second are drawn again from the same clusters; the same calls are missing in both, some of them in query rows"""
    _, geno = cu.clustered_dataset(I, L, CLUSTERS, 11)
    _, other = cu.clustered_dataset(I, L, CLUSTERS, 12)
    assert not QUERY[3]
    a = codes_of(geno)
    a[3, :] = bf.HET
    rng = np.random.default_rng(5)
    holes = rng.random((I, L)) < 0.01
    holes[3, :] = False
    b = a.copy()
    b[QUERY] = codes_of(other)[QUERY]
    a[holes] = bf.MISS
    b[holes] = bf.MISS
    assert holes[QUERY].any() and (a[~QUERY] == b[~QUERY]).all() and (a[QUERY] != b[QUERY]).any()
    return a, b


def write_inputs(d, codes, bed=False):
    d.mkdir()
    qfile = os.path.join(str(d), "query.txt")
    with open(qfile, "w") as f:
        f.write("\n".join("1" if x else "0" for x in QUERY) + "\n")
    stru = os.path.join(str(d), "data.stru")
    bf.write_equivalent_stru(stru, codes)
    if bed:
        bf.write_fileset(os.path.join(str(d), "data"), codes)
        return ["--bed", os.path.join(str(d), "data")], qfile, stru
    return ["-f", stru], qfile, stru


def run(data, args, d):
    others, own, files = run_fresh(data + args, d / "out", own=QUERY_LINE)
    return others, [m.groups() for m in own], files


def query_table(text):
    rows = [ln.split("\t") for ln in text.decode().strip().split("\n")]
    return rows[0], rows[1:]


def test_hidden_means_hidden(tmp_path):
    a, b = datasets()
    data_a, qfile_a, stru_a = write_inputs(tmp_path / "a", a)
    data_b, qfile_b, stru_b = write_inputs(tmp_path / "b", b)
    (rc_a, da), (rc_b, db) = host.read_structure(stru_a), host.read_structure(stru_b)
    assert rc_a == 0 and rc_b == 0 and np.array_equal(da["ua"], db["ua"]) and da["L_alleles"] == db["L_alleles"]
    assert not np.array_equal(da["geno"], db["geno"]) and np.array_equal(da["geno"][~QUERY], db["geno"][~QUERY])
    args = ARGS + ["-k", "3"]
    lines_a, q_a, files_a = run(data_a, args + ["--query", qfile_a], tmp_path / "a")
    lines_b, q_b, files_b = run(data_b, args + ["--query", qfile_b], tmp_path / "b")
    assert len(q_a) == 1 and len(q_b) == 1
    # the data file's name is part of some lines: the two runs name theirs alike but for the directory
    assert [ln.replace(stru_b, stru_a) for ln in lines_b] == lines_a
    standard = [f % 3 for f in STANDARD]
    assert sorted(files_a) == sorted(standard + ["stem.admix.K=3.query.txt"]) and sorted(files_b) == sorted(files_a)
    for f in standard:
        assert files_a[f] == files_b[f], f
    assert files_a["stem.admix.K=3.query.txt"] != files_b["stem.admix.K=3.query.txt"]
    # the same command again: the same bytes
    lines_c, q_c, files_c = run(data_a, args + ["--query", qfile_a], tmp_path / "a" / "again")
    assert lines_c == lines_a and q_c == q_a and files_c == files_a
    # the rows of the query file sum to 1
    head, rows = query_table(files_a["stem.admix.K=3.query.txt"])
    assert head == ["i", "iter", "converged", "logL", "eta0", "eta1", "eta2"] and len(rows) == int(QUERY.sum())
    assert [int(r[0]) for r in rows] == np.flatnonzero(QUERY).tolist()
    assert all(abs(sum(float(x) for x in r[4:]) - 1) <= 1e-9 for r in rows)


@pytest.mark.parametrize("form", ["structure", "bed"])
def test_command_line_equals_library_and_recovers_the_clusters(form, tmp_path):
    a, _ = datasets()
    data, qfile, stru = write_inputs(tmp_path / "in", a, bed=form == "bed")
    _, qlines, files = run(data, ARGS + ["-k", "3", "--query", qfile], tmp_path / "in")
    rc, d = host.read_structure(stru)
    assert rc == 0
    fit = host.Fit(d["ua"], d["geno"], 3, admixture=1, accel_scheme=3, seed=7)
    try:
        fit.hide_queries(QUERY)
        ll = [fit.fit_unit(7, u).logL for u in (0, 1)]
        fit.fit_unit(7, 0 if ll[0] >= ll[1] else 1)
        panel_q = fit.get_q(fit.mod.pindex)
        r = fit.fit_queries()
        # the context is as it was: the hold-out in force, the estimate in its slot
        assert np.array_equal(np.isnan(panel_q).all(axis=1), QUERY)
        assert np.array_equal(fit.get_q(fit.mod.pindex), panel_q, equal_nan=True)
    finally:
        fit.close()
    assert qlines == [("3", "%d" % r["rows"].size, "%d" % r["n_converged"], "%d" % r["n_failed"], "%d" % r["max_iter"],
                       "%.6f" % r["sum_logL"])]
    _, rows = query_table(files["stem.admix.K=3.query.txt"])
    want = [["%d" % r["rows"][x], "%d" % r["iter"][x], "%d" % r["converged"][x], "%.6f" % r["logL"][x]] +
            ["%.10f" % v for v in r["q"][x]] for x in range(r["rows"].size)]
    assert rows == want
    assert r["n_failed"] == 0 and r["n_converged"] == r["rows"].size and np.array_equal(r["rows"], np.flatnonzero(QUERY))
    # recovery: a cluster's label is the component most of its panel individuals have their largest proportion in
    truth = np.arange(I) % CLUSTERS
    label = [np.bincount(np.argmax(panel_q[~QUERY & (truth == c)], axis=1), minlength=3).argmax() for c in range(CLUSTERS)]
    assert sorted(label) == [0, 1, 2]
    own = r["q"][np.arange(r["rows"].size), np.array(label)[truth[r["rows"]]]]
    print("smallest proportion of a query individual in its own cluster: %.4f" % own.min())
    # Beta(0.3, 0.3) cluster frequencies over 400 loci: on the CPU the oracle's fit of the panel (tests/oracle_bind.py: random start
    # from seed 7, SQUAREM 3) followed by the numpy restatement (query_util.fit_rows, abs_error 1e-4) gives every one of the twelve
    # at least 0.9734 on its own cluster; the bound asserted here leaves room for another local fit of the panel
    assert own.min() >= 0.9


def test_one_line_and_one_file_per_k(tmp_path):
    a, _ = datasets()
    data, qfile, _ = write_inputs(tmp_path / "in", a)
    _, qlines, files = run(data, ARGS + ["-1", "2", "-2", "3", "--query", qfile], tmp_path / "in")
    assert [ln[0] for ln in qlines] == ["2", "3"] and all(ln[1] == "12" for ln in qlines)
    assert sorted(f for f in files if f.endswith(".query.txt")) == ["stem.admix.K=2.query.txt", "stem.admix.K=3.query.txt"]
    for K in (2, 3):
        head, rows = query_table(files["stem.admix.K=%d.query.txt" % K])
        assert len(head) == 4 + K and len(rows) == 12
