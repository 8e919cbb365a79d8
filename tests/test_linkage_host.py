"""The single-linkage tree's numpy definition and host helpers, without a GPU: sequence.single_linkage_tree against a brute-force
Kruskal and a naive agglomeration (tests/linkage_data.py), the cut against sequence.threshold_clusters, the counts, the linkage matrix,
the edges of the interface, and the two files main() writes."""
import numpy as np
import pytest

from genomad_amd import nn_classification, sequence
from genomad_amd.engine import LinkageResult
from tests.clusters_data import THRESHOLDS, planted
from tests.linkage_data import agglomerate, integer_rows, integer_rows_with_two_invalid, kruskal
from tests.neighbours_data import rows


def unit64(r):
    r = r.astype(np.float64)
    return r / np.sqrt((r * r).sum(axis=1))[:, None]


def pair_values(u):
    """the definition's float64 value of every pair: one pair at a time, the same sum either way round"""
    return np.stack([(u * u[i]).sum(axis=1) for i in range(len(u))])


@pytest.fixture(scope="module")
def integer_tree():
    r = integer_rows_with_two_invalid()
    return r, sequence.single_linkage_tree(r, "dot")


@pytest.fixture(scope="module")
def planted_tree():
    r, _ = planted()
    return r, sequence.single_linkage_tree(r)


def test_integer_rows_with_ties_equal_the_brute_force_kruskal(integer_tree):
    r, (a, b, sim, valid) = integer_tree
    ok = np.ones(200, bool)
    ok[[5, 77]] = False
    assert valid.dtype == np.uint8 and np.array_equal(valid.astype(bool), ok)
    dots = np.where(ok[:, None] & ok[None, :], np.nan_to_num(r, nan=0.0, posinf=0.0).astype(np.float64) @ np.nan_to_num(r, nan=0.0, posinf=0.0).astype(np.float64).T, np.nan)
    wa, wb, ws = kruskal(dots, ok)
    assert a.dtype == b.dtype == np.int64 and sim.dtype == np.float32
    assert len(a) == 197 and len(np.unique(sim)) == 153                # ties among the tree's own edges
    assert np.array_equal(a, wa) and np.array_equal(b, wb) and np.array_equal(sim.astype(np.float64), ws)
    assert (a < b).all() and not np.isin([5, 77], np.concatenate([a, b])).any()
    order = list(zip(-sim.astype(np.float64), a, b))
    assert order == sorted(order)


def test_small_trees_equal_a_naive_agglomeration_and_the_matrix_follows_it():
    for n, seed in ((2, 1), (5, 2), (12, 3)):
        r = rows(n, seed)
        r[n - 1] = r[0]                                                # a tie at 1 among the best pairs
        values = pair_values(unit64(r))
        wa, wb, ws, wz = agglomerate(values)
        a, b, sim, valid = sequence.single_linkage_tree(r)
        assert valid.all() and np.array_equal(a, wa) and np.array_equal(b, wb) and np.array_equal(sim, ws.astype(np.float32))
        z = sequence.linkage_matrix(a, b, sim, n)
        assert z.dtype == np.float64 and z.shape == (n - 1, 4)
        assert np.array_equal(z[:, [0, 1, 3]], wz[:, [0, 1, 3]]) and np.array_equal(z[:, 2], 1.0 - sim.astype(np.float64))
        assert z[-1, 3] == n and (np.diff(z[:, 2]) >= 0).all()
        res = LinkageResult.build((a, b, sim, valid), "cosine")
        assert np.array_equal(res.matrix(), z)


def test_the_cut_is_threshold_clusters_on_the_planted_rows(planted_tree):
    r, (a, b, sim, valid) = planted_tree
    assert len(a) == 332 and int((sim >= 0.9).sum()) == 79 and int((sim >= 0.8).sum()) == 79
    tie = float(sim[100])                                              # a threshold that equals one merge's similarity: a tie is an edge
    for t in THRESHOLDS + (tie, -1.0, 1.5):
        label = sequence.linkage_cut(a, b, sim, valid, t)
        want = sequence.threshold_clusters(r, t)[0]
        assert label.dtype == np.int64 and np.array_equal(label, want), t
        count = sequence.linkage_cluster_counts(sim, int(valid.sum()), [t])
        assert count.dtype == np.int64 and count[0] == len(np.unique(label[label >= 0])), t
    assert (sequence.linkage_cut(a, b, sim, valid, tie) == sequence.linkage_cut(a, b, sim, valid, np.nextafter(np.float32(tie), np.float32(-1)))).all()
    assert list(sequence.linkage_cluster_counts(sim, 333, [-1.0, 0.9, 1.5])) == [1, 333 - 79, 333]


def test_the_cut_is_threshold_clusters_on_the_integer_rows(integer_tree):
    r, (a, b, sim, valid) = integer_tree
    ok = valid.astype(bool)
    clean = np.where(ok[:, None], r, 0).astype(np.float64)
    upper = (clean @ clean.T)[np.triu_indices(200, 1)]
    upper = upper[(ok[:, None] & ok[None, :])[np.triu_indices(200, 1)]]
    seen = set()
    for q in (0.5, 0.9, 0.99):
        t = float(np.quantile(upper, q, method="lower"))              # one of the pair values: ties exactly at the threshold
        label = sequence.linkage_cut(a, b, sim, valid, t)
        want = sequence.threshold_clusters(r, t, "dot")[0]
        assert np.array_equal(label, want), q
        n_clusters = len(np.unique(label[label >= 0]))
        assert sequence.linkage_cluster_counts(sim, int(ok.sum()), [t])[0] == n_clusters
        assert (label[~ok] == -1).all()
        seen.add(n_clusters)
    assert len(seen) == 3 and min(seen) >= 2                           # three different cuts, none of them trivial


def test_edges_of_the_interface():
    e = np.zeros((0, 512), np.float32)
    for r, n_valid in ((e, 0), (rows(1, 4), 1)):
        a, b, sim, valid = sequence.single_linkage_tree(r)
        assert a.shape == b.shape == sim.shape == (0,) and a.dtype == np.int64 and sim.dtype == np.float32
        assert valid.shape == (len(r),) and int(valid.sum()) == n_valid
        assert sequence.linkage_cut(a, b, sim, valid, 0.5).tolist() == list(range(len(r)))
        assert sequence.linkage_cluster_counts(sim, n_valid, [0.0, 1.0]).tolist() == [n_valid, n_valid]
    assert sequence.linkage_matrix([], [], [], 1).shape == (0, 4)
    two = rows(2, 4)
    a, b, sim, valid = sequence.single_linkage_tree(two)
    assert (a.tolist(), b.tolist()) == ([0], [1]) and abs(float(sim[0]) - float(unit64(two)[0] @ unit64(two)[1])) < 1e-7
    assert sequence.linkage_cut(a, b, sim, valid, float(sim[0])).tolist() == [0, 0]
    assert sequence.linkage_cut(a, b, sim, valid, 1.0).tolist() == [0, 1]
    bad = rows(4, 4)
    bad[:, 0] = np.nan
    a, b, sim, valid = sequence.single_linkage_tree(bad)
    assert len(a) == 0 and not valid.any() and sequence.linkage_cut(a, b, sim, valid, 0.0).tolist() == [-1] * 4
    zero = rows(4, 5)
    zero[2] = 0
    a, b, sim, valid = sequence.single_linkage_tree(zero)
    assert valid.tolist() == [1, 1, 0, 1] and len(a) == 2 and 2 not in np.concatenate([a, b])
    a, b, sim, valid = sequence.single_linkage_tree(zero, "dot")       # a zero row is valid under dot: its dots are 0
    assert valid.all() and len(a) == 3 and sim[(a == 2) | (b == 2)].tolist() == [0.0]
    with pytest.raises(ValueError, match="metric 'l2'"):
        sequence.single_linkage_tree(zero, "l2")
    with pytest.raises(ValueError, match=r"\(n, 512\) rows are required"):
        sequence.single_linkage_tree(np.zeros((3, 8), np.float32))
    with pytest.raises(ValueError, match="finite float"):
        sequence.linkage_cut([0], [1], [0.5], [1, 1], float("nan"))


def test_linkage_matrix_refuses_what_is_no_spanning_tree():
    a, b, sim, valid = sequence.single_linkage_tree(rows(5, 6))
    with pytest.raises(ValueError, match="spanning tree"):
        sequence.linkage_matrix(a[:-1], b[:-1], sim[:-1], 5)           # a forest
    with pytest.raises(ValueError, match="spanning tree"):
        sequence.linkage_matrix([], [], [], 0)
    with pytest.raises(ValueError, match="not a tree"):
        sequence.linkage_matrix([0, 0, 1, 3], [1, 2, 2, 4], [0.9, 0.8, 0.7, 0.6], 5)
    with pytest.raises(ValueError, match=r"outside \[0, 5\)"):
        sequence.linkage_matrix([0, 0, 1, 3], [1, 2, 5, 4], [0.9, 0.8, 0.7, 0.6], 5)
    with pytest.raises(ValueError, match="one of each per edge"):
        sequence.linkage_matrix([0], [1, 2], [0.5], 3)
    res = LinkageResult.build((a, b, sim, valid), "dot")
    with pytest.raises(ValueError, match="cosine only"):
        res.matrix()
    r = rows(5, 6)
    r[2] = 0
    res = LinkageResult.build(sequence.single_linkage_tree(r), "cosine")
    assert res.n_edges == 3 and res.n_valid == 4 and res.n == 5
    with pytest.raises(ValueError, match="1 of 5 rows are invalid"):
        res.matrix()


def test_the_result_and_the_files_of_main(tmp_path, monkeypatch):
    r = rows(6, 7)
    r[4] = 0                                                           # a contig without a kept window
    r[5] = r[1]
    res = LinkageResult.build(sequence.single_linkage_tree(r), "cosine", rounds=2)
    names = np.array([f"contig_{i}" for i in range(6)])
    table = res.table(names)
    assert [m["rank"] for m in table] == [1, 2, 3, 4] and [m["clusters_left"] for m in table] == [4, 3, 2, 1]
    assert (table[0]["a"], table[0]["b"], table[0]["sim"]) == ("contig_1", "contig_5", 1.0)
    assert [m["clusters_left"] for m in table] == list(res.cluster_counts([m["sim"] for m in table]))      # no two merges tie here
    assert np.array_equal(res.cut(0.999), [0, 1, 2, 3, -1, 1])
    npz, tsv = tmp_path / "x_nn_linkage.npz", tmp_path / "x_nn_linkage.tsv"
    nn_classification.write_linkage(npz, tsv, "contig_names", names, res)
    z = np.load(npz)
    assert sorted(z.files) == ["a", "b", "contig_names", "metric", "rounds", "sim", "valid"]
    assert np.array_equal(z["a"], res.a) and np.array_equal(z["b"], res.b) and np.array_equal(z["sim"], res.sim)
    assert z["valid"].tolist() == [1, 1, 1, 1, 0, 1] and int(z["rounds"]) == 2 and str(z["metric"]) == "cosine"
    lines = tsv.read_text().splitlines()
    assert lines[0].split("\t") == ["rank", "contig_a", "contig_b", "similarity", "clusters_left"]
    assert lines[1].split("\t") == ["1", "contig_1", "contig_5", "1.000000", "4"] and len(lines) == 5
    nn_classification.write_linkage(npz, tsv, "contig_names", names, res, "both")
    assert str(np.load(npz)["strand"]) == "both"
    for v, want in (("", False), ("0", False), ("1", True)):
        monkeypatch.setenv("GENOMAD_AMD_LINKAGE", v)
        assert nn_classification.linkage_requested() is want
    monkeypatch.setenv("GENOMAD_AMD_LINKAGE", "yes")
    with pytest.raises(ValueError, match="GENOMAD_AMD_LINKAGE='yes'"):
        nn_classification.linkage_requested()
