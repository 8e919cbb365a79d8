"""The numpy definitions of the density-aware linkage tree (sequence.core_similarity, mutual_reachability_tree, density_tree_cut,
hdbscan_clusters) against brute force that shares no code with them, hand-built trees whose stabilities are worked out here, the
planted partition (and scikit-learn's answer on it, where scikit-learn is there), DensityTreeResult, and the GENOMAD_AMD_HDBSCAN row
of main() over a fake engine.  No GPU."""
import numpy as np
import pytest

from genomad_amd import nn_classification as nnc, sequence
from genomad_amd.engine import DensityTreeResult
from tests.clusters_data import planted
from tests.density_tree_data import brute_hdbscan, hdbscan_plant, mutual
from tests.linkage_data import integer_rows_with_two_invalid, kruskal
from tests.neighbours_data import rows
from tests.test_analyses_host import ENV, FakeAnalysisEngine, fake_main, same_file
from tests.test_strand_host import _npz, _same_npz, _tree, _write_fasta

HDBSCAN_ENV = ("GENOMAD_AMD_HDBSCAN", "GENOMAD_AMD_HDBSCAN_MIN_POINTS")


def tree_of(edges, n):
    """(a, b, sim, valid) of hand-written (lo, hi, sim) edges over n valid rows"""
    a, b, sim = zip(*edges)
    return np.asarray(a, np.int64), np.asarray(b, np.int64), np.asarray(sim, np.float32), np.ones(n, np.uint8)


def table(h):
    """{smallest member: (birth, stability, size, selected)} - two clusters on one path may share their smallest member: a list"""
    return sorted(zip(h["cluster"].tolist(), h["birth"].tolist(), h["stability"].tolist(), h["size"].tolist(), h["selected"].tolist()))


# ---- core similarities and the tree ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small():
    r = planted(140, 3)[0]
    r[17, 5] = np.nan
    r[90] = 0
    return r


def test_core_similarity_is_the_kth_largest_pair_value(small):
    s, ok = sequence._pair_values(small, "cosine")
    assert np.array_equal(s, s.T, equal_nan=True) and ok.sum() == 138
    for m in (1, 2, 5, 65):
        core, valid = sequence.core_similarity(small, m)
        assert np.array_equal(valid.astype(bool), ok) and np.isnan(core[[17, 90]]).all()
        for i in (0, 3, 139):
            v = sorted((s[i, j] for j in range(140) if j != i and ok[j]), reverse=True)
            assert core[i] == (np.inf if m == 1 else v[m - 2])
    few = small[:12]                                                    # 12 valid rows at min_points 65: the least similar partner
    core, _ = sequence.core_similarity(few, 65)
    s, _ = sequence._pair_values(few, "cosine")
    assert core[0] == min(s[0, 1:]) and np.isnan(sequence.core_similarity(few[:1], 5)[0][0])
    for bad in (0, 66, 2.5, True, "5"):
        with pytest.raises(ValueError, match="min_points"):
            sequence.core_similarity(small, bad)
    with pytest.raises(ValueError, match="metric 'l2'"):
        sequence.mutual_reachability_tree(small, 5, "l2")


@pytest.mark.parametrize("metric,m", (("cosine", 1), ("cosine", 5), ("cosine", 17), ("dot", 5)))
def test_the_tree_is_kruskal_over_the_float64_matrix(small, metric, m):
    a, b, sim, core, valid = sequence.mutual_reachability_tree(small, m, metric)
    s, ok = sequence._pair_values(small, metric)
    core64, _ = sequence.core_similarity(small, m, metric)
    want = kruskal(mutual(s, core64), ok)
    assert len(a) == int(ok.sum()) - 1 and np.array_equal(a, want[0]) and np.array_equal(b, want[1]) and np.array_equal(sim, want[2].astype(np.float32))
    assert core.dtype == np.float32 and np.array_equal(core, core64.astype(np.float32), equal_nan=True)
    assert np.array_equal(valid.astype(bool), ok) and (np.diff(sim) <= 0).all()
    if m == 1:                                                          # min_points 1 is the single-linkage tree
        for x, y in zip((a, b, sim, valid), sequence.single_linkage_tree(small, metric)):
            assert np.array_equal(x, y)
    else:
        assert len(np.unique(sim)) < len(sim)                           # mutual reachability ties


def test_integer_dots_tie_and_a_forest_cuts_per_tree():
    base = integer_rows_with_two_invalid()
    a, b, sim, core, valid = sequence.mutual_reachability_tree(base, 5, "dot")
    assert len(a) == 197 and len(np.unique(sim)) < len(sim) and np.isnan(core[[5, 77]]).all()
    res = DensityTreeResult.build((a, b, sim, core, valid), 5, "dot", rounds=3)
    assert (res.n, res.n_valid, res.n_edges, res.rounds, res.min_points, res.metric) == (200, 198, 197, 3, 5, "dot")
    with pytest.raises(ValueError, match="cosine only"):
        res.hdbscan(5)
    with pytest.raises(ValueError, match="cosine only"):
        res.matrix()
    keep = np.arange(197) != 100                                        # one edge less: a forest of two trees
    forest = DensityTreeResult.build((a[keep], b[keep], sim[keep], core, valid), 5, "dot")
    assert np.array_equal(forest.cut(float(sim[50])), res.cut(float(sim[50])))      # above the edge left out: the same components
    low = float(sim[-1])                                                # below it: cut works per tree, one component more
    assert len(set(forest.cut(low).tolist())) == len(set(res.cut(low).tolist())) + 1 and forest.cluster_counts([low])[0] == 2
    with pytest.raises(ValueError, match="spanning tree, not a forest"):
        sequence.hdbscan_clusters(a[keep], b[keep], sim[keep], valid, 5)


@pytest.mark.parametrize("metric,m", (("cosine", 2), ("cosine", 5), ("cosine", 12), ("dot", 5)))
def test_the_cut_is_density_clusters_at_its_core_rows(small, metric, m):
    a, b, sim, core, valid = sequence.mutual_reachability_tree(small, m, metric)
    s, ok = sequence._pair_values(small, metric)
    res = DensityTreeResult.build((a, b, sim, core, valid), m, metric)
    mid = np.sort(np.unique(s[np.isfinite(s)]))
    ts = [float(np.float32(x)) for x in (0.8, 0.9)] if metric == "cosine" else []
    ts += [float((mid[k] + mid[k + 1]) / 2) for k in (len(mid) // 2, len(mid) - 40, len(mid) - 400)]
    for t in ts:
        t32 = float(np.float32(t))
        assert np.abs(s[np.isfinite(s)] - t32).min() > 1e-9, t         # density_clusters sums its pairs in another order
        label, _, _, _, _, kind = sequence.density_clusters(small, t, m, metric)
        want = np.where(kind == 3, label, -1)
        assert np.array_equal(res.cut(t), want) and np.array_equal(sequence.density_tree_cut(a, b, sim, core, valid, t), want), t
        assert res.cluster_counts([t]).tolist() == [len(set(want[want >= 0].tolist()))], t
    assert (res.cut(2.0 if metric == "cosine" else 1e9) == -1).all()


# ---- hdbscan_clusters -----------------------------------------------------------------------------------------------------------------

def test_hdbscan_equals_the_brute_force_by_levels():
    pool, _ = hdbscan_plant()
    rng = np.random.default_rng(1)
    seen = 0
    for trial in range(40):
        n, m, size = int(rng.integers(3, 15)), int(rng.integers(1, 5)), int(rng.integers(2, 5))
        r = pool[rng.permutation(len(pool))[:n]].copy()
        if trial % 3 == 0:
            r[1] = r[0]                                                 # a duplicate: sim = 1, the floor of the distance
        a, b, sim, core, valid = sequence.mutual_reachability_tree(r, m)
        w = mutual(sequence._pair_values(r, "cosine")[0], sequence.core_similarity(r, m)[0]).astype(np.float32)
        for single in (False, True):
            h = sequence.hdbscan_clusters(a, b, sim, valid, size, single)
            label, lam, clusters = brute_hdbscan(w, size, single)
            assert np.array_equal(h["label"], label), (trial, single)
            assert np.allclose(h["lambda_out"], lam, rtol=1e-12, atol=0), trial
            assert np.allclose(sorted(h["stability"]), sorted(c["stability"] for c in clusters), rtol=1e-9), trial
            assert sorted(h["size"].tolist()) == sorted(len(c["members"]) for c in clusters)
            seen += len(clusters) > 1
    assert seen >= 10                                                   # the draw does split


def test_a_tie_at_the_selection_keeps_the_parent():
    """sim 0.5, 0.75, 0.875 are lambda 2, 4, 8.  Ten rows, min_cluster_size 2.  The root (10 rows, born at 0) splits at 2 into
    P = {0..7} and Q = {8, 9}: S(root) = 10 * 2 = 20.  P (born at 2) falls apart at 4 into A = {0, 1}, B = {2, 3} and the four
    single rows 4..7, which fall out: S(P) = 8 * (4 - 2) = 16.  A and B end at 8: S(A) = S(B) = 2 * (8 - 4) = 8, together 16 = S(P):
    the tie keeps P.  Q ends at 8: S(Q) = 2 * (8 - 2) = 12.  Selected: P and Q (28 > 20, so also where the root is allowed)."""
    edges = [(0, 1, .875), (2, 3, .875), (8, 9, .875), (0, 2, .75), (0, 4, .75), (0, 5, .75), (0, 6, .75), (0, 7, .75), (0, 8, .5)]
    for single in (False, True):
        h = sequence.hdbscan_clusters(*tree_of(edges, 10), 2, single)
        assert table(h) == [(0, 0.0, 20.0, 10, False), (0, 2.0, 16.0, 8, True), (0, 4.0, 8.0, 2, False), (2, 4.0, 8.0, 2, False),
                            (8, 2.0, 12.0, 2, True)]
        assert h["label"].tolist() == [0] * 8 + [8, 8]
        assert h["lambda_out"].tolist() == [8, 8, 8, 8, 4, 4, 4, 4, 8, 8]
        assert h["parent"].tolist() == [-1, 0, 0, 1, 1] or sorted(h["parent"].tolist()) == [-1, 0, 0, 1, 1]


def test_allow_single_cluster():
    """sim 0.875, 0.9375 are lambda 8, 16.  Four rows, min_cluster_size 2: the root splits at 8 into {0, 1} and {2, 3}, S(root) = 4 * 8
    = 32; each child ends at 16: S = 2 * (16 - 8) = 16, together 32.  Where the root may be selected the tie keeps it: one cluster.
    Otherwise the two children are the clusters.  With {2, 3} ending at 32 (sim 0.96875) the children hold 16 + 48 = 64 > 32 and
    win either way."""
    edges = [(0, 1, .9375), (2, 3, .9375), (1, 2, .875)]
    assert sequence.hdbscan_clusters(*tree_of(edges, 4), 2)["label"].tolist() == [0, 0, 2, 2]
    h = sequence.hdbscan_clusters(*tree_of(edges, 4), 2, True)
    assert h["label"].tolist() == [0, 0, 0, 0] and h["selected"].tolist() == [True, False, False]
    assert h["stability"].tolist() == [32.0, 16.0, 16.0] and h["lambda_out"].tolist() == [16.0] * 4
    edges[1] = (2, 3, .96875)
    h = sequence.hdbscan_clusters(*tree_of(edges, 4), 2, True)
    assert h["label"].tolist() == [0, 0, 2, 2] and sorted(h["stability"].tolist()) == [16.0, 32.0, 48.0]


def test_duplicates_sit_on_the_floor_of_the_distance():
    """{0, 1, 2} and {3, 4} are duplicates (sim 1, and one pair that rounded to just above 1), joined at sim 0.5 = lambda 2.  d = max(1 -
    sim, 2^-24) makes their lambda 2^24 instead of infinity: S({0, 1, 2}) = 3 * (2^24 - 2), S({3, 4}) = 2 * (2^24 - 2), S(root) = 10."""
    above = float(np.nextafter(np.float32(1), np.float32(2)))
    h = sequence.hdbscan_clusters(*tree_of([(0, 1, 1.0), (0, 2, above), (3, 4, above), (0, 3, .5)], 5), 2)
    top = 2.0 ** 24
    assert h["label"].tolist() == [0, 0, 0, 3, 3] and h["lambda_out"].tolist() == [top] * 5
    assert table(h) == [(0, 0.0, 10.0, 5, False), (0, 2.0, 3 * (top - 2), 3, True), (3, 2.0, 2 * (top - 2), 2, True)]
    assert np.isfinite(h["stability"]).all()


def test_every_similarity_equal():
    """a star of five rows at sim 0.5: at the only level every row is on its own, the root ends there: S(root) = 5 * 2 = 10, no child"""
    edges = [(0, k, .5) for k in range(1, 5)]
    h = sequence.hdbscan_clusters(*tree_of(edges, 5), 2)
    assert h["label"].tolist() == [-1] * 5 and table(h) == [(0, 0.0, 10.0, 5, False)] and h["lambda_out"].tolist() == [2.0] * 5
    h = sequence.hdbscan_clusters(*tree_of(edges, 5), 2, True)
    assert h["label"].tolist() == [0] * 5 and h["selected"].tolist() == [True]
    assert sequence.hdbscan_clusters(*tree_of(edges, 5), 6, True)["label"].tolist() == [0] * 5      # fewer rows than a cluster needs


def test_small_and_wrong_inputs():
    none = np.zeros(0, np.int64)
    h = sequence.hdbscan_clusters(none, none, np.zeros(0, np.float32), np.zeros(3, np.uint8), 2)
    assert h["label"].tolist() == [-1] * 3 and np.isnan(h["lambda_out"]).all() and len(h["cluster"]) == 0
    h = sequence.hdbscan_clusters(none, none, np.zeros(0, np.float32), np.array([0, 1, 0], np.uint8), 2, True)
    assert h["label"].tolist() == [-1, 1, -1] and h["size"].tolist() == [1]
    h = sequence.hdbscan_clusters([1], [3], [0.5], np.array([0, 1, 0, 1], np.uint8), 2, True)
    assert h["label"].tolist() == [-1, 1, -1, 1] and np.isnan(h["lambda_out"][[0, 2]]).all()
    for size in (1, 0, 2.5, True):
        with pytest.raises(ValueError, match="min_cluster_size"):
            sequence.hdbscan_clusters([0], [1], [0.5], [1, 1], size)
    with pytest.raises(ValueError, match="not a tree"):
        sequence.hdbscan_clusters([0, 0, 1], [1, 1, 2], [0.5, 0.5, 0.25], [1, 1, 1, 1], 2)
    with pytest.raises(ValueError, match="not valid"):
        sequence.hdbscan_clusters([0], [2], [0.5], [1, 1, 0], 2)
    with pytest.raises(ValueError, match="not a number"):
        sequence.hdbscan_clusters([0], [1], [np.nan], [1, 1], 2)


def test_the_labels_do_not_depend_on_the_order_of_tied_edges():
    r, _ = hdbscan_plant()
    a, b, sim, core, valid = sequence.mutual_reachability_tree(r, 5)
    assert len(np.unique(sim)) < len(sim)
    want = sequence.hdbscan_clusters(a, b, sim, valid, 5)
    rng = np.random.default_rng(2)
    for _ in range(5):
        p = rng.permutation(len(a))
        got = sequence.hdbscan_clusters(a[p], b[p], sim[p], valid, 5)
        assert np.array_equal(got["label"], want["label"]) and np.array_equal(got["lambda_out"], want["lambda_out"])
        assert np.allclose(sorted(got["stability"]), sorted(want["stability"]), rtol=1e-12)
    # another spanning tree of the same levels: a tied edge swapped for one that joins the same two components at that level
    s = sequence._pair_values(r, "cosine")[0]
    w = mutual(s, sequence.core_similarity(r, 5)[0]).astype(np.float32)
    label, lam, _ = brute_hdbscan(w, 5)
    assert np.array_equal(label, want["label"]) and np.allclose(lam, want["lambda_out"], rtol=1e-12)


def test_the_planted_partition_is_returned_and_the_isolated_rows_are_noise():
    r, family = hdbscan_plant()
    a, b, sim, core, valid = sequence.mutual_reachability_tree(r, 5)
    res = DensityTreeResult.build((a, b, sim, core, valid), 5, "cosine")
    h = res.hdbscan(5)
    assert (h["label"][family < 0] == -1).all()
    for f in range(3):
        members = np.flatnonzero(family == f)
        assert (h["label"][members] == members.min()).all(), f
    assert h["selected"].sum() == 3 and (h["lambda_out"][family < 0] < h["lambda_out"][family >= 0].min()).all()
    recs = sequence.hdbscan_table(h)
    assert [x["size"] for x in recs] == [int((family == f).sum()) for f in np.argsort([np.flatnonzero(family == f).min() for f in range(3)])]
    assert res.matrix().shape == (45, 4) and len(res.table()) == 45


def test_scikit_learn_finds_the_same_partition_on_the_plant():
    cluster = pytest.importorskip("sklearn.cluster")
    if not hasattr(cluster, "HDBSCAN"):
        pytest.skip("this scikit-learn has no HDBSCAN")
    r, family = hdbscan_plant()
    s = sequence._pair_values(r, "cosine")[0]
    d = np.maximum(1.0 - s, 0.0)
    np.fill_diagonal(d, 0.0)
    theirs = cluster.HDBSCAN(min_cluster_size=5, min_samples=5, metric="precomputed").fit(d).labels_

    def partition(label):
        return sorted(sorted(np.flatnonzero(label == x).tolist()) for x in set(label.tolist()) if x >= 0), np.flatnonzero(label < 0).tolist()

    assert partition(np.asarray(theirs)) == partition(family)           # scikit-learn alone returns the plant
    a, b, sim, core, valid = sequence.mutual_reachability_tree(r, 5)
    assert partition(sequence.hdbscan_clusters(a, b, sim, valid, 5)["label"]) == partition(np.asarray(theirs))


def test_the_table_of_a_contig_without_an_embedding(tmp_path):
    r = hdbscan_plant()[0][:20].copy()
    r[3] = 0
    res = DensityTreeResult.build(sequence.mutual_reachability_tree(r, 3), 3, "cosine")
    found = res.hdbscan(3, True)
    names = [f"s{i}" for i in range(20)]
    nnc.write_hdbscan_tsv(tmp_path / "t.tsv", names, res, found)
    lines = [x.split("\t") for x in (tmp_path / "t.tsv").read_text().splitlines()]
    assert lines[0] == nnc.HDBSCAN_TSV_HEADER.strip().split("\t") and len(lines) == 21
    assert lines[4] == ["s3", "NA", "0", "NA", "NA"]
    for i, x in enumerate(lines[1:]):
        if i != 3:
            assert x[1] == ("NA" if found["label"][i] < 0 else names[found["label"][i]]) and float(x[3]) == pytest.approx(res.core[i], abs=1e-6)
            assert int(x[2]) == (0 if found["label"][i] < 0 else int((found["label"] == found["label"][i]).sum()))
            assert float(x[4]) == pytest.approx(found["lambda_out"][i], rel=1e-5)


# ---- main() ---------------------------------------------------------------------------------------------------------------------------

class FakeTreeEngine(FakeAnalysisEngine):
    """the stand-in of tests/test_analyses_host.py plus the density tree, served from its definition"""

    def density_tree(self, rows, min_points=5, metric="cosine"):
        type(self).calls.append(("density_tree", len(rows), int(min_points), metric))
        return DensityTreeResult.build(sequence.mutual_reachability_tree(rows, min_points, metric), min_points, metric, rounds=1)


def set_env(mp, env):
    mp.setattr(nnc, "_engine", lambda: FakeTreeEngine())
    for k in ENV + HDBSCAN_ENV:
        mp.delenv(k, raising=False)
    for k, v in env.items():
        mp.setenv(k, v)


def tree_calls():
    return [c for c in FakeTreeEngine.calls if c != "plain" and c[0] == "density_tree"]


def test_the_switch_of_main(tmp_path, monkeypatch, capsys):
    fa = tmp_path / "m.fna"
    recs = _write_fasta(fa, n=6)
    with open(fa, "a") as f:
        for k in range(2):
            f.write(f">twin{k} of c2\n{dict(recs)['c2']}\n")
    on, d = tmp_path / "on", tmp_path / "on" / "m_nn_classification"
    files = ["m_nn_hdbscan.npz", "m_nn_hdbscan.tsv"]
    set_env(monkeypatch, {"GENOMAD_AMD_EMBEDDINGS": "1"})
    fake_main(fa, tmp_path / "unset")
    plain = _tree(tmp_path / "unset" / "m_nn_classification")
    del FakeTreeEngine.calls[:]
    env = {"GENOMAD_AMD_EMBEDDINGS": "1", "GENOMAD_AMD_HDBSCAN": "2"}
    set_env(monkeypatch, env)
    fake_main(fa, on)
    assert _tree(d) == sorted(plain + files) and [c[1:] for c in tree_calls()] == [(len(recs) + 2, 2, "cosine")]
    for rel in plain:                                                   # every other output is what it was
        if rel.endswith(".npz"):
            assert _same_npz(tmp_path / "unset" / "m_nn_classification" / rel, d / rel), rel
        elif rel.endswith(".tsv"):
            assert (tmp_path / "unset" / "m_nn_classification" / rel).read_bytes() == (d / rel).read_bytes(), rel
    z = _npz(d / files[0])
    n = len(recs) + 2
    assert int(z["min_cluster_size"]) == 2 and int(z["min_points"]) == 2 and str(z["metric"]) == "cosine" and "strand" not in z
    assert z["core"].shape == z["label"].shape == z["lambda_out"].shape == z["valid"].shape == (n,)
    assert len(z["a"]) == len(z["b"]) == len(z["sim"]) == int(z["valid"].sum()) - 1
    names = [str(x) for x in z["contig_names"]]
    emb = _npz(d / "m_nn_embeddings.npz")["embeddings"]
    want = sequence.mutual_reachability_tree(emb, 2)
    found = sequence.hdbscan_clusters(want[0], want[1], want[2], want[4], 2)
    assert np.array_equal(z["a"], want[0]) and np.array_equal(z["sim"], want[2]) and np.array_equal(z["label"], found["label"])
    assert np.array_equal(z["cluster_stability"], found["stability"]) and np.array_equal(z["cluster"], found["cluster"])
    lines = (d / files[1]).read_text().splitlines()
    assert lines[0].split("\t") == ["seq_name", "cluster", "cluster_size", "core_similarity", "lambda_out"] and len(lines) == n + 1
    rows_of = {x.split("\t")[0]: x.split("\t")[1:] for x in lines[1:]}
    assert sorted(rows_of) == sorted(names) and z["valid"].all()
    twins = [rows_of[k] for k in ("c2", "twin0", "twin1")]
    assert twins[0] == twins[1] == twins[2] and int(twins[0][1]) >= 3 and twins[0][2] == "1.000000" and twins[0][3] == "1.67772e+07"
    log = (on / "m_nn_classification.log").read_text()
    assert "HDBSCAN clusters of the sequences (" in log and "m_nn_hdbscan.npz" in log
    # the same command again: nothing runs
    del FakeTreeEngine.calls[:]
    fake_main(fa, on)
    assert FakeTreeEngine.calls == []
    # another request: the stage runs again and the file spells it
    set_env(monkeypatch, dict(env, GENOMAD_AMD_HDBSCAN_MIN_POINTS="3"))
    fake_main(fa, on)
    assert [c[2] for c in tree_calls()] == [3] and int(_npz(d / files[0])["min_points"]) == 3 and _tree(d) == sorted(plain + files)
    # one of the pair gone: again; an unreadable npz: again
    set_env(monkeypatch, env)
    fake_main(fa, on)
    (tmp_path / "first.npz").write_bytes((d / files[0]).read_bytes())
    (d / files[1]).unlink()
    fake_main(fa, on)
    (d / files[0]).write_bytes(b"")
    fake_main(fa, on)
    assert len(tree_calls()) == 4 and _tree(d) == sorted(plain + files) and same_file(d / files[0], tmp_path / "first.npz")
    # the switch unset: its files go, and only they
    set_env(monkeypatch, {"GENOMAD_AMD_EMBEDDINGS": "1"})
    fake_main(fa, on)
    assert _tree(d) == plain and len(tree_calls()) == 4
    # refused without the embeddings; the companion alone is refused; bad values are errors
    set_env(monkeypatch, {"GENOMAD_AMD_HDBSCAN": "2"})
    capsys.readouterr()
    with pytest.raises(SystemExit) as exc:
        fake_main(fa, tmp_path / "refused")
    err = capsys.readouterr().err.strip().splitlines()
    assert exc.value.code == 1 and len(err) == 1 and "GENOMAD_AMD_HDBSCAN " in err[0] and "GENOMAD_AMD_EMBEDDINGS=1" in err[0]
    assert not list((tmp_path / "refused").rglob("*.npz"))
    for env, what in (({"GENOMAD_AMD_HDBSCAN_MIN_POINTS": "3"}, "needs GENOMAD_AMD_HDBSCAN"), ({"GENOMAD_AMD_HDBSCAN": "1"}, ">= 2"),
                      ({"GENOMAD_AMD_HDBSCAN": "5", "GENOMAD_AMD_HDBSCAN_MIN_POINTS": "66"}, r"in \[1, 65\]"),
                      ({"GENOMAD_AMD_HDBSCAN": "x"}, "expected an integer")):
        set_env(monkeypatch, env)
        with pytest.raises(ValueError, match=what):
            nnc.hdbscan_requested()
    set_env(monkeypatch, {"GENOMAD_AMD_HDBSCAN": "100"})
    assert nnc.hdbscan_requested() == (100, 65)
    set_env(monkeypatch, {})
    assert nnc.hdbscan_requested() is None
