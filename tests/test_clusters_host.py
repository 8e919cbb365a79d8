"""Clusters among encoder embeddings without a GPU: the numpy definition (sequence.threshold_clusters) against a brute-force labelling
on planted rows and on integer rows, the margin of the planted thresholds the GPU tests rest on, ties at the threshold, invalid rows,
the edges of n and of the threshold, the representative's tie rule, cluster_table, the ABI's argument checks (before the ctx is looked
at: no GPU needed), and main()'s GENOMAD_AMD_CLUSTERS switch over a fake engine served from the definition."""
import os

import numpy as np
import pytest

from genomad_amd import _lib, nn_classification as nnc, sequence
from genomad_amd.engine import ClusterResult, NNEngine
from tests.clusters_data import CHAIN, FAMILY, THRESHOLDS, components, planted, sims64
from tests.neighbours_data import rows
from tests.test_neighbours_host import SWITCHES, FakeNeighbourEngine
from tests.test_strand_host import FakeStrandEngine, _npz, _same_npz, _tree, _write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(got, want):
    return all(a.dtype == np.int64 and np.array_equal(a, b) for a, b in zip(got, want)) and len(got) == len(want) == 4


@pytest.fixture(scope="module")
def plant():
    r, groups = planted()
    return r, groups, sims64(r, r)


@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_planted_thresholds_keep_their_distance_from_every_similarity(plant, threshold):
    """the GPU tests compare with the definition exactly: the device's f32 similarity is within 1e-5 of the fp64 one, so no pair may
    lie closer to the threshold than that - asserted with a factor of ten"""
    r, _, s64 = plant
    gap = np.abs(s64[np.triu_indices(len(r), 1)] - float(np.float32(threshold))).min()
    print(f"\nplanted: min |sim64 - {threshold}| = {gap:.3e}")
    assert gap >= 1e-4


@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_definition_equals_the_brute_force_on_planted_rows(plant, threshold):
    r, groups, s64 = plant
    got = sequence.threshold_clusters(r, threshold)
    assert same(got, components(s64 >= float(np.float32(threshold))))
    label, degree, size, rep = got
    sizes = sorted(size[label == np.arange(len(r))])
    assert [s for s in sizes if s > 1] == [2] + [FAMILY] * 5 + [CHAIN]
    for name, members in groups.items():
        assert len(set(label[members])) == 1 and label[members[0]] == members.min() and size[members[0]] == len(members), name
        clique = (degree[members] == len(members) - 1).all()
        assert clique == (name != "chain"), name                # the chain is the one component that is not a clique
    chain = groups["chain"]
    assert s64[chain[0], chain[-1]] < 0.8 and (s64[chain[:-1], chain[1:]] >= 0.9).all()       # the links hold, the ends do not


def integer_rows():
    rng = np.random.default_rng(11)
    base = rng.integers(0, 8, (200, 512)).astype(np.float32)          # every dot is an integer below 512 * 49 < 2^24
    base[40:60] = base[10]
    base[150] = base[3]
    base[199] = base[3]
    return base


def test_definition_equals_the_brute_force_on_integer_rows_under_dot():
    r = integer_rows()
    dots = sims64(r, r, "dot")
    threshold = float(np.median(dots[np.triu_indices(200, 1)]))
    assert (dots[np.triu_indices(200, 1)] == threshold).sum() > 10                  # ties exactly at the threshold: edges
    assert same(sequence.threshold_clusters(r, threshold, "dot"), components(dots >= threshold))


def test_a_tie_at_the_threshold_is_an_edge():
    r = np.zeros((4, 512), np.float32)
    r[0, :2], r[1, :2], r[2, 2], r[3, 3] = (3, 0), (2, 1), 5, 1
    label, degree, size, rep = sequence.threshold_clusters(r, 6.0, "dot")           # r0.r1 = 6 exactly
    assert list(label) == [0, 0, 2, 3] and list(degree) == [1, 1, 0, 0] and list(size) == [2, 2, 1, 1] and list(rep) == [0, 0, 2, 3]
    label, _, _, _ = sequence.threshold_clusters(r, np.nextafter(np.float32(6), np.float32(7)), "dot")
    assert list(label) == [0, 1, 2, 3]
    # the threshold is compared as the float32 it rounds to: 6 + 1e-9 is 6
    assert list(sequence.threshold_clusters(r, 6.0 + 1e-9, "dot")[0]) == [0, 0, 2, 3]


def test_invalid_rows_join_nobody():
    r = np.tile(rows(1, 4), (7, 1))
    r[1] = 0
    r[3, 100] = np.nan
    r[5, 511] = np.inf
    label, degree, size, rep = sequence.threshold_clusters(r, 0.5)
    assert list(label) == [0, -1, 0, -1, 0, -1, 0] and list(degree) == [3, 0, 3, 0, 3, 0, 3]
    assert list(size) == [4, 0, 4, 0, 4, 0, 4] and list(rep) == [0, -1, 0, -1, 0, -1, 0]
    label, degree, size, rep = sequence.threshold_clusters(r, 0.0, "dot")           # a zero row is valid under dot: 0 >= 0 everywhere
    assert list(label) == [0, 0, 0, -1, 0, -1, 0] and list(size) == [5, 5, 5, 0, 5, 0, 5] and degree[1] == 4


def test_edges_of_n_and_of_the_threshold():
    r = rows(9, 2)
    for n in (0, 1):
        out = sequence.threshold_clusters(r[:n], 0.5)
        assert all(a.dtype == np.int64 and a.shape == (n,) for a in out)
    assert [list(a) for a in sequence.threshold_clusters(r[:1], 0.5)] == [[0], [0], [1], [0]]
    label, degree, size, rep = sequence.threshold_clusters(r, 1.0)                  # above every similarity: all singletons
    assert list(label) == list(range(9)) == list(rep) and (degree == 0).all() and (size == 1).all()
    r[4] = 0
    label, degree, size, rep = sequence.threshold_clusters(r, -1.0)                 # one cluster of the valid rows
    ok = np.arange(9) != 4
    assert (label[ok] == 0).all() and (degree[ok] == 7).all() and (size[ok] == 8).all() and (rep[ok] == 0).all()
    assert (label[4], degree[4], size[4], rep[4]) == (-1, 0, 0, -1)
    for bad in (np.nan, np.inf, -np.inf, 1e39, "x"):
        with pytest.raises(ValueError, match="threshold"):
            sequence.threshold_clusters(r, bad)
    with pytest.raises(ValueError, match="metric"):
        sequence.threshold_clusters(r, 0.5, "euclid")
    with pytest.raises(ValueError, match="512"):
        sequence.threshold_clusters(r[:, :100], 0.5)


def path_rows():
    """rows whose dots draw a graph: 5 - 1 - 3 - 0 (a path), 2 - 4 (a pair), 6 alone; element e of a row is 1 iff the row is at edge e"""
    r = np.zeros((7, 512), np.float32)
    for e, (a, b) in enumerate([(5, 1), (1, 3), (3, 0), (2, 4)]):
        r[a, e] = r[b, e] = 1
    r[6, 9] = 1
    return r


def test_the_representative_has_the_most_edges_and_ties_go_to_the_lowest_index():
    label, degree, size, rep = sequence.threshold_clusters(path_rows(), 1.0, "dot")
    assert list(label) == [0, 0, 2, 0, 2, 0, 6] and list(degree) == [1, 2, 1, 2, 1, 1, 0]
    assert list(size) == [4, 4, 2, 4, 2, 4, 1]
    assert list(rep) == [1, 1, 2, 1, 2, 1, 6]                     # rows 1 and 3 have two edges each: 1; rows 2 and 4 one each: 2


def test_cluster_table():
    out = sequence.threshold_clusters(path_rows(), 1.0, "dot")
    want = [{"label": 0, "size": 4, "rep": 1, "members": [0, 1, 3, 5], "edges": 3}, {"label": 2, "size": 2, "rep": 2, "members": [2, 4], "edges": 1},
            {"label": 6, "size": 1, "rep": 6, "members": [6], "edges": 0}]
    assert sequence.cluster_table(out) == want
    assert sequence.cluster_table(dict(zip(sequence.CLUSTER_FIELDS, out))) == want
    res = ClusterResult.build(out, 1.0, "dot")
    assert res.table() == want and res.n_clusters == 3 and res.n_edges == 4 and res.threshold == 1.0 and res.metric == "dot"
    names = list("abcdefg")
    named = res.table(names)
    assert named[0] == {"label": "a", "size": 4, "rep": "b", "members": ["a", "b", "d", "f"], "edges": 3}
    r = path_rows()
    r[3, 0] = np.nan                                              # an invalid row belongs to no record
    tab = sequence.cluster_table(sequence.threshold_clusters(r, 1.0, "dot"))
    assert [c["members"] for c in tab] == [[0], [1, 5], [2, 4], [6]]
    assert sequence.cluster_table(sequence.threshold_clusters(r[:0], 1.0)) == []


def test_abi_declares_the_entry_points_and_checks_arguments_before_the_ctx():
    text = open(os.path.join(ROOT, "include", "genomad_nn.h")).read()
    lib = _lib.load()
    for name in ("gnn_cluster", "gnn_cluster_dev"):
        assert f"int {name}(" in text and name in _lib.SIGNATURES and hasattr(lib, name)
    assert "#define GNN_K_COUNT 8" in text
    for m in ("cluster", "cluster_dev"):
        assert hasattr(NNEngine, m)
    q = rows(2, 1)
    out = [np.full(2, 7, np.int64) for _ in range(4)]
    ptrs = [a.ctypes.data for a in out]
    for fn in (lib.gnn_cluster, lib.gnn_cluster_dev):
        name = b"gnn_cluster_dev" if fn is lib.gnn_cluster_dev else b"gnn_cluster:"
        for n in (-1, 1 << 31):
            assert fn(None, q.ctypes.data, n, 0.5, 0, *ptrs) == _lib.ERR_ARG
            assert f"{n} rows is outside [0, 2^31)".encode() in lib.gnn_last_error() and name in lib.gnn_last_error()
        for t, word in ((float("nan"), b"nan"), (float("inf"), b"inf"), (float("-inf"), b"-inf"), (1e39, b"inf")):
            assert fn(None, q.ctypes.data, 2, t, 0, *ptrs) == _lib.ERR_ARG
            assert b"threshold " + word in lib.gnn_last_error() and b"finite" in lib.gnn_last_error()
        for metric in (2, -1, 9):
            assert fn(None, q.ctypes.data, 2, 0.5, metric, *ptrs) == _lib.ERR_ARG
            assert f"metric {metric} is outside [0, 1]".encode() in lib.gnn_last_error()
        for hole in range(5):
            args = [q.ctypes.data] + ptrs
            args[hole] = None
            assert fn(None, args[0], 2, 0.5, 0, *args[1:]) == _lib.ERR_ARG
            assert b"the rows and the four outputs are required" in lib.gnn_last_error()
        assert fn(None, q.ctypes.data, 2, 0.5, 1, *ptrs) == _lib.ERR_ARG           # valid, but no ctx
        assert b"ctx is NULL" in lib.gnn_last_error()
        assert fn(None, None, 0, 0.5, 0, None, None, None, None) == _lib.ERR_ARG    # n = 0 needs no pointer, but a ctx
        assert b"ctx is NULL" in lib.gnn_last_error()
    assert all((a == 7).all() for a in out)                       # nothing was written


# ---- main() over a fake engine ---------------------------------------------------------------------------------------------------
class FakeClusterEngine(FakeNeighbourEngine):
    """the stand-in of tests/test_neighbours_host.py plus cluster, served from sequence.threshold_clusters"""
    calls = []

    def cluster(self, rows, threshold, metric="cosine"):
        type(self).calls.append(("cluster", len(rows), float(threshold), metric))
        return ClusterResult.build(sequence.threshold_clusters(rows, threshold, metric), threshold, metric)


@pytest.fixture
def fake_main(monkeypatch):
    monkeypatch.setattr(nnc, "_engine", lambda: FakeClusterEngine())
    for k in SWITCHES + ("GENOMAD_AMD_CLUSTERS",):
        monkeypatch.delenv(k, raising=False)
    del FakeClusterEngine.calls[:]
    return lambda fa, out, **kw: nnc.main(fa, out, False, 128, False, 1, False, False, **kw)


def test_cluster_switch_values(monkeypatch):
    monkeypatch.delenv("GENOMAD_AMD_CLUSTERS", raising=False)
    assert nnc.clusters_requested() is None
    for v, want in (("", None), (" 0.9 ", float(np.float32(0.9))), ("1", 1.0), ("-1", -1.0), ("0", 0.0), ("5e-1", 0.5)):
        monkeypatch.setenv("GENOMAD_AMD_CLUSTERS", v)
        assert nnc.clusters_requested() == want
    for v in ("1.01", "-1.5", "nan", "inf", "high", "0,9"):
        monkeypatch.setenv("GENOMAD_AMD_CLUSTERS", v)
        with pytest.raises(ValueError, match=r"GENOMAD_AMD_CLUSTERS.*\[-1, 1\]"):
            nnc.clusters_requested()


def test_main_refuses_the_switch_without_embeddings(tmp_path, monkeypatch, fake_main, capsys):
    fa = tmp_path / "s.fna"
    _write_fasta(fa, n=3)
    monkeypatch.setenv("GENOMAD_AMD_CLUSTERS", "1.5")
    with pytest.raises(ValueError, match="GENOMAD_AMD_CLUSTERS"):
        fake_main(fa, tmp_path / "bad")
    assert not (tmp_path / "bad").exists()                  # before anything is written
    monkeypatch.setenv("GENOMAD_AMD_CLUSTERS", "0.9")
    with pytest.raises(SystemExit) as exc:
        fake_main(fa, tmp_path / "refused")
    assert exc.value.code == 1
    err = capsys.readouterr().err
    assert "GENOMAD_AMD_CLUSTERS needs GENOMAD_AMD_EMBEDDINGS=1" in err and len(err.strip().splitlines()) == 1
    assert not list((tmp_path / "refused").rglob("*.npz")) and not list((tmp_path / "refused").rglob("*.tsv"))
    assert FakeClusterEngine.calls == []


def test_main_writes_both_files_follows_the_threshold_and_removes_stale_ones(tmp_path, monkeypatch, fake_main):
    fa = tmp_path / "m.fna"
    recs = _write_fasta(fa, n=6)
    with open(fa, "a") as f:
        f.write(f">twin of c2\n{dict(recs)['c2']}\n")        # the same bytes as c2: the same embedding
    monkeypatch.setenv("GENOMAD_AMD_EMBEDDINGS", "1")
    fake_main(fa, tmp_path / "unset")
    assert not any(c[0] == "cluster" for c in FakeClusterEngine.calls)
    monkeypatch.setenv("GENOMAD_AMD_CLUSTERS", "0.999")
    out = tmp_path / "on"
    fake_main(fa, out)
    d0, d1 = tmp_path / "unset" / "m_nn_classification", out / "m_nn_classification"
    assert _tree(d1) == sorted(_tree(d0) + ["m_nn_clusters.npz", "m_nn_clusters.tsv"])
    for rel in _tree(d0):                                   # every other output: the same arrays, the same bytes
        if rel.endswith(".npz"):
            assert _same_npz(d0 / rel, d1 / rel), rel
        elif rel.endswith(".tsv"):
            assert (d0 / rel).read_bytes() == (d1 / rel).read_bytes(), rel
    z, emb = _npz(d1 / "m_nn_clusters.npz"), _npz(d1 / "m_nn_embeddings.npz")
    n = len(emb["contig_names"])
    t32 = float(np.float32(0.999))
    assert sorted(z) == ["contig_names", "degree", "label", "metric", "rep", "size", "threshold"]
    assert list(z["contig_names"]) == list(emb["contig_names"])
    assert float(z["threshold"]) == t32 and z["threshold"].dtype == np.float64 and str(z["metric"]) == "cosine"
    assert FakeClusterEngine.calls.count(("cluster", n, t32, "cosine")) == 1
    want = sequence.threshold_clusters(emb["embeddings"], 0.999)
    assert same([z[k] for k in sequence.CLUSTER_FIELDS], want)
    names = list(z["contig_names"])
    a, b = sorted((names.index("c2"), names.index("twin")))
    assert z["label"][a] == z["label"][b] == a and z["size"][a] == z["size"][b] == 2 and z["degree"][a] == z["degree"][b] == 1
    assert z["rep"][a] == z["rep"][b] == a
    lines = (d1 / "m_nn_clusters.tsv").read_text().splitlines()
    assert lines[0] == "seq_name\tcluster\tcluster_size\trepresentative\tdegree" and len(lines) == n + 1
    for i, line in enumerate(lines[1:]):
        assert line == f"{names[i]}\t{names[z['label'][i]]}\t{z['size'][i]}\t{names[z['rep'][i]]}\t{z['degree'][i]}"
    assert lines[1 + b] == f"{names[b]}\t{names[a]}\t2\t{names[a]}\t1"
    runs = lambda: sum(1 for c in FakeClusterEngine.calls if c == "plain")       # noqa: E731
    before = runs()
    fake_main(fa, out)
    assert runs() == before                                  # same request, everything there: nothing runs
    monkeypatch.setenv("GENOMAD_AMD_CLUSTERS", "-1")
    fake_main(fa, out)                                       # another threshold: recomputed
    z = _npz(d1 / "m_nn_clusters.npz")
    assert runs() == before + 1 and float(z["threshold"]) == -1.0 and (z["label"] == 0).all() and (z["size"] == n).all()
    (d1 / "m_nn_clusters.tsv").unlink()
    fake_main(fa, out)                                       # one of the pair is gone: recomputed
    assert runs() == before + 2 and (d1 / "m_nn_clusters.tsv").exists()
    monkeypatch.delenv("GENOMAD_AMD_CLUSTERS")
    fake_main(fa, out)                                       # no request: both files go
    assert runs() == before + 3 and not (d1 / "m_nn_clusters.npz").exists() and not (d1 / "m_nn_clusters.tsv").exists()
    assert _tree(d1) == _tree(d0)
    monkeypatch.setenv("GENOMAD_AMD_CLUSTERS", "0.5")
    monkeypatch.setenv("GENOMAD_AMD_NEIGHBOURS", "2")        # both searches in one run
    monkeypatch.setenv("GENOMAD_AMD_STRAND", "both")
    FakeClusterEngine.classify_contigs_strand = lambda self, seq, offsets, strand="both", single_window=False, precision=None, embed=False: (
        lambda r: (r[0], r[1], FakeClusterEngine.embed_contigs(self, seq, offsets)[1], r[3], r[4]))(
            FakeStrandEngine.classify_contigs_strand(self, seq, offsets, strand, single_window, precision, embed))
    try:
        fake_main(fa, out)
    finally:
        del FakeClusterEngine.classify_contigs_strand
    assert str(_npz(d1 / "m_nn_clusters.npz")["strand"]) == "both" and str(_npz(d1 / "m_nn_neighbours.npz")["strand"]) == "both"


def test_a_contig_without_a_valid_embedding_is_na_in_the_table(tmp_path):
    res = ClusterResult.build(sequence.threshold_clusters(np.concatenate([rows(2, 3), np.zeros((1, 512), np.float32)]), -1.0), -1.0, "cosine")
    nnc.write_clusters_tsv(tmp_path / "t.tsv", ["a", "b", "c"], res)
    assert (tmp_path / "t.tsv").read_text() == ("seq_name\tcluster\tcluster_size\trepresentative\tdegree\n"
                                                "a\ta\t2\ta\t1\nb\ta\t2\ta\t1\nc\tNA\t0\tNA\t0\n")
