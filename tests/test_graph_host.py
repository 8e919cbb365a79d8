"""The similarity graph among encoder embeddings without a GPU: the numpy definition (sequence.threshold_graph) against a brute-force
double loop and against the adjacency of the cluster tests, GraphResult's views (degree and components are what threshold_clusters
returns, symmetric round-trips, edges and table), the ABI's argument checks (before the ctx is looked at: no GPU needed), and main()'s
GENOMAD_AMD_GRAPH switch over a fake engine served from the definition."""
import os

import numpy as np
import pytest

from genomad_amd import _lib, nn_classification as nnc, sequence
from genomad_amd.engine import GraphResult, NNEngine
from tests.clusters_data import THRESHOLDS, device_edges, planted, sims64
from tests.neighbours_data import rows
from tests.test_clusters_host import FakeClusterEngine, integer_rows, path_rows
from tests.test_neighbours_host import SWITCHES
from tests.test_strand_host import _npz, _same_npz, _tree, _write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def result(r, threshold, metric="cosine"):
    return GraphResult.build(sequence.threshold_graph(r, threshold, metric), sequence.valid_rows(r, metric), threshold, metric)


def csr_of(adj):
    """the upper triangle of a symmetric adjacency as (indptr, col)"""
    upper = np.triu(np.asarray(adj, bool), 1)
    return np.concatenate([[0], np.cumsum(upper.sum(axis=1))]).astype(np.int64), np.nonzero(upper)[1].astype(np.int32)


def rows_with_invalid():
    r = rows(40, 6)
    r[20:26] = r[2] + np.float32(0.1) * r[20:26]              # a family around row 2
    r[5] = 0
    r[17, 3] = np.nan
    r[33, 500] = -np.inf
    return r


@pytest.mark.parametrize("metric", ("cosine", "dot"))
def test_definition_equals_a_double_loop_with_invalid_rows(metric):
    r = rows_with_invalid()
    x = r.astype(np.float64)
    ok = [bool(np.isfinite(v).all() and (metric == "dot" or np.sqrt((v * v).sum()) > 0)) for v in x]
    if metric == "cosine":
        x = np.stack([v / np.sqrt((v * v).sum()) if o else v for v, o in zip(x, ok)])
    good = rows(40, 6)
    thr = 0.5 if metric == "cosine" else float(np.median(sims64(good, good, "dot")[np.triu_indices(40, 1)]))     # about half the pairs
    t32 = float(np.float32(thr))
    ptr, col, sim = [0], [], []
    for i in range(40):
        for j in range(i + 1, 40):
            if ok[i] and ok[j] and (float(x[i] @ x[j]) >= t32 or float(x[j] @ x[i]) >= t32):
                col.append(j)
                sim.append(float(x[i] @ x[j]))
        ptr.append(len(col))
    indptr, c, s = sequence.threshold_graph(r, thr, metric)
    assert indptr.dtype == np.int64 and c.dtype == np.int32 and s.dtype == np.float64
    assert list(indptr) == ptr and list(c) == col and len(col) > 10
    assert np.allclose(s, sim, rtol=1e-12, atol=1e-12)
    for bad in (5, 17, 33) if metric == "cosine" else (17, 33):
        assert indptr[bad] == indptr[bad + 1] and bad not in col
    assert list(sequence.valid_rows(r, metric)) == ok


@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_definition_has_the_adjacency_of_the_cluster_tests(threshold):
    r, _ = planted()
    s64 = sims64(r, r)
    indptr, col, sim = sequence.threshold_graph(r, threshold)
    want_ptr, want_col = csr_of(device_edges(s64, float(np.float32(threshold))))
    assert np.array_equal(indptr, want_ptr) and np.array_equal(col, want_col)
    a, _ = sequence.graph_edges(indptr, col)
    assert np.abs(sim - s64[a, col]).max() < 1e-12


@pytest.mark.parametrize("case", ("planted0.8", "planted0.9", "integer", "invalid", "path"))
def test_degree_and_components_are_those_of_threshold_clusters(case):
    if case.startswith("planted"):
        r, thr, metric = planted()[0], float(case[7:]), "cosine"
    elif case == "integer":
        r, metric = integer_rows(), "dot"
        thr = float(np.median(sims64(r, r, "dot")[np.triu_indices(200, 1)]))
    elif case == "invalid":
        r, thr, metric = rows_with_invalid(), 0.3, "cosine"
    else:
        r, thr, metric = path_rows(), 1.0, "dot"
    res = result(r, thr, metric)
    label, degree, _, _ = sequence.threshold_clusters(r, thr, metric)
    assert res.degree().dtype == np.int64 and np.array_equal(res.degree(), degree)
    assert res.components().dtype == np.int64 and np.array_equal(res.components(), label)
    assert res.n == len(r) and res.n_edges == int(degree.sum()) // 2 == len(res.col)
    assert res.threshold == float(np.float32(thr)) and res.metric == metric


def test_symmetric_round_trips():
    r, _ = planted()
    res = result(r, 0.8)
    full_ptr, full_col, full_sim = res.symmetric()
    assert full_ptr.dtype == np.int64 and full_col.dtype == np.int32 and full_sim.dtype == res.sim.dtype
    assert np.array_equal(np.diff(full_ptr), res.degree()) and len(full_col) == 2 * res.n_edges
    dense = np.zeros((res.n, res.n))
    a, b, s = res.edges()
    dense[a, b] = dense[b, a] = s
    for i in range(res.n):
        seg = slice(full_ptr[i], full_ptr[i + 1])
        assert np.array_equal(full_col[seg], np.flatnonzero(dense[i])) and np.array_equal(full_sim[seg], dense[i][dense[i] != 0])
    keep = full_col > np.repeat(np.arange(res.n), np.diff(full_ptr))          # the upper triangle of the full CSR is the result
    assert np.array_equal(full_col[keep], res.col) and np.array_equal(full_sim[keep], res.sim)
    empty = result(r[:0], 0.8)
    assert [len(x) for x in empty.symmetric()] == [1, 0, 0] and list(empty.indptr) == [0] and empty.n == 0 and empty.n_edges == 0


def test_edges_and_table_give_the_expected_records():
    res = result(path_rows(), 1.0, "dot")                         # 5 - 1 - 3 - 0, 2 - 4, 6 alone
    a, b, s = res.edges()
    assert a.dtype == np.int64 and b.dtype == np.int64
    assert list(zip(a, b)) == [(0, 3), (1, 3), (1, 5), (2, 4)] and list(s) == [1.0] * 4
    assert list(res.indptr) == [0, 1, 3, 4, 4, 4, 4, 4] and res.col.dtype == np.int32
    assert res.table() == [{"a": 0, "b": 3, "sim": 1.0}, {"a": 1, "b": 3, "sim": 1.0}, {"a": 1, "b": 5, "sim": 1.0},
                           {"a": 2, "b": 4, "sim": 1.0}]
    assert res.table(list("abcdefg"))[2] == {"a": "b", "b": "f", "sim": 1.0}
    assert sorted(res.asdict()) == sorted(GraphResult.FIELDS) and list(res.valid) == [True] * 7
    for bad in (np.nan, np.inf, "x"):
        with pytest.raises(ValueError, match="threshold"):
            sequence.threshold_graph(path_rows(), bad)
    with pytest.raises(ValueError, match="metric"):
        sequence.threshold_graph(path_rows(), 0.5, "euclid")


def test_abi_declares_the_entry_points_and_checks_arguments_before_the_ctx():
    text = open(os.path.join(ROOT, "include", "genomad_nn.h")).read()
    lib = _lib.load()
    names = ("gnn_graph_count", "gnn_graph_fill", "gnn_graph_count_dev", "gnn_graph_fill_dev")
    for name in names:
        assert f"int {name}(" in text and name in _lib.SIGNATURES and hasattr(lib, name)
    for m in ("graph", "graph_count_dev", "graph_fill_dev"):
        assert hasattr(NNEngine, m)
    assert "gnn_graph" in open(os.path.join(ROOT, "genomad_amd", "csrc", "build.sh")).read()
    q = rows(2, 1)
    indptr, nnz, col, sim = np.full(3, 7, np.int64), np.full(1, 7, np.int64), np.full(4, 7, np.int32), np.full(4, 7, np.float32)
    calls = {"gnn_graph_count": lambda n, t, m: lib.gnn_graph_count(None, q.ctypes.data, n, t, m, indptr.ctypes.data, nnz.ctypes.data),
             "gnn_graph_count_dev": lambda n, t, m: lib.gnn_graph_count_dev(None, q.ctypes.data, n, t, m, indptr.ctypes.data, nnz.ctypes.data),
             "gnn_graph_fill": lambda n, t, m: lib.gnn_graph_fill(None, n, t, m, col.ctypes.data, sim.ctypes.data, 4),
             "gnn_graph_fill_dev": lambda n, t, m: lib.gnn_graph_fill_dev(None, q.ctypes.data, n, t, m, col.ctypes.data, sim.ctypes.data, 4)}
    for name in names:
        fn = calls[name]
        for n in (-1, 1 << 31):
            assert fn(n, 0.5, 0) == _lib.ERR_ARG
            assert f"{name}: {n} rows is outside [0, 2^31)".encode() in lib.gnn_last_error()
        for t, word in ((float("nan"), b"nan"), (float("inf"), b"inf"), (float("-inf"), b"-inf"), (1e39, b"inf")):
            assert fn(2, t, 0) == _lib.ERR_ARG
            assert name.encode() + b": threshold " + word in lib.gnn_last_error() and b"finite" in lib.gnn_last_error()
        for metric in (2, -1, 9):
            assert fn(2, 0.5, metric) == _lib.ERR_ARG
            assert f"{name}: metric {metric} is outside [0, 1]".encode() in lib.gnn_last_error()
        assert fn(2, 0.5, 1) == _lib.ERR_ARG                      # valid, but no ctx
        assert b"ctx is NULL" in lib.gnn_last_error()
    for fn in (lib.gnn_graph_count, lib.gnn_graph_count_dev):
        for hole in range(3):
            args = [q.ctypes.data, indptr.ctypes.data, nnz.ctypes.data]
            args[hole] = None
            assert fn(None, args[0], 2, 0.5, 0, args[1], args[2]) == _lib.ERR_ARG
            assert b"the rows, indptr and nnz are required" in lib.gnn_last_error()
    assert all((a == 7).all() for a in (indptr, nnz, col, sim))   # nothing was written


# ---- main() over a fake engine ---------------------------------------------------------------------------------------------------
class FakeGraphEngine(FakeClusterEngine):
    """the stand-in of tests/test_clusters_host.py plus graph, served from sequence.threshold_graph"""

    def graph(self, rows, threshold, metric="cosine", max_edges=1 << 28):
        type(self).calls.append(("graph", len(rows), float(threshold), metric))
        indptr, col, sim = sequence.threshold_graph(rows, threshold, metric)
        if len(col) > type(self).cap:
            raise ValueError(f"the graph has {len(col)} edges at the threshold {float(np.float32(threshold)):g}, more than max_edges = "
                             f"{type(self).cap}: raise the threshold or max_edges")
        return GraphResult.build((indptr, col, sim.astype(np.float32)), sequence.valid_rows(rows, metric), threshold, metric)


@pytest.fixture
def fake_main(monkeypatch):
    monkeypatch.setattr(nnc, "_engine", lambda: FakeGraphEngine())
    for k in SWITCHES + ("GENOMAD_AMD_CLUSTERS", "GENOMAD_AMD_REPRESENTATIVES", "GENOMAD_AMD_LINKAGE", "GENOMAD_AMD_GRAPH"):
        monkeypatch.delenv(k, raising=False)
    del FakeGraphEngine.calls[:]
    FakeGraphEngine.cap = 1 << 28
    return lambda fa, out, **kw: nnc.main(fa, out, False, 128, False, 1, False, False, **kw)


def test_graph_switch_values(monkeypatch):
    monkeypatch.delenv("GENOMAD_AMD_GRAPH", raising=False)
    assert nnc.graph_requested() is None
    for v, want in (("", None), (" 0.9 ", float(np.float32(0.9))), ("1", 1.0), ("-1", -1.0), ("0", 0.0), ("5e-1", 0.5)):
        monkeypatch.setenv("GENOMAD_AMD_GRAPH", v)
        assert nnc.graph_requested() == want
    for v in ("1.01", "-1.5", "nan", "inf", "high", "0,9"):
        monkeypatch.setenv("GENOMAD_AMD_GRAPH", v)
        with pytest.raises(ValueError, match=r"GENOMAD_AMD_GRAPH.*\[-1, 1\]"):
            nnc.graph_requested()


def test_the_tsv_writer_writes_one_line_per_edge(tmp_path):
    r = np.concatenate([path_rows(), np.zeros((1, 512), np.float32)])
    r[1, 1] = 0.5                                                 # 1 . 3 = 0.5; the zero row is valid under dot and joins nobody
    res = result(r, 0.4, "dot")
    res.sim = res.sim.astype(np.float32)
    nnc.write_graph_tsv(tmp_path / "g.tsv", list("abcdefgh"), res)
    assert (tmp_path / "g.tsv").read_text() == ("contig_a\tcontig_b\tsimilarity\n"
                                                "a\td\t1.000000\nb\td\t0.500000\nb\tf\t1.000000\nc\te\t1.000000\n")
    nnc.write_graph_tsv(tmp_path / "e.tsv", [], result(r[:0], 0.4))
    assert (tmp_path / "e.tsv").read_text() == "contig_a\tcontig_b\tsimilarity\n"


def test_main_refuses_the_switch_without_embeddings(tmp_path, monkeypatch, fake_main, capsys):
    fa = tmp_path / "s.fna"
    _write_fasta(fa, n=3)
    monkeypatch.setenv("GENOMAD_AMD_GRAPH", "1.5")
    with pytest.raises(ValueError, match="GENOMAD_AMD_GRAPH"):
        fake_main(fa, tmp_path / "bad")
    assert not (tmp_path / "bad").exists()                  # before anything is written
    monkeypatch.setenv("GENOMAD_AMD_GRAPH", "0.9")
    with pytest.raises(SystemExit) as exc:
        fake_main(fa, tmp_path / "refused")
    assert exc.value.code == 1
    err = capsys.readouterr().err
    assert "GENOMAD_AMD_GRAPH needs GENOMAD_AMD_EMBEDDINGS=1" in err and len(err.strip().splitlines()) == 1
    assert FakeGraphEngine.calls == []


def test_main_writes_both_files_follows_the_threshold_and_removes_stale_ones(tmp_path, monkeypatch, fake_main, capsys):
    fa = tmp_path / "m.fna"
    recs = _write_fasta(fa, n=6)
    with open(fa, "a") as f:
        f.write(f">twin of c2\n{dict(recs)['c2']}\n")        # the same bytes as c2: the same embedding
    monkeypatch.setenv("GENOMAD_AMD_EMBEDDINGS", "1")
    fake_main(fa, tmp_path / "unset")
    assert not any(c[0] == "graph" for c in FakeGraphEngine.calls)
    monkeypatch.setenv("GENOMAD_AMD_GRAPH", "0.999")
    out = tmp_path / "on"
    fake_main(fa, out)
    d0, d1 = tmp_path / "unset" / "m_nn_classification", out / "m_nn_classification"
    assert _tree(d1) == sorted(_tree(d0) + ["m_nn_graph.npz", "m_nn_graph.tsv"])
    for rel in _tree(d0):                                   # every other output: the same arrays, the same bytes
        if rel.endswith(".npz"):
            assert _same_npz(d0 / rel, d1 / rel), rel
        elif rel.endswith(".tsv"):
            assert (d0 / rel).read_bytes() == (d1 / rel).read_bytes(), rel
    z, emb = _npz(d1 / "m_nn_graph.npz"), _npz(d1 / "m_nn_embeddings.npz")
    n = len(emb["contig_names"])
    t32 = float(np.float32(0.999))
    assert sorted(z) == ["col", "contig_names", "indptr", "metric", "sim", "threshold"]
    assert list(z["contig_names"]) == list(emb["contig_names"])
    assert float(z["threshold"]) == t32 and z["threshold"].dtype == np.float64 and str(z["metric"]) == "cosine"
    assert FakeGraphEngine.calls.count(("graph", n, t32, "cosine")) == 1
    indptr, col, sim = sequence.threshold_graph(emb["embeddings"], 0.999)
    assert z["indptr"].dtype == np.int64 and z["col"].dtype == np.int32 and z["sim"].dtype == np.float32
    assert np.array_equal(z["indptr"], indptr) and np.array_equal(z["col"], col) and np.array_equal(z["sim"], sim.astype(np.float32))
    names = list(z["contig_names"])
    a, b = sorted((names.index("c2"), names.index("twin")))
    assert b in z["col"][z["indptr"][a]:z["indptr"][a + 1]]
    lines = (d1 / "m_nn_graph.tsv").read_text().splitlines()
    assert lines[0] == "contig_a\tcontig_b\tsimilarity" and len(lines) == len(col) + 1
    rows_of = np.repeat(np.arange(n), np.diff(indptr))
    for e, line in enumerate(lines[1:]):
        assert line == f"{names[rows_of[e]]}\t{names[col[e]]}\t{np.float32(sim[e]):.6f}"
    assert f"{names[a]}\t{names[b]}\t1.000000" in lines
    runs = lambda: sum(1 for c in FakeGraphEngine.calls if c == "plain")       # noqa: E731
    before = runs()
    fake_main(fa, out)
    assert runs() == before                                  # same request, everything there: nothing runs
    monkeypatch.setenv("GENOMAD_AMD_GRAPH", "-1")
    fake_main(fa, out)                                       # another threshold: recomputed
    z = _npz(d1 / "m_nn_graph.npz")
    assert runs() == before + 1 and float(z["threshold"]) == -1.0 and len(z["col"]) == n * (n - 1) // 2
    (d1 / "m_nn_graph.tsv").unlink()
    fake_main(fa, out)                                       # one of the pair is gone: recomputed
    assert runs() == before + 2 and (d1 / "m_nn_graph.tsv").exists()
    FakeGraphEngine.cap = 3                                  # too many edges: a console error that names the variable
    (d1 / "m_nn_graph.tsv").unlink()
    capsys.readouterr()
    with pytest.raises(SystemExit) as exc:
        fake_main(fa, out)
    err = capsys.readouterr().err
    assert exc.value.code == 1 and "GENOMAD_AMD_GRAPH=-1" in err and f"{n * (n - 1) // 2} edges" in err and "max_edges = 3" in err
    FakeGraphEngine.cap = 1 << 28
    monkeypatch.delenv("GENOMAD_AMD_GRAPH")
    fake_main(fa, out)                                       # no request: both files go
    assert not (d1 / "m_nn_graph.npz").exists() and not (d1 / "m_nn_graph.tsv").exists()
    assert _tree(d1) == _tree(d0)
    monkeypatch.setenv("GENOMAD_AMD_GRAPH", "0.5")
    monkeypatch.setenv("GENOMAD_AMD_CLUSTERS", "0.5")        # both searches in one run: the graph's edges are the clusters'
    fake_main(fa, out)
    z, c = _npz(d1 / "m_nn_graph.npz"), _npz(d1 / "m_nn_clusters.npz")
    res = GraphResult.build((z["indptr"], z["col"], z["sim"]), c["label"] >= 0, 0.5, "cosine")
    assert np.array_equal(res.degree(), c["degree"]) and np.array_equal(res.components(), c["label"])
