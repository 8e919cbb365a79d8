"""Matches against a reference without a GPU: the numpy definition (sequence.threshold_matches) against a brute-force double loop,
sequence.graph_extend on the definition's own outputs against the graph of the concatenation, MatchResult's views on a hand-made CSR,
the ABI's argument checks (before the ctx is looked at: no GPU needed), and main()'s GENOMAD_AMD_MATCH / GENOMAD_AMD_MATCH_BASE
switches over a fake engine served from the definition."""
import os

import numpy as np
import pytest

from genomad_amd import _lib, nn_classification as nnc, sequence
from genomad_amd.engine import GraphResult, MatchResult, NNEngine
from tests.clusters_data import THRESHOLDS, planted
from tests.neighbours_data import rows, sims64
from tests.test_graph_host import FakeGraphEngine
from tests.test_neighbours_host import SWITCHES
from tests.test_strand_host import _npz, _same_npz, _tree, _write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATCH_SWITCHES = ("GENOMAD_AMD_MATCH", "GENOMAD_AMD_MATCH_BASE")


def graph_result(r, threshold, metric="cosine"):
    return GraphResult.build(sequence.threshold_graph(r, threshold, metric), sequence.valid_rows(r, metric), threshold, metric)


def match_result(q, b, threshold, metric="cosine"):
    return MatchResult.build(sequence.threshold_matches(q, b, threshold, metric), sequence.valid_rows(q, metric),
                             sequence.valid_rows(b, metric), threshold, metric)


def two_sides():
    """40 queries and 30 base rows with a family across both, and a zero, a NaN and an inf row on each side"""
    q, b = rows(40, 6), rows(30, 6)[::-1].copy()
    b[10:16] = q[2] + np.float32(0.1) * b[10:16]              # a family around query 2
    q[20:23] = q[2] + np.float32(0.1) * q[20:23]
    q[5] = 0
    q[17, 3] = np.nan
    q[33, 500] = -np.inf
    b[4] = 0
    b[21, 9] = np.inf
    b[29, 0] = np.nan
    return q, b


@pytest.mark.parametrize("metric", ("cosine", "dot"))
def test_definition_equals_a_double_loop_with_invalid_rows_on_both_sides(metric):
    q, b = two_sides()

    def prepared(r):
        x = r.astype(np.float64)
        ok = [bool(np.isfinite(v).all() and (metric == "dot" or np.sqrt((v * v).sum()) > 0)) for v in x]
        if metric == "cosine":
            x = np.stack([v / np.sqrt((v * v).sum()) if o else v for v, o in zip(x, ok)])
        return x, ok

    (x, x_ok), (y, y_ok) = prepared(q), prepared(b)
    thr = 0.5 if metric == "cosine" else float(np.median(sims64(rows(40, 6), rows(30, 6), "dot")))     # about half the pairs
    t32 = float(np.float32(thr))
    ptr, col, sim = [0], [], []
    for i in range(40):
        for j in range(30):
            if x_ok[i] and y_ok[j] and float(x[i] @ y[j]) >= t32:
                col.append(j)
                sim.append(float(x[i] @ y[j]))
        ptr.append(len(col))
    indptr, c, s = sequence.threshold_matches(q, b, thr, metric)
    assert indptr.dtype == np.int64 and c.dtype == np.int32 and s.dtype == np.float64
    assert list(indptr) == ptr and list(c) == col and len(col) > 10
    assert np.allclose(s, sim, rtol=1e-12, atol=1e-12)
    for bad in (5, 17, 33) if metric == "cosine" else (17, 33):
        assert indptr[bad] == indptr[bad + 1]
    for bad in (4, 21, 29) if metric == "cosine" else (21, 29):
        assert bad not in col
    if metric == "dot":                                       # a zero row is valid under dot: 0 >= a threshold <= 0 matches
        ip0, c0, _ = sequence.threshold_matches(q, b, 0.0, "dot")
        assert ip0[6] - ip0[5] == 28 and (c0 == 4).sum() == 38
    for bad in (np.nan, np.inf, "x"):
        with pytest.raises(ValueError, match="threshold"):
            sequence.threshold_matches(q, b, bad)
    with pytest.raises(ValueError, match="metric"):
        sequence.threshold_matches(q, b, 0.5, "euclid")
    with pytest.raises(ValueError, match="base has the shape"):
        sequence.threshold_matches(q, b[:, :5], 0.5)
    same = sequence.threshold_matches(rows(9, 3), rows(9, 3), -1.0)       # the same rows: (i, i) and both orientations
    assert list(same[0]) == list(range(0, 82, 9)) and list(same[1]) == list(range(9)) * 9


@pytest.mark.parametrize("cut", (200, 0, 1, 333))
@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_graph_extend_on_the_definition_is_the_graph_of_all_rows(threshold, cut):
    r, _ = planted()
    old, new = graph_result(r[:cut], threshold), graph_result(r[cut:], threshold)
    cross = match_result(r[:cut], r[cut:], threshold)
    both, whole = old.extend(cross, new), graph_result(r, threshold)
    assert both.indptr.dtype == np.int64 and both.col.dtype == np.int32 and both.sim.dtype == np.float64
    assert np.array_equal(both.indptr, whole.indptr) and np.array_equal(both.col, whole.col)
    assert len(whole.sim) == 0 or np.abs(both.sim - whole.sim).max() <= 1e-12
    assert both.n == 333 and both.n_edges == whole.n_edges and np.array_equal(both.valid, whole.valid)
    assert both.threshold == whole.threshold and both.metric == "cosine"
    assert np.array_equal(both.components(), sequence.threshold_clusters(r, threshold)[0])       # new rows in old clusters
    arrays = sequence.graph_extend((old.indptr, old.col, old.sim), (cross.indptr, cross.col, cross.sim), (new.indptr, new.col, new.sim))
    assert all(np.array_equal(a, b) for a, b in zip(arrays, (both.indptr, both.col, both.sim)))


def test_graph_extend_refuses_every_mismatch():
    r, _ = planted()
    old, new, cross = graph_result(r[:200], 0.8), graph_result(r[200:], 0.8), match_result(r[:200], r[200:], 0.8)
    with pytest.raises(ValueError, match=r"199 x 133.*200 and 133 rows"):
        old.extend(match_result(r[:199], r[200:], 0.8), new)
    with pytest.raises(ValueError, match=r"200 x 132.*200 and 133 rows"):
        old.extend(match_result(r[:200], r[201:], 0.8), new)
    with pytest.raises(ValueError, match=r"200 x 133.*200 and 132 rows"):
        old.extend(cross, graph_result(r[201:], 0.8))
    with pytest.raises(ValueError, match="thresholds .* differ"):
        old.extend(match_result(r[:200], r[200:], 0.9), new)
    with pytest.raises(ValueError, match="thresholds .* differ"):
        old.extend(cross, graph_result(r[200:], np.nextafter(np.float32(0.8), np.float32(1))))    # one bit
    with pytest.raises(ValueError, match="metrics .* differ"):
        old.extend(match_result(r[:200], r[200:], 0.8, "dot"), new)
    with pytest.raises(ValueError, match="metrics .* differ"):
        graph_result(r[:200], 0.8, "dot").extend(cross, new)
    triple = lambda x: (x.indptr, x.col, x.sim)          # noqa: E731
    with pytest.raises(ValueError, match="199 query rows, the old graph 200 rows"):
        sequence.graph_extend(triple(old), triple(match_result(r[:199], r[200:], 0.8)), triple(new))
    with pytest.raises(ValueError, match=r"base row \d+, the new graph has 20 rows"):
        sequence.graph_extend(triple(old), triple(cross), triple(graph_result(r[200:220], 0.8)))
    assert old.extend(cross, new).n == 333                    # the matching pieces pass


def hand_made():
    """4 queries x 5 base rows: query 0 -> {1: .5, 3: .9, 4: .9}, query 1 -> {}, query 2 -> {0: .7}, query 3 -> {0: .6, 3: .6}"""
    indptr = np.array([0, 3, 3, 4, 6], np.int64)
    col = np.array([1, 3, 4, 0, 0, 3], np.int32)
    sim = np.array([.5, .9, .9, .7, .6, .6], np.float32)
    return MatchResult.build((indptr, col, sim), [True, False, True, True], [True, True, False, True, True], 0.5, "cosine")


def test_views_of_a_hand_made_result():
    res = hand_made()
    assert (res.n_query, res.n_base, res.n_edges, res.threshold, res.metric) == (4, 5, 6, 0.5, "cosine")
    assert sorted(res.asdict()) == sorted(MatchResult.FIELDS) and res.query_valid.dtype == bool and res.base_valid.dtype == bool
    a, b, s = res.edges()
    assert a.dtype == np.int64 and b.dtype == np.int64 and list(zip(a, b)) == [(0, 1), (0, 3), (0, 4), (2, 0), (3, 0), (3, 3)] and s is res.sim
    assert res.hits().dtype == np.int64 and list(res.hits()) == [3, 0, 1, 2]
    assert res.base_hits().dtype == np.int64 and list(res.base_hits()) == [2, 1, 0, 2, 1]
    idx, best = res.best()
    assert idx.dtype == np.int64 and best.dtype == np.float32
    assert list(idx) == [3, -1, 0, 0] and list(best[[0, 2, 3]]) == list(np.float32([.9, .7, .6])) and np.isnan(best[1])     # ties: the smaller
    t_ptr, t_col, t_sim = res.transpose()
    assert t_ptr.dtype == np.int64 and t_col.dtype == np.int32 and t_sim.dtype == np.float32
    assert list(t_ptr) == [0, 2, 3, 3, 5, 6] and list(t_col) == [2, 3, 0, 0, 3, 0]
    assert list(t_sim) == list(np.float32([.7, .6, .5, .9, .6, .9]))
    back = sequence.match_transpose(t_ptr, t_col, t_sim, 4)                  # transposing twice is the identity
    assert all(np.array_equal(x, y) for x, y in zip(back, (res.indptr, res.col, res.sim)))
    assert res.table()[1] == {"query": 0, "base": 3, "sim": float(np.float32(.9))} and len(res.table()) == 6
    assert res.table(list("wxyz"), list("abcde"))[3] == {"query": "y", "base": "a", "sim": float(np.float32(.7))}
    assert res.table(None, list("abcde"))[5]["base"] == "d" and res.table(None, list("abcde"))[5]["query"] == 3
    with pytest.raises(ValueError, match="beyond the 3 base rows"):
        sequence.match_transpose(res.indptr, res.col, res.sim, 3)
    with pytest.raises(ValueError, match="query_valid has 3 flags"):
        MatchResult.build((res.indptr, res.col, res.sim), [True] * 3, [True] * 5, 0.5, "cosine")
    empty = match_result(rows(0, 1), rows(7, 1), 0.5)
    assert list(empty.indptr) == [0] and empty.n_edges == 0 and list(empty.base_hits()) == [0] * 7 and len(empty.best()[0]) == 0
    assert [len(x) for x in empty.transpose()] == [8, 0, 0]
    none = match_result(rows(3, 1), rows(0, 1), 0.5)
    assert list(none.indptr) == [0] * 4 and list(none.best()[0]) == [-1] * 3 and none.n_base == 0 and list(none.transpose()[0]) == [0]


def test_best_is_the_nearest_neighbour_wherever_it_reaches_the_threshold():
    q, b = two_sides()
    idx, sim = sequence.nearest_neighbours(q, b, 1)
    res = match_result(q, b, 0.5)
    best_idx, best_sim = res.best()
    keep = sim[:, 0] >= np.float32(0.5)                               # NaN (an invalid query) fails it
    assert keep.any() and not keep.all()
    assert np.array_equal(best_idx, np.where(keep, idx[:, 0], -1))
    assert np.allclose(best_sim[keep], sim[keep, 0], rtol=0, atol=1e-6) and np.isnan(best_sim[~keep]).all()


def test_abi_declares_the_entry_points_and_checks_arguments_before_the_ctx():
    text = open(os.path.join(ROOT, "include", "genomad_nn.h")).read()
    lib = _lib.load()
    names = ("gnn_match_count", "gnn_match_fill", "gnn_match_count_dev", "gnn_match_fill_dev")
    for name in names + ("gnn_debug_match_pass_ms",):
        assert f"int {name}(" in text and name in _lib.SIGNATURES and hasattr(lib, name)
    for m in ("match", "match_count_dev", "match_fill_dev", "match_pass_ms"):
        assert hasattr(NNEngine, m)
    q = rows(2, 1)
    indptr, nnz, col, sim = np.full(3, 7, np.int64), np.full(1, 7, np.int64), np.full(4, 7, np.int32), np.full(4, 7, np.float32)
    qp, ip, zp, cp, sp = (x.ctypes.data for x in (q, indptr, nnz, col, sim))
    calls = {"gnn_match_count": lambda nq, nb, t, m: lib.gnn_match_count(None, qp, nq, qp, nb, t, m, ip, zp),
             "gnn_match_count_dev": lambda nq, nb, t, m: lib.gnn_match_count_dev(None, qp, nq, qp, nb, t, m, ip, zp),
             "gnn_match_fill": lambda nq, nb, t, m: lib.gnn_match_fill(None, nq, nb, t, m, cp, sp, 4),
             "gnn_match_fill_dev": lambda nq, nb, t, m: lib.gnn_match_fill_dev(None, qp, nq, qp, nb, t, m, cp, sp, 4)}
    for name in names:
        fn = calls[name]
        for n in (-1, 1 << 31):
            assert fn(n, 2, 0.5, 0) == _lib.ERR_ARG
            assert f"{name}: n_query {n} is outside [0, 2^31)".encode() in lib.gnn_last_error()
            assert fn(2, n, 0.5, 0) == _lib.ERR_ARG
            assert f"{name}: n_base {n} is outside [0, 2^31)".encode() in lib.gnn_last_error()
        for t, word in ((float("nan"), b"nan"), (float("inf"), b"inf"), (float("-inf"), b"-inf"), (1e39, b"inf")):
            assert fn(2, 2, t, 0) == _lib.ERR_ARG
            assert name.encode() + b": threshold " + word in lib.gnn_last_error() and b"finite" in lib.gnn_last_error()
        for metric in (2, -1, 9):
            assert fn(2, 2, 0.5, metric) == _lib.ERR_ARG
            assert f"{name}: metric {metric} is outside [0, 1]".encode() in lib.gnn_last_error()
        for nq, nb in ((2, 2), (0, 2), (2, 0), (0, 0)):
            assert fn(nq, nb, 0.5, 1) == _lib.ERR_ARG             # valid, but no ctx
            assert b"ctx is NULL" in lib.gnn_last_error()
    for fn in (lib.gnn_match_count, lib.gnn_match_count_dev):
        for hole in range(4):
            args = [qp, qp, ip, zp]
            args[hole] = None
            assert fn(None, args[0], 2, args[1], 2, 0.5, 0, args[2], args[3]) == _lib.ERR_ARG
            assert b"the query, the base, indptr and nnz are required" in lib.gnn_last_error()
        assert fn(None, None, 0, None, 0, 0.5, 0, ip, zp) == _lib.ERR_ARG and b"ctx is NULL" in lib.gnn_last_error()    # empty sides need no rows
    assert lib.gnn_debug_match_pass_ms(None, None, 0, zp) == _lib.ERR_ARG and b"ctx is NULL" in lib.gnn_last_error()
    assert all((a == 7).all() for a in (indptr, nnz, col, sim))   # nothing was written


# ---- main() over a fake engine ---------------------------------------------------------------------------------------------------
class FakeMatchEngine(FakeGraphEngine):
    """the stand-in of tests/test_graph_host.py plus match, served from sequence.threshold_matches"""

    def match(self, query, base, threshold, metric="cosine", max_edges=1 << 28):
        type(self).calls.append(("match", len(query), len(base), float(threshold), metric))
        indptr, col, sim = sequence.threshold_matches(query, base, threshold, metric)
        if len(col) > type(self).cap:
            raise ValueError(f"there are {len(col)} matches at the threshold {float(np.float32(threshold)):g}, more than max_edges = "
                             f"{type(self).cap}: raise the threshold or max_edges")
        return MatchResult.build((indptr, col, sim.astype(np.float32)), sequence.valid_rows(query, metric), sequence.valid_rows(base, metric),
                                 threshold, metric)


@pytest.fixture
def fake_main(monkeypatch):
    monkeypatch.setattr(nnc, "_engine", lambda: FakeMatchEngine())
    for k in SWITCHES + ("GENOMAD_AMD_CLUSTERS", "GENOMAD_AMD_REPRESENTATIVES", "GENOMAD_AMD_LINKAGE", "GENOMAD_AMD_GRAPH") + MATCH_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    del FakeMatchEngine.calls[:]
    FakeMatchEngine.cap = 1 << 28
    return lambda fa, out, **kw: nnc.main(fa, out, False, 128, False, 1, False, False, **kw)


def test_match_switch_values(monkeypatch):
    for k in MATCH_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    assert nnc.match_requested() is None and nnc.match_base_requested() is None
    for v, want in (("", None), (" 0.9 ", float(np.float32(0.9))), ("1", 1.0), ("-1", -1.0), ("0", 0.0), ("5e-1", 0.5)):
        monkeypatch.setenv("GENOMAD_AMD_MATCH", v)
        assert nnc.match_requested() == want
    for v in ("1.01", "-1.5", "nan", "inf", "high", "0,9"):
        monkeypatch.setenv("GENOMAD_AMD_MATCH", v)
        with pytest.raises(ValueError, match=r"GENOMAD_AMD_MATCH=.*\[-1, 1\]"):
            nnc.match_requested()
    for v, want in (("", None), ("  ", None), (" ref/old.npz ", "ref/old.npz")):
        monkeypatch.setenv("GENOMAD_AMD_MATCH_BASE", v)
        got = nnc.match_base_requested()
        assert (got is None) if want is None else (str(got) == want)


def reference_file(path, n=5, seed=3, **extra):
    emb = rows(n, seed)
    np.savez_compressed(path, **{"contig_names": np.array([f"ref{i}" for i in range(n)]), "embeddings": emb, **extra})
    return emb


def test_the_base_loader_accepts_what_the_embeddings_switch_writes_and_names_every_fault(tmp_path):
    emb = reference_file(tmp_path / "ok.npz")
    names, got = nnc.load_match_base(tmp_path / "ok.npz")
    assert list(names) == [f"ref{i}" for i in range(5)] and got.dtype == np.float32 and np.array_equal(got, emb) and got.flags.c_contiguous
    np.savez_compressed(tmp_path / "pro.npz", provirus_names=np.array(["a", "b"]), embeddings=rows(2, 1), strand=np.array("both"))
    assert list(nnc.load_match_base(tmp_path / "pro.npz", "both")[0]) == ["a", "b"]          # the names' key is free
    for strand, base in (("forward", "pro.npz"), ("reverse", "pro.npz"), ("both", "ok.npz")):
        with pytest.raises(ValueError, match=r"GENOMAD_AMD_MATCH_BASE=.*GENOMAD_AMD_STRAND=(both|forward), this run's are under " + strand):
            nnc.load_match_base(tmp_path / base, strand)
    with pytest.raises(ValueError, match=r"GENOMAD_AMD_MATCH_BASE=.*gone\.npz.*no such file"):
        nnc.load_match_base(tmp_path / "gone.npz")
    (tmp_path / "text.npz").write_text("not an archive")
    with pytest.raises(ValueError, match=r"GENOMAD_AMD_MATCH_BASE=.*not a readable \.npz"):
        nnc.load_match_base(tmp_path / "text.npz")
    np.savez_compressed(tmp_path / "noemb.npz", contig_names=np.array(["a"]))
    np.savez_compressed(tmp_path / "narrow.npz", contig_names=np.array(["a", "b"]), embeddings=np.zeros((2, 256), np.float32))
    np.savez_compressed(tmp_path / "flat.npz", contig_names=np.array(["a"]), embeddings=np.zeros(512, np.float32))
    for bad in ("noemb.npz", "narrow.npz", "flat.npz"):
        with pytest.raises(ValueError, match=r"GENOMAD_AMD_MATCH_BASE=.*'embeddings' of shape \(n, 512\)"):
            nnc.load_match_base(tmp_path / bad)
    np.savez_compressed(tmp_path / "nonames.npz", embeddings=rows(2, 1))
    np.savez_compressed(tmp_path / "short.npz", contig_names=np.array(["a"]), embeddings=rows(2, 1))
    np.savez_compressed(tmp_path / "twice.npz", contig_names=np.array(["a", "b"]), other_names=np.array(["c", "d"]), embeddings=rows(2, 1))
    for bad in ("nonames.npz", "short.npz", "twice.npz"):
        with pytest.raises(ValueError, match=r"GENOMAD_AMD_MATCH_BASE=.*one 1-D array of the 2 names"):
            nnc.load_match_base(tmp_path / bad)


def test_the_tsv_writer_writes_one_line_per_match(tmp_path):
    res = hand_made()
    nnc.write_matches_tsv(tmp_path / "m.tsv", list("wxyz"), list("abcde"), res)
    assert (tmp_path / "m.tsv").read_text() == ("seq_name\treference\tsimilarity\n"
                                                "w\tb\t0.500000\nw\td\t0.900000\nw\te\t0.900000\ny\ta\t0.700000\nz\ta\t0.600000\nz\td\t0.600000\n")
    nnc.write_matches_tsv(tmp_path / "e.tsv", [], list("ab"), match_result(rows(0, 1), rows(2, 1), 0.4))
    assert (tmp_path / "e.tsv").read_text() == "seq_name\treference\tsimilarity\n"


def test_main_refuses_half_a_request_and_a_bad_base(tmp_path, monkeypatch, fake_main, capsys):
    fa = tmp_path / "s.fna"
    _write_fasta(fa, n=3)
    reference_file(tmp_path / "ref.npz")
    both = "GENOMAD_AMD_MATCH and GENOMAD_AMD_MATCH_BASE need each other and GENOMAD_AMD_EMBEDDINGS=1"

    def refused(message):
        capsys.readouterr()
        with pytest.raises(SystemExit) as exc:
            fake_main(fa, tmp_path / "refused")
        err = capsys.readouterr().err
        assert exc.value.code == 1 and message in err and len(err.strip().splitlines()) == 1, err
        assert FakeMatchEngine.calls == []                      # before any classification starts
        assert not (tmp_path / "refused" / "s_nn_classification").exists()

    monkeypatch.setenv("GENOMAD_AMD_MATCH", "1.5")
    with pytest.raises(ValueError, match="GENOMAD_AMD_MATCH="):
        fake_main(fa, tmp_path / "bad")
    assert not (tmp_path / "bad").exists()                  # before anything is written
    monkeypatch.setenv("GENOMAD_AMD_EMBEDDINGS", "1")
    monkeypatch.setenv("GENOMAD_AMD_MATCH", "0.9")
    refused(both)                                           # the threshold without the base
    monkeypatch.delenv("GENOMAD_AMD_MATCH")
    monkeypatch.setenv("GENOMAD_AMD_MATCH_BASE", str(tmp_path / "ref.npz"))
    refused(both)                                           # the base without the threshold
    monkeypatch.setenv("GENOMAD_AMD_MATCH", "0.9")
    monkeypatch.delenv("GENOMAD_AMD_EMBEDDINGS")
    refused(both)                                           # both, without the embeddings
    monkeypatch.setenv("GENOMAD_AMD_EMBEDDINGS", "1")
    monkeypatch.setenv("GENOMAD_AMD_MATCH_BASE", str(tmp_path / "gone.npz"))
    refused("no such file")
    np.savez_compressed(tmp_path / "narrow.npz", contig_names=np.array(["a", "b"]), embeddings=np.zeros((2, 256), np.float32))
    monkeypatch.setenv("GENOMAD_AMD_MATCH_BASE", str(tmp_path / "narrow.npz"))
    refused("'embeddings' of shape (n, 512)")
    np.savez_compressed(tmp_path / "nonames.npz", embeddings=rows(2, 1))
    monkeypatch.setenv("GENOMAD_AMD_MATCH_BASE", str(tmp_path / "nonames.npz"))
    refused("one 1-D array of the 2 names")
    reference_file(tmp_path / "both.npz", strand=np.array("both"))
    monkeypatch.setenv("GENOMAD_AMD_MATCH_BASE", str(tmp_path / "both.npz"))
    refused("GENOMAD_AMD_STRAND=both, this run's are under forward")
    monkeypatch.setenv("GENOMAD_AMD_MATCH_BASE", str(tmp_path / "ref.npz"))
    monkeypatch.setenv("GENOMAD_AMD_STRAND", "both")
    refused("GENOMAD_AMD_STRAND=forward, this run's are under both")


def test_main_writes_both_files_follows_the_request_and_removes_stale_ones(tmp_path, monkeypatch, fake_main, capsys):
    fa = tmp_path / "m.fna"
    _write_fasta(fa, n=6)
    monkeypatch.setenv("GENOMAD_AMD_EMBEDDINGS", "1")
    fake_main(fa, tmp_path / "unset")
    assert not any(c[0] == "match" for c in FakeMatchEngine.calls)
    d0 = tmp_path / "unset" / "m_nn_classification"
    emb = _npz(d0 / "m_nn_embeddings.npz")
    # the reference: an earlier run's embeddings file, as it is - every contig matches itself there - under other names
    ref = tmp_path / "reference.npz"
    ref_names = np.array([f"old_{n}" for n in emb["contig_names"]])
    np.savez_compressed(ref, contig_names=ref_names, embeddings=emb["embeddings"])
    monkeypatch.setenv("GENOMAD_AMD_MATCH", "0.999")
    monkeypatch.setenv("GENOMAD_AMD_MATCH_BASE", str(ref))
    out = tmp_path / "on"
    fake_main(fa, out)
    d1 = out / "m_nn_classification"
    assert _tree(d1) == sorted(_tree(d0) + ["m_nn_matches.npz", "m_nn_matches.tsv"])
    for rel in _tree(d0):                                   # every other output: the same arrays, the same bytes
        if rel.endswith(".npz"):
            assert _same_npz(d0 / rel, d1 / rel), rel
        elif rel.endswith(".tsv"):
            assert (d0 / rel).read_bytes() == (d1 / rel).read_bytes(), rel
    z = _npz(d1 / "m_nn_matches.npz")
    n = len(emb["contig_names"])
    t32 = float(np.float32(0.999))
    assert sorted(z) == ["base_names", "col", "contig_names", "indptr", "metric", "sim", "threshold"]
    assert list(z["contig_names"]) == list(emb["contig_names"]) and list(z["base_names"]) == list(ref_names)
    assert float(z["threshold"]) == t32 and z["threshold"].dtype == np.float64 and str(z["metric"]) == "cosine"
    assert FakeMatchEngine.calls.count(("match", n, n, t32, "cosine")) == 1
    indptr, col, sim = sequence.threshold_matches(emb["embeddings"], emb["embeddings"], 0.999)
    assert z["indptr"].dtype == np.int64 and z["col"].dtype == np.int32 and z["sim"].dtype == np.float32
    assert np.array_equal(z["indptr"], indptr) and np.array_equal(z["col"], col) and np.array_equal(z["sim"], sim.astype(np.float32))
    names = list(z["contig_names"])
    valid = sequence.valid_rows(emb["embeddings"])
    assert valid.sum() >= 5 and all(i in col[indptr[i]:indptr[i + 1]] for i in np.flatnonzero(valid))
    lines = (d1 / "m_nn_matches.tsv").read_text().splitlines()
    assert lines[0] == "seq_name\treference\tsimilarity" and len(lines) == len(col) + 1
    rows_of = np.repeat(np.arange(n), np.diff(indptr))
    for e, line in enumerate(lines[1:]):
        assert line == f"{names[rows_of[e]]}\t{ref_names[col[e]]}\t{np.float32(sim[e]):.6f}"
    assert f"{names[0]}\told_{names[0]}\t1.000000" in lines
    runs = lambda: sum(1 for c in FakeMatchEngine.calls if c == "plain")       # noqa: E731
    before = runs()
    fake_main(fa, out)
    assert runs() == before                                  # same request, everything there: nothing runs
    monkeypatch.setenv("GENOMAD_AMD_MATCH", "-1")
    fake_main(fa, out)                                       # another threshold: recomputed
    z = _npz(d1 / "m_nn_matches.npz")
    assert runs() == before + 1 and float(z["threshold"]) == -1.0 and len(z["col"]) == int(valid.sum()) ** 2
    (d1 / "m_nn_matches.tsv").unlink()
    fake_main(fa, out)                                       # one of the pair is gone: recomputed
    assert runs() == before + 2 and (d1 / "m_nn_matches.tsv").exists()
    ref2 = tmp_path / "reference2.npz"
    np.savez_compressed(ref2, contig_names=ref_names[:3], embeddings=emb["embeddings"][:3])
    monkeypatch.setenv("GENOMAD_AMD_MATCH_BASE", str(ref2))
    fake_main(fa, out)                                       # another reference: recomputed
    z = _npz(d1 / "m_nn_matches.npz")
    assert runs() == before + 3 and list(z["base_names"]) == list(ref_names[:3]) and z["col"].max() <= 2
    FakeMatchEngine.cap = 3                                  # too many matches: a console error that names the variable
    (d1 / "m_nn_matches.tsv").unlink()
    capsys.readouterr()
    with pytest.raises(SystemExit) as exc:
        fake_main(fa, out)
    err = capsys.readouterr().err
    assert exc.value.code == 1 and "GENOMAD_AMD_MATCH=-1" in err and " matches at the threshold -1" in err and "max_edges = 3" in err
    FakeMatchEngine.cap = 1 << 28
    for k in MATCH_SWITCHES:
        monkeypatch.delenv(k)
    fake_main(fa, out)                                       # no request: both files go
    assert not (d1 / "m_nn_matches.npz").exists() and not (d1 / "m_nn_matches.tsv").exists()
    assert _tree(d1) == _tree(d0)
    # with the graph in the same run, the reference being the run's own rows: the matches' j > i part is the graph
    monkeypatch.setenv("GENOMAD_AMD_MATCH", "0.5")
    monkeypatch.setenv("GENOMAD_AMD_MATCH_BASE", str(ref))
    monkeypatch.setenv("GENOMAD_AMD_GRAPH", "0.5")
    fake_main(fa, out)
    z, g = _npz(d1 / "m_nn_matches.npz"), _npz(d1 / "m_nn_graph.npz")
    a = np.repeat(np.arange(n), np.diff(z["indptr"]))
    assert np.array_equal(z["col"][z["col"] > a], g["col"]) and np.array_equal(np.bincount(a[z["col"] > a], minlength=n), np.diff(g["indptr"]))
