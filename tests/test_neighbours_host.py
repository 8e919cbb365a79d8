"""Nearest neighbours among encoder embeddings without a GPU: the numpy definition (sequence.nearest_neighbours) against a brute-force
Python loop - ties, padding, zero / NaN / Inf rows under both metrics, the self-search -, the ABI's argument checks (before the ctx is
looked at: no GPU needed), and main()'s GENOMAD_AMD_NEIGHBOURS switch over a fake engine served from the definition."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from genomad_amd import _lib, nn_classification as nnc, sequence
from tests.neighbours_data import rows
from tests.test_strand_host import FakeStrandEngine, _npz, _same_npz, _tree, _write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute(query, base, k, metric):
    """the definition, one pair at a time in Python floats (float64)"""
    self_search = base is None
    base = query if self_search else base

    def ok(r):
        return all(math.isfinite(float(v)) for v in r) and (metric == "dot" or any(float(v) != 0.0 for v in r))

    def sim(x, y):
        d = math.fsum(float(a) * float(b) for a, b in zip(x, y))
        if metric == "dot":
            return d
        return d / (math.sqrt(math.fsum(float(a) ** 2 for a in x)) * math.sqrt(math.fsum(float(b) ** 2 for b in y)))

    idx = np.full((len(query), k), -1, np.int64)
    val = np.full((len(query), k), np.nan, np.float64)
    for i, x in enumerate(query):
        if not ok(x):
            continue
        cand = [(-sim(x, y), j) for j, y in enumerate(base) if ok(y) and not (self_search and i == j)]
        for o, (s, j) in enumerate(sorted(cand)[:k]):
            idx[i, o], val[i, o] = j, -s
    return idx, val


def twelve():
    """12 rows: integer-valued (exact dots, so ties are ties), two duplicates, a zero row, a NaN and an Inf element"""
    r = np.zeros((12, 512), np.float32)
    r[:, :8] = np.random.default_rng(3).integers(0, 4, (12, 8))
    r[5] = r[1]
    r[9] = r[1]
    r[3] = 0
    r[6, 100] = np.nan
    r[7, 511] = np.inf
    return r


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("k", [1, 3, 11, 64])
@pytest.mark.parametrize("self_search", [False, True])
def test_definition_equals_the_brute_force_loop(metric, k, self_search):
    base = twelve()
    query = base if self_search else np.concatenate([base[[1, 3, 6, 7, 2]], rows(2, 5)])
    idx, sim = sequence.nearest_neighbours(query, None if self_search else base, k, metric)
    want_idx, want_sim = brute(query, None if self_search else base, k, metric)
    assert idx.dtype == np.int64 and sim.dtype == np.float32 and idx.shape == sim.shape == (len(query), k)
    assert np.array_equal(idx, want_idx)
    assert np.allclose(sim, want_sim, rtol=0, atol=1e-6, equal_nan=True) and np.array_equal(np.isnan(sim), idx < 0)


def test_ties_go_to_the_lower_index_and_rows_are_padded():
    base = twelve()
    idx, sim = sequence.nearest_neighbours(base[[1]], base, 4, "cosine")
    assert list(idx[0, :3]) == [1, 5, 9] and np.all(sim[0, :3] == 1)          # three copies of the row, in index order
    idx, sim = sequence.nearest_neighbours(base, None, 64, "cosine")
    assert list(idx[1, :2]) == [5, 9] and list(idx[5, :2]) == [1, 9]          # the self pair is excluded, its duplicates are not
    valid = 9                                                                  # 12 rows less the zero, the NaN and the Inf one
    for i in range(12):
        n = 0 if i in (3, 6, 7) else valid - 1
        assert (idx[i, :n] >= 0).all() and (idx[i, n:] == -1).all() and np.isnan(sim[i, n:]).all() and not np.isnan(sim[i, :n]).any()
        assert i not in idx[i] and not set(idx[i, :n]) & {3, 6, 7}


def test_zero_rows_are_valid_under_dot_only():
    base = twelve()
    idx, sim = sequence.nearest_neighbours(base[[3]], base, 64, "dot")
    assert list(idx[0, :10]) == [0, 1, 2, 3, 4, 5, 8, 9, 10, 11] and np.all(sim[0, :10] == 0) and (idx[0, 10:] == -1).all()
    idx, _ = sequence.nearest_neighbours(base, None, 64, "dot")
    assert 3 in idx[0] and 6 not in idx[0] and 7 not in idx[0] and (idx[6] == -1).all() and (idx[7] == -1).all()


def test_empty_sides_and_bad_arguments():
    r = rows(4, 1)
    idx, sim = sequence.nearest_neighbours(r[:0], r, 3)
    assert idx.shape == sim.shape == (0, 3)
    idx, sim = sequence.nearest_neighbours(r, r[:0], 3)
    assert (idx == -1).all() and np.isnan(sim).all()
    idx, sim = sequence.nearest_neighbours(r[:1], None, 2)
    assert (idx == -1).all() and np.isnan(sim).all()                        # one row searched among itself: nobody is left
    for k in (0, 65, -1):
        with pytest.raises(ValueError, match=r"\[1, 64\]"):
            sequence.nearest_neighbours(r, None, k)
    with pytest.raises(ValueError, match="metric"):
        sequence.nearest_neighbours(r, None, 2, "euclid")
    with pytest.raises(ValueError, match="512"):
        sequence.nearest_neighbours(r[:, :100], None, 2)


def test_abi_declares_the_entry_points_and_checks_arguments_before_the_ctx():
    text = open(os.path.join(ROOT, "include", "genomad_nn.h")).read()
    lib = _lib.load()
    for name in ("gnn_neighbours", "gnn_neighbours_dev", "gnn_debug_set_neighbour_split"):
        assert f"int {name}(" in text and name in _lib.SIGNATURES and hasattr(lib, name)
    assert "#define GNN_K_NEIGHBOURS 7" in text and "#define GNN_K_COUNT 8" in text and _lib.K_NEIGHBOURS == 7
    assert _lib.KNN_METRICS == {"cosine": 0, "dot": 1} and "GNN_KNN_COSINE = 0, GNN_KNN_DOT = 1" in text
    from genomad_amd.engine import NNEngine
    for m in ("neighbours", "neighbours_dev", "set_neighbour_split"):
        assert hasattr(NNEngine, m)
    q = rows(2, 1)
    idx, sim = np.full((2, 64), 7, np.int64), np.zeros((2, 64), np.float32)
    for fn in (lib.gnn_neighbours, lib.gnn_neighbours_dev):
        for k in (0, 65, -3):
            assert fn(None, q.ctypes.data, 2, None, 0, k, 0, idx.ctypes.data, sim.ctypes.data) == _lib.ERR_ARG
            assert b"[1, 64]" in lib.gnn_last_error() and str(k).encode() in lib.gnn_last_error()
        assert fn(None, q.ctypes.data, 2, None, 0, 3, 9, idx.ctypes.data, sim.ctypes.data) == _lib.ERR_ARG
        assert b"metric 9" in lib.gnn_last_error() and b"[0, 1]" in lib.gnn_last_error()
        assert fn(None, q.ctypes.data, -1, None, 0, 3, 0, idx.ctypes.data, sim.ctypes.data) == _lib.ERR_ARG
        assert b"n_query -1" in lib.gnn_last_error()
        assert fn(None, q.ctypes.data, 2, q.ctypes.data, -5, 3, 0, idx.ctypes.data, sim.ctypes.data) == _lib.ERR_ARG
        assert b"-5 base rows" in lib.gnn_last_error() and b"[0, 2^31)" in lib.gnn_last_error()
        assert fn(None, q.ctypes.data, 2, None, 0, 3, 0, idx.ctypes.data, sim.ctypes.data) == _lib.ERR_ARG      # valid, but no ctx
        assert b"ctx is NULL" in lib.gnn_last_error()
    assert (idx == 7).all()                                  # nothing was written


# ---- main() over a fake engine ---------------------------------------------------------------------------------------------------
class FakeNeighbourEngine(FakeStrandEngine):
    """the stand-in of tests/test_strand_host.py plus embed_contigs - a fixed function of each contig's bytes, two contigs with the
    same bytes get the same row - and neighbours, served from sequence.nearest_neighbours"""
    calls = []

    def embed_contigs(self, seq, offsets, single_window=False, precision=None):
        scores, ids = self.classify_contigs(seq, offsets, single_window, precision)
        off = np.asarray(offsets, np.int64)
        emb = np.stack([rows(1, int(np.asarray(seq[a:b], np.int64).sum() % 1000))[0] for a, b in zip(off[:-1], off[1:])])
        return scores, emb.astype(np.float32), ids

    def neighbours(self, query, base=None, k=10, metric="cosine"):
        type(self).calls.append(("neighbours", len(query), base is None, int(k), metric))
        return sequence.nearest_neighbours(query, base, k, metric)


SWITCHES = ("GENOMAD_AMD_FRONT_END", "GENOMAD_AMD_STRAND", "GENOMAD_AMD_EMBEDDINGS", "GENOMAD_AMD_SCAN_STRIDE", "GENOMAD_AMD_PRECISION",
            "GENOMAD_AMD_OCCLUSION_BLOCK", "GENOMAD_AMD_ATTRIBUTION_BIN", "GENOMAD_AMD_REGION_PENALTY", "GENOMAD_AMD_NEIGHBOURS")


@pytest.fixture
def fake_main(monkeypatch):
    monkeypatch.setattr(nnc, "_engine", lambda: FakeNeighbourEngine())
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    del FakeNeighbourEngine.calls[:]
    return lambda fa, out, **kw: nnc.main(fa, out, False, 128, False, 1, False, False, **kw)


def test_neighbour_switch_values(monkeypatch):
    monkeypatch.delenv("GENOMAD_AMD_NEIGHBOURS", raising=False)
    assert nnc.neighbours_requested() is None
    for v, want in (("", None), (" 1 ", 1), ("10", 10), ("64", 64)):
        monkeypatch.setenv("GENOMAD_AMD_NEIGHBOURS", v)
        assert nnc.neighbours_requested() == want
    for v in ("0", "65", "-2", "ten", "2.5"):
        monkeypatch.setenv("GENOMAD_AMD_NEIGHBOURS", v)
        with pytest.raises(ValueError, match=r"GENOMAD_AMD_NEIGHBOURS.*\[1, 64\]"):
            nnc.neighbours_requested()


def test_main_refuses_the_switch_without_embeddings(tmp_path, monkeypatch, fake_main, capsys):
    fa = tmp_path / "s.fna"
    _write_fasta(fa, n=3)
    monkeypatch.setenv("GENOMAD_AMD_NEIGHBOURS", "65")
    with pytest.raises(ValueError, match="GENOMAD_AMD_NEIGHBOURS"):
        fake_main(fa, tmp_path / "bad")
    assert not (tmp_path / "bad").exists()                  # before anything is written
    monkeypatch.setenv("GENOMAD_AMD_NEIGHBOURS", "5")
    with pytest.raises(SystemExit) as exc:
        fake_main(fa, tmp_path / "refused")
    assert exc.value.code == 1
    err = capsys.readouterr().err
    assert "GENOMAD_AMD_NEIGHBOURS needs GENOMAD_AMD_EMBEDDINGS=1" in err and len(err.strip().splitlines()) == 1
    assert not list((tmp_path / "refused").rglob("*.npz")) and FakeNeighbourEngine.calls == []


def test_main_writes_the_file_follows_k_and_removes_a_stale_one(tmp_path, monkeypatch, fake_main):
    fa = tmp_path / "m.fna"
    recs = _write_fasta(fa, n=6)
    with open(fa, "a") as f:
        f.write(f">twin of c2\n{dict(recs)['c2']}\n")        # the same bytes as c2: the same embedding
    monkeypatch.setenv("GENOMAD_AMD_EMBEDDINGS", "1")
    fake_main(fa, tmp_path / "unset")
    assert not any(c[0] == "neighbours" for c in FakeNeighbourEngine.calls)
    monkeypatch.setenv("GENOMAD_AMD_NEIGHBOURS", "3")
    out = tmp_path / "on"
    fake_main(fa, out)
    d0, d1 = tmp_path / "unset" / "m_nn_classification", out / "m_nn_classification"
    assert _tree(d1) == sorted(_tree(d0) + ["m_nn_neighbours.npz"])
    for rel in _tree(d0):                                   # every other output: the same arrays, the same bytes
        if rel.endswith(".npz"):
            assert _same_npz(d0 / rel, d1 / rel), rel
        elif rel.endswith(".tsv"):
            assert (d0 / rel).read_bytes() == (d1 / rel).read_bytes(), rel
    z, emb = _npz(d1 / "m_nn_neighbours.npz"), _npz(d1 / "m_nn_embeddings.npz")
    n = len(emb["contig_names"])
    assert sorted(z) == ["contig_names", "idx", "k", "metric", "sim"] and list(z["contig_names"]) == list(emb["contig_names"])
    assert int(z["k"]) == 3 and z["k"].dtype == np.int64 and str(z["metric"]) == "cosine"
    assert FakeNeighbourEngine.calls.count(("neighbours", n, True, 3, "cosine")) == 1
    want_idx, want_sim = sequence.nearest_neighbours(emb["embeddings"], None, 3)
    assert np.array_equal(z["idx"], want_idx) and np.array_equal(z["sim"], want_sim) and z["idx"].shape == (n, 3)
    names = list(z["contig_names"])
    a, b = names.index("c2"), names.index("twin")
    assert z["idx"][a, 0] == b and z["idx"][b, 0] == a and abs(z["sim"][a, 0] - 1) < 1e-6
    runs = lambda: sum(1 for c in FakeNeighbourEngine.calls if c == "plain")       # noqa: E731
    before = runs()
    fake_main(fa, out)
    assert runs() == before                                  # same request, everything there: nothing runs
    monkeypatch.setenv("GENOMAD_AMD_NEIGHBOURS", "2")
    fake_main(fa, out)                                       # another k: recomputed
    assert runs() == before + 1 and int(_npz(d1 / "m_nn_neighbours.npz")["k"]) == 2
    monkeypatch.delenv("GENOMAD_AMD_NEIGHBOURS")
    fake_main(fa, out)                                       # no request: the file goes
    assert runs() == before + 2 and not (d1 / "m_nn_neighbours.npz").exists()
    monkeypatch.setenv("GENOMAD_AMD_NEIGHBOURS", "2")
    monkeypatch.setenv("GENOMAD_AMD_STRAND", "both")
    FakeNeighbourEngine.classify_contigs_strand = lambda self, seq, offsets, strand="both", single_window=False, precision=None, embed=False: (
        lambda r: (r[0], r[1], FakeNeighbourEngine.embed_contigs(self, seq, offsets)[1], r[3], r[4]))(
            FakeStrandEngine.classify_contigs_strand(self, seq, offsets, strand, single_window, precision, embed))
    try:
        fake_main(fa, out)
    finally:
        del FakeNeighbourEngine.classify_contigs_strand
    assert str(_npz(d1 / "m_nn_neighbours.npz")["strand"]) == "both"
