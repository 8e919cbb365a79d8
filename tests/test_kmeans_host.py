"""Spherical k-means among encoder embeddings without a GPU: the numpy definition (sequence.spherical_kmeans) on planted families - the
families recovered, farthest-first one row per family, the margins the exact GPU comparisons rest on (best and second-best centroid
>= 1e-4 apart at every assignment, every group's resultant >= 0.5 of its size), the objective's monotonicity -, empty and zero-sum
clusters, max_iter = 0, the converged flag, invalid rows, argument errors, group_centroids against a plain loop, the table and
KMeansResult, the ABI's argument checks (before the ctx is looked at: no GPU needed), and main()'s GENOMAD_AMD_KMEANS switches over a
fake engine served from the definition."""
import os

import numpy as np
import pytest

from genomad_amd import _lib, nn_classification as nnc, sequence
from genomad_amd.engine import KMeansResult, NNEngine
from tests.kmeans_data import INITS, KS, N, SIZES, defined, init_rows, loop_centroids, planted, resultant, signed_init, signed_rows, unit64
from tests.neighbours_data import rows
from tests.test_neighbours_host import SWITCHES, FakeNeighbourEngine
from tests.test_strand_host import FakeStrandEngine, _npz, _same_npz, _tree, _write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(k, kind) for k in KS for kind in INITS]


def test_planted_families_are_recovered_and_farthest_first_picks_one_row_per_family():
    r, family = planted()
    (label, sim, cent, size, iterations, converged, picks), _ = defined(len(SIZES))
    assert sorted(family[picks]) == list(range(len(SIZES)))               # one pick per family
    assert picks[0] == np.flatnonzero(family >= 0)[0]                     # the first centre: the valid row of smallest index
    for f in range(len(SIZES)):
        assert len(set(label[family == f])) == 1, f                       # a family is one cluster ...
    assert len(set(label[family >= 0])) == len(SIZES)                     # ... of its own
    assert sorted(size) == sorted(SIZES) and converged and iterations >= 1
    assert (label[family < 0] == -1).all() and np.isnan(sim[family < 0]).all() and (sim[family >= 0] > 0.6).all()
    assert label.dtype == np.int64 and sim.dtype == np.float32 and cent.dtype == np.float32 and cent.shape == (7, 512)
    assert size.dtype == np.int64 and picks.dtype == np.int64 and np.allclose((cent.astype(np.float64) ** 2).sum(axis=1), 1, atol=1e-6)


@pytest.mark.parametrize("k,kind", CASES)
def test_the_margins_the_gpu_comparisons_rest_on(k, kind):
    """the device assigns by an argmax over f32 similarities (within 1e-5 of the float64 ones): on every input that a GPU test compares
    with the definition exactly, best and second-best centroid keep 1e-4 apart at every assignment; and every group's resultant keeps
    0.5 of its size, which the 1e-6 bound on the centroids assumes (tests/test_kmeans_gpu.py)"""
    r, _ = planted()
    out, trace = defined(k, kind)
    gap = min(t["gap"] for t in trace)
    res = np.nanmin(resultant(r, out[0], k))
    print(f"\nk {k}, init {kind}: {out[4]} updates, converged {out[5]}, smallest gap {gap:.3e}, smallest resultant {res:.3f}")
    assert gap >= 1e-4 and res >= 0.5
    assert len(trace) == out[4] + 1                                       # one assignment more than updates
    if (k, kind) == (7, "first"):
        assert out[4] >= 3                                                # the poor init takes several updates


@pytest.mark.parametrize("k,kind", CASES)
def test_the_objective_never_falls(k, kind):
    obj = [t["objective"] for t in defined(k, kind)[1]]
    assert all(b >= a - 1e-9 * N for a, b in zip(obj, obj[1:]))
    out = defined(k, kind)[0]
    assert abs(KMeansResult.build(out).objective - obj[-1]) <= 1e-4 * N   # sim is f32


def test_farthest_first_ties_go_to_the_smaller_row():
    r = np.zeros((6, 512), np.float32)
    r[0, 0] = r[1, 1] = r[2, 1] = r[3, 2] = r[4, 2] = 1                   # rows 1, 2 and rows 3, 4 are twins; row 5 is a zero row
    out = sequence.spherical_kmeans(r, 3, max_iter=0)
    assert list(out[6]) == [0, 1, 3] and list(out[0]) == [0, 1, 1, 2, 2, -1] and list(out[3]) == [1, 2, 2]
    assert list(sequence.spherical_kmeans(r[::-1], 3, max_iter=0)[6]) == [1, 3, 5]


def test_an_empty_cluster_and_a_zero_sum_cluster_keep_their_centroid():
    r = np.zeros((3, 512), np.float32)
    r[0, 0], r[1, 0], r[2, :2] = 1, 2, (3, 1)
    init = np.zeros((2, 512), np.float32)
    init[0, 0], init[1, 2] = 1, 1                                         # centroid 1 is orthogonal to every row: nobody ever chooses it
    label, sim, cent, size, iterations, converged, picks = sequence.spherical_kmeans(r, 2, init)
    assert list(size) == [3, 0] and list(label) == [0, 0, 0] and converged and iterations == 1
    assert np.array_equal(cent[1], init[1]) and (picks == -1).all()       # the empty cluster kept its value
    assert cent[0, 1] > 0 and not np.array_equal(cent[0], init[0])        # the other one moved
    dup = np.stack([init[0], init[0], init[1]])                           # a copy of centroid 0: the tie goes to the smaller index
    label, sim, cent, size, iterations, converged, picks = sequence.spherical_kmeans(r, 3, dup, 0)
    assert list(label) == [0, 0, 0] and list(size) == [3, 0, 0] and np.array_equal(cent, dup)
    x = np.zeros((2, 512), np.float32)
    x[0, 3], x[1, 3] = 1, -1
    init = np.zeros((1, 512), np.float32)
    init[0, :5] = (1, 2, 3, 4, 5)
    label, sim, cent, size, iterations, converged, picks = sequence.spherical_kmeans(x, 1, init)
    assert list(label) == [0, 0] and list(size) == [2] and converged      # the sum of x and -x is exactly zero: kept
    assert np.array_equal(cent[0], (init[0].astype(np.float64) / np.sqrt(55)).astype(np.float32))


def test_max_iter_zero_is_a_pure_assignment_and_the_converged_flag():
    r, family = planted()
    init = init_rows("first", 7)
    label, sim, cent, size, iterations, converged, _ = sequence.spherical_kmeans(r, 7, init, 0)
    assert iterations == 0 and not converged
    assert np.array_equal(cent, unit64(init).astype(np.float32))
    valid = family >= 0
    s = unit64(r[valid]) @ unit64(init).T
    assert np.array_equal(label[valid], s.argmax(axis=1)) and np.array_equal(sim[valid], s.max(axis=1).astype(np.float32))
    full = defined(7, "first")[0]
    for cap in range(full[4] + 2):
        out = sequence.spherical_kmeans(r, 7, init, cap)
        assert out[4] == min(cap, full[4]) and out[5] == (cap >= full[4]), cap      # converged exactly when the cap did not bite
    again = sequence.spherical_kmeans(r, 7, init, full[4])
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(again[:4], full[:4]))


def test_invalid_rows_and_argument_errors():
    r = np.tile(rows(1, 4), (7, 1))
    r[1] = 0
    r[3, 100] = np.nan
    r[5, 511] = np.inf
    label, sim, cent, size, iterations, converged, picks = sequence.spherical_kmeans(r, 1)
    assert list(label) == [0, -1, 0, -1, 0, -1, 0] and list(size) == [4] and list(picks) == [0] and converged
    assert np.isnan(sim[[1, 3, 5]]).all() and np.allclose(sim[[0, 2, 4, 6]], 1, atol=1e-6)
    assert list(sequence.spherical_kmeans(r, 4)[3]) == [4, 0, 0, 0]       # k = the valid rows; identical rows: ties to the smaller centroid
    with pytest.raises(ValueError, match="k 5 is more than the 4 valid rows of 7"):
        sequence.spherical_kmeans(r, 5)
    with pytest.raises(ValueError, match="k 1 is more than the 0 valid rows of 0"):
        sequence.spherical_kmeans(r[:0], 1)
    for bad in (0, -1, 65536, 2.5, "x", None, True):
        with pytest.raises(ValueError, match=r"k .*\[1, 65535\]"):
            sequence.spherical_kmeans(r, bad)
    for bad in (-1, 1001, 0.5, "x", None, False):
        with pytest.raises(ValueError, match=r"max_iter .*\[0, 1000\]"):
            sequence.spherical_kmeans(r, 2, None, bad)
    with pytest.raises(ValueError, match="init has 3 rows: k = 2"):
        sequence.spherical_kmeans(r, 2, r[[0, 2, 4]])
    with pytest.raises(ValueError, match="1 of the 2 init rows are not valid"):
        sequence.spherical_kmeans(r, 2, r[[0, 1]])
    with pytest.raises(ValueError, match="512"):
        sequence.spherical_kmeans(r[:, :100], 2)
    with pytest.raises(ValueError, match="512"):
        sequence.spherical_kmeans(r, 2, r[:2, :100])


def test_group_centroids_against_a_plain_loop():
    r, family = planted()
    r = r.copy()
    label = family.copy()
    label[::7] = -1                                                       # unlabelled rows are skipped
    label[label == 5] = 9                                                 # a group without members (5) and room to spare (7, 8)
    label[np.flatnonzero(family < 0)] = 2                                 # invalid rows are skipped whatever their label
    cent, size = sequence.group_centroids(r, label, 10)
    want, want_size = loop_centroids(r, label, 10)
    assert cent.dtype == np.float32 and cent.shape == (10, 512) and size.dtype == np.int64
    assert np.array_equal(size, want_size) and np.abs(cent - want).max() <= 1e-7
    assert (cent[[5, 7, 8]] == 0).all() and list(size[[5, 7, 8]]) == [0, 0, 0] and size[9] > 0
    x = np.zeros((2, 512), np.float32)
    x[0, 3], x[1, 3] = 2, -0.5
    cent, size = sequence.group_centroids(x, [0, 0], 1)                   # a zero sum: a zero row, two members
    assert (cent == 0).all() and list(size) == [2]
    cent, size = sequence.group_centroids(r[:0], np.zeros(0, np.int64), 3)
    assert cent.shape == (3, 512) and (cent == 0).all() and list(size) == [0, 0, 0]
    for bad in ([0, 3], [-2, 0]):
        with pytest.raises(ValueError, match=r"a label is outside \[-1, 3\)"):
            sequence.group_centroids(x, bad, 3)
    with pytest.raises(ValueError, match="one integer per row"):
        sequence.group_centroids(x, [0], 3)
    with pytest.raises(ValueError, match="one integer per row"):
        sequence.group_centroids(x, [0.0, 1.0], 3)


def test_the_signed_rows_are_negative_to_every_init_row():
    """the GPU test of padded columns: every similarity is negative, so a padded column's 0 would win wherever it is not masked"""
    r = signed_rows()
    for k in (7, 33):
        assert (unit64(r) @ unit64(signed_init(k)).T).max() < -0.5


def test_kmeans_table_and_result():
    r = np.zeros((6, 512), np.float32)
    r[0, 0], r[1, :2], r[2, 1], r[3, :3], r[4, 5] = 1, (4, 3), 1, (0, 4, 3), np.nan
    init = np.zeros((3, 512), np.float32)
    init[0, 0], init[1, 1], init[2, 9] = 1, 1, 1
    out = sequence.spherical_kmeans(r, 3, init, 0)
    assert list(out[0]) == [0, 0, 1, 1, -1, -1] and list(out[3]) == [2, 2, 0]
    want = [{"cluster": 0, "size": 2, "mean_sim": pytest.approx(0.9), "nearest": 0},
            {"cluster": 1, "size": 2, "mean_sim": pytest.approx(0.9), "nearest": 2},
            {"cluster": 2, "size": 0, "mean_sim": None, "nearest": None}]
    assert sequence.KMEANS_FIELDS == ("label", "sim", "centroids", "size", "iterations", "converged", "init_rows")
    assert sequence.kmeans_table(out) == want and sequence.kmeans_table(dict(zip(sequence.KMEANS_FIELDS, out))) == want
    res = KMeansResult.build(out)
    assert res.table() == want and res.k == 3 and res.iterations == 0 and res.converged is False
    assert res.objective == pytest.approx(3.6) and list(res.asdict()) == list(sequence.KMEANS_FIELDS)
    assert res.table(list("abcdef"))[1]["nearest"] == "c"


def test_abi_declares_the_entry_points_and_checks_arguments_before_the_ctx():
    text = open(os.path.join(ROOT, "include", "genomad_nn.h")).read()
    lib = _lib.load()
    for name in ("gnn_kmeans", "gnn_kmeans_dev", "gnn_centroids", "gnn_centroids_dev", "gnn_debug_kmeans_pass_ms", "gnn_debug_set_kmeans_lds"):
        assert f"int {name}(" in text and name in _lib.SIGNATURES and hasattr(lib, name)
    for m in ("kmeans", "kmeans_dev", "centroids", "centroids_dev", "kmeans_pass_ms", "set_kmeans_lds"):
        assert hasattr(NNEngine, m)
    for f in ("spherical_kmeans", "group_centroids", "kmeans_table"):
        assert hasattr(sequence, f)
    q = rows(2, 1)
    out = [np.full(2, 7, np.int64), np.full(2, 7, np.float32), np.full((2, 512), 7, np.float32), np.full(2, 7, np.int64),
           np.full(2, 7, np.int64), np.full(1, 7, np.int64), np.full(1, 7, np.int32)]
    ptrs = [a.ctypes.data for a in out]
    for fn in (lib.gnn_kmeans, lib.gnn_kmeans_dev):
        name = b"gnn_kmeans_dev" if fn is lib.gnn_kmeans_dev else b"gnn_kmeans:"
        for n in (-1, (1 << 30) + 1):
            assert fn(None, q.ctypes.data, n, 0, None, -1, *ptrs) == _lib.ERR_ARG              # the first of three bad arguments
            assert f"{n} rows is outside [0, 2^30]".encode() in lib.gnn_last_error() and name in lib.gnn_last_error()
        for k in (0, -1, 65536):
            assert fn(None, q.ctypes.data, 2, k, None, -1, *ptrs) == _lib.ERR_ARG              # before max_iter
            assert f"k {k} is outside [1, 65535]".encode() in lib.gnn_last_error() and name in lib.gnn_last_error()
        for it in (-1, 1001):
            assert fn(None, None, 2, 2, None, it, *ptrs) == _lib.ERR_ARG                       # before the pointers
            assert f"max_iter {it} is outside [0, 1000]".encode() in lib.gnn_last_error()
        for hole in range(8):
            args = [q.ctypes.data] + ptrs
            args[hole] = None
            assert fn(None, args[0], 2, 2, None, 5, *args[1:]) == _lib.ERR_ARG
            assert b"bad argument to " + name.rstrip(b":") in lib.gnn_last_error()
        assert fn(None, q.ctypes.data, 2, 2, None, 5, *ptrs) == _lib.ERR_ARG                   # valid, but no ctx
        assert b"ctx is NULL" in lib.gnn_last_error()
    lab = np.zeros(2, np.int64)
    for fn in (lib.gnn_centroids, lib.gnn_centroids_dev):
        assert fn(None, q.ctypes.data, -1, lab.ctypes.data, 0, ptrs[2], ptrs[3]) == _lib.ERR_ARG and b"-1 rows" in lib.gnn_last_error()
        assert fn(None, q.ctypes.data, 2, lab.ctypes.data, 0, ptrs[2], ptrs[3]) == _lib.ERR_ARG and b"k 0 is outside" in lib.gnn_last_error()
        for args in ((None, lab.ctypes.data, ptrs[2], ptrs[3]), (q.ctypes.data, None, ptrs[2], ptrs[3]),
                     (q.ctypes.data, lab.ctypes.data, None, ptrs[3]), (q.ctypes.data, lab.ctypes.data, ptrs[2], None)):
            assert fn(None, args[0], 2, args[1], 2, args[2], args[3]) == _lib.ERR_ARG
            assert b"the rows, the labels and both outputs are required" in lib.gnn_last_error()
        assert fn(None, q.ctypes.data, 2, lab.ctypes.data, 2, ptrs[2], ptrs[3]) == _lib.ERR_ARG and b"ctx is NULL" in lib.gnn_last_error()
    zp = np.zeros(1, np.int64).ctypes.data
    assert lib.gnn_debug_kmeans_pass_ms(None, None, 0, zp) == _lib.ERR_ARG and b"ctx is NULL" in lib.gnn_last_error()
    assert lib.gnn_debug_set_kmeans_lds(None, 3) == _lib.ERR_ARG and b"ctx is NULL" in lib.gnn_last_error()
    assert all((a == 7).all() for a in out)                       # nothing was written


# ---- main() over a fake engine ---------------------------------------------------------------------------------------------------
class FakeKMeansEngine(FakeNeighbourEngine):
    """the stand-in of tests/test_neighbours_host.py plus kmeans, served from sequence.spherical_kmeans"""
    calls = []

    def kmeans(self, rows, k, init=None, max_iter=50):
        type(self).calls.append(("kmeans", len(rows), int(k), init is None, int(max_iter)))
        return KMeansResult.build(sequence.spherical_kmeans(rows, k, init, max_iter))


ENV = ("GENOMAD_AMD_KMEANS", "GENOMAD_AMD_KMEANS_MAX_ITER")


@pytest.fixture
def fake_main(monkeypatch):
    monkeypatch.setattr(nnc, "_engine", lambda: FakeKMeansEngine())
    for k in SWITCHES + ("GENOMAD_AMD_CLUSTERS", "GENOMAD_AMD_DENSITY", "GENOMAD_AMD_DENSITY_MIN_POINTS") + ENV:
        monkeypatch.delenv(k, raising=False)
    del FakeKMeansEngine.calls[:]
    return lambda fa, out, **kw: nnc.main(fa, out, False, 128, False, 1, False, False, **kw)


def test_kmeans_switch_values(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    assert nnc.kmeans_requested() is None
    for v, want in (("", None), (" 4 ", 4), ("1", 1), ("65535", 65535)):
        monkeypatch.setenv("GENOMAD_AMD_KMEANS", v)
        assert nnc.kmeans_requested() == (None if want is None else (want, 50))
    for v in ("0", "-2", "65536", "2.5", "many", "1e2"):
        monkeypatch.setenv("GENOMAD_AMD_KMEANS", v)
        with pytest.raises(ValueError, match=r"GENOMAD_AMD_KMEANS=.*\[1, 65535\]"):
            nnc.kmeans_requested()
    monkeypatch.setenv("GENOMAD_AMD_KMEANS", "3")
    for v, want in (("", 50), ("0", 0), (" 12 ", 12), ("1000", 1000)):
        monkeypatch.setenv("GENOMAD_AMD_KMEANS_MAX_ITER", v)
        assert nnc.kmeans_requested() == (3, want)
    for v in ("-1", "1001", "2.5", "many"):
        monkeypatch.setenv("GENOMAD_AMD_KMEANS_MAX_ITER", v)
        with pytest.raises(ValueError, match=r"GENOMAD_AMD_KMEANS_MAX_ITER=.*\[0, 1000\]"):
            nnc.kmeans_requested()
    monkeypatch.delenv("GENOMAD_AMD_KMEANS")                     # max_iter alone is refused
    monkeypatch.setenv("GENOMAD_AMD_KMEANS_MAX_ITER", "3")
    with pytest.raises(ValueError, match="GENOMAD_AMD_KMEANS_MAX_ITER='3' needs GENOMAD_AMD_KMEANS"):
        nnc.kmeans_requested()


def test_main_refuses_the_switches_before_anything_is_written(tmp_path, monkeypatch, fake_main, capsys):
    fa = tmp_path / "s.fna"
    _write_fasta(fa, n=3)
    monkeypatch.setenv("GENOMAD_AMD_KMEANS", "0")
    with pytest.raises(ValueError, match="GENOMAD_AMD_KMEANS"):
        fake_main(fa, tmp_path / "bad")
    assert not (tmp_path / "bad").exists()                  # before anything is written
    monkeypatch.setenv("GENOMAD_AMD_KMEANS", "2")
    with pytest.raises(SystemExit) as exc:
        fake_main(fa, tmp_path / "refused")
    assert exc.value.code == 1
    err = capsys.readouterr().err
    assert "GENOMAD_AMD_KMEANS needs GENOMAD_AMD_EMBEDDINGS=1" in err and len(err.strip().splitlines()) == 1
    assert not list((tmp_path / "refused").rglob("*.npz")) and not list((tmp_path / "refused").rglob("*.tsv"))
    assert FakeKMeansEngine.calls == []


def test_main_writes_both_files_follows_the_request_and_removes_stale_ones(tmp_path, monkeypatch, fake_main, capsys):
    fa = tmp_path / "m.fna"
    recs = _write_fasta(fa, n=6)
    with open(fa, "a") as f:
        for k in range(2):
            f.write(f">twin{k} of c2\n{dict(recs)['c2']}\n")  # the same bytes as c2: the same embedding
    monkeypatch.setenv("GENOMAD_AMD_EMBEDDINGS", "1")
    fake_main(fa, tmp_path / "unset")
    assert not any(c[0] == "kmeans" for c in FakeKMeansEngine.calls)
    monkeypatch.setenv("GENOMAD_AMD_KMEANS", "3")
    out = tmp_path / "on"
    fake_main(fa, out)
    d0, d1 = tmp_path / "unset" / "m_nn_classification", out / "m_nn_classification"
    assert _tree(d1) == sorted(_tree(d0) + ["m_nn_kmeans.npz", "m_nn_kmeans.tsv"])
    for rel in _tree(d0):                                   # every other output: the same arrays, the same bytes
        if rel.endswith(".npz"):
            assert _same_npz(d0 / rel, d1 / rel), rel
        elif rel.endswith(".tsv"):
            assert (d0 / rel).read_bytes() == (d1 / rel).read_bytes(), rel
    z, emb = _npz(d1 / "m_nn_kmeans.npz"), _npz(d1 / "m_nn_embeddings.npz")
    n = len(emb["contig_names"])
    assert sorted(z) == ["centroids", "contig_names", "converged", "init_rows", "iterations", "k", "label", "max_iter", "metric", "objective",
                         "sim", "size"]
    assert list(z["contig_names"]) == list(emb["contig_names"]) and str(z["metric"]) == "cosine"
    assert int(z["k"]) == 3 and z["k"].dtype == np.int64 and int(z["max_iter"]) == 50 and z["centroids"].shape == (3, 512)
    assert FakeKMeansEngine.calls.count(("kmeans", n, 3, True, 50)) == 1
    want = sequence.spherical_kmeans(emb["embeddings"], 3)
    for key, a in zip(sequence.KMEANS_FIELDS, want):
        assert np.array_equal(z[key], a, equal_nan=True), key
    names = list(z["contig_names"])
    trio = [names.index(k) for k in ("c2", "twin0", "twin1")]
    assert len(set(z["label"][trio])) == 1                  # identical embeddings share a cluster
    lines = (d1 / "m_nn_kmeans.tsv").read_text().splitlines()
    assert lines[0] == "seq_name\tcluster\tcluster_size\tsimilarity" and len(lines) == n + 1
    i = trio[0]
    assert lines[1 + i] == f"{names[i]}\t{z['label'][i]}\t{z['size'][z['label'][i]]}\t{z['sim'][i]:.6f}"
    runs = lambda: sum(1 for c in FakeKMeansEngine.calls if c == "plain")       # noqa: E731
    before = runs()
    fake_main(fa, out)
    assert runs() == before                                  # same request, everything there: nothing runs
    monkeypatch.setenv("GENOMAD_AMD_KMEANS_MAX_ITER", "0")
    fake_main(fa, out)                                       # another max_iter: recomputed
    z = _npz(d1 / "m_nn_kmeans.npz")
    assert runs() == before + 1 and int(z["max_iter"]) == 0 and int(z["iterations"]) == 0
    monkeypatch.setenv("GENOMAD_AMD_KMEANS", "2")
    fake_main(fa, out)                                       # another k: recomputed
    assert runs() == before + 2 and int(_npz(d1 / "m_nn_kmeans.npz")["k"]) == 2
    (d1 / "m_nn_kmeans.tsv").unlink()
    fake_main(fa, out)                                       # one of the pair is gone: recomputed
    assert runs() == before + 3 and (d1 / "m_nn_kmeans.tsv").exists()
    monkeypatch.delenv("GENOMAD_AMD_KMEANS_MAX_ITER")
    monkeypatch.setenv("GENOMAD_AMD_KMEANS", str(n + 1))     # more groups than contigs: one line, exit 1
    capsys.readouterr()
    with pytest.raises(SystemExit) as exc:
        fake_main(fa, out)
    assert exc.value.code == 1 and f"GENOMAD_AMD_KMEANS={n + 1}: k {n + 1} is more than the" in capsys.readouterr().err
    monkeypatch.delenv("GENOMAD_AMD_KMEANS")
    fake_main(fa, out)                                       # no request: both files go
    assert not (d1 / "m_nn_kmeans.npz").exists() and not (d1 / "m_nn_kmeans.tsv").exists()
    assert _tree(d1) == _tree(d0)
    monkeypatch.setenv("GENOMAD_AMD_KMEANS", "2")
    monkeypatch.setenv("GENOMAD_AMD_NEIGHBOURS", "2")        # both searches in one run
    monkeypatch.setenv("GENOMAD_AMD_STRAND", "both")
    FakeKMeansEngine.classify_contigs_strand = lambda self, seq, offsets, strand="both", single_window=False, precision=None, embed=False: (
        lambda r: (r[0], r[1], FakeKMeansEngine.embed_contigs(self, seq, offsets)[1], r[3], r[4]))(
            FakeStrandEngine.classify_contigs_strand(self, seq, offsets, strand, single_window, precision, embed))
    try:
        fake_main(fa, out)
    finally:
        del FakeKMeansEngine.classify_contigs_strand
    assert str(_npz(d1 / "m_nn_kmeans.npz")["strand"]) == "both" and str(_npz(d1 / "m_nn_neighbours.npz")["strand"]) == "both"


def test_the_table_writes_na_for_a_contig_without_an_embedding(tmp_path):
    r = np.zeros((4, 512), np.float32)
    r[0, 0], r[1, :2], r[2, 1] = 1, (4, 3), 1
    init = np.zeros((2, 512), np.float32)
    init[0, 0], init[1, 1] = 1, 1
    res = KMeansResult.build(sequence.spherical_kmeans(r, 2, init, 0))
    nnc.write_kmeans_tsv(tmp_path / "t.tsv", list("abcd"), res)
    assert (tmp_path / "t.tsv").read_text() == ("seq_name\tcluster\tcluster_size\tsimilarity\n"
                                                "a\t0\t2\t1.000000\nb\t0\t2\t0.800000\nc\t1\t1\t1.000000\nd\tNA\t0\tNA\n")
