"""Principal components among encoder embeddings without a GPU: the numpy definitions (sequence.pca_moments, pca_from_moments,
pca_project) against plain loops, pca_from_moments on a planted spectrum (the subspace, the order, the sign rule, the ratios),
center=False, fewer than two valid rows and the zero-variance case, invalid rows, the exact rows' condition the GPU test rests on,
PCAResult.table, the ABI's argument checks (before the ctx is looked at: no GPU needed), and main()'s GENOMAD_AMD_PCA switch over a
fake engine served from the definitions."""
import os

import numpy as np
import pytest

from genomad_amd import _lib, nn_classification as nnc, sequence
from genomad_amd.engine import NNEngine, PCAResult
from tests.neighbours_data import rows
from tests.pca_data import (EXACT_NS, SPECTRUM_RANK, exact_moments, exact_rows, loop_moments, loop_project, planted_rows, spectrum_rows,
                            subspace_residual, with_invalid)
from tests.test_neighbours_host import SWITCHES, FakeNeighbourEngine
from tests.test_strand_host import _npz, _same_npz, _tree, _write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_pca(r, n_components=2, center=True, engine=None):
    """NNEngine.pca's composition over the float64 definitions"""
    G, S, n_valid = sequence.pca_moments(r)
    m = sequence.pca_from_moments(G, S, n_valid, n_components, center)
    comp = m["components"].astype(np.float32)
    proj = sequence.pca_project(r, comp, m["mean"] if center else None).astype(np.float32)
    return PCAResult(engine=engine, mean=m["mean"], components=comp, explained_variance=m["explained_variance"],
                     explained_variance_ratio=m["explained_variance_ratio"], total_variance=m["total_variance"], n_valid=n_valid,
                     valid=~np.isnan(proj[:, 0]), projection=proj)


def test_the_definitions_equal_plain_loops():
    r, keep = with_invalid(planted_rows()[:60], (0, 7, 31, 62))
    G, S, n_valid = sequence.pca_moments(r)
    lG, lS, ln = loop_moments(r)
    assert n_valid == ln == 60 and G.dtype == np.float64 and G.shape == (512, 512) and S.shape == (512,)
    assert np.abs(G - lG).max() <= 1e-13 and np.abs(S - lS).max() <= 1e-13
    comp = planted_rows()[100:103]
    mean = S / n_valid
    for m in (None, mean):
        got, want = sequence.pca_project(r, comp, m), loop_project(r, comp, m)
        assert got.shape == (64, 3) and np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[~keep]).all()
        assert np.nanmax(np.abs(got - want)) <= 1e-14
    off = sequence.pca_offsets(comp, mean)
    assert off.dtype == np.float64 and np.abs(off - (loop_project(r[1:2], comp) - loop_project(r[1:2], comp, mean))[0]).max() <= 1e-14
    assert not sequence.pca_offsets(comp, None).any()


def test_invalid_rows_change_nothing():
    base = planted_rows()[:50]
    r, keep = with_invalid(base, (3, 20, 52))
    a, b = sequence.pca_moments(base), sequence.pca_moments(r)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] == 50


def test_the_planted_spectrum_is_recovered():
    r, basis = spectrum_rows()
    G, S, n_valid = sequence.pca_moments(r)
    m = sequence.pca_from_moments(G, S, n_valid, SPECTRUM_RANK)
    comp, var, ratio = m["components"], m["explained_variance"], m["explained_variance_ratio"]
    assert comp.shape == (SPECTRUM_RANK, 512) and comp.dtype == np.float64
    assert np.abs(comp @ comp.T - np.eye(SPECTRUM_RANK)).max() <= 1e-12
    # the noise holds 4e-4 / 2 of a row's energy: the planted subspace is found to a few percent of a radian
    res = subspace_residual(comp, basis)
    print(f"\nplanted spectrum: eigenvalues {var}, ratios {ratio}, subspace residual {res:.3e}")
    assert res <= 0.05
    assert (np.diff(var) < 0).all() and var[0] / var[1] > 1.2 and var[-1] > 20 * (m["total_variance"] - var.sum()) / (512 - SPECTRUM_RANK)
    for c in range(SPECTRUM_RANK):                                    # the sign rule: the entry of largest magnitude is positive
        assert comp[c, np.argmax(np.abs(comp[c]))] > 0
    assert 0.99 < ratio.sum() <= 1 + 1e-12 and (ratio > 0).all()
    assert np.isclose(m["total_variance"], np.trace(G) / n_valid - (m["mean"] ** 2).sum())
    # the scores: mean 0, variance = the eigenvalue, uncorrelated
    p = sequence.pca_project(r, comp.astype(np.float32), m["mean"])
    assert np.abs(p.mean(axis=0)).max() <= 1e-9 and np.abs(p.T @ p / n_valid - np.diag(var)).max() <= 1e-8
    six = sequence.pca_from_moments(G, S, n_valid, 64)
    assert six["components"].shape == (64, 512) and np.allclose(six["explained_variance"][:5], var)


def test_the_sign_rule_ties_go_to_the_smallest_index():
    G = np.zeros((512, 512))
    G[3, 3] = G[9, 9] = 2.0
    G[3, 9] = G[9, 3] = -1.0                  # eigenvectors (e3 - e9) / sqrt 2 (value 3) and (e3 + e9) / sqrt 2 (value 1)
    m = sequence.pca_from_moments(G * 10, np.zeros(512), 10, 2, center=False)
    assert np.allclose(m["explained_variance"], [3, 1]) and m["components"][0, 3] > 0 > m["components"][0, 9]
    assert m["components"][1, 3] > 0 and m["components"][1, 9] > 0


def test_center_false_and_the_edges():
    r = planted_rows()[:40:2]                 # the unflipped rows: a mean far from zero
    G, S, n_valid = sequence.pca_moments(r)
    raw = sequence.pca_from_moments(G, S, n_valid, 2, center=False)
    cen = sequence.pca_from_moments(G, S, n_valid, 2)
    assert not raw["mean"].any() and np.isclose(raw["total_variance"], 1.0)               # unit rows: trace(G / n) = 1
    mu = S / n_valid
    assert abs(raw["components"][0] @ mu / np.sqrt(mu @ mu)) > 0.99                       # uncentred: the first axis is the mean's
    assert cen["total_variance"] < 0.5 and np.allclose(cen["mean"], mu)
    for nv in (1, 0, -3):
        with pytest.raises(ValueError, match="valid rows"):
            sequence.pca_from_moments(G, S, nv, 2)
    for c in (0, 65, 2.5, True):
        with pytest.raises(ValueError, match="n_components"):
            sequence.pca_from_moments(G, S, n_valid, c)
    with pytest.raises(ValueError, match="are required"):
        sequence.pca_from_moments(G[:5], S, n_valid, 2)
    same = np.zeros((4, 512), np.float32)                                                 # four equal rows: no variance at all
    same[:, :4] = 3                                                                       # unit entries 0.5: every step below is exact
    z = sequence.pca_from_moments(*sequence.pca_moments(same), 3)
    assert z["total_variance"] == 0 and np.isnan(z["explained_variance_ratio"]).all() and not z["explained_variance"].any()
    assert np.array_equal(z["mean"][:5], [0.5, 0.5, 0.5, 0.5, 0]) and z["components"].shape == (3, 512)
    with pytest.raises(ValueError, match="components"):
        sequence.pca_project(r, np.zeros((1, 512), np.float32))                           # a zero direction
    with pytest.raises(ValueError, match="components"):
        sequence.pca_project(r, np.ones((65, 512), np.float32))
    with pytest.raises(ValueError, match="mean"):
        sequence.pca_project(r, r[:2], np.zeros(5))


@pytest.mark.parametrize("n", EXACT_NS)
def test_the_exact_rows_keep_their_condition(n):
    """what tests/test_pca_gpu.py's exact comparison rests on: unit entries that are powers of two down to 2^-4 (exact_moments asserts
    it), all 10 block pairs of G occupied once a 256-entry row is there, and the integer definition equal to the float64 one"""
    r = exact_rows(n)
    G, S = exact_moments(r)
    G64, S64, n_valid = sequence.pca_moments(r)
    assert n_valid == n
    assert np.abs(G.astype(np.float64) / 2.0 ** 32 - G64).max() <= 1e-12 and np.abs(S.astype(np.float64) / 2.0 ** 32 - S64).max() <= 1e-12
    assert np.array_equal(G, G.T)
    if n >= 5:
        blocks = np.abs(G).reshape(4, 128, 4, 128).sum(axis=(1, 3))
        assert (blocks > 0).all()


def test_the_result_and_its_table():
    r, keep = with_invalid(planted_rows()[:30], (4, 31))
    res = host_pca(r, 3)
    assert list(res.asdict()) == list(PCAResult.FIELDS) and res.n_components == 3 and res.n_valid == 30
    assert res.projection.shape == (32, 3) and res.projection.dtype == np.float32 and np.array_equal(res.valid, keep)
    t = res.table()
    assert len(t) == 32 and t[4] == {"row": 4, "pc": None} and t[0]["row"] == 0 and len(t[0]["pc"]) == 3
    assert t[1]["pc"] == [float(x) for x in res.projection[1]]
    assert res.table([f"c{i}" for i in range(32)])[31] == {"row": "c31", "pc": None}
    with pytest.raises(ValueError, match="no engine"):
        res.transform(r)


def test_abi_declares_the_entry_points_and_checks_arguments_before_the_ctx():
    text = open(os.path.join(ROOT, "include", "genomad_nn.h")).read()
    lib = _lib.load()
    for name in ("gnn_pca_moments", "gnn_pca_moments_dev", "gnn_pca_project", "gnn_pca_project_dev", "gnn_debug_set_pca_split",
                 "gnn_debug_pca_pass_ms"):
        assert f"int {name}(" in text and name in _lib.SIGNATURES and hasattr(lib, name)
    for m in ("pca", "pca_moments", "pca_moments_dev", "project", "project_dev", "set_pca_split", "pca_pass_ms"):
        assert hasattr(NNEngine, m)
    for f in ("pca_moments", "pca_from_moments", "pca_project"):
        assert hasattr(sequence, f)
    q = rows(2, 1)
    G, S, nv = np.full(512 * 512, 7, np.int64), np.full(512, 7, np.int64), np.full(1, 7, np.int64)
    out = np.full(2 * 64, 7, np.float32)
    for fn in (lib.gnn_pca_moments, lib.gnn_pca_moments_dev):
        name = b"gnn_pca_moments_dev" if fn is lib.gnn_pca_moments_dev else b"gnn_pca_moments:"
        for n in (0, -1, (1 << 30) + 1):
            assert fn(None, None, n, G.ctypes.data, S.ctypes.data, nv.ctypes.data) == _lib.ERR_ARG         # before the pointers
            assert f"{n} rows is outside [1, 2^30]".encode() in lib.gnn_last_error() and name in lib.gnn_last_error()
        for hole in range(4):
            args = [q.ctypes.data, G.ctypes.data, S.ctypes.data, nv.ctypes.data]
            args[hole] = None
            assert fn(None, args[0], 2, *args[1:]) == _lib.ERR_ARG
            assert b"bad argument to " + name.rstrip(b":") in lib.gnn_last_error()
        assert fn(None, q.ctypes.data, 2, G.ctypes.data, S.ctypes.data, nv.ctypes.data) == _lib.ERR_ARG    # valid, but no ctx
        assert b"ctx is NULL" in lib.gnn_last_error()
    for fn in (lib.gnn_pca_project, lib.gnn_pca_project_dev):
        name = b"gnn_pca_project_dev" if fn is lib.gnn_pca_project_dev else b"gnn_pca_project:"
        for n in (0, -1, (1 << 30) + 1):
            assert fn(None, q.ctypes.data, n, q.ctypes.data, 0, None, out.ctypes.data) == _lib.ERR_ARG     # before ncomp
            assert f"{n} rows is outside [1, 2^30]".encode() in lib.gnn_last_error() and name in lib.gnn_last_error()
        for c in (0, -1, 65):
            assert fn(None, None, 2, q.ctypes.data, c, None, out.ctypes.data) == _lib.ERR_ARG              # before the pointers
            assert f"{c} components is outside [1, 64]".encode() in lib.gnn_last_error()
        for hole in range(3):
            args = [q.ctypes.data, q.ctypes.data, out.ctypes.data]
            args[hole] = None
            assert fn(None, args[0], 2, args[1], 2, None, args[2]) == _lib.ERR_ARG
            assert b"bad argument to " + name.rstrip(b":") in lib.gnn_last_error()
        assert fn(None, q.ctypes.data, 2, q.ctypes.data, 2, None, out.ctypes.data) == _lib.ERR_ARG         # off may be NULL; no ctx
        assert b"ctx is NULL" in lib.gnn_last_error()
    assert lib.gnn_debug_set_pca_split(None, 256) == _lib.ERR_ARG and b"ctx is NULL" in lib.gnn_last_error()
    assert lib.gnn_debug_pca_pass_ms(None, None, 0, nv.ctypes.data) == _lib.ERR_ARG and b"ctx is NULL" in lib.gnn_last_error()
    assert (G == 7).all() and (S == 7).all() and (nv == 7).all() and (out == 7).all()                      # nothing was written


# ---- main() over a fake engine ---------------------------------------------------------------------------------------------------
class FakePCAEngine(FakeNeighbourEngine):
    """the stand-in of tests/test_neighbours_host.py plus pca, served from the float64 definitions"""
    calls = []

    def pca(self, rows, n_components=2, center=True):
        type(self).calls.append(("pca", len(rows), int(n_components), bool(center)))
        return host_pca(rows, n_components, center)


@pytest.fixture
def fake_main(monkeypatch):
    monkeypatch.setattr(nnc, "_engine", lambda: FakePCAEngine())
    for k in SWITCHES + ("GENOMAD_AMD_CLUSTERS", "GENOMAD_AMD_KMEANS", "GENOMAD_AMD_KMEANS_MAX_ITER", "GENOMAD_AMD_PCA"):
        monkeypatch.delenv(k, raising=False)
    del FakePCAEngine.calls[:]
    return lambda fa, out, **kw: nnc.main(fa, out, False, 128, False, 1, False, False, **kw)


def test_pca_switch_values(monkeypatch):
    monkeypatch.delenv("GENOMAD_AMD_PCA", raising=False)
    assert nnc.pca_requested() is None
    for v, want in (("", None), (" 4 ", 4), ("1", 1), ("64", 64)):
        monkeypatch.setenv("GENOMAD_AMD_PCA", v)
        assert nnc.pca_requested() == want
    for v in ("0", "-2", "65", "2.5", "many", "1e1"):
        monkeypatch.setenv("GENOMAD_AMD_PCA", v)
        with pytest.raises(ValueError, match=r"GENOMAD_AMD_PCA=.*\[1, 64\]"):
            nnc.pca_requested()


def test_main_refuses_the_switch_before_anything_is_written(tmp_path, monkeypatch, fake_main, capsys):
    fa = tmp_path / "s.fna"
    _write_fasta(fa, n=3)
    monkeypatch.setenv("GENOMAD_AMD_PCA", "0")
    with pytest.raises(ValueError, match="GENOMAD_AMD_PCA"):
        fake_main(fa, tmp_path / "bad")
    assert not (tmp_path / "bad").exists()                  # before anything is written
    monkeypatch.setenv("GENOMAD_AMD_PCA", "2")
    with pytest.raises(SystemExit) as exc:
        fake_main(fa, tmp_path / "refused")
    assert exc.value.code == 1
    err = capsys.readouterr().err
    assert "GENOMAD_AMD_PCA needs GENOMAD_AMD_EMBEDDINGS=1" in err and len(err.strip().splitlines()) == 1
    assert not list((tmp_path / "refused").rglob("*.npz")) and not list((tmp_path / "refused").rglob("*.tsv"))
    assert FakePCAEngine.calls == []


def test_main_writes_both_files_follows_the_request_and_removes_stale_ones(tmp_path, monkeypatch, fake_main, capsys):
    fa = tmp_path / "m.fna"
    _write_fasta(fa, n=6)
    monkeypatch.setenv("GENOMAD_AMD_EMBEDDINGS", "1")
    fake_main(fa, tmp_path / "unset")
    assert FakePCAEngine.calls == [c for c in FakePCAEngine.calls if c[0] != "pca"]
    monkeypatch.setenv("GENOMAD_AMD_PCA", "3")
    out = tmp_path / "on"
    fake_main(fa, out)
    d0, d1 = tmp_path / "unset" / "m_nn_classification", out / "m_nn_classification"
    assert _tree(d1) == sorted(_tree(d0) + ["m_nn_pca.npz", "m_nn_pca.tsv"])
    for rel in _tree(d0):                                   # every other output: the same arrays, the same bytes
        if rel.endswith(".npz"):
            assert _same_npz(d0 / rel, d1 / rel), rel
        elif rel.endswith(".tsv"):
            assert (d0 / rel).read_bytes() == (d1 / rel).read_bytes(), rel
    z, emb = _npz(d1 / "m_nn_pca.npz"), _npz(d1 / "m_nn_embeddings.npz")
    n = len(emb["contig_names"])
    assert sorted(z) == ["components", "contig_names", "explained_variance", "explained_variance_ratio", "mean", "metric", "n_components",
                         "n_valid", "projection", "total_variance"]
    assert list(z["contig_names"]) == list(emb["contig_names"]) and int(z["n_components"]) == 3 and z["n_components"].dtype == np.int64
    assert z["components"].shape == (3, 512) and z["components"].dtype == np.float32 and z["projection"].shape == (n, 3)
    assert z["mean"].shape == (512,) and z["explained_variance"].shape == (3,) and z["explained_variance_ratio"].shape == (3,)
    assert FakePCAEngine.calls.count(("pca", n, 3, True)) == 1
    want = host_pca(emb["embeddings"], 3)
    for key in ("mean", "components", "explained_variance", "explained_variance_ratio", "projection"):
        assert np.array_equal(z[key], getattr(want, key), equal_nan=True), key
    lines = (d1 / "m_nn_pca.tsv").read_text().splitlines()
    assert lines[0] == "seq_name\tpc1\tpc2\tpc3" and len(lines) == n + 1
    names = list(z["contig_names"])
    assert lines[2] == f"{names[1]}\t" + "\t".join(f"{x:.6f}" for x in z["projection"][1])
    runs = lambda: sum(1 for c in FakePCAEngine.calls if c == "plain")       # noqa: E731
    before = runs()
    fake_main(fa, out)
    assert runs() == before                                  # same request, everything there: nothing runs
    monkeypatch.setenv("GENOMAD_AMD_PCA", "2")
    fake_main(fa, out)                                       # another number of components: recomputed
    assert runs() == before + 1 and int(_npz(d1 / "m_nn_pca.npz")["n_components"]) == 2
    assert (d1 / "m_nn_pca.tsv").read_text().splitlines()[0] == "seq_name\tpc1\tpc2"
    (d1 / "m_nn_pca.tsv").unlink()
    fake_main(fa, out)                                       # one of the pair is gone: recomputed
    assert runs() == before + 2 and (d1 / "m_nn_pca.tsv").exists()
    monkeypatch.delenv("GENOMAD_AMD_PCA")
    fake_main(fa, out)                                       # no request: both files go
    assert not (d1 / "m_nn_pca.npz").exists() and not (d1 / "m_nn_pca.tsv").exists()
    assert _tree(d1) == _tree(d0)


def test_main_ends_with_one_line_when_fewer_than_two_contigs_have_an_embedding(tmp_path, monkeypatch, fake_main, capsys):
    fa = tmp_path / "one.fna"
    fa.write_text(">only note\n" + "".join(np.random.default_rng(4).choice(list("ACGT"), 5000)) + "\n")
    monkeypatch.setenv("GENOMAD_AMD_EMBEDDINGS", "1")
    monkeypatch.setenv("GENOMAD_AMD_PCA", "2")
    capsys.readouterr()
    with pytest.raises(SystemExit) as exc:
        fake_main(fa, tmp_path / "one")
    err = capsys.readouterr().err
    assert exc.value.code == 1 and "GENOMAD_AMD_PCA=2: 1 valid rows" in err and len(err.strip().splitlines()) == 1
    assert not list((tmp_path / "one").rglob("*_nn_pca.*"))


def test_the_table_writes_na_for_a_contig_without_an_embedding(tmp_path):
    r = np.zeros((4, 512), np.float32)
    r[0, 0], r[1, :2], r[2, 1] = 1, (4, 3), 1
    res = host_pca(r, 2)
    assert list(res.valid) == [True, True, True, False]
    nnc.write_pca_tsv(tmp_path / "t.tsv", list("abcd"), res)
    lines = (tmp_path / "t.tsv").read_text().splitlines()
    assert lines[0] == "seq_name\tpc1\tpc2" and lines[4] == "d\tNA\tNA"
    assert lines[1] == "a\t" + "\t".join(f"{x:.6f}" for x in res.projection[0])
