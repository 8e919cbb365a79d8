"""Label transfer on the CPU: sequence.class_votes against a plain double loop (ties at the threshold, ties of the nearest, the self
form), vote_predict's three rules, rint half to even, the gap the GPU test relies on, the C entry points' argument checks, the
labelled reference's loader, and main()'s wiring over a fake engine."""
import os

import numpy as np
import pytest

from genomad_amd import _lib, nn_classification as nnc, sequence
from genomad_amd.engine import NNEngine, VoteResult
from tests import votes_data as V
from tests.neighbours_data import rows
from tests.test_match_host import MATCH_SWITCHES, FakeMatchEngine
from tests.test_neighbours_host import SWITCHES
from tests.test_strand_host import _npz, _same_npz, _tree, _write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOTE_SWITCHES = ("GENOMAD_AMD_VOTE", "GENOMAD_AMD_VOTE_BASE", "GENOMAD_AMD_VOTE_MIN_VOTES")


def same(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w, equal_nan=True) for g, w in zip(got, want))


def test_definition_equals_a_double_loop_on_the_tied_rows():
    """cosines that are exact multiples of 1 / 256: 900 pairs tie with the threshold and count (>=); the 21 copies of one row tie as
    the nearest of their class and the smallest index wins"""
    r, s, threshold, label = V.tie_case()
    ok = np.ones(len(r), bool)
    assert int((s == threshold).sum()) >= 100 and float(np.float32(threshold)) == threshold
    got = sequence.class_votes(r[:70], r, label, 5, threshold)
    want = V.loop_votes(s[:70], ok[:70], ok, label, 5, threshold)
    assert same(got, want) and got[0].dtype == np.int64 and got[3].dtype == np.float32
    above = sequence.class_votes(r[:70], r, label, 5, np.nextafter(np.float32(threshold), np.float32(2)))
    assert got[0].sum() - above[0].sum() == int((s[:70][:, label >= 0] == threshold).sum()) > 0       # the ties were counted
    copies = np.r_[10, 40:60]
    c = int(label[copies].max())
    first = int(copies[label[copies] == c].min())
    assert (label[copies] == c).sum() >= 2 and got[2][10, c] == first and got[3][10, c] == 1.0
    # weight is the similarity sum in units of 2^-32, exactly: every s is a multiple of 2^-8
    cols = [np.flatnonzero(label == k) for k in range(5)]
    for k in range(5):
        v = s[:70][:, cols[k]]
        assert np.array_equal(got[1][:, k], (np.where(v >= threshold, v, 0).sum(axis=1) * V.UNIT).astype(np.int64))


def test_the_self_form_is_the_rectangle_without_the_diagonal():
    r, s, threshold, label = V.tie_case()
    ok = np.ones(len(r), bool)
    count, weight, nearest, nearest_sim = sequence.class_votes(r, None, label, 5, threshold)
    assert same((count, weight, nearest, nearest_sim), V.loop_votes(s, ok, ok, label, 5, threshold, leave_one_out=True))
    full = sequence.class_votes(r, r, label, 5, threshold)
    own = np.flatnonzero(label >= 0)
    diag = np.zeros_like(count)
    diag[own, label[own]] = 1                                    # s_ii = 1 >= threshold: the row's own vote in the rectangle
    assert np.array_equal(full[0] - diag, count) and np.array_equal(full[1] - diag * (1 << 32), weight)
    assert (full[2][own, label[own]] <= own).all() and (nearest[own, label[own]] != own).all()
    # a row alone in its class gets no vote from that class
    lone = label.copy()
    lone[lone == 4] = -1
    lone[17] = 4
    alone = sequence.class_votes(r, None, lone, 5, -1.0)
    assert alone[0][17, 4] == 0 and alone[2][17, 4] == -1 and np.isnan(alone[3][17, 4]) and (np.delete(alone[0][:, 4], 17) == 1).all()


@pytest.mark.parametrize("n_base", V.BASES)
def test_float_inputs_keep_the_gap_the_gpu_test_relies_on(n_base):
    """No pair's float64 cosine lies within 1e-5 of a threshold the GPU test compares counts at (the device's f32 value is within
    1e-5 of it: tests/test_neighbours_gpu.py), and the cells whose top two voters are within 2e-5 - where the device may name the
    other one - are few."""
    s, q_ok, b_ok = V.cosines(n_base)
    pairs = s[np.ix_(q_ok, b_ok)]
    assert q_ok.sum() == V.NQ - 2 and b_ok.sum() == n_base - 2
    for t in V.GAPPED:
        thr = float(np.float32(t))
        gap = float(np.abs(pairs - thr).min())
        print(f"\nn_base {n_base}, t {t}: min |s - t| = {gap:.3e}, {int((pairs >= thr).sum())} pairs within")
        assert gap > V.GAP
        for nc in V.CLASSES:
            label = V.labels(n_base, nc)
            assert label.min() == -1 and label.max() <= nc - 2 and (label == -1).sum() >= 1
            got = sequence.class_votes(V.query()[0], V.base(n_base), label, nc, t)
            if n_base <= 33 and nc <= 17:                    # the double loop, where it takes no time
                assert same(got, V.loop_votes(s, q_ok, b_ok, label, nc, t))
            assert (got[0][:, nc - 1] == 0).all() and (got[0][~q_ok] == 0).all() and (got[2][~q_ok] == -1).all()
            cells, close = int((got[0] > 0).sum()), close_cells(s, q_ok, b_ok, label, nc, thr)
            print(f"  {nc} classes: {cells} non-empty cells, {close} with the top two within {V.NEAREST_GAP:g}")
            assert cells > 0 and close <= 0.05 * cells


def close_cells(s, q_ok, b_ok, label, n_classes, thr):
    """the cells whose two most similar voters are within NEAREST_GAP of each other"""
    close = 0
    for c in range(n_classes):
        cols = np.flatnonzero((label == c) & b_ok)
        if len(cols) >= 2:
            v = np.where((s[:, cols] >= thr) & q_ok[:, None], s[:, cols], -np.inf)
            top = np.sort(v, axis=1)[:, -2:]
            with np.errstate(invalid="ignore"):
                close += int((top[:, 1] - top[:, 0] <= V.NEAREST_GAP).sum())
    return close


def test_rint_rounds_half_to_even():
    """s = k * 2^-33: s * 2^32 = k / 2 - an odd k is a tie between two integers, and the even one is taken, as the device's llrint
    does"""
    q = np.zeros((1, 512), np.float32)
    q[0, 0] = 1
    ks = np.array([1, 3, 5, 7, 2, 6, -1, -3, (1 << 20) + 1, (1 << 20) + 3], dtype=np.int64)
    s = (ks.astype(np.float64) / 2.0 ** 33)[None, :]
    assert np.array_equal(s.astype(np.float32).astype(np.float64), s)                  # every s is an f32
    b = np.ones((len(ks), 512), np.float32)
    label = np.arange(len(ks), dtype=np.int64)
    count, weight, nearest, nearest_sim = sequence.class_votes(q, b, label, len(ks), -1.0, sims=s)
    assert list(weight[0]) == [0, 2, 2, 4, 1, 3, 0, -2, 1 << 19, (1 << 19) + 2] and (count == 1).all()
    assert np.array_equal(nearest[0], label) and np.array_equal(nearest_sim[0].astype(np.float64), s[0])


def test_vote_predict_rules_ties_min_votes_and_totals():
    U = 1 << 32
    count = np.array([[2, 1, 0], [1, 1, 0], [0, 0, 0], [3, 0, 0], [0, 2, 2], [1, 0, 1]], np.int64)
    weight = np.array([[U, U + U // 2, 0], [U // 2, U // 2, 0], [0, 0, 0], [2 * U, 0, 0], [0, -U, -U], [-U, 0, U]], np.int64)
    nsim = np.array([[0.6, 0.9, np.nan], [0.5, 0.5, np.nan], [np.nan] * 3, [0.8, np.nan, np.nan], [np.nan, -0.4, -0.3], [-1.0, np.nan, 1.0]],
                    np.float32)
    label, conf, margin = sequence.vote_predict(count, weight)                        # weight
    assert list(label) == [1, 0, -1, 0, 1, 2] and label.dtype == np.int64
    assert conf[0] == 1.5 / 2.5 and conf[1] == 0.5 and np.isnan(conf[2]) and conf[3] == 1.0
    assert np.isnan(conf[4]) and np.isnan(conf[5])                                    # totals -2 and 0: not positive
    assert margin[0] == 0.5 and margin[1] == 0.0 and np.isnan(margin[2]) and margin[3] == 2.0 and margin[4] == 0.0 and margin[5] == 2.0
    label, conf, margin = sequence.vote_predict(count, weight, "count")
    assert list(label) == [0, 0, -1, 0, 1, 0] and conf[0] == 2 / 3 and conf[4] == 0.5 and list(margin[[0, 1, 3]]) == [1.0, 0.0, 3.0]
    label, conf, margin = sequence.vote_predict(count, weight, "nearest", nsim)
    assert list(label) == [1, 0, -1, 0, 2, 2] and np.isnan(conf).all()
    assert np.allclose(margin[[0, 1, 3, 4, 5]], [0.3, 0.0, 0.8, 0.1, 2.0], atol=1e-6)
    label, _, _ = sequence.vote_predict(count, weight, "weight", min_votes=3)
    assert list(label) == [1, -1, -1, 0, 1, -1]
    # the integers decide: two weights that round to the same float64
    big = np.array([[(1 << 60) + 1, 1 << 60]], np.int64)
    assert list(sequence.vote_predict(np.array([[1, 1]]), big[:, ::-1])[0]) == [1]
    for bad in ({"rule": "mean"}, {"min_votes": 0}, {"min_votes": 1.5}, {"rule": "nearest"}):
        with pytest.raises(ValueError):
            sequence.vote_predict(count, weight, **bad)
    with pytest.raises(ValueError):
        sequence.vote_predict(count, weight[:, :2])


def test_argument_errors_of_the_definition_and_the_result_views():
    q, b = rows(4, 1), rows(3, 2)
    lab = np.array([0, 1, -1])
    for bad, match in (((q, b, np.array([0, 1, 2]), 2, 0.5), r"a label is outside \[-1, 2\)"), ((q, b, np.array([0, -2, 1]), 2, 0.5), "a label is outside"),
                       ((q, b, lab[:2], 2, 0.5), "one integer per base row"), ((q, b, lab.astype(float), 2, 0.5), "one integer per base row"),
                       ((q, None, lab, 2, 0.5), "one integer per base row"),
                       ((q, b, lab, 0, 0.5), r"n_classes 0.*\[1, 1024\]"), ((q, b, lab, 1025, 0.5), r"n_classes 1025.*\[1, 1024\]"),
                       ((q, b, lab, 2, float("nan")), "finite float"), ((q, b, lab, 2, float("inf")), "finite float"),
                       ((q[:, :100], b, lab, 2, 0.5), r"\(n, 512\)")):
        with pytest.raises(ValueError, match=match):
            sequence.class_votes(*bad)
    arrays = sequence.class_votes(q, b, lab, 3, -1.0)
    res = VoteResult.build(arrays, sequence.valid_rows(q), 3, -1.0)
    assert res.n_classes == 3 and res.threshold == -1.0 and res.query_valid.all() and sorted(res.asdict()) == sorted(VoteResult.FIELDS)
    assert np.array_equal(res.count, [[1, 1, 0]] * 4)
    s = sims(q, b)
    assert np.abs(res.similarity_sum()[:, :2] - s[:, :2]).max() <= 2.0 ** -32 and (res.similarity_sum()[:, 2] == 0).all()
    assert np.array_equal(np.isnan(res.mean_similarity()), res.count == 0)
    label, conf, margin = res.predict()
    assert np.array_equal(label, np.argmax(s[:, :2], axis=1)) and np.array_equal(res.predict("count")[0], [0] * 4)
    table = res.table(list("wxyz"), ["virus", "plasmid", "host"], ["b0", "b1", "b2"])
    assert [t["query"] for t in table] == list("wxyz") and table[0]["label"] == ("virus", "plasmid")[label[0]]
    assert table[0]["votes"] == 1 and table[0]["total_votes"] == 2 and table[0]["nearest"] == f"b{label[0]}"
    assert abs(table[0]["similarity"] - s[0, label[0]]) <= 1e-6 and abs(table[0]["confidence"] - conf[0]) == 0
    none = VoteResult.build(sequence.class_votes(q, b, lab, 3, 1.0), sequence.valid_rows(q), 3, 1.0).table()
    assert none[0] == {"query": 0, "label": None, "confidence": None, "votes": 0, "total_votes": 0, "nearest": None, "similarity": None}
    with pytest.raises(ValueError, match="count has the shape"):
        VoteResult.build(arrays, np.ones(5, bool), 3, 0.5)


def sims(q, b):
    from tests.neighbours_data import sims64
    return sims64(q, b)


def test_abi_declares_the_entry_points_and_checks_arguments_before_the_ctx():
    text = open(os.path.join(ROOT, "include", "genomad_nn.h")).read()
    lib = _lib.load()
    for name in ("gnn_vote", "gnn_vote_dev", "gnn_debug_set_vote_lds", "gnn_debug_vote_pass_ms"):
        assert f"int {name}(" in text and name in _lib.SIGNATURES and hasattr(lib, name)
    for m in ("vote", "vote_dev", "set_vote_lds", "vote_pass_ms"):
        assert hasattr(NNEngine, m)
    q = rows(2, 1)
    lab = np.zeros(2, np.int64)
    out = [np.full((2, 3), 7, np.int64) for _ in range(3)] + [np.full((2, 3), 7, np.float32)]
    qp, lp = q.ctypes.data, lab.ctypes.data
    op = [a.ctypes.data for a in out]
    for name in ("gnn_vote", "gnn_vote_dev"):
        fn = getattr(lib, name)
        call = lambda nq, nb, nc, t, base=qp: fn(None, qp, nq, base, nb, lp, nc, t, *op)        # noqa: E731
        for n in (-1, 1 << 31):
            assert call(n, 2, 3, 0.5) == _lib.ERR_ARG and f"{name}: n_query {n} is outside [0, 2^31)".encode() in lib.gnn_last_error()
        for n in (-1, (1 << 30) + 1):
            assert call(2, n, 3, 0.5) == _lib.ERR_ARG and f"{name}: {n} base rows is outside [0, 2^30]".encode() in lib.gnn_last_error()
        assert call((1 << 30) + 1, 0, 3, 0.5, None) == _lib.ERR_ARG and b"base rows is outside [0, 2^30]" in lib.gnn_last_error()    # the self form
        for nc in (0, 1025, -3):
            assert call(2, 2, nc, 0.5) == _lib.ERR_ARG and f"{name}: n_classes {nc} is outside [1, 1024]".encode() in lib.gnn_last_error()
        for t, word in ((float("nan"), b"nan"), (float("inf"), b"inf"), (1e39, b"inf")):
            assert call(2, 2, 3, t) == _lib.ERR_ARG
            assert name.encode() + b": threshold " + word in lib.gnn_last_error() and b"finite" in lib.gnn_last_error()
        for hole in range(6):
            args = [qp, lp] + op
            args[hole] = None
            assert fn(None, args[0], 2, qp, 2, args[1], 3, 0.5, *args[2:]) == _lib.ERR_ARG
            assert b"the query, the labels and the four outputs are required" in lib.gnn_last_error()
        for nq, nb, base in ((2, 2, qp), (2, 0, None), (0, 2, qp), (2, 0, qp)):
            assert call(nq, nb, 3, 0.5, base) == _lib.ERR_ARG and b"ctx is NULL" in lib.gnn_last_error()     # valid, but no ctx
    assert lib.gnn_debug_set_vote_lds(None, 3) == _lib.ERR_ARG and b"ctx is NULL" in lib.gnn_last_error()
    assert lib.gnn_debug_vote_pass_ms(None, None, 0, lp) == _lib.ERR_ARG and b"ctx is NULL" in lib.gnn_last_error()
    assert all((a == 7).all() for a in out)                      # nothing was written


# ---- main() over a fake engine ---------------------------------------------------------------------------------------------------
class FakeVoteEngine(FakeMatchEngine):
    """the stand-in of tests/test_match_host.py plus vote, served from sequence.class_votes"""

    def vote(self, query, base, label, n_classes, threshold):
        type(self).calls.append(("vote", len(query), None if base is None else len(base), int(n_classes), float(threshold)))
        return VoteResult.build(sequence.class_votes(query, base, label, n_classes, threshold), sequence.valid_rows(query), n_classes, threshold)


@pytest.fixture
def fake_main(monkeypatch):
    monkeypatch.setattr(nnc, "_engine", lambda: FakeVoteEngine())
    for k in (SWITCHES + ("GENOMAD_AMD_CLUSTERS", "GENOMAD_AMD_REPRESENTATIVES", "GENOMAD_AMD_LINKAGE", "GENOMAD_AMD_GRAPH", "GENOMAD_AMD_DENSITY",
                          "GENOMAD_AMD_KMEANS", "GENOMAD_AMD_PCA") + MATCH_SWITCHES + VOTE_SWITCHES):
        monkeypatch.delenv(k, raising=False)
    del FakeVoteEngine.calls[:]
    return lambda fa, out, **kw: nnc.main(fa, out, False, 128, False, 1, False, False, **kw)


def test_vote_switch_values(monkeypatch):
    for k in VOTE_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    assert nnc.vote_requested() is None and nnc.vote_base_requested() is None and nnc.vote_min_votes_requested() == 1
    for v, want in (("", None), (" 0.9 ", float(np.float32(0.9))), ("1", 1.0), ("-1", -1.0), ("5e-1", 0.5)):
        monkeypatch.setenv("GENOMAD_AMD_VOTE", v)
        assert nnc.vote_requested() == want
    for v in ("1.01", "-1.5", "nan", "inf", "high", "0,9"):
        monkeypatch.setenv("GENOMAD_AMD_VOTE", v)
        with pytest.raises(ValueError, match=r"GENOMAD_AMD_VOTE=.*\[-1, 1\]"):
            nnc.vote_requested()
    for v, want in (("", None), ("  ", None), (" ref/old.npz ", "ref/old.npz")):
        monkeypatch.setenv("GENOMAD_AMD_VOTE_BASE", v)
        got = nnc.vote_base_requested()
        assert (got is None) if want is None else (str(got) == want)
    for v, want in (("", 1), (" 3 ", 3), ("1", 1)):
        monkeypatch.setenv("GENOMAD_AMD_VOTE_MIN_VOTES", v)
        assert nnc.vote_min_votes_requested() == want
    for v in ("0", "-2", "1.5", "many"):
        monkeypatch.setenv("GENOMAD_AMD_VOTE_MIN_VOTES", v)
        with pytest.raises(ValueError, match=r"GENOMAD_AMD_VOTE_MIN_VOTES=.*integer >= 1"):
            nnc.vote_min_votes_requested()


def labelled_file(path, labels, seed=3, **extra):
    emb = rows(len(labels), seed)
    np.savez_compressed(path, **{"contig_names": np.array([f"ref{i}" for i in range(len(labels))]), "embeddings": emb,
                                 "labels": np.array(labels), **extra})
    return emb


def test_the_labelled_base_loader_names_every_fault(tmp_path):
    emb = labelled_file(tmp_path / "ok.npz", ["virus", "", "plasmid", "virus", "chromosome"])
    names, got, classes, label = nnc.load_vote_base(tmp_path / "ok.npz")
    assert list(names) == [f"ref{i}" for i in range(5)] and np.array_equal(got, emb) and got.dtype == np.float32 and got.flags.c_contiguous
    assert list(classes) == ["chromosome", "plasmid", "virus"] and list(label) == [2, -1, 1, 2, 0] and label.dtype == np.int64
    with pytest.raises(ValueError, match=r"GENOMAD_AMD_MATCH_BASE=.*one 1-D array of the 5 names"):
        nnc.load_match_base(tmp_path / "ok.npz")                 # the match's loader stays as it is: a second string array is refused
    labelled_file(tmp_path / "both.npz", ["a", "b"], strand=np.array("both"))
    assert list(nnc.load_vote_base(tmp_path / "both.npz", "both")[2]) == ["a", "b"]
    with pytest.raises(ValueError, match=r"GENOMAD_AMD_VOTE_BASE=.*GENOMAD_AMD_STRAND=both, this run's are under forward"):
        nnc.load_vote_base(tmp_path / "both.npz")
    with pytest.raises(ValueError, match=r"GENOMAD_AMD_VOTE_BASE=.*gone\.npz.*no such file"):
        nnc.load_vote_base(tmp_path / "gone.npz")
    (tmp_path / "text.npz").write_text("not an archive")
    with pytest.raises(ValueError, match=r"GENOMAD_AMD_VOTE_BASE=.*not a readable \.npz"):
        nnc.load_vote_base(tmp_path / "text.npz")
    np.savez_compressed(tmp_path / "narrow.npz", contig_names=np.array(["a", "b"]), labels=np.array(["x", "y"]), embeddings=np.zeros((2, 256), np.float32))
    with pytest.raises(ValueError, match=r"GENOMAD_AMD_VOTE_BASE=.*'embeddings' of shape \(n, 512\)"):
        nnc.load_vote_base(tmp_path / "narrow.npz")
    np.savez_compressed(tmp_path / "plain.npz", contig_names=np.array(["a", "b"]), embeddings=rows(2, 1))
    np.savez_compressed(tmp_path / "short.npz", contig_names=np.array(["a", "b"]), embeddings=rows(2, 1), labels=np.array(["x"]))
    np.savez_compressed(tmp_path / "ints.npz", contig_names=np.array(["a", "b"]), embeddings=rows(2, 1), labels=np.array([0, 1]))
    for bad in ("plain.npz", "short.npz", "ints.npz"):
        with pytest.raises(ValueError, match=r"GENOMAD_AMD_VOTE_BASE=.*'labels', a 1-D array of the 2 class names"):
            nnc.load_vote_base(tmp_path / bad)
    np.savez_compressed(tmp_path / "nonames.npz", embeddings=rows(2, 1), labels=np.array(["x", "y"]))
    with pytest.raises(ValueError, match=r"GENOMAD_AMD_VOTE_BASE=.*one 1-D array of the 2 names"):
        nnc.load_vote_base(tmp_path / "nonames.npz")
    labelled_file(tmp_path / "blank.npz", ["", ""])
    with pytest.raises(ValueError, match=r"GENOMAD_AMD_VOTE_BASE=.*no row has a label"):
        nnc.load_vote_base(tmp_path / "blank.npz")
    labelled_file(tmp_path / "many.npz", [f"c{i}" for i in range(1025)])
    with pytest.raises(ValueError, match=r"GENOMAD_AMD_VOTE_BASE=.*1025 classes, more than 1024"):
        nnc.load_vote_base(tmp_path / "many.npz")
    labelled_file(tmp_path / "most.npz", [f"c{i}" for i in range(1024)])
    assert len(nnc.load_vote_base(tmp_path / "most.npz")[2]) == 1024


def test_main_refuses_half_a_request_and_a_bad_base(tmp_path, monkeypatch, fake_main, capsys):
    fa = tmp_path / "s.fna"
    _write_fasta(fa, n=3)
    labelled_file(tmp_path / "ref.npz", ["a", "b", "", "a"])
    both = "GENOMAD_AMD_VOTE and GENOMAD_AMD_VOTE_BASE need each other and GENOMAD_AMD_EMBEDDINGS=1"

    def refused(message):
        capsys.readouterr()
        with pytest.raises(SystemExit) as exc:
            fake_main(fa, tmp_path / "refused")
        err = capsys.readouterr().err
        assert exc.value.code == 1 and message in err and len(err.strip().splitlines()) == 1, err
        assert FakeVoteEngine.calls == []                       # before any classification starts
        assert not (tmp_path / "refused" / "s_nn_classification").exists()

    for k, v, match in (("GENOMAD_AMD_VOTE", "1.5", "GENOMAD_AMD_VOTE="), ("GENOMAD_AMD_VOTE_MIN_VOTES", "0", "GENOMAD_AMD_VOTE_MIN_VOTES=")):
        monkeypatch.setenv(k, v)
        with pytest.raises(ValueError, match=match):
            fake_main(fa, tmp_path / "bad")
        assert not (tmp_path / "bad").exists()                  # before anything is written
        monkeypatch.delenv(k)
    monkeypatch.setenv("GENOMAD_AMD_EMBEDDINGS", "1")
    monkeypatch.setenv("GENOMAD_AMD_VOTE", "0.9")
    refused(both)                                               # the threshold without the base
    monkeypatch.delenv("GENOMAD_AMD_VOTE")
    monkeypatch.setenv("GENOMAD_AMD_VOTE_BASE", str(tmp_path / "ref.npz"))
    refused(both)                                               # the base without the threshold
    monkeypatch.setenv("GENOMAD_AMD_VOTE", "0.9")
    monkeypatch.delenv("GENOMAD_AMD_EMBEDDINGS")
    refused(both)                                               # both, without the embeddings
    monkeypatch.setenv("GENOMAD_AMD_EMBEDDINGS", "1")
    monkeypatch.setenv("GENOMAD_AMD_VOTE_BASE", str(tmp_path / "gone.npz"))
    refused("no such file")
    np.savez_compressed(tmp_path / "plain.npz", contig_names=np.array(["a", "b"]), embeddings=rows(2, 1))
    monkeypatch.setenv("GENOMAD_AMD_VOTE_BASE", str(tmp_path / "plain.npz"))
    refused("'labels', a 1-D array of the 2 class names")
    monkeypatch.setenv("GENOMAD_AMD_VOTE_BASE", str(tmp_path / "ref.npz"))
    monkeypatch.setenv("GENOMAD_AMD_STRAND", "both")
    refused("GENOMAD_AMD_STRAND=forward, this run's are under both")


def test_main_writes_both_files_follows_the_request_and_removes_stale_ones(tmp_path, monkeypatch, fake_main):
    fa = tmp_path / "m.fna"
    _write_fasta(fa, n=6)
    monkeypatch.setenv("GENOMAD_AMD_EMBEDDINGS", "1")
    fake_main(fa, tmp_path / "unset")
    assert not any(c[0] == "vote" for c in FakeVoteEngine.calls)
    d0 = tmp_path / "unset" / "m_nn_classification"
    emb = _npz(d0 / "m_nn_embeddings.npz")
    n = len(emb["contig_names"])
    # the reference: an earlier run's embeddings file with labels added - every contig finds itself there
    ref = tmp_path / "reference.npz"
    ref_names = np.array([f"old_{x}" for x in emb["contig_names"]])
    ref_labels = np.array((["virus", "plasmid", "", "virus", "plasmid", "host"] * n)[:n])
    np.savez_compressed(ref, contig_names=ref_names, embeddings=emb["embeddings"], labels=ref_labels)
    monkeypatch.setenv("GENOMAD_AMD_VOTE", "0.999")
    monkeypatch.setenv("GENOMAD_AMD_VOTE_BASE", str(ref))
    out = tmp_path / "on"
    fake_main(fa, out)
    d1 = out / "m_nn_classification"
    assert _tree(d1) == sorted(_tree(d0) + ["m_nn_votes.npz", "m_nn_votes.tsv"])
    for rel in _tree(d0):                                       # every other output: the same arrays, the same bytes
        if rel.endswith(".npz"):
            assert _same_npz(d0 / rel, d1 / rel), rel
        elif rel.endswith(".tsv"):
            assert (d0 / rel).read_bytes() == (d1 / rel).read_bytes(), rel
    z = _npz(d1 / "m_nn_votes.npz")
    t32 = float(np.float32(0.999))
    assert sorted(z) == sorted(["contig_names", "base_names", "base_label", "classes", "threshold", "min_votes", "count", "weight", "nearest",
                                "nearest_sim", "label", "confidence", "margin"])
    classes = ["host", "plasmid", "virus"]
    base_label = np.array([-1 if x == "" else classes.index(x) for x in ref_labels])
    assert list(z["classes"]) == classes and np.array_equal(z["base_label"], base_label) and list(z["base_names"]) == list(ref_names)
    assert float(z["threshold"]) == t32 and int(z["min_votes"]) == 1 and FakeVoteEngine.calls.count(("vote", n, n, 3, t32)) == 1
    want = sequence.class_votes(emb["embeddings"], emb["embeddings"], base_label, 3, 0.999)
    assert same([z[k] for k in sequence.VOTE_FIELDS], want)
    label, conf, margin = sequence.vote_predict(want[0], want[1])
    assert np.array_equal(z["label"], label) and np.array_equal(z["confidence"], conf, equal_nan=True) and np.array_equal(z["margin"], margin, equal_nan=True)
    valid = sequence.valid_rows(emb["embeddings"])
    labelled = valid & (base_label >= 0)
    assert labelled.sum() >= 3 and np.array_equal(label[labelled], base_label[labelled])       # every labelled contig finds itself
    lines = (d1 / "m_nn_votes.tsv").read_text().splitlines()
    assert lines[0] == "seq_name\tlabel\tconfidence\tvotes\ttotal_votes\tnearest\tsimilarity" and len(lines) == n + 1
    names = list(z["contig_names"])
    for i, line in enumerate(lines[1:]):
        if label[i] < 0:
            assert line == f"{names[i]}\tNA\tNA\t0\t{want[0][i].sum()}\tNA\tNA"
        else:
            c = label[i]
            assert line == (f"{names[i]}\t{classes[c]}\t{conf[i]:.6f}\t{want[0][i, c]}\t{want[0][i].sum()}\t{ref_names[want[2][i, c]]}\t"
                            f"{want[3][i, c]:.6f}")
    assert any(line.endswith("\tNA\tNA") for line in lines[1:]) and f"{names[0]}\tvirus\t1.000000\t1\t1\told_{names[0]}\t1.000000" in lines
    runs = lambda: sum(1 for c in FakeVoteEngine.calls if c == "plain")        # noqa: E731
    before = runs()
    fake_main(fa, out)
    assert runs() == before                                     # same request, everything there: nothing runs
    monkeypatch.setenv("GENOMAD_AMD_VOTE", "-1")
    fake_main(fa, out)                                          # another threshold: recomputed
    z = _npz(d1 / "m_nn_votes.npz")
    assert runs() == before + 1 and float(z["threshold"]) == -1.0 and z["count"][valid].sum() == valid.sum() * labelled.sum()
    monkeypatch.setenv("GENOMAD_AMD_VOTE_MIN_VOTES", "100")
    fake_main(fa, out)                                          # another min_votes: recomputed, and nobody has 100 voters
    z = _npz(d1 / "m_nn_votes.npz")
    assert runs() == before + 2 and int(z["min_votes"]) == 100 and (z["label"] == -1).all()
    assert all(line.endswith("\tNA\tNA") for line in (d1 / "m_nn_votes.tsv").read_text().splitlines()[1:])
    monkeypatch.delenv("GENOMAD_AMD_VOTE_MIN_VOTES")
    fake_main(fa, out)
    (d1 / "m_nn_votes.tsv").unlink()
    fake_main(fa, out)                                          # one of the pair is gone: recomputed
    assert runs() == before + 4 and (d1 / "m_nn_votes.tsv").exists()
    ref2 = tmp_path / "reference2.npz"
    relabelled = ref_labels.copy()
    relabelled[0] = "host"
    np.savez_compressed(ref2, contig_names=ref_names, embeddings=emb["embeddings"], labels=relabelled)
    monkeypatch.setenv("GENOMAD_AMD_VOTE_BASE", str(ref2))
    fake_main(fa, out)                                          # the same names under other labels: recomputed
    assert runs() == before + 5 and _npz(d1 / "m_nn_votes.npz")["base_label"][0] == 0
    res = VoteResult.build(want, valid, 3, 0.999)               # the strand is written where it is not forward
    nnc.write_votes(tmp_path / "v.npz", tmp_path / "v.tsv", "provirus_names", z["contig_names"], z["classes"], ref_names, base_label, res, 1, "both")
    v = _npz(tmp_path / "v.npz")
    assert str(v["strand"]) == "both" and "provirus_names" in v and nnc._npz_strand(d1 / "m_nn_votes.npz") == "forward"
    assert (tmp_path / "v.tsv").read_text().splitlines() == lines
    for k in VOTE_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    fake_main(fa, out)                                          # no request: both files go
    assert not (d1 / "m_nn_votes.npz").exists() and not (d1 / "m_nn_votes.tsv").exists()
    assert _tree(d1) == _tree(d0)
