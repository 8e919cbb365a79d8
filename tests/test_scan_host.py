"""CPU checks of the scan feature (score tracks along contigs): the window rule in its three forms (gnn_scan_plan, the vectorised
sequence.scan_spans, a plain loop) and against the reference's own seq_windows / Sequence / tokenize_dna, the track definition,
main()'s switch, and the rank-0 gather of the scan arrays."""
import ctypes as C
import os
import socket

import numpy as np
import pytest

from genomad_amd import _lib, sequence, sharding
from oracle import reference_harness, sequence_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, T = 6000, 2500
LENGTHS = [1, 29, 2499, 2500, 5999, 6000, 6001, 8499, 8500, 8501, 11999, 12000, 14499, 14500, 70000]
STRIDES = [8, 500, 1000, 2000, 3500, 3501, 4000, 5999, 6000]


def _rule_loop(length, stride, single_window):
    """the issue's rule, literally: [(start, len)] of one contig"""
    out = []
    k = 0
    while k * stride < length:
        l = min(W, length - k * stride)
        if k > 0 and (l < T or (k - 1) * stride + W >= length):
            break
        out.append((k * stride, l))
        if single_window:
            break
        k += 1
    return out


def _closed_form_count(length, stride):
    if length == 0:
        return 0
    kstar = max(0, -(-(length - W) // stride))
    return kstar + int(kstar == 0 or length - kstar * stride >= T)


def _plan(offsets, stride, single_window):
    lib = _lib.load()
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n = len(offsets) - 1
    nw, nb = C.c_int64(-1), C.c_int64(-1)
    head = (offsets.ctypes.data, n, stride, int(single_window), C.byref(nw), C.byref(nb))
    _lib.check(lib.gnn_scan_plan(*head, None, None, None, None))
    wo, bo = np.full(n + 1, -1, np.int64), np.full(n + 1, -1, np.int64)
    st, ln = np.full(nw.value, -1, np.int64), np.full(nw.value, -1, np.int32)
    _lib.check(lib.gnn_scan_plan(*head, wo.ctypes.data, bo.ctypes.data, st.ctypes.data, ln.ctypes.data))
    return nw.value, nb.value, wo, bo, st, ln


def _lengths():
    rng = np.random.default_rng(2024)
    return [0] + LENGTHS + [0, 0] + [int(x) for x in rng.integers(1, 200001, 400)]


@pytest.mark.parametrize("single_window", [False, True])
@pytest.mark.parametrize("stride", STRIDES)
def test_plan_equals_scan_spans_equals_the_rule(stride, single_window):
    lengths = _lengths()
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    want = [(c, a, l) for c, length in enumerate(lengths) for a, l in _rule_loop(length, stride, single_window)]
    starts, lens, ids, window_n, win_off, bin_off = sequence.scan_spans(offsets, stride, single_window)
    assert list(ids) == [w[0] for w in want]
    assert list(window_n.astype(np.int64) * stride) == [w[1] for w in want] and list(lens) == [w[2] for w in want]
    assert np.array_equal(starts, offsets[:-1][ids] + window_n.astype(np.int64) * stride)
    assert starts.dtype == np.int64 and lens.dtype == np.int32 and window_n.dtype == np.int32
    per_contig = np.diff(win_off)
    if not single_window:
        assert list(per_contig) == [_closed_form_count(length, stride) for length in lengths]
    else:
        assert list(per_contig) == [min(1, length) for length in lengths]
    assert list(np.diff(bin_off)) == [-(-length // stride) for length in lengths]
    partial = np.flatnonzero(lens < W)                     # one partial window per contig at most, and it is the last
    assert np.all(partial + 1 == win_off[1:][ids[partial]])
    nw, nb, wo, bo, st, ln = _plan(offsets, stride, single_window)
    assert nw == len(starts) and nb == int(bin_off[-1])
    assert np.array_equal(wo, win_off) and np.array_equal(bo, bin_off)
    assert np.array_equal(st, window_n.astype(np.int64) * stride) and np.array_equal(ln, lens)
    if stride == W:
        for a, b in zip(sequence.candidate_spans(offsets, single_window), (starts, lens, ids, window_n)):
            assert np.array_equal(a, b) and a.dtype == b.dtype


@pytest.mark.parametrize("single_window", [False, True])
def test_stride_one_on_short_contigs(single_window):
    lengths = [0, 1, 29, 2499, 2500, 5999, 6000, 6001, 8499, 8500, 8501]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    starts, lens, ids, window_n, win_off, bin_off = sequence.scan_spans(offsets, 1, single_window)
    want = [(c, a, l) for c, length in enumerate(lengths) for a, l in _rule_loop(length, 1, single_window)]
    assert [(int(c), int(k), int(l)) for c, k, l in zip(ids, window_n, lens)] == want
    assert list(np.diff(bin_off)) == lengths
    if not single_window:
        assert list(np.diff(win_off)) == [_closed_form_count(length, 1) for length in lengths]
    nw, nb, wo, bo, st, ln = _plan(offsets, 1, single_window)
    assert np.array_equal(wo, win_off) and np.array_equal(bo, bin_off) and np.array_equal(st, window_n) and np.array_equal(ln, lens)


def test_plan_and_scan_spans_refuse_bad_arguments():
    lib = _lib.load()
    off = np.array([0, 7000, 9000], np.int64)
    nw, nb = C.c_int64(), C.c_int64()
    for stride in (0, -3, 6001):
        assert lib.gnn_scan_plan(off.ctypes.data, 2, stride, 0, C.byref(nw), C.byref(nb), None, None, None, None) == _lib.ERR_ARG
        assert b"[1, 6000]" in lib.gnn_last_error()
        with pytest.raises(ValueError, match="6000"):
            sequence.scan_spans(off, stride)
    bad = np.array([0, 7000, 6999], np.int64)
    assert lib.gnn_scan_plan(bad.ctypes.data, 2, 1000, 0, C.byref(nw), C.byref(nb), None, None, None, None) == _lib.ERR_ARG
    with pytest.raises(ValueError, match="non-decreasing"):
        sequence.scan_spans(bad, 1000)
    assert lib.gnn_scan_plan(off.ctypes.data, 2, 1000, 0, C.byref(nw), C.byref(nb), None, None, None, None) == 0
    assert (nw.value, nb.value) == (2 + 1, 7 + 2)


# ---- against the reference's own code, executed live ----------------------------------------------------------------------------
FASTA_TEXT = (">a lower case and IUPAC\n" + "acgtRYKMswbdhvn" * 700 + "ACGT" * 900 + "\n"
              ">b N runs\n" + "ACGTTGCA" * 800 + "N" * 4500 + "GATTACA" * 1300 + "n" * 300 + "CCGT" * 500 + "\n"
              ">c short\n" + "ACGTN" * 120 + "\n"
              ">d long\n" + "TTGACCA" * 3000 + "\n")


def _records():
    out, name = [], None
    for line in FASTA_TEXT.splitlines():
        if line.startswith(">"):
            name = line[1:]
        else:
            out.append((name, line))
    return out


@pytest.mark.skipif(not reference_harness.available(), reason="the reference checkout is not on this machine")
@pytest.mark.parametrize("single_window", [False, True])
def test_stride_6000_is_the_references_seq_windows(single_window):
    ref = reference_harness.load_reference_sequence()
    rng = np.random.default_rng(7)
    lengths = LENGTHS + [int(x) for x in rng.integers(1, 40001, 60)]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    _, lens, ids, window_n, _, _ = sequence.scan_spans(offsets, W, single_window)
    want = []
    for c, length in enumerate(lengths):
        s = ref.Sequence(f"s{c}", "A" * length)
        want += [(c, k, len(win)) for k, win in enumerate(ref.seq_windows(s, W, T, max_windows=1 if single_window else None))]
    assert [(int(c), int(k), int(l)) for c, k, l in zip(ids, window_n, lens)] == want


@pytest.mark.skipif(not reference_harness.available(), reason="the reference checkout is not on this machine")
@pytest.mark.parametrize("stride", [500, 2000, 3501])
def test_window_content_is_the_references_slice_padded_and_tokenised(stride):
    ref = reference_harness.load_reference_sequence()
    recs = _records()
    seq = np.frombuffer("".join(s for _, s in recs).encode(), dtype=np.uint8)
    offsets = np.concatenate([[0], np.cumsum([len(s) for _, s in recs])]).astype(np.int64)
    starts, lens, ids, window_n, _, _ = sequence.scan_spans(offsets, stride)
    wins = sequence.materialize_spans(seq, starts, lens)
    tokens = sequence_oracle.tokenize_closed_form(wins)
    assert len(wins) > 10 and (lens < W).any() and (wins == ord("N")).any()
    pick = sorted(set(range(0, len(wins), 3)) | set(np.flatnonzero(lens < W).tolist()))
    for i in pick:
        s = ref.Sequence(*recs[int(ids[i])])
        k = int(window_n[i])
        want = s[k * stride:k * stride + W].seq_ascii.ljust(W, b"N")
        assert wins[i].tobytes() == want, i
        assert list(tokens[i]) == list(ref.tokenize_dna(want, 4)), i


# ---- the track ------------------------------------------------------------------------------------------------------------------
def test_track_definition_on_hand_made_scores():
    """one contig of 9000 bases at stride 2000: windows at 0 (6000 long) and 2000 (6000), the one at 4000 (5000) ends the scan;
    5 bins, the last 1000 wide.  A second contig of 7000 bases at the same stride: windows 0 and 2000 (5000); window 1 masked."""
    offsets = np.array([0, 9000, 16000, 16000, 16100], np.int64)
    starts, lens, ids, window_n, win_off, bin_off = sequence.scan_spans(offsets, 2000)
    assert list(window_n) == [0, 1, 2, 0, 1, 0] and list(lens) == [6000, 6000, 5000, 6000, 5000, 100]
    assert list(win_off) == [0, 3, 5, 5, 6] and list(bin_off) == [0, 5, 9, 9, 10]
    sc = np.array([[.1, .2, .7], [.3, .3, .4], [.6, .1, .3], [.5, .25, .25], [0, 0, 1], [1, 0, 0]], np.float32)
    kept = np.array([1, 1, 1, 1, 0, 1], bool)
    track, cover = sequence.scan_track(sc, kept, lens, win_off, bin_off, 2000)
    assert list(cover) == [1, 2, 3, 2, 1, 1, 1, 1, 0, 1]
    f = np.float32
    assert np.array_equal(track[0], sc[0]) and np.array_equal(track[1], (sc[0] + sc[1]) / f(2))
    assert np.array_equal(track[2], ((sc[0] + sc[1]) + sc[2]) / f(3))          # sequential f32 sum, one division
    assert np.array_equal(track[3], (sc[1] + sc[2]) / f(2)) and np.array_equal(track[4], sc[2])
    assert np.array_equal(track[5:8], np.stack([sc[3]] * 3))                   # the masked window does not enter
    assert np.isnan(track[8]).all()                                            # covered by the masked window only
    assert np.array_equal(track[9], sc[5])
    assert track.dtype == np.float32 and cover.dtype == np.int32


def test_track_dropped_tail_is_nan():
    """8400 bases at stride 6000: the 2400-base tail is dropped, its bin has no window"""
    offsets = np.array([0, 8400], np.int64)
    _, lens, _, _, win_off, bin_off = sequence.scan_spans(offsets, W)
    assert list(lens) == [6000] and list(bin_off) == [0, 2]
    track, cover = sequence.scan_track(np.array([[.2, .3, .5]], np.float32), np.array([True]), lens, win_off, bin_off, W)
    assert list(cover) == [1, 0] and np.isnan(track[1]).all() and not np.isnan(track[0]).any()


# ---- main() ---------------------------------------------------------------------------------------------------------------------
def test_scan_switch_values(monkeypatch):
    from genomad_amd import nn_classification as nnc
    monkeypatch.delenv("GENOMAD_AMD_SCAN_STRIDE", raising=False)
    assert nnc.scan_stride_requested() is None
    for v, want in (("", None), ("1", 1), ("2000", 2000), (" 6000 ", 6000)):
        monkeypatch.setenv("GENOMAD_AMD_SCAN_STRIDE", v)
        assert nnc.scan_stride_requested() == want
    for v in ("0", "6001", "-5", "1e3", "yes"):
        monkeypatch.setenv("GENOMAD_AMD_SCAN_STRIDE", v)
        with pytest.raises(ValueError, match=r"GENOMAD_AMD_SCAN_STRIDE.*\[1, 6000\]"):
            nnc.scan_stride_requested()


class _MustNotRun:
    def score(self, windows):
        raise AssertionError("classified although the scan cannot be produced on this path")

    def segment_mean(self, scores, ids, n_segments):
        raise AssertionError("classified although the scan cannot be produced on this path")


def test_main_with_scan_on_the_host_front_end_exits_before_classifying(tmp_path, monkeypatch, capsys):
    from genomad_amd import nn_classification as nnc
    fa = tmp_path / "s.fna"
    fa.write_text(">a\n" + "ACGT" * 2000 + "\n>b\n" + "GATTACA" * 900 + "\n")
    monkeypatch.setenv("GENOMAD_AMD_SCAN_STRIDE", "2000")
    with pytest.raises(SystemExit) as exc:
        nnc.main(fa, tmp_path / "out", False, 128, False, 1, False, False, _backend=_MustNotRun())
    assert exc.value.code == 1
    assert "GENOMAD_AMD_SCAN_STRIDE" in capsys.readouterr().err
    assert not list((tmp_path / "out").rglob("*.npz")) and not list((tmp_path / "out").rglob("*.tsv"))
    monkeypatch.setenv("GENOMAD_AMD_SCAN_STRIDE", "7000")
    with pytest.raises(ValueError, match="GENOMAD_AMD_SCAN_STRIDE"):
        nnc.main(fa, tmp_path / "out2", False, 128, False, 1, False, False, _backend=_MustNotRun())


def test_abi_declares_the_scan_entry_points():
    text = open(os.path.join(ROOT, "include", "genomad_nn.h")).read()
    lib = _lib.load()
    for name in ("gnn_scan_plan", "gnn_scan_contigs"):
        assert f"int {name}(" in text and name in _lib.SIGNATURES and hasattr(lib, name)
    from genomad_amd.engine import NNEngine
    assert hasattr(NNEngine, "scan_contigs") and hasattr(NNEngine, "scan_contigs_dev")


# ---- gather of the scan arrays (sharding.gather_contig_scans) --------------------------------------------------------------------
STRIDE = 1500


def _write_fasta(path):
    rng = np.random.default_rng(33)
    recs = [(f"c{i}", "".join(rng.choice(list("ACGTN"), int(rng.integers(500, 40000)), p=[.24, .24, .24, .24, .04])))
            for i in range(23)]
    path.write_text("".join(f">{n} note\n{s}\n" for n, s in recs))


def _fake_scan(seq, offsets):
    """stand-in for NNEngine.scan_contigs: the true window / bin tables, scores that depend only on each window's bytes"""
    offsets = np.asarray(offsets, np.int64)
    starts, lens, ids, window_n, win_off, bin_off = sequence.scan_spans(offsets, STRIDE)
    scores = np.zeros((len(starts), 3), np.float32)
    for i, (a, l) in enumerate(zip(starts, lens)):
        b = np.asarray(seq[a:a + l], dtype=np.int64)
        scores[i] = np.random.default_rng(int(b.sum()) * 31 + int(l)).random(3, dtype=np.float32)
    nn = np.array([np.count_nonzero(seq[a:a + l] == ord("N")) for a, l in zip(starts, lens)], dtype=np.int64)
    kept = (window_n == 0) | (nn <= 60)                    # a low bar, so that the mask is exercised
    track, cover = sequence.scan_track(scores, kept, lens, win_off, bin_off, STRIDE)
    return {"win_offsets": win_off, "starts": window_n.astype(np.int64) * STRIDE, "lens": lens, "kept": kept, "scores": scores,
            "bin_offsets": bin_off, "track": track, "cover": cover}


def _gloo_scan_worker(rank, world, port, path, q):
    from tests.gloo_comm import GlooComm
    comm = GlooComm(rank, world, port)
    parts = []
    for k in (2, 0, 1):               # three pieces per rank (some of them empty at world 3), handed over out of order
        _, seq, offsets = sequence.read_fasta_packed(path, True, sequence.record_aligned_range(path, rank, world, k, 3))
        parts.append((rank * 64 + k, _fake_scan(seq, offsets)))
    out = sharding.gather_contig_scans(comm, parts)
    if rank == 0:
        q.put(out)
    else:
        assert out is None
    comm.close()


def _assert_scans_equal(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k], equal_nan=got[k].dtype.kind == "f"), k


@pytest.mark.parametrize("world", [2, 3])
def test_gloo_contig_scans_gather_equals_single_process(tmp_path, world):
    mp = pytest.importorskip("torch.multiprocessing")
    p = tmp_path / "meta.fna"
    _write_fasta(p)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_scan_worker, args=(r, world, port, str(p), q)) for r in range(world)]
    for pr in procs:
        pr.start()
    got = q.get(timeout=180)
    for pr in procs:
        pr.join(timeout=180)
        assert pr.exitcode == 0
    _, s1, o1 = sequence.read_fasta_packed(p)
    want = _fake_scan(s1, o1)
    assert (~want["kept"]).any() and (want["cover"] == 0).any()
    _assert_scans_equal(got, want)


def test_contig_scans_gather_one_process_and_empty_pieces():
    rng = np.random.default_rng(1)
    seq = rng.choice(np.frombuffer(b"ACGTN", np.uint8), 90000)
    offsets = np.array([0, 100, 100, 20000, 47000, 47001, 90000], np.int64)
    whole = _fake_scan(seq, offsets)
    cut = lambda a, b: _fake_scan(seq[offsets[a]:offsets[b]], offsets[a:b + 1] - offsets[a])        # noqa: E731
    got = sharding.gather_contig_scans(None, [(7, cut(4, 6)), (0, cut(0, 3)), (3, cut(3, 3)), (5, cut(3, 4))])
    _assert_scans_equal(got, whole)
    empty = sharding.gather_contig_scans(None, [])
    assert list(empty["win_offsets"]) == [0] and empty["scores"].shape == (0, 3) and empty["track"].shape == (0, 3)
    with pytest.raises(ValueError, match="duplicate"):
        sharding.gather_contig_scans(None, [(0, cut(0, 3)), (0, cut(3, 4))])
