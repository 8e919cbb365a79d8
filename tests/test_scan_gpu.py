"""Score tracks on the MI355X (gnn_scan_contigs): every scan window against the fp64 oracle, bit identity with the entry points that
exist (classify on the materialised windows, classify_contigs at stride 6000), the track fold against its numpy definition,
invariance under the launch size / input location / call order, the error paths, and main() with GENOMAD_AMD_SCAN_STRIDE."""
import json

import numpy as np
import pytest

from genomad_amd import _lib, sequence
from oracle import igloo_oracle, sequence_oracle
from tests.conftest import need_tables
from tests.test_embeddings_gpu import _contigs, _fasta, _setup_main

pytestmark = pytest.mark.gpu

ARITH = ["f32", "f16x3", "bf16x3", "f16x3tc", "f16x3tk"]
TOL = 1e-4                                  # the project's tolerance on class scores (BASELINE config 2)
COUNTS = {6000: (31, 33), 2000: (75, 88), 1000: (138, 171)}      # (windows, bins) of _contigs(), counted on the CPU


def _numpy_scan(seq, offsets, stride, single_window=False):
    """the scan's tables and masks from the host rules: spans, materialised windows, the N rule on the raw bytes"""
    starts, lens, ids, window_n, win_off, bin_off = sequence.scan_spans(offsets, stride, single_window)
    nn = np.array([np.count_nonzero(seq[a:a + l] == ord("N")) for a, l in zip(starts, lens)], dtype=np.int64)
    kept = (window_n == 0) | (nn <= sequence.MAX_N)
    return dict(starts=starts, lens=lens, ids=ids, window_n=window_n, win_off=win_off, bin_off=bin_off, kept=kept,
                wins=sequence.materialize_spans(seq, starts, lens))


def _assert_tables(res, ref, stride):
    assert res.stride == stride
    assert np.array_equal(res.win_offsets, ref["win_off"]) and np.array_equal(res.bin_offsets, ref["bin_off"])
    assert np.array_equal(res.starts, ref["window_n"].astype(np.int64) * stride) and np.array_equal(res.lens, ref["lens"])
    assert res.kept.dtype == bool and np.array_equal(res.kept, ref["kept"])


def _assert_fold(res, n_contigs):
    """track, cover and contig scores are the numpy definitions applied to the device's own window scores, bit for bit"""
    track, cover = sequence.scan_track(res.scores, res.kept, res.lens, res.win_offsets, res.bin_offsets, res.stride)
    assert np.array_equal(res.cover, cover) and res.cover.dtype == np.int32
    assert np.array_equal(np.isnan(res.track), np.isnan(track))
    assert np.array_equal(res.track.view(np.uint32)[~np.isnan(track)], track.view(np.uint32)[~np.isnan(track)])
    assert np.array_equal(np.isnan(res.track).all(axis=1), res.cover == 0) and not np.isnan(res.track[res.cover > 0]).any()
    want = np.zeros((n_contigs, 3), np.float32)
    for c in range(n_contigs):
        s, k = np.zeros(3, np.float32), 0
        for i in range(int(res.win_offsets[c]), int(res.win_offsets[c + 1])):
            if res.kept[i]:
                s, k = s + res.scores[i], k + 1
        if k:
            want[c] = s / np.float32(k)
    assert np.array_equal(res.contig_scores, want)


def _assert_same(a, b):
    for k in a.FIELDS:
        x, y = getattr(a, k), getattr(b, k)
        assert np.array_equal(x, y, equal_nan=isinstance(x, np.ndarray) and x.dtype.kind == "f"), k


@pytest.fixture(scope="module")
def oracle_2000(synth_weights):
    """fp64 oracle scores of the scan windows of _contigs() at stride 2000, cut by scan_spans in numpy"""
    seq, offsets = _contigs()
    ref = _numpy_scan(seq, offsets, 2000)
    tokens = sequence_oracle.tokenize_closed_form(ref["wins"])
    ref["oracle"] = np.concatenate([igloo_oracle.forward(tokens[a:a + 16], synth_weights, np.float64, literal=False)
                                    for a in range(0, len(tokens), 16)])
    return seq, offsets, ref


def test_the_chosen_contigs_exercise_the_mask_the_nan_bins_and_differ(oracle_2000):
    """checked in numpy before anything is asked of the device: window and bin counts, a window masked by the N rule (the all-N
    window at 6000 of the third contig), a NaN bin (the last bin of the last contig, covered only by its masked final window),
    and oracle scores that are not alike - the parity test below would be vacuous on windows that all score the same"""
    seq, offsets, ref = oracle_2000
    for stride, (n_win, n_bins) in COUNTS.items():
        r = _numpy_scan(seq, offsets, stride)
        assert (len(r["starts"]), int(r["bin_off"][-1])) == (n_win, n_bins), stride
    w0 = int(ref["win_off"][2])
    assert ref["window_n"][w0 + 3] == 3 and not ref["kept"][w0 + 3] and (ref["wins"][w0 + 3] == ord("N")).all()
    track, cover = sequence.scan_track(ref["oracle"], ref["kept"], ref["lens"], ref["win_off"], ref["bin_off"], 2000)
    assert cover[-1] == 0 and np.isnan(track[-1]).all() and not ref["kept"][-1]
    assert np.isfinite(ref["oracle"]).all()
    spread = np.ptp(ref["oracle"], axis=0).max()
    print(f"\noracle scores over the {len(ref['oracle'])} scan windows: max spread per class {spread:.3e}")
    assert spread > 100 * TOL                          # windows differ by far more than what the parity test tolerates


@pytest.mark.parametrize("prec", ARITH)
def test_scan_window_scores_match_the_fp64_oracle(engine, oracle_2000, prec, request):
    need_tables(request, prec)
    seq, offsets, ref = oracle_2000
    res = engine.scan_contigs(seq, offsets, 2000, False, prec)
    _assert_tables(res, ref, 2000)
    assert res.scores.dtype == np.float32 and res.scores.shape == ref["oracle"].shape
    err = np.abs(res.scores.astype(np.float64) - ref["oracle"]).max()
    print(f"\nscan stride 2000 {prec}: max |dscore| vs fp64 oracle over {len(res.scores)} windows = {err:.3e}")
    assert err <= TOL, f"{prec}: {err:.3e}"
    assert (~res.kept).any() and (res.cover == 0).any()
    _assert_fold(res, len(offsets) - 1)


@pytest.mark.parametrize("single_window", [False, True])
@pytest.mark.parametrize("stride", [6000, 2000, 1000, 3501, 500])
def test_scan_is_bit_identical_to_what_exists(engine, stride, single_window):
    seq, offsets = _contigs()
    ref = _numpy_scan(seq, offsets, stride, single_window)
    for prec in ("f16x3tc", "bf16x3"):
        res = engine.scan_contigs(seq, offsets, stride, single_window, prec)
        _assert_tables(res, ref, stride)
        assert np.array_equal(res.scores, engine.classify(ref["wins"], prec))
        _assert_fold(res, len(offsets) - 1)
        if stride == 6000:
            scores, ids = engine.classify_contigs(seq, offsets, single_window, prec)
            assert np.array_equal(res.contig_scores, scores)
            assert np.array_equal(ref["ids"][res.kept], ids)
        assert not res.contig_scores[4].any()                        # the empty record: zero row
    if not single_window:
        assert (~res.kept).any() and (res.cover == 0).any()


def test_scan_does_not_depend_on_launch_size_input_location_or_call_order(synth_weights, engine):
    """4 windows per launch: slabs of 16 windows split contigs and runs of overlapping windows"""
    from genomad_amd.engine import NNEngine
    seq, offsets = _contigs()
    want = {s: engine.scan_contigs(seq, offsets, s) for s in (2000, 1000, 6000)}
    with NNEngine(0, synth_weights, chunk=4) as e2:
        for s in (6000, 1000, 2000):                                 # grow-only buffers: small, large, in between
            _assert_same(e2.scan_contigs(seq, offsets, s), want[s])
        assert np.array_equal(e2.classify_contigs(seq, offsets)[0], want[6000].contig_scores)
        e2.lib.gnn_set_chunk(e2.ctx, 13)
        _assert_same(e2.scan_contigs(seq, offsets, 1000), want[1000])
    dev = engine.alloc(seq.nbytes)
    try:
        dev.upload(seq)
        for s in (1000, 2000):
            _assert_same(engine.scan_contigs_dev(dev.ptr, offsets, s), want[s])
    finally:
        dev.free()
    _assert_same(engine.scan_contigs(seq, offsets, 2000), want[2000])


def test_scan_optional_outputs_may_be_null(engine):
    seq, offsets = _contigs()
    full = engine.scan_contigs(seq, offsets, 2000)
    n = len(full.scores)
    scores = np.zeros((n, 3), np.float32)
    off = np.ascontiguousarray(offsets, np.int64)
    _lib.check(engine.lib.gnn_scan_contigs(engine.ctx, seq.ctypes.data, 1, seq.nbytes, off.ctypes.data, len(off) - 1, 2000, 0,
                                           _lib.PRECISIONS["f16x3tc"], scores.ctypes.data, None, n, None, None, 0, None))
    assert np.array_equal(scores, full.scores)
    empty = engine.scan_contigs(np.zeros(0, np.uint8), np.array([0, 0, 0]), 2000)
    assert empty.scores.shape == (0, 3) and empty.track.shape == (0, 3) and not empty.contig_scores.any()


def test_scan_errors_leave_the_ctx_usable(engine):
    seq, offsets = _contigs()
    for stride in (0, 6001):
        with pytest.raises(_lib.GnnError, match=r"\[1, 6000\]"):
            engine.scan_contigs(seq, offsets, stride)
    off = np.ascontiguousarray(offsets, np.int64)
    n, nb = COUNTS[2000]
    scores, track = np.zeros((n, 3), np.float32), np.zeros((nb, 3), np.float32)
    call = lambda wcap, bcap: engine.lib.gnn_scan_contigs(                                    # noqa: E731
        engine.ctx, seq.ctypes.data, 1, seq.nbytes, off.ctypes.data, len(off) - 1, 2000, 0, _lib.PRECISIONS["f16x3tc"],
        scores.ctypes.data, None, wcap, track.ctypes.data, None, bcap, None)
    assert call(n - 1, nb) == _lib.ERR_ARG and str(n).encode() in engine.lib.gnn_last_error()
    assert call(n, nb - 1) == _lib.ERR_ARG and str(nb).encode() in engine.lib.gnn_last_error()
    assert call(n, nb) == 0
    res = engine.scan_contigs(seq, offsets, 2000)                                              # the ctx is usable afterwards
    assert np.array_equal(res.scores, scores) and np.array_equal(res.track, track, equal_nan=True)
    c6 = engine.scan_contigs(seq, offsets, 2000, False, "f16c6")         # the contig path accepts the frozen mode: so does the scan
    assert np.array_equal(c6.scores, engine.classify(_numpy_scan(seq, offsets, 2000)["wins"], "f16c6"))


# ---- every family on one ctx ---------------------------------------------------------------------------------------------------
EDGE_LENS = [0, 1, 2499, 2500, 20600, 6000, 8499, 8500, 12001, 3000]       # the window rule's edges, and one contig for the N rule


def _edge_contigs():
    """ten contigs in lower and upper case; the fifth has a later window the N rule drops (4001 N) and one it keeps (exactly 4000)"""
    rng = np.random.default_rng(20261018)
    alphabet = np.frombuffer(b"ACGTacgt", np.uint8)
    parts = [alphabet[rng.integers(0, 8, n)] for n in EDGE_LENS]
    parts[4][6000:6000 + sequence.MAX_N + 1] = ord("N")
    parts[4][12000 + 17:12000 + 17 + sequence.MAX_N] = ord("N")
    return np.concatenate(parts), np.concatenate([[0], np.cumsum(EDGE_LENS)]).astype(np.int64)


def _bits(res):
    """a call's result as (dtype, shape, bytes) per array: equality of these is equality bit for bit, NaN payloads included"""
    vals = [getattr(res, k) for k in res.FIELDS] if hasattr(res, "FIELDS") else list(res)
    return [(a.dtype, a.shape, a.tobytes()) for a in map(np.asarray, vals)]


# the calls of the interleaved sequence: (name, host-array variant?, call on (engine, packed bytes or device address, offsets, prec))
FAMILY_CALLS = [
    ("classify", True, lambda e, s, o, p: e.classify_contigs(s, o, False, p)),
    ("occlude", False, lambda e, s, o, p: e.occlude_contigs_dev(s, o, 1500, False, p)),
    ("scan", True, lambda e, s, o, p: e.scan_contigs(s, o, 2000, False, p)),
    ("strand both + embeddings", False, lambda e, s, o, p: e.classify_contigs_strand_dev(s, o, "both", False, p, True)),
    ("scan strand", True, lambda e, s, o, p: e.scan_contigs_strand(s, o, 3501, "both", False, p)),
    ("embed", False, lambda e, s, o, p: e.embed_contigs_dev(s, o, False, p)),
    ("classify again", True, lambda e, s, o, p: e.classify_contigs(s, o, False, p)),
]


def _run_calls(synth_weights, seq, offsets, prec, calls):
    """the calls in order on ONE fresh ctx of 2 windows per launch (slabs of 8 windows, 4 under both strands: every call needs
    several), the *_dev ones on a device copy of the packed bytes"""
    from genomad_amd.engine import NNEngine
    with NNEngine(0, synth_weights, chunk=2) as eng:
        dev = eng.alloc(seq.nbytes)
        try:
            dev.upload(seq)
            return [_bits(call(eng, seq if on_host else dev.ptr, offsets, prec)) for _, on_host, call in calls]
        finally:
            dev.free()


def test_the_edge_contigs_sit_on_the_window_and_n_rules():
    seq, offsets = _edge_contigs()
    starts, lens, ids, window_n = sequence.candidate_spans(offsets, False)
    assert np.bincount(ids, minlength=10).tolist() == [0, 1, 1, 1, 4, 1, 1, 2, 2, 1]       # 8499: tail dropped; 8500: tail kept
    assert lens[ids == 7].tolist() == [6000, 2500] and lens[ids == 8].tolist() == [6000, 6000]
    nn = np.array([np.count_nonzero(seq[a:a + n] == ord("N")) for a, n in zip(starts, lens)])
    assert nn[ids == 4].tolist() == [0, sequence.MAX_N + 1, sequence.MAX_N, 0] and window_n[ids == 4].tolist() == [0, 1, 2, 3]
    assert np.isin(seq, np.frombuffer(b"acgt", np.uint8)).any() and np.isin(seq, np.frombuffer(b"ACGT", np.uint8)).any()


@pytest.mark.parametrize("prec", ["f16x3tc", "bf16x3"])
def test_all_families_interleaved_on_one_ctx_equal_each_call_made_first_on_a_fresh_ctx(synth_weights, engine, prec):
    """classify, occlude, scan, strand-both with embeddings, scan-strand, embed, classify - host arrays and resident buffers in
    turn, so the sequence feed and the already-resident path interleave on one workspace - against each call made alone"""
    seq, offsets = _edge_contigs()
    got = _run_calls(synth_weights, seq, offsets, prec, FAMILY_CALLS)
    for i, call in enumerate(FAMILY_CALLS[:-1]):
        assert got[i] == _run_calls(synth_weights, seq, offsets, prec, [call])[0], call[0]
    assert got[6] == got[0]
    kept = np.frombuffer(got[2][4][2], bool)                  # the scan's mask: the N rule dropped a window, on this input too
    assert not kept.all() and kept.any()


# ---- main() -------------------------------------------------------------------------------------------------------------------
SCAN_KEYS = ["bin_offsets", "contig_names", "cover", "stride", "track", "win_offsets", "window_kept", "window_len", "window_scores",
             "window_start"]


def _assert_scan_file(path, res, names, names_key="contig_names"):
    z = np.load(path)
    assert sorted(z.files) == sorted([names_key if k == "contig_names" else k for k in SCAN_KEYS])
    assert list(z[names_key]) == list(names) and int(z["stride"]) == res.stride
    for key, want in (("win_offsets", res.win_offsets), ("window_start", res.starts), ("window_len", res.lens),
                      ("window_kept", res.kept), ("window_scores", res.scores), ("bin_offsets", res.bin_offsets),
                      ("track", res.track), ("cover", res.cover)):
        assert z[key].dtype == want.dtype and np.array_equal(z[key], want, equal_nan=want.dtype.kind == "f"), key


def test_main_writes_the_scan_only_when_asked(engine, synth_weights, tmp_path, monkeypatch):
    nnc = _setup_main(tmp_path, monkeypatch, engine, synth_weights)
    fa = tmp_path / "m.fna"
    _fasta(fa)
    monkeypatch.delenv("GENOMAD_AMD_SCAN_STRIDE", raising=False)
    nnc.main(fa, tmp_path / "off", False, 128, False, 1, False, False)
    monkeypatch.setenv("GENOMAD_AMD_SCAN_STRIDE", "2000")
    nnc.main(fa, tmp_path / "on", False, 128, False, 1, False, False)
    d_off, d_on = tmp_path / "off" / "m_nn_classification", tmp_path / "on" / "m_nn_classification"
    files = lambda d: sorted(str(p.relative_to(d)) for p in d.rglob("*"))      # noqa: E731
    assert files(d_on) == sorted(files(d_off) + ["m_nn_scan.npz"])
    for rel in ("m_nn_classification.npz", "m_encoded_sequences/m_seq_window_id.npz"):
        a, b = np.load(d_off / rel), np.load(d_on / rel)
        assert sorted(a.files) == sorted(b.files) and all(np.array_equal(a[k], b[k]) for k in a.files)
    assert (d_off / "m_nn_classification.tsv").read_bytes() == (d_on / "m_nn_classification.tsv").read_bytes()
    ja = json.loads((d_off / "m_nn_classification.json").read_text())
    jb = json.loads((d_on / "m_nn_classification.json").read_text())
    assert ja["parameters"] == jb["parameters"] == {"single_window": False}
    names, seq, off = sequence.read_fasta_packed(fa)
    res = engine.scan_contigs(seq, off, 2000, False, "f16x3tc")
    _assert_scan_file(d_on / "m_nn_scan.npz", res, names)
    assert np.array_equal(np.load(d_on / "m_nn_classification.npz")["predictions"], engine.classify_contigs(seq, off)[0])


def test_main_scan_provirus_pass_and_resume(engine, synth_weights, tmp_path, monkeypatch):
    nnc = _setup_main(tmp_path, monkeypatch, engine, synth_weights)
    fa = tmp_path / "v.fna"
    recs = _fasta(fa)
    out = tmp_path / "out"
    fp = out / "v_find_proviruses"
    fp.mkdir(parents=True)
    (fp / "v_find_proviruses.json").write_text(json.dumps({"input_md5": nnc.get_md5(fa), "module": "x", "parameters": {}}))
    (fp / "v_provirus.tsv").write_text("h\nk1|provirus_1_9000\n")
    (fp / "v_provirus.fna").write_text(">k1|provirus_1_9000\n" + recs[1][1][:9000] + "\n>k2|provirus_5_3000\n" + recs[2][1][4:3000] + "\n")
    (fp / "v_provirus_proteins.faa").write_text("")
    (fp / "v_provirus_genes.tsv").write_text("")
    monkeypatch.delenv("GENOMAD_AMD_SCAN_STRIDE", raising=False)
    nnc.main(fa, out, False, 128, False, 1, False, False)               # a run without the scan ...
    d = out / "v_nn_classification"
    assert not (d / "v_nn_scan.npz").exists() and not (d / "v_provirus_nn_scan.npz").exists()
    first = np.load(d / "v_nn_classification.npz")["predictions"]
    calls = []
    real = type(engine).scan_contigs
    monkeypatch.setattr(type(engine), "scan_contigs", lambda self, *a, **k: calls.append(a[2]) or real(self, *a, **k))
    monkeypatch.setenv("GENOMAD_AMD_SCAN_STRIDE", "2000")
    nnc.main(fa, out, False, 128, False, 1, False, False)               # ... then asked for it: the stages run again
    assert calls == [2000, 2000]                                        # one piece of the input, one of the proviruses
    assert np.array_equal(np.load(d / "v_nn_classification.npz")["predictions"], first)
    names, seq, off = sequence.read_fasta_packed(fa)
    _assert_scan_file(d / "v_nn_scan.npz", real(engine, seq, off, 2000), names)
    pn, pseq, poff = sequence.read_fasta_packed(fp / "v_provirus.fna")
    assert list(pn) == ["k1|provirus_1_9000", "k2|provirus_5_3000"]
    _assert_scan_file(d / "v_provirus_nn_scan.npz", real(engine, pseq, poff, 2000), pn, "provirus_names")
    del calls[:]
    nnc.main(fa, out, False, 128, False, 1, False, False)               # same stride, everything there: nothing is scanned
    assert calls == []
    monkeypatch.setenv("GENOMAD_AMD_SCAN_STRIDE", "1000")
    nnc.main(fa, out, False, 128, False, 1, False, True)                # another stride: scanned again (--cleanup keeps the file)
    assert calls == [1000, 1000]
    _assert_scan_file(d / "v_nn_scan.npz", real(engine, seq, off, 1000), names)
    assert np.array_equal(np.load(d / "v_nn_classification.npz")["predictions"], first)
    assert json.loads((d / "v_nn_classification.json").read_text())["parameters"] == {"single_window": False}
