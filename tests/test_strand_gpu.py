"""Both strands on the MI355X (gnn_revcomp_spans_dev, gnn_classify_contigs_strand, gnn_scan_contigs_strand): the reverse windows byte
for byte against numpy, their scores against the fp64 oracle, bit identity with the entry points that exist and with the numpy
definitions applied to the device's own window scores, strand symmetry of `both`, the per-strand embedding fold, invariance under the
launch size / input location / call order, the error paths, and main() with GENOMAD_AMD_STRAND."""
import numpy as np
import pytest

from genomad_amd import _lib, sequence
from oracle import igloo_oracle, sequence_oracle
from tests.conftest import need_tables
from tests.test_embeddings_gpu import _contigs, _fasta, _setup_main
from tests.test_scan_gpu import _assert_fold, _assert_same, _assert_tables, _numpy_scan

pytestmark = pytest.mark.gpu

ARITH = ["f32", "f16x3", "bf16x3", "f16x3tc", "f16x3tk"]
TOL = 1e-4                                  # the project's tolerance on class scores (BASELINE config 2)
LENGTHS = [0, 1, 2, 3, 2499, 5999, 6000]
MODES = ("forward", "reverse", "both")


def test_revcomp_spans_dev_equals_the_numpy_definition(engine):
    rng = np.random.default_rng(41)
    alphabet = np.frombuffer(b"ACGTacgtNnRYKMSWBDHVrykmswbdhv-*", np.uint8)
    p = np.array([.11] * 8 + [.005] * 24)
    seq = rng.choice(alphabet, 30011, p=p / p.sum()).astype(np.uint8)
    seq[7001:12002] = ord("N")
    starts, lens = [], []
    for length in LENGTHS + [4, 5, 6, 7, 4001, 4002, 4003]:             # every start and length alignment mod 4
        for start in (0, 1, 2, 3, 6998, 6999, 7000, 7001, len(seq) - length):
            starts.append(start), lens.append(length)
    starts, lens = np.array(starts, np.int64), np.array(lens, np.int32)
    assert {(int(a) % 4, int(l) % 4) for a, l in zip(starts, lens)} >= {(i, j) for i in range(4) for j in range(4)}
    want = sequence.revcomp_spans(seq, starts, lens)
    n = len(starts)
    dseq, dout = engine.alloc(seq.nbytes), engine.alloc((n + 1) * _lib.WINDOW)
    try:
        dseq.upload(seq)
        dout.upload(np.full((n + 1) * _lib.WINDOW, 0x5A, np.uint8))       # a canary row behind the last window
        engine.revcomp_spans_dev(dseq.ptr, starts, lens, dout.ptr)
        got = dout.download((n + 1, _lib.WINDOW), np.uint8)
        assert np.array_equal(got[:n], want)
        assert (got[n] == 0x5A).all()
        engine.revcomp_spans_dev(dseq.ptr, starts[:0], lens[:0], dout.ptr)                 # no span: nothing happens
        with pytest.raises(_lib.GnnError, match="aligned"):
            engine.revcomp_spans_dev(dseq.ptr, starts[:1], lens[:1], dout.ptr + 2)
        with pytest.raises(_lib.GnnError, match="6000"):
            engine.revcomp_spans_dev(dseq.ptr, starts[:1], np.array([6001], np.int32), dout.ptr)
        # the window-level route: materialise, then classify_dev
        dsc = engine.alloc(n * 12)
        try:
            engine.revcomp_spans_dev(dseq.ptr, starts, lens, dout.ptr)
            engine.classify_dev(dout.ptr, n, dsc.ptr)
            engine.sync()
            assert np.array_equal(dsc.download((n, 3), np.float32), engine.classify(want))
        finally:
            dsc.free()
    finally:
        dseq.free(), dout.free()


@pytest.fixture(scope="module")
def oracle_rev_2000(synth_weights):
    """fp64 oracle scores of the numpy REVERSE windows of the stride-2000 scan of _contigs() (75 windows)"""
    seq, offsets = _contigs()
    ref = _numpy_scan(seq, offsets, 2000)
    ref["rev_wins"] = sequence.revcomp_spans(seq, ref["starts"], ref["lens"])
    tokens = sequence_oracle.tokenize_closed_form(ref["rev_wins"])
    ref["oracle_rev"] = np.concatenate([igloo_oracle.forward(tokens[a:a + 16], synth_weights, np.float64, literal=False)
                                        for a in range(0, len(tokens), 16)])
    return seq, offsets, ref


@pytest.mark.parametrize("prec", ARITH)
def test_reverse_window_scores_match_the_fp64_oracle(engine, oracle_rev_2000, prec, request):
    need_tables(request, prec)
    seq, offsets, ref = oracle_rev_2000
    assert len(ref["oracle_rev"]) == 75 and np.isfinite(ref["oracle_rev"]).all()
    res = engine.scan_contigs_strand(seq, offsets, 2000, "reverse", False, prec)
    _assert_tables(res, ref, 2000)
    assert res.strand == "reverse" and res.scores.dtype == np.float32 and res.scores.shape == ref["oracle_rev"].shape
    err = np.abs(res.scores.astype(np.float64) - ref["oracle_rev"]).max()
    print(f"\nreverse strand, scan stride 2000 {prec}: max |dscore| vs fp64 oracle over {len(res.scores)} windows = {err:.3e}")
    assert err <= TOL, f"{prec}: {err:.3e}"
    assert np.array_equal(res.scores, res.scores_rev)
    _assert_fold(res, len(offsets) - 1)


def _contig_mean(res, scores):
    want = np.zeros((len(res.win_offsets) - 1, 3), np.float32)
    for c in range(len(want)):
        s, k = np.zeros(3, np.float32), 0
        for i in range(int(res.win_offsets[c]), int(res.win_offsets[c + 1])):
            if res.kept[i]:
                s, k = s + scores[i], k + 1
        if k:
            want[c] = s / np.float32(k)
    return want


@pytest.mark.parametrize("single_window", [False, True])
@pytest.mark.parametrize("stride", [6000, 2000, 3501])
def test_strand_modes_are_bit_identical_to_what_exists_and_to_the_definitions(engine, stride, single_window):
    seq, offsets = _contigs()
    ref = _numpy_scan(seq, offsets, stride, single_window)
    rev_wins = sequence.revcomp_spans(seq, ref["starts"], ref["lens"])
    n_contigs = len(offsets) - 1
    for prec in ("f16x3tc", "bf16x3"):
        plain = engine.scan_contigs(seq, offsets, stride, single_window, prec)
        got = {m: engine.scan_contigs_strand(seq, offsets, stride, m, single_window, prec) for m in MODES}
        f, r = plain.scores, engine.classify(rev_wins, prec)
        assert np.array_equal(engine.classify(ref["wins"], prec), f)
        for m, res in got.items():
            assert res.strand == m
            _assert_tables(res, ref, stride)                             # window tables and the kept mask: the forward ones
            assert np.array_equal(res.cover, plain.cover)
            assert np.array_equal(res.scores_fwd, f) and np.array_equal(res.scores_rev, r)
            _assert_fold(res, n_contigs)                                 # track, cover, contig scores: numpy on the device's scores
        for k in plain.FIELDS:                                           # forward: today's scan in every field
            x, y = getattr(got["forward"], k), getattr(plain, k)
            assert np.array_equal(x, y, equal_nan=isinstance(x, np.ndarray) and x.dtype.kind == "f"), k
        assert np.array_equal(got["reverse"].scores, r)
        assert np.array_equal(got["both"].scores, sequence.strand_mean(f, r))
        assert not np.array_equal(f, r)
        if stride == 6000:
            sc, ids = engine.classify_contigs(seq, offsets, single_window, prec)
            _, emb0, _ = engine.embed_contigs(seq, offsets, single_window, prec)
            for m in MODES:
                for embed in (False, True):
                    s, i, e, cf, cr = engine.classify_contigs_strand(seq, offsets, m, single_window, prec, embed)
                    assert np.array_equal(s, got[m].contig_scores) and np.array_equal(i, ids)
                    assert np.array_equal(cf, sc) and np.array_equal(cf, _contig_mean(plain, f))
                    assert np.array_equal(cr, got["reverse"].contig_scores) and np.array_equal(cr, _contig_mean(plain, r))
                    assert (e is None) == (not embed)
                    if m == "forward":
                        assert np.array_equal(s, sc) and (not embed or np.array_equal(e, emb0))
                assert not s[4].any() and not cf[4].any() and not cr[4].any()          # the empty record: zero rows
            # under both: the mean of the combined window scores, not the half-sum of the two contig means
            both = engine.classify_contigs_strand(seq, offsets, "both", single_window, prec)[0]
            assert np.array_equal(both, _contig_mean(plain, sequence.strand_mean(f, r)))
    if not single_window:
        assert (~plain.kept).any() and (plain.cover == 0).any()


def test_both_is_the_same_on_a_contig_and_on_its_reverse_complement(engine):
    """contigs of at most one window of upper-case ACGT: the reverse window of the reverse complement is the forward window, so
    `both` averages the same two scores in the other order - the f32 addition commutes, bit for bit"""
    rng = np.random.default_rng(19)
    recs = ["".join(rng.choice(list("ACGT"), k)) for k in (6000, 100, 2500, 5999, 1, 4097)]
    rc = [r.translate(str.maketrans("ACGT", "TGCA"))[::-1] for r in recs]
    pack = lambda rs: (np.frombuffer("".join(rs).encode(), np.uint8).copy(),                         # noqa: E731
                       np.concatenate([[0], np.cumsum([len(r) for r in rs])]).astype(np.int64))
    for prec in ("f16x3tc", "f32"):
        a = engine.classify_contigs_strand(*pack(recs), "both", False, prec, True)
        b = engine.classify_contigs_strand(*pack(rc), "both", False, prec, True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        assert np.array_equal(a[3], b[4]) and np.array_equal(a[4], b[3])               # the strands swap
        assert not np.array_equal(a[3], a[4])


@pytest.mark.parametrize("single_window", [False, True])
def test_strand_embeddings_equal_the_mean_of_window_embeddings(engine, single_window):
    seq, offsets = _contigs()
    prec = "f16x3tc"
    starts, lens, ids, window_n = sequence.candidate_spans(offsets, single_window)
    nn = np.array([np.count_nonzero(seq[s:s + l] == ord("N")) for s, l in zip(starts, lens)])
    keep = (window_n == 0) | (nn <= sequence.MAX_N)
    ef = engine.embed(sequence.materialize_spans(seq, starts, lens), prec).astype(np.float64)
    er = engine.embed(sequence.revcomp_spans(seq, starts, lens), prec).astype(np.float64)
    n = len(offsets) - 1
    want = {m: np.zeros((n, 512)) for m in MODES}
    for c in range(n):
        sel = keep & (ids == c)
        if sel.any():
            want["forward"][c], want["reverse"][c] = ef[sel].mean(axis=0), er[sel].mean(axis=0)
            want["both"][c] = (ef[sel].sum(axis=0) + er[sel].sum(axis=0)) / (2 * sel.sum())
    for m in MODES:
        emb = engine.classify_contigs_strand(seq, offsets, m, single_window, prec, True)[2]
        assert emb.dtype == np.float32 and emb.shape == (n, 512) and not emb[4].any()
        err = np.abs(emb - want[m]) / np.maximum(1.0, np.abs(want[m]))                 # the bound of tests/test_embeddings_gpu.py
        print(f"\ncontig embeddings, strand {m}: max rel err vs f64 mean of engine.embed = {err.max():.3e}")
        assert err.max() <= 1e-6, (m, err.max())
    assert np.abs(want["forward"] - want["reverse"]).max() > 1e-2


def test_strand_results_do_not_depend_on_launch_size_input_location_or_call_order(synth_weights, engine):
    from genomad_amd.engine import NNEngine
    seq, offsets = _contigs()
    scans = {m: engine.scan_contigs_strand(seq, offsets, 2000, m) for m in MODES}
    cls = {m: engine.classify_contigs_strand(seq, offsets, m, False, "f16x3tc", True) for m in MODES}

    def same_cls(a, b):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    with NNEngine(0, synth_weights, chunk=4) as e2:                     # slabs of 16 windows, 8 spans under both: contigs straddle
        for m in ("both", "forward", "reverse"):
            _assert_same(e2.scan_contigs_strand(seq, offsets, 2000, m), scans[m])
            same_cls(e2.classify_contigs_strand(seq, offsets, m, False, "f16x3tc", True), cls[m])
        assert np.array_equal(e2.classify_contigs(seq, offsets)[0], cls["forward"][0])      # interleaved with what exists
        _assert_same(e2.scan_contigs(seq, offsets, 2000), engine.scan_contigs(seq, offsets, 2000))
        e2.lib.gnn_set_chunk(e2.ctx, 13)
        same_cls(e2.classify_contigs_strand(seq, offsets, "both", False, "f16x3tc", True), cls["both"])
        e2.lib.gnn_set_chunk(e2.ctx, 1)
        _assert_same(e2.scan_contigs_strand(seq, offsets, 2000, "both"), scans["both"])
    dev = engine.alloc(seq.nbytes)
    try:
        dev.upload(seq)
        for m in MODES:
            _assert_same(engine.scan_contigs_strand_dev(dev.ptr, offsets, 2000, m), scans[m])
            same_cls(engine.classify_contigs_strand_dev(dev.ptr, offsets, m, False, "f16x3tc", True), cls[m])
    finally:
        dev.free()
    assert np.array_equal(engine.embed_contigs(seq, offsets)[1], cls["forward"][2])
    _assert_same(engine.scan_contigs_strand(seq, offsets, 2000, "both"), scans["both"])


def test_strand_errors_leave_the_ctx_usable(engine):
    seq, offsets = _contigs()
    for bad in (3, -1, 77):
        with pytest.raises(_lib.GnnError, match=f"strand {bad} "):
            engine.classify_contigs_strand(seq, offsets, bad)
        with pytest.raises(_lib.GnnError, match=f"strand {bad} "):
            engine.scan_contigs_strand(seq, offsets, 2000, bad)
    with pytest.raises(_lib.GnnError, match=r"\[1, 6000\]"):
        engine.scan_contigs_strand(seq, offsets, 0, "both")
    with pytest.raises(_lib.GnnError, match="F16C6"):
        engine.classify_contigs_strand(seq, offsets, "both", False, "f16c6", True)
    off = np.ascontiguousarray(offsets, np.int64)
    n_contigs = len(off) - 1
    scores, ids, n = np.zeros((n_contigs, 3), np.float32), np.zeros(31, np.int64), _lib.C.c_int64()
    call = lambda cap: engine.lib.gnn_classify_contigs_strand(                                 # noqa: E731
        engine.ctx, seq.ctypes.data, 1, seq.nbytes, off.ctypes.data, n_contigs, 0, _lib.PRECISIONS["f16x3tc"], scores.ctypes.data,
        ids.ctypes.data, cap, _lib.C.byref(n), None, _lib.STRAND_BOTH, None, None)
    assert call(30) == _lib.ERR_ARG and b"31" in engine.lib.gnn_last_error()
    assert call(31) == 0                                                # the optional outputs may all be NULL
    want = engine.classify_contigs_strand(seq, offsets, "both")
    assert np.array_equal(scores, want[0]) and np.array_equal(ids[:n.value], want[1])
    nw, nb = 75, 88                                                     # the stride-2000 scan of _contigs() (tests/test_scan_gpu.py)
    ws, track = np.zeros((nw, 3), np.float32), np.zeros((nb, 3), np.float32)
    scan = lambda wcap, bcap: engine.lib.gnn_scan_contigs_strand(                              # noqa: E731
        engine.ctx, seq.ctypes.data, 1, seq.nbytes, off.ctypes.data, n_contigs, 2000, 0, _lib.PRECISIONS["f16x3tc"], ws.ctypes.data,
        None, wcap, track.ctypes.data, None, bcap, None, _lib.STRAND_REVERSE, None, None)
    assert scan(nw - 1, nb) == _lib.ERR_ARG and b"75" in engine.lib.gnn_last_error()
    assert scan(nw, nb - 1) == _lib.ERR_ARG and b"88" in engine.lib.gnn_last_error()
    assert scan(nw, nb) == 0
    res = engine.scan_contigs_strand(seq, offsets, 2000, "reverse")
    assert np.array_equal(ws, res.scores) and np.array_equal(track, res.track, equal_nan=True)
    c6 = engine.classify_contigs_strand(seq, offsets, "both", False, "f16c6")        # without an embedding the frozen mode runs
    assert np.isfinite(c6[0]).all()
    empty = engine.classify_contigs_strand(np.zeros(0, np.uint8), np.array([0, 0, 0]), "both", False, "f16x3tc", True)
    assert not empty[0].any() and len(empty[1]) == 0 and empty[2].shape == (2, 512)


# ---- main() -------------------------------------------------------------------------------------------------------------------
def test_main_both_strands_alone_and_with_scan_and_embeddings(engine, synth_weights, tmp_path, monkeypatch):
    nnc = _setup_main(tmp_path, monkeypatch, engine, synth_weights)
    fa = tmp_path / "m.fna"
    _fasta(fa)
    for k in ("GENOMAD_AMD_STRAND", "GENOMAD_AMD_SCAN_STRIDE", "GENOMAD_AMD_EMBEDDINGS"):
        monkeypatch.delenv(k, raising=False)
    nnc.main(fa, tmp_path / "off", False, 128, False, 1, False, False)
    monkeypatch.setenv("GENOMAD_AMD_STRAND", "forward")
    nnc.main(fa, tmp_path / "fwd", False, 128, False, 1, False, False)
    d_off, d_fwd = tmp_path / "off" / "m_nn_classification", tmp_path / "fwd" / "m_nn_classification"
    files = lambda d: sorted(str(p.relative_to(d)) for p in d.rglob("*"))      # noqa: E731
    assert files(d_off) == files(d_fwd)
    assert (d_off / "m_nn_classification.tsv").read_bytes() == (d_fwd / "m_nn_classification.tsv").read_bytes()
    a, b = np.load(d_off / "m_nn_classification.npz"), np.load(d_fwd / "m_nn_classification.npz")
    assert np.array_equal(a["predictions"], b["predictions"])
    names, seq, off = sequence.read_fasta_packed(fa)
    want = engine.classify_contigs_strand(seq, off, "both", False, "f16x3tc", True)
    monkeypatch.setenv("GENOMAD_AMD_STRAND", "both")
    nnc.main(fa, tmp_path / "both", False, 128, False, 1, False, False)
    d = tmp_path / "both" / "m_nn_classification"
    assert files(d) == sorted(files(d_off) + ["m_nn_strand.npz"])
    assert np.array_equal(np.load(d / "m_nn_classification.npz")["predictions"], want[0])
    s = np.load(d / "m_nn_strand.npz")
    assert str(s["strand"]) == "both" and list(s["contig_names"]) == list(names)
    assert np.array_equal(s["scores_fwd"], want[3]) and np.array_equal(s["scores_rev"], want[4])
    assert np.array_equal(s["scores_fwd"], a["predictions"])
    assert np.array_equal(s["max_abs_diff"], np.abs(want[3] - want[4]).max(axis=1)) and s["max_abs_diff"].max() > 100 * TOL
    assert np.array_equal(np.load(d / "m_encoded_sequences" / "m_seq_window_id.npz")["contig_ids"], want[1])
    monkeypatch.setenv("GENOMAD_AMD_SCAN_STRIDE", "2000")
    monkeypatch.setenv("GENOMAD_AMD_EMBEDDINGS", "1")
    nnc.main(fa, tmp_path / "all", False, 128, False, 1, False, False)
    d = tmp_path / "all" / "m_nn_classification"
    assert files(d) == sorted(files(d_off) + ["m_nn_strand.npz", "m_nn_scan.npz", "m_nn_embeddings.npz"])
    assert np.array_equal(np.load(d / "m_nn_classification.npz")["predictions"], want[0])
    assert np.array_equal(np.load(d / "m_nn_embeddings.npz")["embeddings"], want[2])
    res = engine.scan_contigs_strand(seq, off, 2000, "both", False, "f16x3tc")
    z = np.load(d / "m_nn_scan.npz")
    assert str(z["strand"]) == "both" and int(z["stride"]) == 2000
    for key, arr in (("window_scores", res.scores), ("window_scores_fwd", res.scores_fwd), ("window_scores_rev", res.scores_rev),
                     ("track", res.track), ("cover", res.cover), ("window_kept", res.kept), ("win_offsets", res.win_offsets)):
        assert z[key].dtype == arr.dtype and np.array_equal(z[key], arr, equal_nan=arr.dtype.kind == "f"), key
    # resume: the same request finds everything; forward again recomputes and drops the strand file
    calls = []
    real = type(engine).classify_contigs_strand
    monkeypatch.setattr(type(engine), "classify_contigs_strand", lambda self, *a, **k: calls.append(a[2]) or real(self, *a, **k))
    nnc.main(fa, tmp_path / "all", False, 128, False, 1, False, False)
    assert calls == []
    monkeypatch.setenv("GENOMAD_AMD_STRAND", "reverse")
    nnc.main(fa, tmp_path / "all", False, 128, False, 1, False, False)
    assert calls == ["reverse"] and str(np.load(d / "m_nn_strand.npz")["strand"]) == "reverse"
    assert np.array_equal(np.load(d / "m_nn_classification.npz")["predictions"], want[4])
    for k in ("GENOMAD_AMD_STRAND", "GENOMAD_AMD_SCAN_STRIDE", "GENOMAD_AMD_EMBEDDINGS"):
        monkeypatch.delenv(k)
    nnc.main(fa, tmp_path / "all", False, 128, False, 1, False, False)
    assert not (d / "m_nn_strand.npz").exists()
    assert np.array_equal(np.load(d / "m_nn_classification.npz")["predictions"], a["predictions"])
