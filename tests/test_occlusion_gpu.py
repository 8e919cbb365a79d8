"""Occlusion maps on the MI355X (gnn_occlude_spans_dev, gnn_occlude_contigs): the occluded windows byte for byte against the numpy
definition, base scores and deltas against the fp64 oracle, every score bit for bit against classify() on numpy-built windows and
against scan_contigs / classify_contigs, invariance under the launch size and where the sequence lives, the error paths, and main()
end to end with GENOMAD_AMD_OCCLUSION_BLOCK."""
import numpy as np
import pytest

from genomad_amd import _lib, sequence
from oracle import igloo_oracle, sequence_oracle
from tests.conftest import need_tables
from tests.test_embeddings_gpu import _contigs, _fasta, _setup_main
from tests.test_occlusion_host import FIELDS, oracle_occlusion_1500

pytestmark = pytest.mark.gpu

ARITH = ["f32", "f16x3", "bf16x3", "f16x3tc", "f16x3tk"]
TOL = 1e-4                                  # the project's tolerance on class scores
LENGTHS = [0, 1, 2, 3, 2499, 5999, 6000]


def test_occlude_spans_dev_equals_the_numpy_definition(engine):
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
    n = len(starts)
    # intervals: every pair of residues mod 4 of (lo, hi), cycling over the spans; the empty one; the whole row; hi inside the pad
    pairs = [(8 + i, 40 + 4 * i + j) for i in range(4) for j in range(4)] + [(0, 0), (0, 6000), (5999, 6000), (3, 3)]
    lo = np.array([pairs[k % len(pairs)][0] for k in range(n)], np.int32)
    hi = np.array([pairs[k % len(pairs)][1] for k in range(n)], np.int32)
    cut = np.flatnonzero(lens >= 2499)[::2]                              # an interval that starts inside the span and ends in the pad
    lo[cut], hi[cut] = lens[cut] - 3, np.minimum(lens[cut] + 6, 6000)
    assert {(int(a) % 4, int(b) % 4) for a, b in zip(lo, hi)} >= {(i, j) for i in range(4) for j in range(4)}
    assert (hi > lens).any() and (lo == hi).any()
    want = sequence.occlude_spans(seq, starts, lens, lo, hi)
    dseq, dout = engine.alloc(seq.nbytes), engine.alloc((n + 1) * _lib.WINDOW)
    try:
        dseq.upload(seq)
        dout.upload(np.full((n + 1) * _lib.WINDOW, 0x5A, np.uint8))       # a canary row behind the last window
        engine.occlude_spans_dev(dseq.ptr, starts, lens, lo, hi, dout.ptr)
        got = dout.download((n + 1, _lib.WINDOW), np.uint8)
        assert np.array_equal(got[:n], want)
        assert (got[n] == 0x5A).all()
        engine.occlude_spans_dev(dseq.ptr, starts, lens, lo, lo, dout.ptr)                  # empty intervals: the forward windows
        assert np.array_equal(dout.download((n, _lib.WINDOW), np.uint8), sequence.materialize_spans(seq, starts, lens))
        before = dout.download((n + 1, _lib.WINDOW), np.uint8)
        engine.occlude_spans_dev(dseq.ptr, starts[:0], lens[:0], lo[:0], hi[:0], dout.ptr)  # no span: nothing happens
        one = lambda **kw: engine.occlude_spans_dev(dseq.ptr, starts[:1], kw.get("lens", lens[:1]), kw.get("lo", lo[:1]),    # noqa: E731
                                                    kw.get("hi", hi[:1]), kw.get("out", dout.ptr))
        with pytest.raises(_lib.GnnError, match="aligned"):
            one(out=dout.ptr + 2)
        with pytest.raises(_lib.GnnError, match="6001"):
            one(lens=np.array([6001], np.int32))
        with pytest.raises(_lib.GnnError, match=r"\[9, 8\)"):
            one(lo=np.array([9], np.int32), hi=np.array([8], np.int32))
        with pytest.raises(_lib.GnnError, match=r"\[0, 6001\)"):
            one(lo=np.array([0], np.int32), hi=np.array([6001], np.int32))
        assert np.array_equal(dout.download((n + 1, _lib.WINDOW), np.uint8), before)        # and the refused calls wrote nothing
        # the window-level route: materialise, then classify_dev
        dsc = engine.alloc(n * 12)
        try:
            engine.occlude_spans_dev(dseq.ptr, starts, lens, lo, hi, dout.ptr)
            engine.classify_dev(dout.ptr, n, dsc.ptr)
            engine.sync()
            assert np.array_equal(dsc.download((n, 3), np.float32), engine.classify(want))
        finally:
            dsc.free()
    finally:
        dseq.free(), dout.free()


# ---- against the fp64 oracle ----------------------------------------------------------------------------------------------------
def _short_contig():
    """one 300-base contig for B = 14: 22 pairs (the last block 6 long); an N run of 14 - the block - sits at a different offset of
    the window in each pair"""
    rng = np.random.default_rng(19)
    seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), 300).astype(np.uint8)
    return seq, np.array([0, 300], np.int64)


@pytest.fixture(scope="module")
def oracle_refs(synth_weights):
    big = oracle_occlusion_1500(synth_weights)
    seq, offsets = _short_contig()
    starts, lens, _, _ = sequence.candidate_spans(offsets)
    blk_off, owner, lo, hi = sequence.occlusion_blocks(lens, 14)
    assert len(owner) == 22 and hi[-1] - lo[-1] == 6
    wins = np.concatenate([sequence.materialize_spans(seq, starts, lens), sequence.occlude_spans(seq, starts[owner], lens[owner], lo, hi)])
    sc = np.concatenate([igloo_oracle.forward(sequence_oracle.tokenize_closed_form(wins[a:a + 16]), synth_weights, np.float64, literal=False)
                         for a in range(0, len(wins), 16)])
    small = dict(seq=seq, offsets=offsets, block=14, base=sc[:1], delta=sc[:1][owner] - sc[1:], blk_offsets=blk_off)
    return big, small


@pytest.mark.parametrize("prec", ARITH)
def test_base_scores_and_deltas_match_the_fp64_oracle(engine, oracle_refs, prec, request):
    """|delta - oracle delta| <= 2e-4: two scores, each within the project's 1e-4 of the oracle, and one exact-to-half-an-ulp f32
    subtraction of numbers below 1 (6e-8) in between - nothing else."""
    need_tables(request, prec)
    for ref in oracle_refs:
        res = engine.occlude_contigs(ref["seq"], ref["offsets"], ref["block"], False, prec)
        assert np.array_equal(res.blk_offsets, ref["blk_offsets"]) and res.delta.shape == ref["delta"].shape
        e_base = float(np.abs(res.scores.astype(np.float64) - ref["base"]).max())
        e_delta = float(np.abs(res.delta.astype(np.float64) - ref["delta"]).max())
        print(f"\nocclusion {prec} B={ref['block']}: max |base - oracle| = {e_base:.3e}, max |delta - oracle delta| = {e_delta:.3e} "
              f"(largest |oracle delta| {np.abs(ref['delta']).max():.3f})")
        assert e_base <= TOL, f"{prec}: {e_base:.3e}"
        assert e_delta <= 2 * TOL, f"{prec}: {e_delta:.3e}"


# ---- bit identity ---------------------------------------------------------------------------------------------------------------
def _assert_is_the_definition(engine, res, seq, offsets, block, single_window, prec):
    """every field of an OcclusionResult against the entry points and numpy definitions it is specified by"""
    win_off, starts, lens, blk_off = engine.occlusion_plan(offsets, block, single_window)
    for k, a in (("win_offsets", win_off), ("starts", starts), ("lens", lens), ("blk_offsets", blk_off)):
        assert np.array_equal(getattr(res, k), a) and getattr(res, k).dtype == a.dtype, k
    assert res.block == block and tuple(res.asdict()) == FIELDS
    scan = engine.scan_contigs(seq, offsets, 6000, single_window, prec)
    assert np.array_equal(res.scores, scan.scores) and np.array_equal(res.kept, scan.kept) and res.kept.dtype == np.bool_
    cs, ids = engine.classify_contigs(seq, offsets, single_window, prec)
    assert np.array_equal(res.contig_scores, cs)
    abs_starts, lens2, all_ids, _ = sequence.candidate_spans(np.asarray(offsets, np.int64), single_window)
    assert np.array_equal(lens2, lens) and np.array_equal(all_ids[res.kept], ids)
    b2, owner, lo, hi = sequence.occlusion_blocks(lens, block)
    assert np.array_equal(b2, blk_off)
    occ = engine.classify(sequence.occlude_spans(seq, abs_starts[owner], lens[owner], lo, hi), prec)
    assert res.delta.dtype == np.float32 and np.array_equal(res.delta, res.scores[owner] - occ)
    return occ, owner


@pytest.mark.parametrize("single_window", [False, True])
@pytest.mark.parametrize("prec", ["f16x3tc", "bf16x3", "f16x3tk"])
def test_every_score_is_bit_identical_to_its_definition(engine, prec, single_window, request):
    need_tables(request, prec)
    seq, offsets = _contigs()
    cus = engine.device_info()["cus"]
    n_pairs = []
    for block in (6000, 2500, 1500, 97):
        res = engine.occlude_contigs(seq, offsets, block, single_window, prec)
        occ, owner = _assert_is_the_definition(engine, res, seq, offsets, block, single_window, prec)
        n_pairs.append(len(owner))
        if block == 6000:                   # one block per window, and it is the whole window: every occluded window is all N
            all_n = engine.classify(np.full((1, 6000), ord("N"), np.uint8), prec)
            assert len(occ) == len(res.scores) and (occ == all_n).all()
    assert min(n_pairs) < cus < max(n_pairs)            # calls below and above one workgroup per CU: the time split on and off
    # blocks of no ACGT byte leave the tokens alone: exactly +0.0
    res = engine.occlude_contigs(seq, offsets, 1500, single_window, prec)
    win_off, starts, lens, blk_off = engine.occlusion_plan(offsets, 1500, single_window)
    abs_starts, _, _, _ = sequence.candidate_spans(np.asarray(offsets, np.int64), single_window)
    _, owner, lo, hi = sequence.occlusion_blocks(lens, 1500)
    raw = [seq[int(abs_starts[o]) + int(a):int(abs_starts[o]) + int(b)] for o, a, b in zip(owner, lo, hi)]
    blank = np.array([not np.isin(r, np.frombuffer(b"ACGTacgt", np.uint8)).any() for r in raw])
    if not single_window:
        assert blank.sum() >= 4
    assert (res.delta[blank] == 0).all() and not np.signbit(res.delta[blank]).any()


@pytest.mark.parametrize("prec", ["f16x3tc", "bf16x3", "f16x3tk"])
def test_block_edges_at_every_offset_of_the_kernels_steps(engine, prec, request):
    """one 6000-base ACGT contig at B = 13, 14, 15 (block edges at every offset relative to the 14-mer context) and 96 (the 96-row
    steps; against the 128-row steps the edges drift by 32), and one 200-base contig at B = 1"""
    need_tables(request, prec)
    rng = np.random.default_rng(23)
    seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), 6000).astype(np.uint8)
    offsets = np.array([0, 6000], np.int64)
    for block in (13, 14, 15, 96):
        res = engine.occlude_contigs(seq, offsets, block, False, prec)
        _, owner = _assert_is_the_definition(engine, res, seq, offsets, block, False, prec)
        assert len(owner) == -(-6000 // block)
    res = engine.occlude_contigs(seq[:200], np.array([0, 200], np.int64), 1, False, prec)
    _, owner = _assert_is_the_definition(engine, res, seq[:200], np.array([0, 200], np.int64), 1, False, prec)
    assert len(owner) == 200


# ---- invariance -----------------------------------------------------------------------------------------------------------------
def _assert_same(a, b):
    for k in FIELDS:
        x, y = getattr(a, k), getattr(b, k)
        assert np.array_equal(x, y) and np.asarray(x).dtype == np.asarray(y).dtype, k


def test_results_do_not_depend_on_the_launch_size_or_where_the_sequence_lives(synth_weights, engine):
    """a slab is 4 launches: at 4 windows per launch the pairs of B = 700 go in slabs of 16, at 1 per launch in slabs of 4, and
    windows' blocks straddle them"""
    from genomad_amd.engine import NNEngine
    seq, offsets = _contigs()
    want = {b: engine.occlude_contigs(seq, offsets, b) for b in (700, 2500)}
    assert len(want[700].delta) > 64
    with NNEngine(0, synth_weights, chunk=4) as e2:
        _assert_same(e2.occlude_contigs(seq, offsets, 700), want[700])
        e2.lib.gnn_set_chunk(e2.ctx, 13)
        _assert_same(e2.occlude_contigs(seq, offsets, 2500), want[2500])
        e2.lib.gnn_set_chunk(e2.ctx, 1)
        _assert_same(e2.occlude_contigs(seq, offsets, 700), want[700])
    dev = engine.alloc(seq.nbytes)
    try:
        dev.upload(seq)
        _assert_same(engine.occlude_contigs_dev(dev.ptr, offsets, 700), want[700])
        cls = engine.classify_contigs(seq, offsets)
        _assert_same(engine.occlude_contigs_dev(dev.ptr, offsets, 2500), want[2500])
        scan = engine.scan_contigs(seq, offsets, 2000)
        _assert_same(engine.occlude_contigs(seq, offsets, 700), want[700])
        assert np.array_equal(engine.classify_contigs_dev(dev.ptr, offsets)[0], cls[0])
        assert np.array_equal(engine.scan_contigs(seq, offsets, 2000).scores, scan.scores)
    finally:
        dev.free()
    assert np.array_equal(cls[0], want[700].contig_scores)


def test_occlusion_errors_leave_the_ctx_usable(engine):
    seq, offsets = _contigs()
    for bad in (0, -1, 6001):
        with pytest.raises(_lib.GnnError, match=r"\[1, 6000\]"):
            engine.occlude_contigs(seq, offsets, bad)
    off = np.ascontiguousarray(offsets, np.int64)
    n_contigs = len(off) - 1
    _, starts, _, blk_off = engine.occlusion_plan(off, 1500)
    nw, npairs = len(starts), int(blk_off[-1])
    scores, delta = np.zeros((nw, 3), np.float32), np.zeros((npairs, 3), np.float32)
    call = lambda wcap, pcap: engine.lib.gnn_occlude_contigs(                                  # noqa: E731
        engine.ctx, seq.ctypes.data, 1, seq.nbytes, off.ctypes.data, n_contigs, 1500, 0, _lib.PRECISIONS["f16x3tc"], scores.ctypes.data,
        None, wcap, delta.ctypes.data, pcap, None)
    assert call(nw - 1, npairs) == _lib.ERR_ARG and str(nw).encode() in engine.lib.gnn_last_error()
    assert call(nw, npairs - 1) == _lib.ERR_ARG and str(npairs).encode() in engine.lib.gnn_last_error()
    assert not scores.any() and not delta.any()
    empty = engine.occlude_contigs(np.zeros(0, np.uint8), np.array([0, 0, 0]), 100)
    assert empty.scores.shape == (0, 3) and empty.delta.shape == (0, 3) and not empty.contig_scores.any() and len(empty.win_offsets) == 3
    none = engine.occlude_contigs(np.zeros(0, np.uint8), np.array([0]), 100)
    assert none.contig_scores.shape == (0, 3) and list(none.blk_offsets) == [0]
    assert call(nw, npairs) == 0                                        # the optional outputs may be NULL
    want = engine.occlude_contigs(seq, offsets, 1500)
    assert np.array_equal(scores, want.scores) and np.array_equal(delta, want.delta)


# ---- main() -------------------------------------------------------------------------------------------------------------------
def test_main_writes_the_occlusion_map_only_when_asked(engine, synth_weights, tmp_path, monkeypatch):
    nnc = _setup_main(tmp_path, monkeypatch, engine, synth_weights)
    fa = tmp_path / "m.fna"
    _fasta(fa)
    for k in ("GENOMAD_AMD_STRAND", "GENOMAD_AMD_SCAN_STRIDE", "GENOMAD_AMD_EMBEDDINGS", "GENOMAD_AMD_OCCLUSION_BLOCK"):
        monkeypatch.delenv(k, raising=False)
    nnc.main(fa, tmp_path / "off", False, 128, False, 1, False, False)
    monkeypatch.setenv("GENOMAD_AMD_OCCLUSION_BLOCK", "1200")
    nnc.main(fa, tmp_path / "on", False, 128, False, 1, False, False)
    d_off, d_on = tmp_path / "off" / "m_nn_classification", tmp_path / "on" / "m_nn_classification"
    files = lambda d: sorted(str(p.relative_to(d)) for p in d.rglob("*"))      # noqa: E731
    assert files(d_on) == sorted(files(d_off) + ["m_nn_occlusion.npz"])
    for rel in ("m_nn_classification.npz", "m_encoded_sequences/m_seq_window_id.npz"):
        a, b = np.load(d_off / rel), np.load(d_on / rel)
        assert sorted(a.files) == sorted(b.files) and all(a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]) for k in a.files)
    assert (d_off / "m_nn_classification.tsv").read_bytes() == (d_on / "m_nn_classification.tsv").read_bytes()
    names, seq, off = sequence.read_fasta_packed(fa)
    want = engine.occlude_contigs(seq, off, 1200, False, "f16x3tc").asdict()
    z = np.load(d_on / "m_nn_occlusion.npz")
    assert sorted(z.files) == sorted(("contig_names",) + FIELDS) and list(z["contig_names"]) == list(names) and int(z["block"]) == 1200
    for k in FIELDS[1:]:
        assert z[k].dtype == want[k].dtype and np.array_equal(z[k], want[k]), k
    assert np.array_equal(z["contig_scores"], np.load(d_on / "m_nn_classification.npz")["predictions"])
    # resume: the same request runs nothing; without the switch the stage runs again and the file goes
    calls = []
    real = type(engine).occlude_contigs
    monkeypatch.setattr(type(engine), "occlude_contigs", lambda self, *a, **k: calls.append(a[2]) or real(self, *a, **k))
    nnc.main(fa, tmp_path / "on", False, 128, False, 1, False, False)
    assert calls == []
    monkeypatch.setenv("GENOMAD_AMD_OCCLUSION_BLOCK", "3000")
    nnc.main(fa, tmp_path / "on", False, 128, False, 1, False, False)
    assert calls == [3000] and int(np.load(d_on / "m_nn_occlusion.npz")["block"]) == 3000
    monkeypatch.delenv("GENOMAD_AMD_OCCLUSION_BLOCK")
    nnc.main(fa, tmp_path / "on", False, 128, False, 1, False, False)
    assert calls == [3000] and files(d_on) == files(d_off)
    assert (d_off / "m_nn_classification.tsv").read_bytes() == (d_on / "m_nn_classification.tsv").read_bytes()
