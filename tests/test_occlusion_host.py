"""CPU checks of the occlusion feature (per-block score change along contigs): the numpy definitions (sequence.occlude_spans,
occlusion_blocks) against an independent bytes implementation, gnn_occlusion_plan against a Python mirror, the fp64 oracle's deltas on
the contigs the GPU tests use (non-vacuity), the ABI, and main()'s GENOMAD_AMD_OCCLUSION_BLOCK switch over a fake engine (validation,
byte-identical outputs without it, the npz, the resume rule, the two refusals, several ranks)."""
import ctypes as C
import os
import socket

import numpy as np
import pytest

from genomad_amd import _lib, sequence, sharding
from genomad_amd import nn_classification as nnc
from oracle import igloo_oracle, sequence_oracle
from tests.test_strand_host import FakeStrandEngine, _mixed_buffer, _npz, _same_npz, _tree, _window_scores, _write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 6000
LENGTHS = [0, 1, 2, 3, 2499, 5999, 6000]
FIELDS = ("block", "win_offsets", "starts", "lens", "kept", "scores", "blk_offsets", "delta", "contig_scores")


def _occlude_bytes(raw: bytes, lo: int, hi: int) -> bytes:
    """independent of numpy: str.upper, slice assignment on a bytearray, ljust"""
    b = bytearray(raw.upper())
    lo, hi = min(lo, len(b)), min(hi, len(b))
    b[lo:hi] = b"N" * (hi - lo)
    return bytes(b).ljust(W, b"N")


def test_occlude_spans_equals_the_bytes_definition():
    seq = _mixed_buffer()
    starts, lens, lo, hi = [], [], [], []
    for length in LENGTHS:
        for start in (0, 1, 2, 3, 8999, 9001, 17777, len(seq) - length):
            for a, b in ((0, 0), (7, 7), (0, length), (0, W), (max(length - 1, 0), length), (max(length - 5, 0), min(length + 9, W)),
                         (length // 3, length // 2)):
                starts.append(start), lens.append(length), lo.append(a), hi.append(b)
    starts, lens = np.array(starts, np.int64), np.array(lens, np.int32)
    assert {int(a) % 4 for a in starts} == {0, 1, 2, 3}
    got = sequence.occlude_spans(seq, starts, lens, lo, hi)
    assert got.dtype == np.uint8 and got.shape == (len(starts), W)
    raw = seq.tobytes()
    for i, (a, l) in enumerate(zip(starts, lens)):
        assert got[i].tobytes() == _occlude_bytes(raw[a:a + l], lo[i], hi[i]), (a, l, lo[i], hi[i])
    empty = np.array(lo) == np.array(hi)
    assert np.array_equal(got[empty], sequence.materialize_spans(seq, starts[empty], lens[empty]))
    whole = (np.array(lo) == 0) & (np.array(hi) >= lens)
    assert (got[whole] == ord("N")).all()
    for a, b in ((-1, 5), (9, 8), (0, W + 1)):
        with pytest.raises(ValueError, match="lo <= hi"):
            sequence.occlude_spans(seq, [0], [100], [a], [b])


def _plan(offsets, block, single_window):
    lib = _lib.load()
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n = len(offsets) - 1
    nw, npairs = C.c_int64(-1), C.c_int64(-1)
    head = (offsets.ctypes.data, n, block, int(single_window), C.byref(nw), C.byref(npairs))
    _lib.check(lib.gnn_occlusion_plan(*head, None, None, None, None))
    wo, bo = np.full(n + 1, -1, np.int64), np.full(nw.value + 1, -1, np.int64)
    st, ln = np.full(nw.value, -1, np.int64), np.full(nw.value, -1, np.int32)
    _lib.check(lib.gnn_occlusion_plan(*head, wo.ctypes.data, st.ctypes.data, ln.ctypes.data, bo.ctypes.data))
    return nw.value, npairs.value, wo, st, ln, bo


@pytest.mark.parametrize("single_window", [False, True])
@pytest.mark.parametrize("block", [1, 7, 2500, 5999, 6000])
def test_plan_equals_the_python_mirror(block, single_window):
    lengths = [0, 1, 2499, 2500, 5999, 6000, 6001, 8499, 8500, 12000]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    starts, lens, ids, window_n = sequence.candidate_spans(offsets, single_window)
    blk_off, owner, lo, hi = sequence.occlusion_blocks(lens, block)
    nw, npairs, wo, st, ln, bo = _plan(offsets, block, single_window)
    assert nw == len(starts) and npairs == int(blk_off[-1]) == len(owner)
    assert np.array_equal(wo, np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=len(lengths)))]))
    assert np.array_equal(st, window_n.astype(np.int64) * W) and np.array_equal(ln, lens) and np.array_equal(bo, blk_off)
    assert blk_off.dtype == np.int64 and owner.dtype == np.int64 and lo.dtype == np.int32 and hi.dtype == np.int32
    # the blocks, literally: ceil(len / B) per window, [jB, min((j + 1)B, len)), the pad never a block
    want = [(i, j * block, min((j + 1) * block, int(l))) for i, l in enumerate(lens) for j in range(-(-int(l) // block))]
    assert [(int(o), int(a), int(b)) for o, a, b in zip(owner, lo, hi)] == want
    assert (hi > lo).all() and (hi <= lens[owner]).all()
    if block == W:
        assert np.array_equal(np.diff(blk_off), np.ones(len(lens), np.int64))       # exactly one block per window
    # the engine's wrapper returns the same tables
    from genomad_amd.engine import NNEngine
    eng = NNEngine.__new__(NNEngine)
    eng.lib = _lib.load()
    for a, b in zip(eng.occlusion_plan(offsets, block, single_window), (wo, st, ln, bo)):
        assert np.array_equal(a, b) and a.dtype == b.dtype
    eng.ctx = None


def test_plan_refuses_bad_arguments():
    lib = _lib.load()
    off = np.array([0, 7000, 9000], np.int64)
    nw, npairs = C.c_int64(), C.c_int64()
    for block in (0, -1, 6001):
        assert lib.gnn_occlusion_plan(off.ctypes.data, 2, block, 0, C.byref(nw), C.byref(npairs), None, None, None, None) == _lib.ERR_ARG
        assert b"[1, 6000]" in lib.gnn_last_error()
        with pytest.raises(ValueError, match="6000"):
            sequence.occlusion_blocks([100], block)
    bad = np.array([0, 7000, 6999], np.int64)
    assert lib.gnn_occlusion_plan(bad.ctypes.data, 2, 100, 0, C.byref(nw), C.byref(npairs), None, None, None, None) == _lib.ERR_ARG
    assert b"non-decreasing" in lib.gnn_last_error()
    assert lib.gnn_occlusion_plan(off.ctypes.data, 2, 1000, 0, C.byref(nw), C.byref(npairs), None, None, None, None) == 0
    assert (nw.value, npairs.value) == (1 + 1, 6 + 2)
    # a bad block is refused by gnn_occlude_contigs before the ctx is looked at: no GPU needed
    rc = lib.gnn_occlude_contigs(None, None, 1, 0, off.ctypes.data, 0, 6001, 0, 6, None, None, 0, None, 0, None)
    assert rc == _lib.ERR_ARG and b"[1, 6000]" in lib.gnn_last_error() and b"6001" in lib.gnn_last_error()


def oracle_occlusion_1500(weights):
    """The first three records of the GPU tests' contigs (10 windows) at B = 1500 (36 pairs): tables, numpy windows, and the fp64
    oracle's base scores, occluded scores and deltas.  About 10 s of oracle time; the GPU tests share it through a fixture."""
    from tests.test_embeddings_gpu import _contigs
    seq, offsets = _contigs()
    offsets = offsets[:4]
    seq = seq[:offsets[-1]]
    starts, lens, ids, window_n = sequence.candidate_spans(offsets)
    blk_off, owner, lo, hi = sequence.occlusion_blocks(lens, 1500)
    wins = sequence.materialize_spans(seq, starts, lens)
    occ_wins = sequence.occlude_spans(seq, starts[owner], lens[owner], lo, hi)
    score = lambda w: np.concatenate([igloo_oracle.forward(sequence_oracle.tokenize_closed_form(w[a:a + 16]), weights, np.float64,   # noqa: E731
                                                           literal=False) for a in range(0, len(w), 16)])
    base, occ = score(wins), score(occ_wins)
    nn = np.array([np.count_nonzero(seq[a:a + l] == ord("N")) for a, l in zip(starts, lens)])
    return dict(seq=seq, offsets=offsets, block=1500, starts=starts, lens=lens, ids=ids, kept=(window_n == 0) | (nn <= sequence.MAX_N),
                blk_offsets=blk_off, owner=owner, lo=lo, hi=hi, wins=wins, occ_wins=occ_wins, base=base, occ=occ,
                delta=base[owner] - occ)


def test_the_oracles_deltas_are_not_vacuous(synth_weights):
    """keeps the GPU parity test from being vacuous: were the deltas all tiny, a device that ignored the block would pass it.
    Measured: 30 of the 36 blocks move some class by more than 1e-2, at most 0.95."""
    ref = oracle_occlusion_1500(synth_weights)
    assert len(ref["starts"]) == 10 and len(ref["owner"]) == 36
    d = np.abs(ref["delta"]).max(axis=1)
    print(f"\noracle |delta| on 36 blocks of 1500: max {d.max():.3f}, {(d > 1e-2).sum()} above 1e-2")
    assert (d > 1e-2).sum() >= 24
    a, b = int(ref["blk_offsets"][8]), int(ref["blk_offsets"][9])
    assert (ref["wins"][8] == ord("N")).all() and b - a == 4 and list(ref["owner"][a:b]) == [8] * 4    # window 8: all N, four blocks
    assert (ref["delta"][a:b] == 0).all()
    assert not ref["kept"][8] and ref["kept"].sum() == 9


def test_abi_declares_the_occlusion_entry_points():
    text = open(os.path.join(ROOT, "include", "genomad_nn.h")).read()
    lib = _lib.load()
    for name in ("gnn_occlusion_plan", "gnn_occlude_spans_dev", "gnn_occlude_contigs"):
        assert f"int {name}(" in text and name in _lib.SIGNATURES and hasattr(lib, name)
    from genomad_amd.engine import NNEngine, OcclusionResult, ScanResult
    for m in ("occlusion_plan", "occlude_spans_dev", "occlude_contigs", "occlude_contigs_dev"):
        assert hasattr(NNEngine, m)
    assert OcclusionResult.FIELDS == FIELDS
    assert ScanResult.FIELDS == ("stride", "win_offsets", "starts", "lens", "kept", "scores", "bin_offsets", "track", "cover",
                                 "contig_scores")


# ---- main() over a fake engine ---------------------------------------------------------------------------------------------------
class FakeOcclusionEngine(FakeStrandEngine):
    """FakeStrandEngine plus occlude_contigs, computed in numpy from the definitions of sequence.py"""
    calls = []

    def occlude_contigs(self, seq, offsets, block, single_window=False, precision=None):
        from genomad_amd.engine import OcclusionResult
        type(self).calls.append(("occlude", int(block)))
        offsets = np.asarray(offsets, np.int64)
        n, ids, kept, f, _ = self._run(seq, offsets, single_window)
        starts, lens, _, window_n = sequence.candidate_spans(offsets, single_window)
        blk_off, owner, lo, hi = sequence.occlusion_blocks(lens, block)
        occ = _window_scores(sequence.occlude_spans(seq, starts[owner], lens[owner], lo, hi))
        win_off = np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=n))]).astype(np.int64)
        return OcclusionResult(block=int(block), win_offsets=win_off, starts=window_n.astype(np.int64) * W, lens=lens, kept=kept,
                               scores=f, blk_offsets=blk_off, delta=f[owner] - occ, contig_scores=self._mean(n, ids, kept, f))


@pytest.fixture
def fake_main(monkeypatch):
    monkeypatch.setattr(nnc, "_engine", lambda: FakeOcclusionEngine())
    for k in ("GENOMAD_AMD_FRONT_END", "GENOMAD_AMD_STRAND", "GENOMAD_AMD_EMBEDDINGS", "GENOMAD_AMD_SCAN_STRIDE", "GENOMAD_AMD_PRECISION",
              "GENOMAD_AMD_OCCLUSION_BLOCK"):
        monkeypatch.delenv(k, raising=False)
    del FakeOcclusionEngine.calls[:]
    return lambda fa, out, **kw: nnc.main(fa, out, False, 128, False, 1, False, False, **kw)


def test_occlusion_switch_values(monkeypatch):
    monkeypatch.delenv("GENOMAD_AMD_OCCLUSION_BLOCK", raising=False)
    assert nnc.occlusion_block_requested() is None
    for v, want in (("", None), (" 1 ", 1), ("1500", 1500), ("6000", 6000)):
        monkeypatch.setenv("GENOMAD_AMD_OCCLUSION_BLOCK", v)
        assert nnc.occlusion_block_requested() == want
    for v in ("0", "-5", "6001", "1.5", "block", "1e3"):
        monkeypatch.setenv("GENOMAD_AMD_OCCLUSION_BLOCK", v)
        with pytest.raises(ValueError, match=r"GENOMAD_AMD_OCCLUSION_BLOCK.*\[1, 6000\]"):
            nnc.occlusion_block_requested()


def test_main_refuses_a_bad_value_the_other_strands_and_the_host_front_end(tmp_path, monkeypatch, fake_main, capsys):
    from tests.test_scan_host import _MustNotRun
    fa = tmp_path / "s.fna"
    _write_fasta(fa, n=3)
    for v in ("6001", "many"):
        monkeypatch.setenv("GENOMAD_AMD_OCCLUSION_BLOCK", v)
        with pytest.raises(ValueError, match="GENOMAD_AMD_OCCLUSION_BLOCK"):
            fake_main(fa, tmp_path / "bad")
        assert not (tmp_path / "bad").exists()                  # before anything is written
    monkeypatch.setenv("GENOMAD_AMD_OCCLUSION_BLOCK", "500")
    for env, kw, msg in (({"GENOMAD_AMD_FRONT_END": "host"}, {}, "GENOMAD_AMD_OCCLUSION_BLOCK needs the device front end"),
                         ({}, {"_backend": _MustNotRun()}, "GENOMAD_AMD_OCCLUSION_BLOCK needs the device front end"),
                         ({"GENOMAD_AMD_STRAND": "both"}, {}, "GENOMAD_AMD_OCCLUSION_BLOCK is forward-strand only"),
                         ({"GENOMAD_AMD_STRAND": "reverse"}, {}, "GENOMAD_AMD_OCCLUSION_BLOCK is forward-strand only")):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with pytest.raises(SystemExit) as exc:
            fake_main(fa, tmp_path / "refused", **kw)
        assert exc.value.code == 1
        err = capsys.readouterr().err
        assert msg in err and len(err.strip().splitlines()) == 1
        assert not list((tmp_path / "refused").rglob("*.npz")) and not list((tmp_path / "refused").rglob("*.tsv"))
        for k in env:
            monkeypatch.delenv(k)
    assert FakeOcclusionEngine.calls == []
    monkeypatch.setenv("GENOMAD_AMD_STRAND", "forward")         # forward, spelled out, is no other strand
    fake_main(fa, tmp_path / "fwd")
    assert (tmp_path / "fwd" / "s_nn_classification" / "s_nn_occlusion.npz").exists()


def test_main_writes_the_map_and_changes_nothing_else(tmp_path, monkeypatch, fake_main):
    fa = tmp_path / "m.fna"
    _write_fasta(fa)
    fake_main(fa, tmp_path / "unset")
    assert FakeOcclusionEngine.calls == ["plain"]
    monkeypatch.setenv("GENOMAD_AMD_OCCLUSION_BLOCK", "700")
    fake_main(fa, tmp_path / "on")
    assert FakeOcclusionEngine.calls == ["plain", "plain", ("occlude", 700)]     # the classification goes the way it always went
    d0, d1 = tmp_path / "unset" / "m_nn_classification", tmp_path / "on" / "m_nn_classification"
    assert _tree(d1) == sorted(_tree(d0) + ["m_nn_occlusion.npz"])
    assert (d0 / "m_nn_classification.tsv").read_bytes() == (d1 / "m_nn_classification.tsv").read_bytes()
    for rel in ("m_nn_classification.npz", "m_encoded_sequences/m_seq_window_id.npz"):
        assert _same_npz(d0 / rel, d1 / rel)
    names, seq, off = sequence.read_fasta_packed(fa)
    want = FakeOcclusionEngine().occlude_contigs(seq, off, 700).asdict()
    z = _npz(d1 / "m_nn_occlusion.npz")
    assert sorted(z) == sorted(("contig_names",) + FIELDS)
    assert list(z["contig_names"]) == list(names) and int(z["block"]) == 700 and z["block"].dtype == np.int64
    dtypes = {"win_offsets": np.int64, "starts": np.int64, "lens": np.int32, "kept": np.bool_, "scores": np.float32,
              "blk_offsets": np.int64, "delta": np.float32, "contig_scores": np.float32}
    for k, dt in dtypes.items():
        assert z[k].dtype == dt and np.array_equal(z[k], want[k]), k
    assert np.array_equal(z["contig_scores"], _npz(d0 / "m_nn_classification.npz")["predictions"])
    assert z["delta"].shape == (int(z["blk_offsets"][-1]), 3) and np.abs(z["delta"]).max() > 0.05
    assert not z["kept"].all()                                   # the nrun record: the mask travels


def test_main_resume_follows_the_block(tmp_path, monkeypatch, fake_main):
    fa = tmp_path / "r.fna"
    _write_fasta(fa, seed=4, n=6)
    out = tmp_path / "out"
    d = out / "r_nn_classification"
    monkeypatch.setenv("GENOMAD_AMD_OCCLUSION_BLOCK", "1000")
    fake_main(fa, out)
    first = _npz(d / "r_nn_occlusion.npz")
    fake_main(fa, out)
    assert FakeOcclusionEngine.calls == ["plain", ("occlude", 1000)]           # same request, everything there: nothing runs
    monkeypatch.setenv("GENOMAD_AMD_OCCLUSION_BLOCK", "250")
    fake_main(fa, out)                                                         # another block: recomputed
    assert FakeOcclusionEngine.calls[2:] == ["plain", ("occlude", 250)] and int(_npz(d / "r_nn_occlusion.npz")["block"]) == 250
    assert len(_npz(d / "r_nn_occlusion.npz")["delta"]) > len(first["delta"])
    fake_main(fa, out)
    assert len(FakeOcclusionEngine.calls) == 4
    monkeypatch.delenv("GENOMAD_AMD_OCCLUSION_BLOCK")
    fake_main(fa, out)                                                         # no request: the file goes
    assert FakeOcclusionEngine.calls[4:] == ["plain"] and not (d / "r_nn_occlusion.npz").exists()
    fake_main(fa, out)
    assert len(FakeOcclusionEngine.calls) == 5
    monkeypatch.setenv("GENOMAD_AMD_OCCLUSION_BLOCK", "1000")
    fake_main(fa, out)                                                         # scores on disk, no map: the stage runs again
    assert FakeOcclusionEngine.calls[5:] == ["plain", ("occlude", 1000)] and _same_npz(d / "r_nn_occlusion.npz", d / "r_nn_occlusion.npz")
    z = _npz(d / "r_nn_occlusion.npz")
    assert all(np.array_equal(z[k], first[k]) for k in first)


# ---- several ranks ----------------------------------------------------------------------------------------------------------------
def _gloo_occlusion_main_worker(rank, world, port, fasta, out_dir, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), GENOMAD_AMD_OCCLUSION_BLOCK="900")
    for k in ("GENOMAD_AMD_FRONT_END", "GENOMAD_AMD_EMBEDDINGS", "GENOMAD_AMD_SCAN_STRIDE", "GENOMAD_AMD_STRAND"):
        os.environ.pop(k, None)
    from tests.gloo_comm import GlooComm
    nnc._engine = lambda: FakeOcclusionEngine()
    comm = GlooComm(rank, world, port)
    code = 0
    try:
        nnc.main(fasta, out_dir, False, 128, False, 1, False, False, _comm=comm)
    except SystemExit as e:
        code = e.code
    q.put((rank, code))
    comm.close()


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_give_the_files_of_one_process(tmp_path, monkeypatch, fake_main, world):
    mp = pytest.importorskip("torch.multiprocessing")
    fa = tmp_path / "g.fna"
    _write_fasta(fa, seed=9, n=23)
    monkeypatch.setenv("GENOMAD_AMD_OCCLUSION_BLOCK", "900")
    fake_main(fa, tmp_path / "one")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    out = tmp_path / f"ranks{world}"
    procs = [ctx.Process(target=_gloo_occlusion_main_worker, args=(r, world, port, str(fa), str(out), q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=180)
        assert p.exitcode == 0
    assert got == [(r, 0) for r in range(world)]
    d1, dn = tmp_path / "one" / "g_nn_classification", out / "g_nn_classification"
    assert _tree(d1) == _tree(dn)
    assert (d1 / "g_nn_classification.tsv").read_bytes() == (dn / "g_nn_classification.tsv").read_bytes()
    for rel in ("g_nn_classification.npz", "g_nn_occlusion.npz", "g_encoded_sequences/g_seq_window_id.npz"):
        assert _same_npz(d1 / rel, dn / rel), rel


def test_occlusion_gather_one_process_out_of_order_and_empty():
    rng = np.random.default_rng(8)
    seq = rng.choice(np.frombuffer(b"ACGTN", np.uint8), 60000)
    offsets = np.array([0, 100, 20000, 20000, 47000, 60000], np.int64)
    eng = FakeOcclusionEngine()
    piece = lambda a, b: eng.occlude_contigs(seq[offsets[a]:offsets[b]], offsets[a:b + 1] - offsets[a], 1100)      # noqa: E731
    whole = piece(0, 5).asdict()
    got = sharding.gather_contig_occlusions(None, [(7, piece(3, 5)), (0, piece(0, 2)), (3, piece(2, 3).asdict())])
    assert sorted(got) == sorted(FIELDS[1:])
    for k in got:
        assert got[k].dtype == whole[k].dtype and np.array_equal(got[k], whole[k]), k
    empty = sharding.gather_contig_occlusions(None, [])
    assert list(empty["win_offsets"]) == [0] and list(empty["blk_offsets"]) == [0] and empty["delta"].shape == (0, 3)
    assert empty["kept"].dtype == np.bool_ and empty["lens"].dtype == np.int32
    with pytest.raises(ValueError, match="duplicate"):
        sharding.gather_contig_occlusions(None, [(1, piece(0, 1)), (1, piece(1, 2))])
