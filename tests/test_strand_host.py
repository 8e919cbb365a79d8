"""CPU checks of the strand feature (reverse-complement windows): the numpy definitions (sequence.revcomp_spans, strand_mean) against an
independent bytes implementation, the oracle's strand asymmetry on the contigs the GPU tests use, main()'s GENOMAD_AMD_STRAND switch
over a fake engine (validation, byte-identical forward outputs, the resume rule, the host-front-end error) and the rank-0 gather."""
import json
import os
import socket
import zlib

import numpy as np
import pytest

from genomad_amd import _lib, sequence, sharding
from genomad_amd import nn_classification as nnc
from oracle import igloo_oracle, sequence_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 6000
LENGTHS = [0, 1, 2, 3, 2499, 5999, 6000]
TOL = 1e-4                                  # the project's tolerance on class scores


def _revcomp_bytes(raw: bytes) -> bytes:
    """independent of numpy: str.upper, bytes.translate, a reversed slice, ljust"""
    return raw.upper().translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1].ljust(W, b"N")


def _mixed_buffer():
    rng = np.random.default_rng(77)
    alphabet = np.frombuffer(b"ACGTacgtNnRYKMSWBDHVrykmswbdhv-*", np.uint8)
    p = np.array([.11] * 8 + [.005] * 24)
    seq = rng.choice(alphabet, 40000, p=p / p.sum()).astype(np.uint8)
    seq[9000:13500] = ord("N")               # an N run longer than the rule's 4000
    seq[20000:20300] = ord("n")
    return seq


def test_revcomp_spans_equals_the_bytes_definition():
    seq = _mixed_buffer()
    starts, lens = [], []
    for length in LENGTHS:
        for start in (0, 1, 2, 3, 8999, 9001, 17777, len(seq) - length):
            starts.append(start), lens.append(length)
    starts, lens = np.array(starts, np.int64), np.array(lens, np.int32)
    got = sequence.revcomp_spans(seq, starts, lens)
    assert got.dtype == np.uint8 and got.shape == (len(starts), W)
    raw = seq.tobytes()
    for i, (a, l) in enumerate(zip(starts, lens)):
        assert got[i].tobytes() == _revcomp_bytes(raw[a:a + l]), (a, l)
    assert (got[lens == 0] == ord("N")).all()
    # IUPAC codes and every other byte pass through unchanged (upper-cased): only A, C, G, T are swapped
    one = sequence.revcomp_spans(np.frombuffer(b"aRyKn-Tg", np.uint8), [0], [8])[0, :8].tobytes()
    assert one == b"CA-NKYRT"


def test_revcomp_is_an_involution_on_the_unpadded_part_and_keeps_the_n_count():
    seq = _mixed_buffer()
    starts = np.array([0, 5, 8000, 9000, 19000, 33990], np.int64)
    lens = np.array([6000, 2499, 6000, 4500, 3000, 6000], np.int32)
    fwd, rev = sequence.materialize_spans(seq, starts, lens), sequence.revcomp_spans(seq, starts, lens)
    for i, l in enumerate(lens):
        back = sequence.revcomp_spans(rev[i, :l], [0], [l])[0]
        assert np.array_equal(back[:l], fwd[i, :l]) and (back[l:] == ord("N")).all()
        raw = seq[starts[i]:starts[i] + l]
        # the N rule counts literal 'N' on the raw span, case untouched: the complement maps N to N, so the reversed raw span
        # holds as many - and so do the two materialised windows, where n has become N on both
        comp_raw = raw.tobytes().translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))[::-1]
        assert comp_raw.count(b"N") == raw.tobytes().count(b"N")
        assert int(np.count_nonzero(rev[i] == ord("N"))) == int(np.count_nonzero(fwd[i] == ord("N")))
    assert (np.array([np.count_nonzero(seq[a:a + l] == ord("N")) for a, l in zip(starts, lens)]) > sequence.MAX_N).any()


def test_strand_mean_is_f32_with_one_rounding():
    rng = np.random.default_rng(3)
    f, r = rng.random((5000, 3), dtype=np.float32), rng.random((5000, 3), dtype=np.float32)
    got = sequence.strand_mean(f, r)
    assert got.dtype == np.float32 and got.shape == f.shape
    exact = (f.astype(np.float64) + r.astype(np.float64)) / 2           # exact in f64 (25 significant bits at most)
    assert np.array_equal(got, exact.astype(np.float32))                 # = the exact mean rounded once
    assert np.array_equal(sequence.strand_mean(f, f), f)
    assert sequence.strand_mean([[0.25, 0.5, 0.25]], [[0.75, 0.0, 0.25]]).tolist() == [[0.5, 0.25, 0.25]]


def test_the_oracle_is_strand_asymmetric_on_the_gpu_tests_contigs(synth_weights):
    """keeps the GPU parity test from being vacuous: were forward and reverse scores alike, a device that ignored the strand would
    pass it.  Measured: 12 of the first 16 windows differ by more than 1e-2, at most 0.61."""
    from tests.test_embeddings_gpu import _contigs
    seq, offsets = _contigs()
    starts, lens, _, _ = sequence.candidate_spans(offsets)
    starts, lens = starts[:16], lens[:16]
    fwd, rev = sequence.materialize_spans(seq, starts, lens), sequence.revcomp_spans(seq, starts, lens)
    score = lambda wins: igloo_oracle.forward(sequence_oracle.tokenize_closed_form(wins), synth_weights, np.float64, literal=False)  # noqa: E731
    d = np.abs(score(fwd) - score(rev)).max(axis=1)
    print(f"\noracle |forward - reverse| on 16 windows: max {d.max():.3f}, {(d > 100 * TOL).sum()} above {100 * TOL:g}")
    assert (d > 100 * TOL).sum() >= 8


def test_abi_declares_the_strand_entry_points():
    text = open(os.path.join(ROOT, "include", "genomad_nn.h")).read()
    lib = _lib.load()
    for name in ("gnn_revcomp_spans_dev", "gnn_classify_contigs_strand", "gnn_scan_contigs_strand"):
        assert f"int {name}(" in text and name in _lib.SIGNATURES and hasattr(lib, name)
    assert "GNN_STRAND_FORWARD = 0, GNN_STRAND_REVERSE = 1, GNN_STRAND_BOTH = 2" in text
    assert _lib.STRANDS == {"forward": 0, "reverse": 1, "both": 2} and tuple(_lib.STRANDS) == sequence.STRANDS
    from genomad_amd.engine import NNEngine, ScanResult, StrandScanResult
    for m in ("revcomp_spans_dev", "classify_contigs_strand", "classify_contigs_strand_dev", "scan_contigs_strand",
              "scan_contigs_strand_dev"):
        assert hasattr(NNEngine, m)
    assert ScanResult.FIELDS == ("stride", "win_offsets", "starts", "lens", "kept", "scores", "bin_offsets", "track", "cover",
                                 "contig_scores")
    assert StrandScanResult.FIELDS == ScanResult.FIELDS + ("strand", "scores_fwd", "scores_rev")
    # a strand outside the enum is refused before the ctx is looked at: no GPU needed
    n = np.zeros(1, np.int64)
    off = np.zeros(1, np.int64)
    rc = lib.gnn_classify_contigs_strand(None, None, 1, 0, off.ctypes.data, 0, 0, 6, None, None, 0,
                                         n.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int64)), None, 7, None, None)
    assert rc == _lib.ERR_ARG and b"strand 7" in lib.gnn_last_error()
    rc = lib.gnn_scan_contigs_strand(None, None, 1, 0, off.ctypes.data, 0, 2000, 0, 6, None, None, 0, None, None, 0, None, -1, None, None)
    assert rc == _lib.ERR_ARG and b"strand -1" in lib.gnn_last_error()


# ---- main() over a fake engine ---------------------------------------------------------------------------------------------------
def _window_scores(wins):
    """a fixed function of each window's 6000 bytes in place of the network (three f32 that sum to about 1)"""
    out = np.zeros((len(wins), 3), np.float32)
    for i, w in enumerate(wins):
        v = np.random.default_rng(zlib.crc32(w.tobytes())).random(3, dtype=np.float32)
        out[i] = v / v.sum()
    return out


class FakeStrandEngine:
    """the contig entry points of NNEngine that main() calls, computed in numpy from the definitions of sequence.py"""
    calls = []

    def classify(self, windows, precision=None):
        return _window_scores(windows)

    def _run(self, seq, offsets, single_window):
        offsets = np.asarray(offsets, np.int64)
        starts, lens, ids, window_n = sequence.candidate_spans(offsets, single_window)
        nn = np.array([np.count_nonzero(seq[a:a + l] == ord("N")) for a, l in zip(starts, lens)], dtype=np.int64)
        kept = (window_n == 0) | (nn <= sequence.MAX_N)
        f = _window_scores(sequence.materialize_spans(seq, starts, lens))
        r = _window_scores(sequence.revcomp_spans(seq, starts, lens))
        return len(offsets) - 1, ids, kept, f, r

    @staticmethod
    def _mean(n_contigs, ids, kept, scores):
        out = np.zeros((n_contigs, 3), np.float32)
        for c in range(n_contigs):
            s, k = np.zeros(3, np.float32), 0
            for i in np.flatnonzero((ids == c) & kept):
                s, k = s + scores[i], k + 1
            if k:
                out[c] = s / np.float32(k)
        return out

    def classify_contigs(self, seq, offsets, single_window=False, precision=None):
        type(self).calls.append("plain")
        n, ids, kept, f, _ = self._run(seq, offsets, single_window)
        return self._mean(n, ids, kept, f), ids[kept]

    def classify_contigs_strand(self, seq, offsets, strand="both", single_window=False, precision=None, embed=False):
        type(self).calls.append(strand)
        n, ids, kept, f, r = self._run(seq, offsets, single_window)
        mode = {"forward": f, "reverse": r, "both": sequence.strand_mean(f, r)}[strand]
        return self._mean(n, ids, kept, mode), ids[kept], None, self._mean(n, ids, kept, f), self._mean(n, ids, kept, r)


def _write_fasta(path, seed=21, n=17):
    rng = np.random.default_rng(seed)
    recs = [(f"c{i}", "".join(rng.choice(list("ACGTN"), int(rng.integers(800, 30000)), p=[.245, .245, .245, .245, .02])))
            for i in range(n)]
    recs.insert(3, ("nrun", "".join(rng.choice(list("ACGT"), 6000)) + "N" * 5000 + "".join(rng.choice(list("ACGT"), 3000))))
    path.write_text("".join(f">{name} note\n{s}\n" for name, s in recs))
    return recs


@pytest.fixture
def fake_main(monkeypatch):
    monkeypatch.setattr(nnc, "_engine", lambda: FakeStrandEngine())
    for k in ("GENOMAD_AMD_FRONT_END", "GENOMAD_AMD_STRAND", "GENOMAD_AMD_EMBEDDINGS", "GENOMAD_AMD_SCAN_STRIDE", "GENOMAD_AMD_PRECISION"):
        monkeypatch.delenv(k, raising=False)
    del FakeStrandEngine.calls[:]
    return lambda fa, out, **kw: nnc.main(fa, out, False, 128, False, 1, False, False, **kw)


def _tree(d):
    return sorted(str(p.relative_to(d)) for p in d.rglob("*"))


def _npz(path):
    z = np.load(path)
    return {k: z[k] for k in z.files}


def _same_npz(a, b):
    a, b = _npz(a), _npz(b)
    return sorted(a) == sorted(b) and all(a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]) for k in a)


def test_strand_switch_values(monkeypatch):
    monkeypatch.delenv("GENOMAD_AMD_STRAND", raising=False)
    assert nnc.strand_requested() == "forward"
    for v, want in (("", "forward"), ("forward", "forward"), (" reverse ", "reverse"), ("both", "both")):
        monkeypatch.setenv("GENOMAD_AMD_STRAND", v)
        assert nnc.strand_requested() == want
    for v in ("Both", "rc", "1", "forward,reverse"):
        monkeypatch.setenv("GENOMAD_AMD_STRAND", v)
        with pytest.raises(ValueError, match=r"GENOMAD_AMD_STRAND.*forward, reverse, both"):
            nnc.strand_requested()


def test_main_refuses_a_bad_value_and_the_host_front_end(tmp_path, monkeypatch, fake_main, capsys):
    from tests.test_scan_host import _MustNotRun
    fa = tmp_path / "s.fna"
    _write_fasta(fa, n=3)
    monkeypatch.setenv("GENOMAD_AMD_STRAND", "sideways")
    with pytest.raises(ValueError, match="GENOMAD_AMD_STRAND"):
        fake_main(fa, tmp_path / "bad")
    assert not (tmp_path / "bad").exists()
    for env, kw in (({"GENOMAD_AMD_FRONT_END": "host"}, {}), ({}, {"_backend": _MustNotRun()})):
        monkeypatch.setenv("GENOMAD_AMD_STRAND", "both")
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with pytest.raises(SystemExit) as exc:
            fake_main(fa, tmp_path / "host", **kw)
        assert exc.value.code == 1
        assert "GENOMAD_AMD_STRAND needs the device front end" in capsys.readouterr().err
        assert not list((tmp_path / "host").rglob("*.npz")) and not list((tmp_path / "host").rglob("*.tsv"))
        monkeypatch.delenv("GENOMAD_AMD_FRONT_END", raising=False)
    assert FakeStrandEngine.calls == []


def test_main_forward_is_todays_output_and_the_modes_carry_through(tmp_path, monkeypatch, fake_main):
    fa = tmp_path / "m.fna"
    _write_fasta(fa)
    fake_main(fa, tmp_path / "unset")
    monkeypatch.setenv("GENOMAD_AMD_STRAND", "forward")
    fake_main(fa, tmp_path / "forward")
    assert FakeStrandEngine.calls == ["plain", "plain"]                    # forward goes through the entry point it always used
    d0, d1 = tmp_path / "unset" / "m_nn_classification", tmp_path / "forward" / "m_nn_classification"
    assert _tree(d0) == _tree(d1) and not any("strand" in f for f in _tree(d0))
    assert (d0 / "m_nn_classification.tsv").read_bytes() == (d1 / "m_nn_classification.tsv").read_bytes()
    for rel in ("m_nn_classification.npz", "m_encoded_sequences/m_seq_window_id.npz"):
        assert _same_npz(d0 / rel, d1 / rel)
    names, seq, off = sequence.read_fasta_packed(fa)
    eng = FakeStrandEngine()
    for mode in ("reverse", "both"):
        monkeypatch.setenv("GENOMAD_AMD_STRAND", mode)
        fake_main(fa, tmp_path / mode)
        d = tmp_path / mode / "m_nn_classification"
        assert _tree(d) == sorted(_tree(d0) + ["m_nn_strand.npz"])
        want, ids, _, fwd, rev = eng.classify_contigs_strand(seq, off, mode)
        z = _npz(d / "m_nn_classification.npz")
        assert list(z["contig_names"]) == list(names) and np.array_equal(z["predictions"], want)
        assert _same_npz(d / "m_encoded_sequences/m_seq_window_id.npz", d0 / "m_encoded_sequences/m_seq_window_id.npz")
        s = _npz(d / "m_nn_strand.npz")
        assert sorted(s) == ["contig_names", "max_abs_diff", "scores_fwd", "scores_rev", "strand"]
        assert str(s["strand"]) == mode and list(s["contig_names"]) == list(names)
        assert np.array_equal(s["scores_fwd"], fwd) and np.array_equal(s["scores_rev"], rev)
        assert np.array_equal(s["scores_fwd"], _npz(d0 / "m_nn_classification.npz")["predictions"])
        assert s["max_abs_diff"].dtype == np.float32 and np.array_equal(s["max_abs_diff"], np.abs(fwd - rev).max(axis=1))
        assert s["max_abs_diff"].max() > 0.05
        assert (d / "m_nn_classification.tsv").read_bytes() != (d0 / "m_nn_classification.tsv").read_bytes()
        assert json.loads((d / "m_nn_classification.json").read_text())["parameters"] == {"single_window": False}


def test_main_resume_recomputes_when_the_mode_changes(tmp_path, monkeypatch, fake_main):
    fa = tmp_path / "r.fna"
    _write_fasta(fa, seed=4, n=6)
    out = tmp_path / "out"
    d = out / "r_nn_classification"
    fake_main(fa, out)
    forward = _npz(d / "r_nn_classification.npz")["predictions"]
    fake_main(fa, out)
    assert FakeStrandEngine.calls == ["plain"]                             # same mode, everything there: nothing runs
    monkeypatch.setenv("GENOMAD_AMD_STRAND", "both")
    fake_main(fa, out)                                                     # no strand file = forward outputs: recomputed
    assert FakeStrandEngine.calls == ["plain", "both"] and str(_npz(d / "r_nn_strand.npz")["strand"]) == "both"
    both = _npz(d / "r_nn_classification.npz")["predictions"]
    assert not np.array_equal(both, forward)
    fake_main(fa, out)
    assert FakeStrandEngine.calls == ["plain", "both"]
    monkeypatch.setenv("GENOMAD_AMD_STRAND", "reverse")
    fake_main(fa, out)
    assert FakeStrandEngine.calls[-1] == "reverse" and str(_npz(d / "r_nn_strand.npz")["strand"]) == "reverse"
    monkeypatch.delenv("GENOMAD_AMD_STRAND")
    fake_main(fa, out)                                                     # and back: forward again, the strand file goes
    assert FakeStrandEngine.calls[-1] == "plain" and len(FakeStrandEngine.calls) == 4
    assert not (d / "r_nn_strand.npz").exists()
    assert np.array_equal(_npz(d / "r_nn_classification.npz")["predictions"], forward)
    fake_main(fa, out)
    assert len(FakeStrandEngine.calls) == 4


# ---- several ranks ----------------------------------------------------------------------------------------------------------------
def _gloo_strand_main_worker(rank, world, port, fasta, out_dir, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), GENOMAD_AMD_STRAND="both")
    for k in ("GENOMAD_AMD_FRONT_END", "GENOMAD_AMD_EMBEDDINGS", "GENOMAD_AMD_SCAN_STRIDE"):
        os.environ.pop(k, None)
    from tests.gloo_comm import GlooComm
    nnc._engine = lambda: FakeStrandEngine()
    comm = GlooComm(rank, world, port)
    code = 0
    try:
        nnc.main(fasta, out_dir, False, 128, False, 1, False, False, _comm=comm)
    except SystemExit as e:
        code = e.code
    q.put((rank, code))
    comm.close()


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_give_the_bytes_of_one_process(tmp_path, monkeypatch, fake_main, world):
    mp = pytest.importorskip("torch.multiprocessing")
    fa = tmp_path / "g.fna"
    _write_fasta(fa, seed=9, n=23)
    monkeypatch.setenv("GENOMAD_AMD_STRAND", "both")
    fake_main(fa, tmp_path / "one")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    out = tmp_path / f"ranks{world}"
    procs = [ctx.Process(target=_gloo_strand_main_worker, args=(r, world, port, str(fa), str(out), q)) for r in range(world)]
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
    for rel in ("g_nn_classification.npz", "g_nn_strand.npz", "g_encoded_sequences/g_seq_window_id.npz"):
        assert _same_npz(d1 / rel, dn / rel), rel


def test_strand_gathers_one_process_out_of_order_and_empty():
    rng = np.random.default_rng(8)
    f, r = rng.random((9, 3), dtype=np.float32), rng.random((9, 3), dtype=np.float32)
    got = sharding.gather_contig_strand_scores(None, [(5, f[4:], r[4:]), (1, f[:4], r[:4]), (3, f[4:4], r[4:4])])
    assert np.array_equal(got[0], f) and np.array_equal(got[1], r) and got[0].dtype == np.float32
    empty = sharding.gather_contig_strand_scores(None, [])
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3)
    # the scans' extra per-window arrays travel with the windows
    from tests.test_scan_host import _fake_scan, _assert_scans_equal
    seq = rng.choice(np.frombuffer(b"ACGTN", np.uint8), 60000)
    offsets = np.array([0, 100, 20000, 47000, 60000], np.int64)

    def scan(a, b):
        d = _fake_scan(seq[offsets[a]:offsets[b]], offsets[a:b + 1] - offsets[a])
        d["scores_fwd"], d["scores_rev"] = d["scores"] * np.float32(2), d["scores"] + np.float32(1)
        return d
    whole = scan(0, 4)
    got = sharding.gather_contig_scans(None, [(7, scan(2, 4)), (0, scan(0, 2))], extra_window_fields=sharding.SCAN_STRAND_FIELDS)
    _assert_scans_equal(got, whole)
    plain = sharding.gather_contig_scans(None, [(7, scan(2, 4)), (0, scan(0, 2))])
    assert "scores_fwd" not in plain and np.array_equal(plain["scores"], whole["scores"])
