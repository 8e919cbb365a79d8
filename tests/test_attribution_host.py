"""CPU checks of the attention contribution maps: the fp64 reference maps the GPU tests compare against (complete, not vacuous), the
ABI, and main()'s GENOMAD_AMD_ATTRIBUTION_BIN switch over a fake engine (validation, the refusals, byte-identical outputs without it,
the npz, the resume rule, several ranks)."""
import os
import socket
import zlib

import numpy as np
import pytest

from genomad_amd import _lib, sequence, sharding
from genomad_amd import nn_classification as nnc
from tests import attribution_ref as R
from tests.fake_engine import FakeEngine
from tests.test_strand_host import FakeStrandEngine, _npz, _same_npz, _tree, _window_scores, _write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 6000
FIELDS = ("bin", "win_offsets", "starts", "lens", "kept", "window_scores", "contrib", "bias", "logits", "contig_scores")


def test_reference_maps_are_complete_and_not_vacuous():
    """Completeness of the fp64 maps to 1e-12; on every window some (head, position) holds more than 10x the uniform share of
    sum |contrib|; the two heads' maps differ.  Measured on the 32 windows: completeness 2.6e-14, largest |contrib| 8.15."""
    bases, ref = R.reference_32()
    c = ref["contrib"]
    assert c.shape == (32, 2, 749, 3) and ref["bias"].shape == ref["logits"].shape == (32, 3) and c.dtype == np.float64
    gap = np.abs(c.sum(axis=(1, 2)) + ref["bias"] - ref["logits"]).max()
    per_pos = np.abs(c).sum(axis=3).reshape(32, -1)                       # (window, head x position)
    peak = per_pos.max(axis=1) / per_pos.mean(axis=1)
    undecided, undecided_scaled = int((~R.decided(ref)).sum()), int((~R.decided(ref, scaled=True)).sum())
    print(f"\nreference maps: completeness {gap:.2e}, largest |contrib| {np.abs(c).max():.2f}, sum |contrib| per class "
          f"{np.abs(c).sum(axis=(1, 2)).min():.1f} .. {np.abs(c).sum(axis=(1, 2)).max():.1f}, smallest peak / uniform share {peak.min():.1f}, "
          f"{undecided} undecided windows ({undecided_scaled} under the margin scaled by max |h1|)")
    assert gap <= 1e-12
    assert (peak > 10).all()
    assert np.abs(c[:, 0] - c[:, 1]).reshape(32, -1).max(axis=1).min() > 0.1 * np.abs(c).reshape(32, -1).max(axis=1).min()
    assert undecided <= 2 and (R.decided(ref) | ~R.decided(ref, scaled=True)).all()      # compares no less than the scaled rule
    # the gradient really is the head's: logits = g . f + bias on the oracle's own features (the same identity, before the split)
    assert np.abs(np.einsum("nic,ni->nc", ref["g"], ref["f"]) + ref["bias"] - ref["logits"]).max() <= 1e-12
    assert np.abs(ref["g"]).max() > 0 and np.isfinite(c).all()
    # binned(): the helper of the GPU tests sums every bin's positions and nothing else
    c32 = c[:2].astype(np.float32)
    for bin_ in (8, 100, 748, 749):
        b = R.binned(c32, bin_)
        assert b.shape == (2, 2, -(-749 // bin_), 3) and np.allclose(b.sum(axis=2), c32.sum(axis=2, dtype=np.float64), atol=1e-4)
    assert np.array_equal(R.binned(c32, 1), c32)


def test_abi_declares_the_attribution_entry_points():
    text = open(os.path.join(ROOT, "include", "genomad_nn.h")).read()
    lib = _lib.load()
    for name in ("gnn_attribute", "gnn_attribute_dev", "gnn_attribute_contigs"):
        assert f"int {name}(" in text and name in _lib.SIGNATURES and hasattr(lib, name)
    from genomad_amd.engine import AttributionResult, NNEngine
    for m in ("attribute", "attribute_dev", "attribute_contigs", "attribute_contigs_dev"):
        assert hasattr(NNEngine, m)
    assert AttributionResult.FIELDS == FIELDS
    assert [NNEngine.attribution_bins(b) for b in (1, 8, 100, 748, 749)] == [749, 94, 8, 2, 1]
    # a bad bin and the frozen arithmetic are refused before the ctx is looked at: no GPU needed
    off = np.zeros(1, np.int64)
    for bad in (0, 750, -3):
        rc = lib.gnn_attribute_contigs(None, None, 1, 0, off.ctypes.data, 0, bad, 0, _lib.PREC_F16X3TC, None, 0, None, None, None, None, None)
        assert rc == _lib.ERR_ARG and b"[1, 749]" in lib.gnn_last_error() and str(bad).encode() in lib.gnn_last_error()
    rc = lib.gnn_attribute_contigs(None, None, 1, 0, off.ctypes.data, 0, 8, 0, _lib.PREC_F16C6, None, 0, None, None, None, None, None)
    assert rc == _lib.ERR_ARG and b"f16c6" in lib.gnn_last_error()


# ---- main() over a fake engine ---------------------------------------------------------------------------------------------------
class FakeAttributionEngine(FakeStrandEngine, FakeEngine):
    """tests/fake_engine.py's engine with the contig entry points main() calls (FakeStrandEngine: numpy, from the definitions of
    sequence.py) plus attribute_contigs: per window a fixed function of its 6000 bytes in place of the maps"""
    calls = []

    def __init__(self):
        self.device = 0                     # no rendezvous directory: main() brings its own transport

    def attribute_contigs(self, seq, offsets, bin=1, single_window=False, precision=None):
        from genomad_amd.engine import AttributionResult
        type(self).calls.append(("attribute", int(bin)))
        offsets = np.asarray(offsets, np.int64)
        n, ids, kept, f, _ = self._run(seq, offsets, single_window)
        starts, lens, _, window_n = sequence.candidate_spans(offsets, single_window)
        wins = sequence.materialize_spans(seq, starts, lens)
        one = np.zeros((len(wins), 2, 749, 3), np.float32)
        rest = np.zeros((len(wins), 2, 3), np.float32)
        for i, w in enumerate(wins):
            rng = np.random.default_rng(zlib.crc32(w.tobytes()) ^ 0xA77)
            one[i], rest[i] = rng.standard_normal((2, 749, 3), dtype=np.float32), rng.standard_normal((2, 3), dtype=np.float32)
        win_off = np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=n))]).astype(np.int64)
        return AttributionResult(bin=int(bin), win_offsets=win_off, starts=window_n.astype(np.int64) * W, lens=lens, kept=kept,
                                 window_scores=f, contrib=R.binned(one, int(bin)), bias=rest[:, 0], logits=rest[:, 1],
                                 contig_scores=self._mean(n, ids, kept, f))


ENV = ("GENOMAD_AMD_FRONT_END", "GENOMAD_AMD_STRAND", "GENOMAD_AMD_EMBEDDINGS", "GENOMAD_AMD_SCAN_STRIDE", "GENOMAD_AMD_PRECISION",
       "GENOMAD_AMD_OCCLUSION_BLOCK", "GENOMAD_AMD_ATTRIBUTION_BIN")


@pytest.fixture
def fake_main(monkeypatch):
    monkeypatch.setattr(nnc, "_engine", lambda: FakeAttributionEngine())
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    del FakeAttributionEngine.calls[:]
    return lambda fa, out, **kw: nnc.main(fa, out, False, 128, False, 1, False, False, **kw)


def test_attribution_switch_values(monkeypatch):
    monkeypatch.delenv("GENOMAD_AMD_ATTRIBUTION_BIN", raising=False)
    assert nnc.attribution_bin_requested() is None
    for v, want in (("", None), (" 1 ", 1), ("8", 8), ("749", 749)):
        monkeypatch.setenv("GENOMAD_AMD_ATTRIBUTION_BIN", v)
        assert nnc.attribution_bin_requested() == want
    for v in ("0", "750", "-5", "1.5", "bin", "1e2"):
        monkeypatch.setenv("GENOMAD_AMD_ATTRIBUTION_BIN", v)
        with pytest.raises(ValueError, match=r"GENOMAD_AMD_ATTRIBUTION_BIN.*\[1, 749\]"):
            nnc.attribution_bin_requested()


def test_main_refuses_a_bad_value_the_other_strands_and_the_host_front_end(tmp_path, monkeypatch, fake_main, capsys):
    from tests.test_scan_host import _MustNotRun
    fa = tmp_path / "s.fna"
    _write_fasta(fa, n=3)
    for v in ("750", "many"):
        monkeypatch.setenv("GENOMAD_AMD_ATTRIBUTION_BIN", v)
        with pytest.raises(ValueError, match="GENOMAD_AMD_ATTRIBUTION_BIN"):
            fake_main(fa, tmp_path / "bad")
        assert not (tmp_path / "bad").exists()                  # before anything is written
    monkeypatch.setenv("GENOMAD_AMD_ATTRIBUTION_BIN", "8")
    for env, kw, msg in (({"GENOMAD_AMD_FRONT_END": "host"}, {}, "GENOMAD_AMD_ATTRIBUTION_BIN needs the device front end"),
                         ({}, {"_backend": _MustNotRun()}, "GENOMAD_AMD_ATTRIBUTION_BIN needs the device front end"),
                         ({"GENOMAD_AMD_PRECISION": "f16c6", "GENOMAD_AMD_ALLOW_OUT_OF_TOLERANCE": "1"}, {},
                          "GENOMAD_AMD_ATTRIBUTION_BIN cannot be combined with GENOMAD_AMD_PRECISION=f16c6"),
                         ({"GENOMAD_AMD_STRAND": "both"}, {}, "GENOMAD_AMD_ATTRIBUTION_BIN is forward-strand only"),
                         ({"GENOMAD_AMD_STRAND": "reverse"}, {}, "GENOMAD_AMD_ATTRIBUTION_BIN is forward-strand only")):
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
    assert FakeAttributionEngine.calls == []
    monkeypatch.setenv("GENOMAD_AMD_STRAND", "forward")         # forward, spelled out, is no other strand
    fake_main(fa, tmp_path / "fwd")
    assert (tmp_path / "fwd" / "s_nn_classification" / "s_nn_attribution.npz").exists()


def test_main_writes_the_map_and_changes_nothing_else(tmp_path, monkeypatch, fake_main):
    fa = tmp_path / "m.fna"
    _write_fasta(fa)
    fake_main(fa, tmp_path / "unset")
    assert FakeAttributionEngine.calls == ["plain"]
    monkeypatch.setenv("GENOMAD_AMD_ATTRIBUTION_BIN", "100")
    fake_main(fa, tmp_path / "on")
    assert FakeAttributionEngine.calls == ["plain", "plain", ("attribute", 100)]     # the classification goes the way it always went
    d0, d1 = tmp_path / "unset" / "m_nn_classification", tmp_path / "on" / "m_nn_classification"
    assert _tree(d1) == sorted(_tree(d0) + ["m_nn_attribution.npz"])
    assert (d0 / "m_nn_classification.tsv").read_bytes() == (d1 / "m_nn_classification.tsv").read_bytes()
    for rel in ("m_nn_classification.npz", "m_encoded_sequences/m_seq_window_id.npz"):
        assert _same_npz(d0 / rel, d1 / rel)
    names, seq, off = sequence.read_fasta_packed(fa)
    want = FakeAttributionEngine().attribute_contigs(seq, off, 100).asdict()
    z = _npz(d1 / "m_nn_attribution.npz")
    assert sorted(z) == sorted(("contig_names",) + FIELDS)
    assert list(z["contig_names"]) == list(names) and int(z["bin"]) == 100 and z["bin"].dtype == np.int64
    dtypes = {"win_offsets": np.int64, "starts": np.int64, "lens": np.int32, "kept": np.bool_, "window_scores": np.float32,
              "contrib": np.float32, "bias": np.float32, "logits": np.float32, "contig_scores": np.float32}
    for k, dt in dtypes.items():
        assert z[k].dtype == dt and np.array_equal(z[k], want[k]), k
    assert z["contrib"].shape == (len(z["starts"]), 2, 8, 3) and np.abs(z["contrib"]).max() > 1
    assert np.array_equal(z["contig_scores"], _npz(d0 / "m_nn_classification.npz")["predictions"])
    assert not z["kept"].all()                                   # the nrun record: the mask travels


def test_main_resume_follows_the_bin(tmp_path, monkeypatch, fake_main):
    fa = tmp_path / "r.fna"
    _write_fasta(fa, seed=4, n=6)
    out = tmp_path / "out"
    d = out / "r_nn_classification"
    monkeypatch.setenv("GENOMAD_AMD_ATTRIBUTION_BIN", "100")
    fake_main(fa, out)
    first = _npz(d / "r_nn_attribution.npz")
    fake_main(fa, out)
    assert FakeAttributionEngine.calls == ["plain", ("attribute", 100)]        # same request, everything there: nothing runs
    monkeypatch.setenv("GENOMAD_AMD_ATTRIBUTION_BIN", "50")
    fake_main(fa, out)                                                         # another bin: recomputed
    assert FakeAttributionEngine.calls[2:] == ["plain", ("attribute", 50)] and int(_npz(d / "r_nn_attribution.npz")["bin"]) == 50
    assert _npz(d / "r_nn_attribution.npz")["contrib"].shape[2] == 15
    fake_main(fa, out)
    assert len(FakeAttributionEngine.calls) == 4
    monkeypatch.delenv("GENOMAD_AMD_ATTRIBUTION_BIN")
    fake_main(fa, out)                                                         # no request: the file goes
    assert FakeAttributionEngine.calls[4:] == ["plain"] and not (d / "r_nn_attribution.npz").exists()
    fake_main(fa, out)
    assert len(FakeAttributionEngine.calls) == 5
    monkeypatch.setenv("GENOMAD_AMD_ATTRIBUTION_BIN", "100")
    fake_main(fa, out)                                                         # scores on disk, no map: the stage runs again
    assert FakeAttributionEngine.calls[5:] == ["plain", ("attribute", 100)]
    z = _npz(d / "r_nn_attribution.npz")
    assert sorted(z) == sorted(first) and all(np.array_equal(z[k], first[k]) for k in first)


# ---- several ranks ----------------------------------------------------------------------------------------------------------------
def _gloo_attribution_main_worker(rank, world, port, fasta, out_dir, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), GENOMAD_AMD_ATTRIBUTION_BIN="100")
    for k in ENV[:-1]:
        os.environ.pop(k, None)
    from tests.gloo_comm import GlooComm
    nnc._engine = lambda: FakeAttributionEngine()
    comm = GlooComm(rank, world, port)
    code = 0
    try:
        nnc.main(fasta, out_dir, False, 128, False, 1, False, False, _comm=comm)
    except SystemExit as e:
        code = e.code
    q.put((rank, code))
    comm.close()


def test_two_ranks_give_the_files_of_one_process(tmp_path, monkeypatch, fake_main):
    mp = pytest.importorskip("torch.multiprocessing")
    world = 2
    fa = tmp_path / "g.fna"
    _write_fasta(fa, seed=9, n=23)
    monkeypatch.setenv("GENOMAD_AMD_ATTRIBUTION_BIN", "100")
    fake_main(fa, tmp_path / "one")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    out = tmp_path / "ranks"
    procs = [ctx.Process(target=_gloo_attribution_main_worker, args=(r, world, port, str(fa), str(out), q)) for r in range(world)]
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
    for rel in ("g_nn_classification.npz", "g_nn_attribution.npz", "g_encoded_sequences/g_seq_window_id.npz"):
        assert _same_npz(d1 / rel, dn / rel), rel


def test_attribution_gather_one_process_out_of_order_and_empty():
    rng = np.random.default_rng(8)
    seq = rng.choice(np.frombuffer(b"ACGTN", np.uint8), 60000)
    offsets = np.array([0, 100, 20000, 20000, 47000, 60000], np.int64)
    eng = FakeAttributionEngine()
    piece = lambda a, b: eng.attribute_contigs(seq[offsets[a]:offsets[b]], offsets[a:b + 1] - offsets[a], 100)      # noqa: E731
    whole = piece(0, 5).asdict()
    got = sharding.gather_contig_attributions(None, [(7, piece(3, 5)), (0, piece(0, 2)), (3, piece(2, 3).asdict())], 8)
    assert sorted(got) == sorted(FIELDS[1:])
    for k in got:
        assert got[k].dtype == whole[k].dtype and np.array_equal(got[k], whole[k]), k
    empty = sharding.gather_contig_attributions(None, [], 8)
    assert list(empty["win_offsets"]) == [0] and empty["contrib"].shape == (0, 2, 8, 3) and empty["kept"].dtype == np.bool_
    with pytest.raises(ValueError, match="duplicate"):
        sharding.gather_contig_attributions(None, [(1, piece(0, 1)), (1, piece(1, 2))], 8)
