"""CPU checks of the encoder-embedding feature: what "embedding" means (the reference's own create_encoder()), the committed
fixture, the rank-0 gather of per-contig embeddings, and main()'s refusal on the host front end."""
import importlib.util
import os
import socket

import numpy as np
import pytest

from genomad_amd import sharding, synthetic
from oracle import igloo_oracle, reference_harness, sequence_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "encoder_golden.npz")


def _golden_script():
    spec = importlib.util.spec_from_file_location("make_encoder_golden", os.path.join(ROOT, "scripts", "make_encoder_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def oracle_h1_4(synth_weights):
    """fp64 oracle h1 of the first 4 windows of config 2"""
    tokens = sequence_oracle.tokenize_closed_form(synthetic.synth_windows(0, 4))
    return tokens, igloo_oracle.forward(tokens, synth_weights, np.float64, return_taps=True)[1]["h1"]


@pytest.mark.skipif(not reference_harness.available(), reason="the reference checkout is not on this machine")
def test_reference_create_encoder_equals_oracle_h1(synth_weights, oracle_h1_4):
    """The embedding IS create_encoder()'s output (model.py:14-31): the reference's own graph, run live over the numpy stand-ins
    with the seed-42 weights, equals the oracle's h1 - which is what dense_kernel's h1 restates."""
    tokens, h1 = oracle_h1_4
    enc = _golden_script().reference_encoder
    e64 = enc(tokens, synth_weights, np.float64)
    e32 = enc(tokens, synth_weights, np.float32)
    assert e64.shape == e32.shape == (4, 512)
    assert np.abs(e64 - h1).max() <= 1e-10
    assert np.abs(e32.astype(np.float64) - h1).max() <= 1e-5
    g = np.load(GOLDEN)                         # the committed fixture is that same output
    assert np.abs(g["emb_refgraph64"][:4] - e64).max() <= 1e-12
    assert np.abs(g["emb_refgraph32"][:4].astype(np.float64) - e32).max() <= 1e-6


def test_encoder_golden_matches_the_oracle(synth_weights, oracle_h1_4):
    """tests/golden/encoder_golden.npz (written by scripts/make_encoder_golden.py from the reference's graph) against the oracle."""
    g = np.load(GOLDEN)
    assert g["emb_refgraph32"].shape == g["emb_refgraph64"].shape == (64, 512)
    assert g["emb_refgraph32"].dtype == np.float32 and int(g["n"]) == 64 and int(g["data_seed"]) == 1234
    _, h1 = oracle_h1_4
    assert np.abs(g["emb_refgraph64"][:4] - h1).max() <= 1e-10
    assert np.abs(g["emb_refgraph32"][:4].astype(np.float64) - h1).max() <= 1e-5
    assert (g["emb_refgraph64"] > 0).mean() > 0.2             # not a vacuous fixture: the ReLU leaves a good share of units on


# ---- gather of per-contig embeddings (sharding.gather_contig_embeddings) ---------------------------------------------------------
def _write_fasta(path):
    rng = np.random.default_rng(21)
    recs = [(f"c{i}", "".join(rng.choice(list("ACGTN"), int(rng.integers(500, 40000)), p=[.24, .24, .24, .24, .04])))
            for i in range(23)]
    path.write_text("".join(f">{n} note\n{s}\n" for n, s in recs))


def _fake_contig_rows(seq, offsets):
    """stand-in per-contig results: scores, embeddings and window ids that depend only on each contig's bytes"""
    from genomad_amd import sequence
    n = len(offsets) - 1
    scores = np.zeros((n, 3), np.float32)
    emb = np.zeros((n, 512), np.float32)
    for c in range(n):
        b = np.asarray(seq[offsets[c]:offsets[c + 1]], dtype=np.uint8)
        seed = int(b.astype(np.int64).sum()) * 131 + len(b)
        r = np.random.default_rng(seed)
        scores[c] = r.random(3, dtype=np.float32)
        emb[c] = r.standard_normal(512).astype(np.float32)
    _, _, ids, _ = sequence.candidate_spans(np.asarray(offsets, np.int64))
    return scores, emb, ids


def _gloo_emb_worker(rank, world, port, path, q):
    from genomad_amd import sequence
    from tests.gloo_comm import GlooComm
    comm = GlooComm(rank, world, port)
    parts, emb_parts = [], []
    for k in (1, 0):                  # two pieces per rank, handed over out of order
        names, seq, offsets = sequence.read_fasta_packed(path, True, sequence.record_aligned_range(path, rank, world, k, 2))
        scores, emb, ids = _fake_contig_rows(seq, offsets)
        parts.append((rank * 64 + k, names, scores, ids))
        emb_parts.append((rank * 64 + k, emb))
    out = sharding.gather_contig_parts(comm, parts)
    emb = sharding.gather_contig_embeddings(comm, emb_parts)
    if rank == 0:
        q.put((out, emb))
    else:
        assert emb is None and out[0] is None
    comm.close()


@pytest.mark.parametrize("world", [2, 3])
def test_gloo_contig_embeddings_gather_equals_single_process(tmp_path, world):
    """Per-contig embeddings reach rank 0 in the pieces' file order, bit-identical to one process; the existing gather beside it
    returns what it always did."""
    mp = pytest.importorskip("torch.multiprocessing")
    from genomad_amd import sequence
    p = tmp_path / "meta.fna"
    _write_fasta(p)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_emb_worker, args=(r, world, port, str(p), q)) for r in range(world)]
    for pr in procs:
        pr.start()
    (names, preds, ids, total), emb = q.get(timeout=180)
    for pr in procs:
        pr.join(timeout=180)
        assert pr.exitcode == 0
    n1, s1, o1 = sequence.read_fasta_packed(p)
    want_scores, want_emb, want_ids = _fake_contig_rows(s1, o1)
    assert list(names) == list(n1) and np.array_equal(preds, want_scores)
    assert np.array_equal(ids, want_ids) and total == len(want_ids)
    assert emb.dtype == np.float32 and emb.shape == (len(n1), 512)
    assert np.array_equal(emb, want_emb)


def test_contig_embeddings_gather_one_process_and_empty_pieces():
    rows = np.arange(6 * 512, dtype=np.float32).reshape(6, 512)
    got = sharding.gather_contig_embeddings(None, [(3, rows[4:]), (0, rows[:1]), (1, rows[1:1]), (2, rows[1:4])])
    assert np.array_equal(got, rows)
    assert sharding.gather_contig_embeddings(None, []).shape == (0, 512)
    with pytest.raises(ValueError, match="duplicate"):
        sharding.gather_contig_embeddings(None, [(0, rows[:1]), (0, rows[1:2])])


# ---- main() ---------------------------------------------------------------------------------------------------------------------
class _MustNotRun:
    """host front-end backend whose use is a failure: main() has to stop before it classifies anything"""

    def score(self, windows):
        raise AssertionError("classified although the embeddings cannot be produced on this path")

    def segment_mean(self, scores, ids, n_segments):
        raise AssertionError("classified although the embeddings cannot be produced on this path")


def test_main_with_embeddings_on_the_host_front_end_exits_before_classifying(tmp_path, monkeypatch, capsys):
    from genomad_amd import nn_classification as nnc
    fa = tmp_path / "s.fna"
    fa.write_text(">a\n" + "ACGT" * 2000 + "\n>b\n" + "GATTACA" * 900 + "\n")
    monkeypatch.setenv("GENOMAD_AMD_EMBEDDINGS", "1")
    with pytest.raises(SystemExit) as exc:
        nnc.main(fa, tmp_path / "out", False, 128, False, 1, False, False, _backend=_MustNotRun())
    assert exc.value.code == 1
    assert "GENOMAD_AMD_EMBEDDINGS" in capsys.readouterr().err
    assert not list((tmp_path / "out").rglob("*.npz")) and not list((tmp_path / "out").rglob("*.tsv"))


def test_embeddings_switch_values(monkeypatch):
    from genomad_amd import nn_classification as nnc
    monkeypatch.delenv("GENOMAD_AMD_EMBEDDINGS", raising=False)
    assert nnc.embeddings_requested() is False
    for v, want in (("0", False), ("1", True)):
        monkeypatch.setenv("GENOMAD_AMD_EMBEDDINGS", v)
        assert nnc.embeddings_requested() is want
    monkeypatch.setenv("GENOMAD_AMD_EMBEDDINGS", "yes")
    with pytest.raises(ValueError, match="GENOMAD_AMD_EMBEDDINGS"):
        nnc.embeddings_requested()


def test_abi_declares_the_embedding_entry_points():
    from genomad_amd import _lib
    text = open(os.path.join(ROOT, "include", "genomad_nn.h")).read()
    assert "#define GNN_EMBED_DIM 512" in text and "GNN_EMB_BF16 = 1" in text
    lib = _lib.load()
    for name in ("gnn_embed", "gnn_embed_dev", "gnn_classify_contigs_embed"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.EMBED_DIM == _lib.HIDDEN == 512
