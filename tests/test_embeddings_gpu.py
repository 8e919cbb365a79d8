"""Encoder embeddings on the MI355X: per-window parity with the fp64 oracle's h1 and the reference-graph fixture, scores unchanged,
bf16 rounding, batch invariance, the per-contig fold (against a numpy mean of the per-window path), chunk invariance, the range
fallback and main() end to end with GENOMAD_AMD_EMBEDDINGS."""
import json
import os

import numpy as np
import pytest

from genomad_amd import _lib, sequence, synthetic
from oracle import igloo_oracle, sequence_oracle
from tests.conftest import need_tables

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITH = ["f32", "f16x3", "bf16x3", "f16x3tc", "f16x3tk"]
EMB_TOL = 1e-4          # per window: max |de| <= EMB_TOL * max(1, max |h1_ref|)


@pytest.fixture(scope="module")
def oracle_h1(synth_weights):
    """fp64 oracle h1 (= create_encoder()'s output) of the 128 synthetic windows of test_fused_scores_256_windows"""
    bases = synthetic.synth_windows(0, 128)
    tokens = sequence_oracle.tokenize_closed_form(bases)
    h1 = np.concatenate([igloo_oracle.forward(tokens[a:a + 16], synth_weights, np.float64, literal=False, return_taps=True)[1]["h1"]
                         for a in range(0, len(tokens), 16)])
    return bases, h1


def _window_err(got, want):
    """per-window max |d| relative to max(1, max |want|) of that window"""
    d = np.abs(got.astype(np.float64) - want).max(axis=1)
    return d / np.maximum(1.0, np.abs(want).max(axis=1))


def test_oracle_embeddings_are_not_vacuous(oracle_h1):
    """the reference embeddings of these windows are neither mostly zero after the ReLU nor alike across windows"""
    _, h1 = oracle_h1
    assert (h1 > 0).mean() > 0.3
    assert h1.std(axis=0).mean() > 0.05
    assert np.isfinite(h1).all()


@pytest.mark.parametrize("prec", ARITH)
def test_window_embeddings_match_the_oracle_and_the_reference_graph(engine, oracle_h1, prec, request):
    need_tables(request, prec)
    bases, h1 = oracle_h1
    emb = engine.embed(bases, prec)
    assert emb.dtype == np.float32 and emb.shape == (len(bases), 512)
    rel = _window_err(emb, h1)
    golden = np.load(os.path.join(ROOT, "tests", "golden", "encoder_golden.npz"))["emb_refgraph64"]
    rel_g = _window_err(emb[:len(golden)], golden)
    print(f"\nembeddings {prec}: max per-window |de| / max(1, max|h1|) = {rel.max():.3e} vs fp64 oracle, "
          f"{rel_g.max():.3e} vs reference-graph golden; max |de| = {np.abs(emb - h1).max():.3e}")
    assert rel.max() <= EMB_TOL, f"{prec}: {rel.max():.3e}"
    assert rel_g.max() <= EMB_TOL, f"{prec}: {rel_g.max():.3e}"


@pytest.mark.parametrize("prec", ARITH)
def test_embed_scores_equal_classify_bit_for_bit(engine, prec, request):
    need_tables(request, prec)
    bases = synthetic.synth_windows(300, 40)
    emb, scores = engine.embed(bases, prec, with_scores=True)
    assert np.array_equal(scores, engine.classify(bases, prec))
    assert np.array_equal(emb, engine.embed(bases, prec))           # with or without scores: the same pass


def _bf16_rne(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)


@pytest.mark.parametrize("prec", ["f16x3tc", "bf16x3", "f32"])
def test_bf16_embeddings_are_the_rounded_f32_ones(engine, prec):
    bases = synthetic.synth_windows(77, 24)
    e32 = engine.embed(bases, prec)
    e16 = engine.embed(bases, prec, dtype="bf16")
    assert e16.dtype == np.uint16 and e16.shape == e32.shape
    assert np.array_equal(e16, _bf16_rne(e32))
    assert (e16 != 0).mean() > 0.3


def test_embeddings_are_batch_invariant_and_dev_path_agrees(engine):
    bases = engine.synth_windows(0, 4096)
    full = engine.embed(bases)
    for n in (1, 7, 256):
        assert np.array_equal(engine.embed(bases[:n]), full[:n]), n
    assert np.array_equal(engine.embed(bases[4000:4007]), full[4000:4007])
    n = 300
    db, de, ds = engine.alloc(n * _lib.WINDOW), engine.alloc(n * 512 * 4), engine.alloc(n * 3 * 4)
    try:
        db.upload(bases[:n])
        engine.embed_dev(db.ptr, n, de.ptr)
        engine.sync()
        assert np.array_equal(de.download((n, 512), np.float32), full[:n])
        engine.embed_dev(db.ptr, n, de.ptr, dtype="bf16", scores_ptr=ds.ptr)
        engine.sync()
        assert np.array_equal(de.download((n, 512), np.uint16), _bf16_rne(full[:n]))
        assert np.array_equal(ds.download((n, 3), np.float32), engine.classify(bases[:n]))
    finally:
        db.free(), de.free(), ds.free()


def test_f16c6_has_no_embedding_path(engine):
    bases = synthetic.synth_windows(0, 2)
    with pytest.raises(_lib.GnnError, match="F16C6"):
        engine.embed(bases, "f16c6")
    seq = np.frombuffer(b"ACGT" * 3000, dtype=np.uint8)
    with pytest.raises(_lib.GnnError, match="F16C6"):
        engine.embed_contigs(seq, np.array([0, len(seq)]), False, "f16c6")


# ---- contig path --------------------------------------------------------------------------------------------------------------
def _contigs():
    """packed contigs: short ones (< one window, < the 2500 tail), windows that are all N (skipped by the N rule), long ones that
    straddle the slabs of a small launch size, and an empty record"""
    rng = np.random.default_rng(5)
    acgt = lambda k: "".join(rng.choice(list("ACGT"), k))          # noqa: E731
    recs = [acgt(2000), acgt(33000), acgt(6000) + "N" * 6000 + acgt(7000), acgt(100), "",
            acgt(6000) + "N" * 4100 + acgt(1900) + acgt(6000), acgt(70000), acgt(12000).lower(), acgt(2600),
            acgt(8000) + "N" * 5000]
    seq = np.frombuffer("".join(recs).encode(), dtype=np.uint8).copy()
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)
    return seq, offsets


def _numpy_contig_mean(engine, seq, offsets, single_window, prec):
    """f64 mean of embed() over every contig's kept windows (sequence.candidate_spans + the N rule), and the kept ids"""
    from genomad_amd import nn_classification as nnc
    starts, lens, ids, window_n = sequence.candidate_spans(offsets, single_window)
    wins = nnc.sentinel_windows(seq, offsets, single_window, limit=len(starts))
    nn = np.array([np.count_nonzero(seq[s:s + l] == ord("N")) for s, l in zip(starts, lens)])
    keep = (window_n == 0) | (nn <= sequence.MAX_N)
    emb = engine.embed(wins, prec).astype(np.float64)
    n = len(offsets) - 1
    out = np.zeros((n, 512))
    for c in range(n):
        sel = keep & (ids == c)
        if sel.any():
            out[c] = emb[sel].mean(axis=0)
    return out, ids[keep], int((~keep).sum())


@pytest.mark.parametrize("single_window", [False, True])
def test_contig_embeddings_equal_the_mean_of_window_embeddings(engine, single_window):
    seq, offsets = _contigs()
    prec = "f16x3tc"
    scores, emb, ids = engine.embed_contigs(seq, offsets, single_window, prec)
    s0, i0 = engine.classify_contigs(seq, offsets, single_window, prec)
    assert np.array_equal(scores, s0) and np.array_equal(ids, i0)
    want, want_ids, skipped = _numpy_contig_mean(engine, seq, offsets, single_window, prec)
    assert np.array_equal(ids, want_ids)
    if not single_window:
        assert skipped >= 2                                          # the N rule dropped windows: the mask is exercised
    assert emb.dtype == np.float32 and emb.shape == (len(offsets) - 1, 512)
    assert not emb[4].any()                                          # the empty record: zero row, as the scores
    err = np.abs(emb - want) / np.maximum(1.0, np.abs(want))
    assert err.max() <= 1e-6, err.max()
    dev = engine.alloc(seq.nbytes)
    try:
        dev.upload(seq)
        sd, ed, idd = engine.embed_contigs_dev(dev.ptr, offsets, single_window, prec)
    finally:
        dev.free()
    assert np.array_equal(sd, scores) and np.array_equal(ed, emb) and np.array_equal(idd, ids)


def test_contig_embeddings_do_not_depend_on_the_launch_size(synth_weights, engine):
    """a slab is 4 launches: with 4 windows per launch (slabs of 16 of the 31 windows) the 6- and 12-window contigs straddle slabs;
    the fold adds in window order, so the result is bit-identical to 64 windows per launch and to the session engine's default"""
    from genomad_amd.engine import NNEngine
    seq, offsets = _contigs()
    starts, _, ids, _ = sequence.candidate_spans(offsets)
    assert len(starts) > 16 and ids[15] == ids[16]                   # a contig crosses the first slab boundary at 4 windows per launch
    with NNEngine(0, synth_weights, chunk=4) as e2:
        a = e2.embed_contigs(seq, offsets, False, "f16x3tc")
        e2.lib.gnn_set_chunk(e2.ctx, 64)
        b = e2.embed_contigs(seq, offsets, False, "f16x3tc")
        e2.lib.gnn_set_chunk(e2.ctx, 13)
        c = e2.embed_contigs(seq, offsets, False, "bf16x3")
    d = engine.embed_contigs(seq, offsets, False, "f16x3tc")
    for x, y in ((a, b), (a, d)):
        for u, v in zip(x, y):
            assert np.array_equal(u, v)
    assert np.array_equal(c[1], engine.embed_contigs(seq, offsets, False, "bf16x3")[1])


# ---- main() -------------------------------------------------------------------------------------------------------------------
def _setup_main(tmp_path, monkeypatch, engine, synth_weights):
    from genomad_amd import nn_classification as nnc
    from genomad_amd import weights as W
    wpath = tmp_path / "w.npz"
    W.save_npz(wpath, synth_weights)
    monkeypatch.setenv("GENOMAD_AMD_WEIGHTS", str(wpath))
    monkeypatch.setenv("GENOMAD_AMD_KMER_TABLES", "0")
    monkeypatch.setattr(nnc, "_ENGINE", engine)
    return nnc


def _fasta(path):
    rng = np.random.default_rng(12)
    recs = [(f"k{i} d", "".join(rng.choice(list("ACGTN"), int(rng.integers(1500, 26000)), p=[.245, .245, .245, .245, .02])))
            for i in range(7)]
    path.write_text("".join(f">{n}\n{s}\n" for n, s in recs))
    return recs


def test_main_writes_the_embeddings_only_when_asked(engine, synth_weights, tmp_path, monkeypatch):
    nnc = _setup_main(tmp_path, monkeypatch, engine, synth_weights)
    fa = tmp_path / "m.fna"
    _fasta(fa)
    monkeypatch.delenv("GENOMAD_AMD_EMBEDDINGS", raising=False)
    nnc.main(fa, tmp_path / "off", False, 128, False, 1, False, False)
    monkeypatch.setenv("GENOMAD_AMD_EMBEDDINGS", "1")
    nnc.main(fa, tmp_path / "on", False, 128, False, 1, False, False)
    d_off, d_on = tmp_path / "off" / "m_nn_classification", tmp_path / "on" / "m_nn_classification"
    files = lambda d: sorted(str(p.relative_to(d)) for p in d.rglob("*"))      # noqa: E731
    assert files(d_on) == sorted(files(d_off) + ["m_nn_embeddings.npz"])
    for rel in ("m_nn_classification.npz", "m_encoded_sequences/m_seq_window_id.npz"):
        a, b = np.load(d_off / rel), np.load(d_on / rel)
        assert sorted(a.files) == sorted(b.files) and all(np.array_equal(a[k], b[k]) for k in a.files)
    assert (d_off / "m_nn_classification.tsv").read_bytes() == (d_on / "m_nn_classification.tsv").read_bytes()
    ja = json.loads((d_off / "m_nn_classification.json").read_text())
    jb = json.loads((d_on / "m_nn_classification.json").read_text())
    assert ja["parameters"] == jb["parameters"] == {"single_window": False}
    z = np.load(d_on / "m_nn_embeddings.npz")
    p = np.load(d_on / "m_nn_classification.npz")
    assert sorted(z.files) == ["contig_names", "embeddings"]
    assert list(z["contig_names"]) == list(p["contig_names"]) == [f"k{i}" for i in range(7)]
    assert z["embeddings"].dtype == np.float32 and z["embeddings"].shape == (7, 512)
    names, seq, off = sequence.read_fasta_packed(fa)
    _, want, _ = engine.embed_contigs(seq, off, False, "f16x3tc")
    assert np.array_equal(z["embeddings"], want)


def test_main_embeddings_provirus_pass_and_resume(engine, synth_weights, tmp_path, monkeypatch):
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
    monkeypatch.delenv("GENOMAD_AMD_EMBEDDINGS", raising=False)
    nnc.main(fa, out, False, 128, False, 1, False, False)               # a run without embeddings ...
    d = out / "v_nn_classification"
    assert not (d / "v_nn_embeddings.npz").exists() and not (d / "v_provirus_nn_embeddings.npz").exists()
    first = np.load(d / "v_nn_classification.npz")["predictions"]
    monkeypatch.setenv("GENOMAD_AMD_EMBEDDINGS", "1")
    nnc.main(fa, out, False, 128, False, 1, False, False)               # ... then asked for them: the stages run again
    pz = np.load(d / "v_provirus_nn_embeddings.npz")
    assert sorted(pz.files) == ["embeddings", "provirus_names"]
    assert list(pz["provirus_names"]) == ["k1|provirus_1_9000", "k2|provirus_5_3000"] and pz["embeddings"].shape == (2, 512)
    z = np.load(d / "v_nn_embeddings.npz")
    assert np.array_equal(np.load(d / "v_nn_classification.npz")["predictions"], first)
    emb = z["embeddings"].copy()
    # resume: only the embeddings file is missing -> the classification stage runs again and writes the same bytes
    (d / "v_nn_embeddings.npz").unlink()
    calls = []
    real = type(engine).embed_contigs
    monkeypatch.setattr(type(engine), "embed_contigs", lambda self, *a, **k: calls.append(1) or real(self, *a, **k))
    nnc.main(fa, out, False, 128, False, 1, False, False)
    assert calls and np.array_equal(np.load(d / "v_nn_embeddings.npz")["embeddings"], emb)
    assert np.array_equal(np.load(d / "v_nn_classification.npz")["predictions"], first)
    # everything there: nothing is recomputed
    monkeypatch.setattr(type(engine), "embed_contigs", lambda *a, **k: (_ for _ in ()).throw(AssertionError("recomputed")))
    nnc.main(fa, out, False, 128, False, 1, False, True)                 # --cleanup keeps the embeddings
    assert (d / "v_nn_embeddings.npz").exists() and (d / "v_provirus_nn_embeddings.npz").exists()


def test_main_range_fallback_embeddings_come_from_the_recomputation(synth_weights, tmp_path, monkeypatch):
    """the overflowing weights of test_f16_modes_overflow_is_detected_...: the default arithmetic returns non-finite scores, main()
    recomputes the piece with bf16x3, and the embeddings written are that recomputation's, finite"""
    from genomad_amd import nn_classification as nnc
    from genomad_amd import weights as W
    from genomad_amd.engine import NNEngine
    w = dict(synth_weights)
    for k, f in (("conv1_kernel", 3e4), ("conv1_bias", 3e4), ("conv2_kernel", 1 / 3e4),
                 ("iglooA_w_mult", 1 / 3e4), ("iglooA_w_v", 1 / 3e4)):
        w[k] = synth_weights[k] * np.float32(f)
    rng = np.random.default_rng(3)
    fa = tmp_path / "s.fna"
    fa.write_text("".join(f">c{i}\n{''.join(rng.choice(list('ACGT'), 9000))}\n" for i in range(3)))
    with NNEngine(0, w) as e2:
        wpath = tmp_path / "w.npz"
        W.save_npz(wpath, w)
        monkeypatch.setenv("GENOMAD_AMD_WEIGHTS", str(wpath))
        monkeypatch.setenv("GENOMAD_AMD_KMER_TABLES", "0")
        monkeypatch.setenv("GENOMAD_AMD_NO_SENTINEL", "1")
        monkeypatch.setenv("GENOMAD_AMD_EMBEDDINGS", "1")
        monkeypatch.delenv("GENOMAD_AMD_PRECISION", raising=False)
        monkeypatch.setattr(nnc, "_ENGINE", e2)
        names, seq, off = sequence.read_fasta_packed(fa)
        assert not np.isfinite(e2.embed_contigs(seq, off, False, "f16x3tc")[0]).all()
        nnc.main(fa, tmp_path / "out", False, 128, False, 1, False, False)
        z = np.load(tmp_path / "out" / "s_nn_classification" / "s_nn_embeddings.npz")
        ws, we, _ = e2.embed_contigs(seq, off, False, "bf16x3")
        wins = nnc.sentinel_windows(seq, off, False, limit=100)
        per_window = e2.embed(wins, "bf16x3")
    assert np.isfinite(z["embeddings"]).all() and np.array_equal(z["embeddings"], we)
    assert np.array_equal(np.load(tmp_path / "out" / "s_nn_classification" / "s_nn_classification.npz")["predictions"], ws)
    _, _, ids, _ = sequence.candidate_spans(off)
    want = np.stack([per_window[ids == c].astype(np.float64).mean(axis=0) for c in range(3)])
    assert np.abs(z["embeddings"] - want).max() <= 1e-6 * max(1.0, np.abs(want).max())
    assert "recomputing" in (tmp_path / "out" / "s_nn_classification.log").read_text()
