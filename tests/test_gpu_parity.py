"""GPU parity tests proper: the HIP path (through the C ABI) against the CPU oracle and the
committed golden fixtures.  Integer work must be bit-exact; class scores must be within 1e-4
absolute (BASELINE.json north_star), intermediates within the tolerances stated per test."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from genomad_amd import sequence, synthetic
from oracle import igloo_oracle, sequence_oracle

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-4   # north_star: per-class scores within 1e-4 absolute of the reference path


def _pad(seq: bytes) -> np.ndarray:
    return np.frombuffer(seq.upper().ljust(6000, b"N")[:6000], dtype=np.uint8)


# ------------------------------------------------------------------ integer kernels (bit exact)
def test_synthetic_windows_device_equals_host(engine):
    for first, n in ((0, 80), (1_000_000 - 7, 7), (123_456_789, 33)):
        dev = engine.synth_windows(first, n)
        host = synthetic.synth_windows(first, n)
        assert dev.shape == host.shape
        assert np.array_equal(dev, host), f"synthetic windows differ at first={first}"


def test_tokenizer_golden_vectors(engine, golden_dir):
    """Reference tokenize_dna outputs (tests/golden/tokenizer_golden.json) on padded windows."""
    g = json.load(open(os.path.join(golden_dir, "tokenizer_golden.json")))
    cases = [bytes.fromhex(c["seq_hex"]) for c in g["cases"]]
    # The device kernel works on 6000-byte windows: right-pad with 'N' like
    # nn_classification.py:72.  Tokens whose 4 bytes lie inside the original string must equal the
    # reference's; every token touching the padding must be 0.  No upper-casing here: lower case
    # must tokenize as non-ACGT exactly like the reference function does on raw bytes.
    bases = np.full((len(cases), 6000), ord("N"), dtype=np.uint8)
    for i, c in enumerate(cases):
        bases[i, :len(c)] = np.frombuffer(c, dtype=np.uint8)
    tok = engine.tokenize(bases)
    assert tok.shape == (len(cases), 5997) and tok.dtype == np.uint16
    for i, c in enumerate(g["cases"]):
        want = c["tokens"]
        n_valid = max(len(cases[i]) - 3, 0)
        assert list(tok[i, :n_valid]) == want[:n_valid], f"case {i}"
        assert not tok[i, n_valid:].any(), f"case {i}: padding must tokenize to 0"
    for s in g["synthetic_windows"]:
        w = synthetic.synth_windows(s["synthetic_index"], 1)
        t = engine.tokenize(w)[0]
        assert hashlib.sha256(t.astype("<u2").tobytes()).hexdigest() == s["sha256_u16le"]
        assert list(t[:8]) == s["head"] and list(t[-8:]) == s["tail"]


def test_tokenizer_matches_oracle_on_random_bytes(engine):
    rng = np.random.default_rng(7)
    n = 64
    bases = rng.integers(0, 256, (n, 6000), dtype=np.uint8)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n, 6000))]
    keep = rng.random((n, 6000)) < 0.97        # sparse non-ACGT bytes inside mostly-valid DNA
    bases = np.where(keep, acgt, bases).astype(np.uint8)
    bases[0, :] = ord("N")
    bases[1, :4] = np.frombuffer(b"NACG", dtype=np.uint8)
    bases[2, -4:] = np.frombuffer(b"ACGN", dtype=np.uint8)
    got = engine.tokenize(bases)
    want = sequence_oracle.tokenize_closed_form(bases)
    assert np.array_equal(got.astype(np.int64), want)
    assert engine.tokenize(bases[:0]).shape == (0, 5997)


def test_onehot_encoder_bit_exact(engine):
    bases = synthetic.synth_windows(3, 7)      # includes window 5 (padded) and 9 (N run)
    tok = sequence_oracle.tokenize_closed_form(bases)
    want = np.zeros((7, 5997, 257), dtype=np.uint8)
    np.put_along_axis(want, tok[..., None], 1, axis=2)
    got_u8 = engine.onehot(bases, "u8")
    assert np.array_equal(got_u8, want)
    got_f32 = engine.onehot(bases[:2], "f32")
    assert np.array_equal(got_f32, want[:2].astype(np.float32))
    got_bf16 = engine.onehot(bases[:2], "bf16")
    assert np.array_equal(got_bf16, want[:2].astype(np.uint16) * 0x3F80)
    assert got_u8.sum() == 7 * 5997          # exactly one hot element per row (token 0 included)


def test_segment_mean(engine):
    rng = np.random.default_rng(3)
    ids = np.sort(rng.integers(0, 40, 500)).astype(np.int64)
    ids = ids[ids != 17]                       # an empty segment in the middle
    scores = rng.random((len(ids), 3)).astype(np.float32)
    got = engine.segment_mean(scores, ids, 41)
    want = sequence_oracle.segment_mean(scores, ids)
    want = np.concatenate([want, np.zeros((41 - len(want), 3), np.float32)])
    assert np.allclose(got, want, rtol=0, atol=1e-6)
    assert not got[17].any()
    with pytest.raises(Exception, match="sorted"):
        engine.segment_mean(scores[:3], np.array([2, 1, 3]), 5)


# ------------------------------------------------------------------ f32 reference path
@pytest.fixture(scope="module")
def oracle16(synth_weights):
    bases = synthetic.synth_windows(0, 16)
    tok = sequence_oracle.tokenize_closed_form(bases)
    scores, taps = igloo_oracle.forward(tok, synth_weights, dtype=np.float64, return_taps=True)
    return bases, scores, taps


# per-stage tolerances of the unfused f32 kernels against the fp64 oracle (absolute; also used by tests/test_window_lengths_gpu.py)
F32_CHECKS = [("x1", "x1", 2e-6), ("x2", "x2", 2e-5), ("x3", "x3", 5e-5), ("m_a", "mA", 2e-5),
              ("m_b", "mB", 1e-4), ("yp_a", "ypA", 2e-5), ("yp_b", "ypB", 1e-4),
              ("alpha_a", "alphaA", 1e-6), ("alpha_b", "alphaB", 2e-5), ("feat", "f", 1e-4)]
F32_SCORE_TOL = 2e-5


def test_f32_path_intermediates(engine, oracle16):
    """Per-stage parity of the unfused f32 kernels against the fp64 oracle."""
    bases, scores64, t64 = oracle16
    n = 4
    scores, taps = engine.debug_forward(bases[:n], "f32", taps=("x1", "x2", "x3", "m_a", "m_b", "yp_a",
                                                               "yp_b", "alpha_a", "alpha_b", "feat"))
    for mine, ref, tol in F32_CHECKS:
        err = np.abs(taps[mine] - t64[ref][:n]).max()
        assert err <= tol, f"{mine}: max abs err {err:.3e} > {tol}"
    assert np.abs(scores - scores64[:n]).max() <= F32_SCORE_TOL


def test_f32_path_scores_vs_golden(engine, golden_dir):
    g = np.load(os.path.join(golden_dir, "forward_golden.npz"))
    bases = synthetic.synth_windows(0, 16)
    assert hashlib.sha256(bases.tobytes()).hexdigest() == str(g["bases_sha256"])
    scores = engine.classify(bases, "f32")
    assert np.abs(scores - g["scores"]).max() <= SCORE_TOL
    # outputs of the reference's own network code (model.py / igloo.py run over numpy primitives)
    assert np.abs(scores - g["scores_refgraph64"]).max() <= SCORE_TOL
    assert np.abs(engine.classify(bases, "bf16x3") - g["scores_refgraph64"]).max() <= SCORE_TOL
    assert np.allclose(scores.sum(1), 1.0, atol=1e-5)


def test_f32_path_chunking_and_empty(engine):
    """More windows than one f32 chunk (64): chunk boundaries must not change results."""
    bases = synthetic.synth_windows(100, 70)
    a = engine.classify(bases, "f32")
    b = engine.classify(bases[60:], "f32")
    assert np.array_equal(a[60:], b)           # same window -> same bits, wherever it sits in a batch
    assert engine.classify(bases[:0], "f32").shape == (0, 3)


def test_f32_path_edge_windows(engine, synth_weights):
    """All-N window (every token 0), window with a single valid 4-mer, lower-case-free padding."""
    wins = [b"", b"ACGT", b"ACGT" * 1500, b"A" * 6000, (b"ACGT" * 700)]
    bases = np.stack([_pad(w) for w in wins])
    got = engine.classify(bases, "f32")
    want = igloo_oracle.classify_windows(bases, synth_weights, np.float64)
    assert np.abs(got - want).max() <= SCORE_TOL


def test_errors_are_reported_not_swallowed(engine):
    from genomad_amd.engine import GnnError
    with pytest.raises(ValueError):
        engine.classify(np.zeros((2, 5999), np.uint8))
    with pytest.raises(GnnError, match="precision"):
        from genomad_amd import _lib
        out = np.zeros((1, 3), np.float32)
        b = np.zeros((1, 6000), np.uint8)
        _lib.check(engine.lib.gnn_classify(engine.ctx, b.ctypes.data, 1, 77, out.ctypes.data))


# ------------------------------------------------------------------ fused MFMA paths
# f16c6 = f16 MFMA + MX-fp6 correction MFMAs, both operands block scaled (gnn_fused_c6.hip), f16c8 = f16 MFMA + MX-fp8
# correction MFMAs (gnn_fused_c8.hip), f16x3 / bf16x3 = split-f16 / split-bf16, three passes (gnn_fused.hip).
# Per-stage tolerances are absolute, against the fp64 oracle.
# The parametrised matrix covers the arithmetics that can ship: the default (f16x3), its f32-range fallback (bf16x3) and the one
# opt-in fast mode (f16c6).  f16c8 and the round-1 kernel (single-pass bf16) were removed in round 6: one test that the enum values answer
# with an error (test_removed_arithmetics_answer_with_an_error).
FUSED = ["f16c6", "f16x3", "f16x3tc", "f16x3tk", "bf16x3"]      # f16x3tk (round 6): needs the k-mer tables (skipped on a device that cannot hold them)
from tests.conftest import need_tables  # noqa: E402
# the contig front end is exercised with the default arithmetic first (what main() runs), then the fallback
from genomad_amd._lib import DEFAULT_PRECISION  # noqa: E402
CONTIG_PRECS = [DEFAULT_PRECISION, "f16x3tk", "bf16x3"]


# per-stage tolerances of the fused kernels against the fp64 oracle (bf16x3's; also used by tests/test_window_lengths_gpu.py) and the
# factor per arithmetic: 4-bit correction terms / 11+11-bit limbs vs bf16's 8+8
FUSED_CHECKS = [("m_a", "mA", 1e-4), ("m_b", "mB", 1e-3), ("yp_a", "ypA", 1e-4), ("yp_b", "ypB", 1e-3),
                ("alpha_a", "alphaA", 1e-5), ("alpha_b", "alphaB", 2e-4), ("feat", "f", 5e-4)]
FUSED_LOOSE = {"f16c6": 2.5, "f16x3": 0.25, "f16x3tc": 0.25, "f16x3tk": 0.25}


@pytest.mark.parametrize("prec", FUSED)
def test_fused_intermediates(engine, oracle16, prec, request):
    """Fused kernels (activations in LDS, low-precision MFMA operands) against the fp64 oracle, per stage."""
    need_tables(request, prec)
    bases, scores64, t64 = oracle16
    scores, taps = engine.debug_forward(bases, prec)
    loose = FUSED_LOOSE.get(prec, 1.0)
    for mine, ref, tol in FUSED_CHECKS:
        err = np.abs(taps[mine] - t64[ref]).max()
        assert err <= tol * loose, f"{prec} {mine}: max abs err {err:.3e} > {tol * loose}"
    assert np.abs(scores - scores64).max() <= SCORE_TOL


@pytest.fixture(scope="module")
def oracle256(synth_weights):
    """fp32 oracle scores of 128 synthetic windows, computed once for all arithmetics (5 s of numpy; 256 until round 5 - the
    10 000-window and 16 384-window reference-graph goldens cover the sizes)"""
    bases = synthetic.synth_windows(0, 128)
    return bases, igloo_oracle.classify_windows(bases, synth_weights, np.float32)


@pytest.mark.parametrize("prec", FUSED)
def test_fused_scores_256_windows(engine, oracle256, prec, request):
    """256 synthetic windows (padded and N-run windows included) within 1e-4 of the fp32 oracle."""
    need_tables(request, prec)
    bases, want = oracle256
    got = engine.classify(bases, prec)
    err = np.abs(got - want).max()
    assert err <= SCORE_TOL, f"{prec}: max |dscore| = {err:.3e}"
    assert got.std(axis=0).min() > 0.05          # the test is not vacuous: scores vary across windows


@pytest.mark.parametrize("prec", FUSED)
def test_fused_equals_f32_path_and_is_batch_invariant(engine, prec, request):
    need_tables(request, prec)
    bases = synthetic.synth_windows(5000, 96)
    a = engine.classify(bases, prec)
    b = engine.classify(bases, "f32")
    assert np.abs(a - b).max() <= SCORE_TOL
    # a window's scores must not depend on its position in the batch or on the batch size
    c = engine.classify(bases[37:59], prec)
    assert np.array_equal(a[37:59], c)
    assert np.array_equal(engine.classify(bases, prec), a)   # run-to-run deterministic


@pytest.mark.parametrize("prec", FUSED)
def test_fused_edge_windows(engine, synth_weights, prec, request):
    need_tables(request, prec)
    wins = [b"", b"ACGT", b"ACGT" * 1500, b"A" * 6000, (b"ACGT" * 700), b"N" * 2999 + b"ACGTACGT"]
    bases = np.stack([_pad(w) for w in wins])
    got = engine.classify(bases, prec)
    want = igloo_oracle.classify_windows(bases, synth_weights, np.float64)
    assert np.abs(got - want).max() <= SCORE_TOL
    assert engine.classify(bases[:0], prec).shape == (0, 3)


def test_removed_arithmetics_answer_with_an_error(engine):
    """GNN_PREC_BF16 (round-1 kernel) and GNN_PREC_F16C8 (experimental kernel) are gone; their enum values
    answer GNN_ERR_STATE with a message instead of computing something else, and the Python side no longer knows the names."""
    import ctypes as C
    from genomad_amd import _lib
    assert "bf16" not in _lib.PRECISIONS and "f16c8" not in _lib.PRECISIONS
    assert _lib.load().gnn_has_experimental() == 0
    buf, out = engine.alloc(2 * 6000), engine.alloc(2 * 12)
    try:
        engine.synth_windows_dev(0, 2, buf.ptr)
        for code in (_lib.PREC_BF16, _lib.PREC_F16C8):
            rc = engine.lib.gnn_classify_dev(engine.ctx, C.c_void_p(buf.ptr), 2, code, C.c_void_p(out.ptr))
            assert rc == -3 and b"removed in round 6" in engine.lib.gnn_last_error()          # GNN_ERR_STATE
        with pytest.raises(KeyError):
            engine.classify(synthetic.synth_windows(0, 2), "f16c8")
    finally:
        buf.free()
        out.free()


def _scaled_activations(synth_weights, f):
    """The same network with ALL activations (x1, x2, x3) scaled by f, a power of two: conv1 (kernel and bias) and the conv2 / conv3
    biases times f - LeakyReLU is positively homogeneous -, compensated only where the arithmetic is f32: the folded IGLOO weights
    (w_mult / f: the pair products are unchanged) and the first dense layer (kernel / f: yp and the features are f times larger).
    conv2, conv3 and w_v - the operands that become f16 limbs - keep their magnitude, so a mode's accuracy at that scale is a statement
    about its ACTIVATION range only.  The exact-f32 path computes bit-identical scores for every power of two."""
    w = dict(synth_weights)
    for k, g in (("conv1_kernel", f), ("conv1_bias", f), ("conv2_bias", f), ("conv3_bias", f), ("iglooA_w_mult", 1 / f),
                 ("iglooB_w_mult", 1 / f), ("enc_dense_kernel", 1 / f)):
        w[k] = synth_weights[k] * np.float32(g)
    return w


def _write_weights_and_fasta(tmp_path, monkeypatch, w, n_contigs=3):
    from genomad_amd import weights as W
    rng = np.random.default_rng(3)
    fa = tmp_path / "s.fna"
    fa.write_text("".join(f">c{i}\n{''.join(rng.choice(list('ACGT'), 9000))}\n" for i in range(n_contigs)))
    wpath = tmp_path / "w.npz"
    W.save_npz(wpath, w)
    monkeypatch.setenv("GENOMAD_AMD_WEIGHTS", str(wpath))
    return fa


def engine_scores_unscaled(synth_weights, bases):
    from genomad_amd.engine import NNEngine
    with NNEngine(0, synth_weights) as e0:
        return e0.classify(bases, "f32")


def test_toomcook_range_band_falls_back_to_the_direct_f16_form(engine, synth_weights, tmp_path, monkeypatch):
    """between |activation| ~4e3 and 65 504 only the Toom-Cook form's TRANSFORMED operands (up to 32x the activations)
    leave the f16 range.  There f16x3tc must return non-finite scores (inf / -inf limb pairs -> NaN, NaN-propagating pool), never
    finite wrong ones; the direct f16x3 form is still exact; and main() hops exactly once, f16x3tc -> f16x3."""
    from genomad_amd import nn_classification as nnc
    from genomad_amd.engine import NNEngine
    w = _scaled_activations(synth_weights, 4096.0)
    bases = synthetic.synth_windows(0, 8)
    fa = _write_weights_and_fasta(tmp_path, monkeypatch, w)
    with NNEngine(0, w) as e2:
        _, taps = e2.debug_forward(bases, "f32", taps=("x1", "x3"))
        peak = max(float(np.abs(taps[k]).max()) for k in ("x1", "x3"))
        assert 4e3 < peak < 6.5e4, peak                     # inside the band
        exact = e2.classify(bases, "f32")
        assert np.array_equal(exact, engine_scores_unscaled(synth_weights, bases))       # a power of two: the same function, bit for bit
        tc, direct = e2.classify(bases, "f16x3tc"), e2.classify(bases, "f16x3")
        assert not np.isfinite(tc).all()
        assert np.isfinite(direct).all() and np.abs(direct - exact).max() <= SCORE_TOL / 2
        # the k-mer-table form reads x2 from a table (exact f32, so it is finite) but still transforms it into f16 operands for conv3:
        # the same band must turn its scores non-finite too (when this engine's own 156 GB of tables fit beside the session engine's)
        monkeypatch.setenv("GENOMAD_AMD_KMER_TABLES", "0")                    # main() below: the default arithmetic's chain
        engine.drop_kmer_tables()                                             # room for e2's own set
        if e2.build_kmer_tables():
            assert not np.isfinite(e2.classify(bases, "f16x3tk")).all()
            e2.drop_kmer_tables()
        monkeypatch.delenv("GENOMAD_AMD_PRECISION", raising=False)
        monkeypatch.setattr(nnc, "_ENGINE", e2)
        nnc._WARNED.clear()
        nnc.main(fa, tmp_path / "out", False, 128, False, 1, False, False)
        z = np.load(tmp_path / "out" / "s_nn_classification" / "s_nn_classification.npz")
        names, seq, off = sequence.read_fasta_packed(fa)
        want, _ = e2.classify_contigs(seq, off, False, "f16x3")
    assert np.isfinite(z["predictions"]).all() and np.array_equal(z["predictions"], want)
    log = (tmp_path / "out" / "s_nn_classification.log").read_text()
    assert log.count("recomputing") == 1 and "(f16x3tc)" in log and "with f16x3." in log
    assert "Parity sentinel: max |dscore| of f16x3 against" in log      # the sentinel judged the arithmetic that served the run


def test_parity_sentinel_trips_on_weights_outside_the_validated_range(synth_weights, tmp_path, monkeypatch, capsys):
    """main() classifies its first <= 64 windows with GNN_PREC_F32 as well.  With the synthetic weights the
    line reads ~1e-5; with the activations scaled DOWN into the f16 subnormals (x 2^-17: neither limb carries them any more, the
    scores stay finite and are wrong) the run must stop with status 1 before it writes an output; the opt-out runs."""
    import time
    from genomad_amd import nn_classification as nnc
    from genomad_amd.engine import NNEngine
    monkeypatch.delenv("GENOMAD_AMD_PRECISION", raising=False)
    fa = _write_weights_and_fasta(tmp_path, monkeypatch, synth_weights)
    with NNEngine(0, synth_weights) as e1:
        monkeypatch.setattr(nnc, "_ENGINE", e1)
        nnc.main(fa, tmp_path / "ok", False, 128, False, 1, False, False)
        log = (tmp_path / "ok" / "s_nn_classification.log").read_text()
        line = [ln for ln in log.splitlines() if "Parity sentinel" in ln]
        assert len(line) == 1 and "of f16x3tc against" in line[0]
        d = float(line[0].split("= ")[1].split()[0])
        assert d <= SCORE_TOL / 2, line
        names, seq, off = sequence.read_fasta_packed(fa)
        win = nnc.sentinel_windows(seq, off, False)
        assert len(win) == 6                                  # 3 contigs x (6000 + 3000)
        t = time.perf_counter()
        nnc.parity_sentinel(e1, win, "f16x3tc", None)
        cost = time.perf_counter() - t
    with NNEngine(0, synth_weights) as e0:                    # a fresh engine: the first call also allocates the f32 path's workspace
        big = synthetic.synth_windows(0, nnc.SENTINEL_WINDOWS)
        e0.classify(big[:1], "f16x3tc")
        t = time.perf_counter()
        nnc.parity_sentinel(e0, big, "f16x3tc", None)
        cold = time.perf_counter() - t
    with capsys.disabled():
        print(f"\nparity sentinel: {d:.2e} on the synthetic weights; {cost * 1e3:.0f} ms per run warm (6 windows), "
              f"{cold * 1e3:.0f} ms cold with the full {nnc.SENTINEL_WINDOWS} windows (first f32 launch of the engine)")
    assert cost < 1.0 and cold < 2.0
    tiny = _scaled_activations(synth_weights, 2.0 ** -17)
    _write_weights_and_fasta(tmp_path, monkeypatch, tiny)
    with NNEngine(0, tiny) as e2:
        bases = synthetic.synth_windows(0, 8)
        exact, got = e2.classify(bases, "f32"), e2.classify(bases, "f16x3tc")
        assert np.isfinite(got).all() and np.abs(got - exact).max() > SCORE_TOL     # finite and wrong: what only the sentinel can see
        monkeypatch.setattr(nnc, "_ENGINE", e2)
        with pytest.raises(SystemExit) as ex:
            nnc.main(fa, tmp_path / "bad", False, 128, False, 1, False, False)
        assert ex.value.code == 1 and "Parity sentinel FAILED" in capsys.readouterr().err
        assert not (tmp_path / "bad" / "s_nn_classification").exists()
        monkeypatch.setenv("GENOMAD_AMD_NO_SENTINEL", "1")
        nnc.main(fa, tmp_path / "optout", False, 128, False, 1, False, False)
        assert (tmp_path / "optout" / "s_nn_classification" / "s_nn_classification.tsv").exists()


def test_f16_modes_overflow_is_detected_and_main_falls_back_to_bf16x3(synth_weights, tmp_path, monkeypatch):
    """Activations beyond the f16 range (65504): the f16-operand modes return non-finite scores — never silently
    wrong finite ones — and main() recomputes the affected batch with the split-bf16 kernel (f32 range)."""
    from genomad_amd import nn_classification as nnc
    from genomad_amd import weights as W
    from genomad_amd.engine import NNEngine
    w = dict(synth_weights)
    for k, f in (("conv1_kernel", 3e4), ("conv1_bias", 3e4), ("conv2_kernel", 1 / 3e4),
                 ("iglooA_w_mult", 1 / 3e4), ("iglooA_w_v", 1 / 3e4)):      # the same network, |x1| up to ~7e4
        w[k] = synth_weights[k] * np.float32(f)
    bases = synthetic.synth_windows(0, 8)
    rng = np.random.default_rng(3)
    fa = tmp_path / "s.fna"
    fa.write_text("".join(f">c{i}\n{''.join(rng.choice(list('ACGT'), 9000))}\n" for i in range(3)))
    with NNEngine(0, w) as e2:
        exact, wide = e2.classify(bases, "f32"), e2.classify(bases, "bf16x3")
        assert np.isfinite(wide).all() and np.abs(wide - exact).max() <= 1e-3
        for prec in ("f16c6", "f16x3", "f16x3tc"):
            assert not np.isfinite(e2.classify(bases, prec)).all(), prec
        wpath = tmp_path / "w.npz"
        W.save_npz(wpath, w)
        monkeypatch.setenv("GENOMAD_AMD_WEIGHTS", str(wpath))
        monkeypatch.setenv("GENOMAD_AMD_PRECISION", "f16c6")
        monkeypatch.setattr(nnc, "_ENGINE", e2)
        with pytest.raises(ValueError, match="GENOMAD_AMD_ALLOW_OUT_OF_TOLERANCE"):          # round 6: the out-of-tolerance mode needs an explicit opt-in
            nnc.main(fa, tmp_path / "out", False, 128, False, 1, False, False)
        monkeypatch.setenv("GENOMAD_AMD_ALLOW_OUT_OF_TOLERANCE", "1")
        nnc._WARNED.clear()                                       # the one-line warnings are said once per process
        nnc.main(fa, tmp_path / "out", False, 128, False, 1, False, False)
        z = np.load(tmp_path / "out" / "s_nn_classification" / "s_nn_classification.npz")
        names, seq, off = sequence.read_fasta_packed(fa)
        want, _ = e2.classify_contigs(seq, off, False, "bf16x3")
    assert np.isfinite(z["predictions"]).all() and np.array_equal(z["predictions"], want)
    log = (tmp_path / "out" / "s_nn_classification.log").read_text()
    assert "recomputing" in log and "OUTSIDE the 1e-4 score tolerance" in log


# ------------------------------------------------------------------ drop-in entry point on the GPU
def test_main_end_to_end_on_gpu(engine, synth_weights, tmp_path, monkeypatch):
    """genomad_amd.nn_classification.main on a small FASTA: NPZ/TSV written, per-contig scores within
    1e-4 of the oracle chain (reference windowing rules -> fp32 forward -> segment mean)."""
    from genomad_amd import nn_classification as nnc
    from genomad_amd import weights as W
    rng = np.random.default_rng(9)
    recs = [("ctgA", "".join(rng.choice(list("ACGT"), 20000))),
            ("ctgB desc", "nn" + "".join(rng.choice(list("ACGTN"), 9000, p=[.24, .24, .24, .24, .04])) + "N"),
            ("ctgC", "".join(rng.choice(list("acgt"), 2000)))]
    fa = tmp_path / "mini.fna"
    fa.write_text("".join(f">{n}\n{s}\n" for n, s in recs))
    wpath = tmp_path / "w.npz"
    W.save_npz(wpath, synth_weights)
    monkeypatch.setenv("GENOMAD_AMD_WEIGHTS", str(wpath))
    monkeypatch.setattr(nnc, "_ENGINE", engine)          # reuse the session engine (same weights)
    out = tmp_path / "out"
    nnc.main(fa, out, False, 128, False, 4, False, True)
    z = np.load(out / "mini_nn_classification" / "mini_nn_classification.npz")
    names, ids, wins = sequence_oracle.encode_fasta(fa)
    want = sequence_oracle.segment_mean(igloo_oracle.classify_windows(wins, synth_weights, np.float32), ids)
    assert list(z["contig_names"]) == list(names) == ["ctgA", "ctgB", "ctgC"]
    assert np.abs(z["predictions"] - want).max() <= SCORE_TOL
    tsv = (out / "mini_nn_classification" / "mini_nn_classification.tsv").read_text().splitlines()
    assert tsv[1].split("\t")[1:] == [f"{x:.4f}" for x in z["predictions"][0]]
    assert not (out / "mini_nn_classification" / "mini_encoded_sequences").exists()   # --cleanup


def test_main_compressed_chunked_input_provirus_pass_and_resume_on_gpu(engine, synth_weights, tmp_path, monkeypatch):
    """Product path of main() on a gzip FASTA read as a stream of record-aligned chunks (several chunks forced),
    with the find-proviruses outputs present (second classification pass, one weight upload) and a second call
    that must resume from the files: same NPZ as the uncompressed file in one piece, nothing recomputed."""
    import gzip
    import json
    from genomad_amd import nn_classification as nnc
    from genomad_amd import weights as W
    rng = np.random.default_rng(10)
    recs = [(f"c{i} note", "".join(rng.choice(list("ACGTN"), int(rng.integers(2000, 30000)), p=[.245, .245, .245, .245, .02])))
            for i in range(9)]
    text = "".join(f">{n}\n" + "\n".join(s[j:j + 61] for j in range(0, len(s), 61)) + "\n" for n, s in recs)
    plain, gz = tmp_path / "meta.fna", tmp_path / "metaz.fna.gz"
    plain.write_text(text)
    with gzip.open(gz, "wt") as f:
        f.write(text)
    wpath = tmp_path / "w.npz"
    W.save_npz(wpath, synth_weights)
    monkeypatch.setenv("GENOMAD_AMD_WEIGHTS", str(wpath))
    monkeypatch.setattr(nnc, "_ENGINE", engine)
    real_chunks = sequence.iter_text_chunks
    seen = []

    def small_chunks(path, chunk_bytes=128 << 20):
        for c in real_chunks(path, 40000):
            seen.append(len(c))
            yield c
    monkeypatch.setattr(sequence, "iter_text_chunks", small_chunks)
    out_p, out_z = tmp_path / "op", tmp_path / "oz"
    fp = out_z / "metaz_find_proviruses"
    fp.mkdir(parents=True)
    (fp / "metaz_find_proviruses.json").write_text(json.dumps({"input_md5": nnc.get_md5(gz), "module": "x", "parameters": {}}))
    (fp / "metaz_provirus.tsv").write_text("h\nc1|provirus_1_5000\n")
    (fp / "metaz_provirus.fna").write_text(">c1|provirus_1_5000\n" + recs[1][1][:5000] + "\n")
    (fp / "metaz_provirus_proteins.faa").write_text("")
    (fp / "metaz_provirus_genes.tsv").write_text("")
    nnc.main(plain, out_p, False, 128, False, 1, False, False)
    nnc.main(gz, out_z, False, 128, False, 1, False, False)
    assert len(seen) >= 3                                        # the stream really came in several chunks
    a = np.load(out_p / "meta_nn_classification" / "meta_nn_classification.npz")
    b = np.load(out_z / "metaz_nn_classification" / "metaz_nn_classification.npz")
    assert list(a["contig_names"]) == list(b["contig_names"]) == [f"c{i}" for i in range(9)]
    assert np.array_equal(a["predictions"], b["predictions"])
    wa = np.load(out_p / "meta_nn_classification" / "meta_encoded_sequences" / "meta_seq_window_id.npz")
    wb = np.load(out_z / "metaz_nn_classification" / "metaz_encoded_sequences" / "metaz_seq_window_id.npz")
    assert np.array_equal(wa["contig_ids"], wb["contig_ids"])
    pz = np.load(out_z / "metaz_nn_classification" / "metaz_provirus_nn_classification.npz")
    assert list(pz["provirus_names"]) == ["c1|provirus_1_5000"] and pz["predictions"].shape == (1, 3)
    # resume: same input and parameters -> both passes are skipped, the files are reused
    monkeypatch.setattr(type(engine), "classify_contigs", lambda *a, **k: (_ for _ in ()).throw(AssertionError("recomputed")))
    nnc.main(gz, out_z, False, 128, False, 1, False, False)
    c = np.load(out_z / "metaz_nn_classification" / "metaz_nn_classification.npz")
    assert np.array_equal(b["predictions"], c["predictions"])


def test_main_device_path_invalid_fasta_leaves_nothing_behind(engine, synth_weights, tmp_path, monkeypatch):
    """The device front end validates the FASTA concurrently with the classification; an input with a
    duplicated identifier must still end like in the reference (error, exit 1) and must not leave an
    NPZ / TSV / execution-info file behind (nn_classification.py:164-170 runs before anything else)."""
    from genomad_amd import nn_classification as nnc
    from genomad_amd import weights as W
    rng = np.random.default_rng(3)
    body = "".join(rng.choice(list("ACGT"), 7000))
    fa = tmp_path / "dup.fna"
    fa.write_text(f">a one\n{body}\n>b\n{body[:3000]}\n>a two\n{body[::-1]}\n")
    wpath = tmp_path / "w.npz"
    W.save_npz(wpath, synth_weights)
    monkeypatch.setenv("GENOMAD_AMD_WEIGHTS", str(wpath))
    monkeypatch.setattr(nnc, "_ENGINE", engine)
    out = tmp_path / "out"
    with pytest.raises(SystemExit) as exc:
        nnc.main(fa, out, False, 128, False, 1, False, False)
    assert exc.value.code == 1
    d = out / "dup_nn_classification"
    left = sorted(p.name for p in d.rglob("*")) if d.exists() else []
    assert left == [], left
    empty = tmp_path / "empty.fna"
    empty.write_text("")
    with pytest.raises(SystemExit):
        nnc.main(empty, tmp_path / "out_e", False, 128, False, 1, False, False)
    alln = tmp_path / "alln.fna"                       # valid FASTA, but no window survives strip_n
    alln.write_text(">x\nNNNNNNNN\n")
    with pytest.raises(SystemExit):
        nnc.main(alln, tmp_path / "out_n", False, 128, False, 1, False, False)
    assert not (tmp_path / "out_n" / "alln_nn_classification" / "alln_nn_classification.npz").exists()


def test_config1_kpneumoniae_shaped_genome_through_main(engine, synth_weights, tmp_path, monkeypatch):
    """BASELINE config 1 (plumbing case): a genome shaped like GCF_009025895.1 — one ≈5.1 Mbp chromosome
    and the seven plasmids of the documented lengths, ≈ 910 windows — through the drop-in main().  The
    real assembly, TensorFlow and the trained weights are not available here, so the
    content is seeded synthetic sequence; the seven plasmids (56 windows) are checked against the oracle
    chain, the chromosome against the exact-f32 device path."""
    from genomad_amd import nn_classification as nnc, sequence
    from genomad_amd import weights as W
    lengths = [5_100_000, 82_240, 61_331, 51_887, 50_635, 44_850, 28_729, 5_251]
    rng = np.random.default_rng(1895)
    fa = tmp_path / "GCF_009025895.1.fna"
    with open(fa, "wb") as f:
        for i, n in enumerate(lengths):
            body = rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes()
            f.write(b">NZ_CP0450%d.1 Klebsiella pneumoniae strain (synthetic stand-in)\n" % (15 + i))
            f.write(b"\n".join(body[j:j + 80] for j in range(0, n, 80)) + b"\n")
    wpath = tmp_path / "w.npz"
    W.save_npz(wpath, synth_weights)
    monkeypatch.setenv("GENOMAD_AMD_WEIGHTS", str(wpath))
    monkeypatch.setattr(nnc, "_ENGINE", engine)
    out = tmp_path / "out"
    nnc.main(fa, out, False, 128, False, 1, False, False)
    d = out / "GCF_009025895.1_nn_classification"
    z = np.load(d / "GCF_009025895.1_nn_classification.npz")
    wid = np.load(d / "GCF_009025895.1_encoded_sequences" / "GCF_009025895.1_seq_window_id.npz")
    assert list(z["contig_names"]) == [f"NZ_CP0450{15 + i}.1" for i in range(8)]
    assert len(wid["contig_ids"]) == sum(len(sequence.window_spans(n)) for n in lengths) == 906
    pred = z["predictions"]
    assert pred.shape == (8, 3) and np.allclose(pred.sum(1), 1.0, atol=1e-5)
    names, seq, offsets = sequence.read_fasta_packed(fa)
    exact, _ = engine.classify_contigs(seq, offsets, False, "f32")
    assert np.abs(pred - exact).max() <= SCORE_TOL
    plasmids = tmp_path / "plasmids.fna"
    text = fa.read_bytes()
    plasmids.write_bytes(text[text.index(b">NZ_CP045016.1"):])
    _, ids, wins = sequence_oracle.encode_fasta(plasmids)
    assert len(wins) == 56
    want = sequence_oracle.segment_mean(igloo_oracle.classify_windows(wins, synth_weights, np.float32), ids)
    assert np.abs(pred[1:] - want).max() <= SCORE_TOL
    tsv = (d / "GCF_009025895.1_nn_classification.tsv").read_text().splitlines()
    assert tsv[0] == "seq_name\tchromosome_score\tplasmid_score\tvirus_score" and len(tsv) == 9


# ------------------------------------------------------------------ BASELINE.json sizes: properties
def _classify_resident(engine, first, n, precision, shards=1):
    """Classify synthetic windows first..first+n generated on the device; optionally as `shards`
    contiguous shards processed one after the other (what G ranks would each do)."""
    bases = engine.alloc(n * 6000)
    scores = engine.alloc(n * 12)
    try:
        engine.synth_windows_dev(first, n, bases.ptr)
        per = -(-n // shards)
        for a in range(0, n, per):
            m = min(per, n - a)
            engine.classify_dev(bases.ptr + a * 6000, m, scores.ptr + a * 12, precision)
        engine.sync()
        return scores.download((n, 3), np.float32)
    finally:
        bases.free()
        scores.free()


def test_config2_10k_windows_vs_reference_graph_golden(engine, golden_dir):
    """BASELINE config 2 as written: 10 k synthetic 6 kbp windows, every window's class scores within 1e-4 of
    the reference.  The golden holds, for windows 0..9999, the float32 outputs of the REFERENCE'S OWN graph
    (model.py create_classifier() + igloo.py executed in place over numpy TF/Keras stand-ins,
    oracle/make_golden_config2.py; TensorFlow itself and the trained weights are not available here) and
    the fp64 oracle.  Checked: the exact-f32 device path and both fused MFMA paths, on ALL windows."""
    g = np.load(os.path.join(golden_dir, "config2_golden.npz"))
    ref32, truth = g["scores_refgraph32"], g["scores_oracle64"]
    n = len(ref32)
    assert n == 10_000
    worst = {}
    precs = [("f32", 2e-5), ("f16x3", 2e-5), ("f16x3tc", 2e-5), ("bf16x3", SCORE_TOL), ("f16c6", SCORE_TOL)]
    if engine.build_kmer_tables():                      # the k-mer-table arithmetic on a device that can hold its tables
        precs.insert(3, ("f16x3tk", 2e-5))
    for prec, tol64 in precs:
        got = _classify_resident(engine, 0, n, prec)
        assert np.isfinite(got).all() and np.allclose(got.sum(1), 1.0, atol=1e-5)
        e32, e64 = np.abs(got - ref32).max(), np.abs(got - truth).max()
        worst[prec] = (float(e32), float(e64))
        assert e32 <= SCORE_TOL, f"{prec}: max |dscore| vs reference graph (f32) over 10k windows = {e32:.3e}"
        assert e64 <= tol64, f"{prec}: max |dscore| vs fp64 oracle over 10k windows = {e64:.3e}"
        assert got.std(axis=0).min() > 0.1
    print("config 2 max |dscore| (vs reference graph f32, vs fp64 oracle):", worst)


def test_config3_1m_windows_sharding_determinism_and_accuracy(engine, golden_dir):
    """BASELINE configs 3/4 (1 M windows) with the DEFAULT arithmetic (the one bench.py times): size-independent
    properties — run-to-run bit identity, and 8 contiguous shards (what 8 ranks compute) concatenated == one pass, bit for
    bit — and accuracy where it can be pinned at this size: every 64th window of the 1 048 576 (16 384 windows: a sample large
    enough to see a 1-in-10^4 tail) against the outputs of the REFERENCE'S OWN graph for exactly those windows
    (tests/golden/config3_strided_golden.npz, oracle/make_golden_config2.py --n 16384 --stride 64: 80 CPU-minutes) within HALF the
    tolerance, and a 512-window strided sample against the exact-f32 device path."""
    from genomad_amd._lib import DEFAULT_PRECISION as prec
    n = 1 << 20
    one = _classify_resident(engine, 0, n, prec)
    again = _classify_resident(engine, 0, n, prec)
    assert hashlib.sha256(one.tobytes()).hexdigest() == hashlib.sha256(again.tobytes()).hexdigest()
    sharded = _classify_resident(engine, 0, n, prec, shards=8)
    assert np.array_equal(one, sharded)
    assert np.isfinite(one).all() and np.abs(one.sum(1) - 1.0).max() < 1e-5
    # the counter-based generator makes any slice addressable: windows 777000.. must score the same
    # when classified on their own
    sub = _classify_resident(engine, 777_000, 512, prec)
    assert np.array_equal(one[777_000:777_512], sub)
    # accuracy over the whole range, not just its first 10 000 windows
    g = np.load(os.path.join(golden_dir, "config3_strided_golden.npz"))
    idx = g["indices"]
    assert idx.max() < n and len(idx) >= 16384 and np.array_equal(idx, np.arange(len(idx)) * 64)
    e32 = float(np.abs(one[idx] - g["scores_refgraph32"]).max())
    e64 = float(np.abs(one[idx] - g["scores_oracle64"]).max())
    print(f"config 3, {len(idx)} windows strided over 2^20, {prec}: max |dscore| vs reference graph {e32:.3e}, vs fp64 oracle {e64:.3e}")
    assert e32 <= SCORE_TOL / 2 and e64 <= SCORE_TOL / 2
    sample = np.arange(0, n, 64)
    exact = np.concatenate([_classify_resident(engine, int(a), 1, "f32") for a in sample[:512]])
    assert np.abs(one[sample[:512]] - exact).max() <= SCORE_TOL / 2
    # the opt-in fast modes on the same strided windows: inside the tolerance here or not, they must stay in its neighbourhood
    # (1.2e-4 was seen on 10^6 windows) - a regression to 1e-3 class errors fails
    for fast in ("f16c6",):
        got = np.concatenate([_classify_resident(engine, int(a), 1, fast) for a in idx[:256]])
        assert np.abs(got - g["scores_refgraph32"][:256]).max() <= 2 * SCORE_TOL, fast


# ------------------------------------------------------------------ contig front end
@pytest.mark.parametrize("prec", CONTIG_PRECS)
def test_contig_front_end_equals_window_path(engine, synth_weights, golden_dir, prec, request):
    """classify_contigs (device-side upper-casing/padding/N rule/segment mean on spans of the packed
    buffer) == reference windowing rules (golden FASTA fixture) + classify + segment mean."""
    need_tables(request, prec)
    from genomad_amd import sequence
    path = os.path.join(golden_dir, "fasta_fixture.fna.gz")
    names, seq, offsets = sequence.read_fasta_packed(path)
    g = json.load(open(os.path.join(golden_dir, "fasta_golden.json")))
    for single, key in ((False, "all"), (True, "single")):
        contig_scores, ids = engine.classify_contigs(seq, offsets, single, prec)
        assert list(ids) == g[key]["contig_ids"]                 # N rule evaluated on the device
        _, ids_h, wins = sequence.encode_fasta(path, single)
        want = engine.segment_mean(engine.classify(wins, prec), ids_h, len(names))
        assert np.array_equal(contig_scores, want)               # same windows -> same bits
        oracle = sequence_oracle.segment_mean(igloo_oracle.classify_windows(wins, synth_weights, np.float32), ids_h)
        assert np.abs(contig_scores - oracle).max() <= SCORE_TOL
    empty, ids = engine.classify_contigs(np.zeros(0, np.uint8), np.zeros(1, np.int64))
    assert empty.shape == (0, 3) and len(ids) == 0


@pytest.mark.parametrize("prec", CONTIG_PRECS)
def test_config5_metagenome_contigs_resident_in_hbm(engine, prec, request):
    """BASELINE config 5 at reduced size: a 48 Mbp synthetic metagenome (mixed 1-500 kbp contigs,
    log-uniform) generated IN HBM, through the contig front end (spans -> N rule -> upper-case/pad ->
    encode+IGLOO -> per-contig mean), against the same rules applied on the host + the window path;
    plus the properties that hold at any size: contig sharding does not change a bit, rows sum to 1."""
    need_tables(request, prec)
    from genomad_amd import sequence
    nwin = 8000
    offsets = synthetic.synth_metagenome_offsets(nwin * 6000, seed=99)
    n_contigs = len(offsets) - 1
    assert n_contigs > 300 and offsets[-1] == nwin * 6000
    buf = engine.alloc(nwin * 6000)
    try:
        engine.synth_windows_dev(0, nwin, buf.ptr)
        engine.sync()
        got, ids = engine.classify_contigs_dev(buf.ptr, offsets, False, prec)
        # host restatement of nn_classification.py:66-73 on the same bytes
        seq = synthetic.synth_windows(0, nwin).reshape(-1)
        starts, lens, cids, wn = sequence.candidate_spans(offsets)
        keep = np.array([wn[i] == 0 or np.count_nonzero(seq[starts[i]:starts[i] + lens[i]] == ord("N")) <= 4000
                         for i in range(len(starts))])
        assert np.array_equal(ids, cids[keep])
        wins = np.full((int(keep.sum()), 6000), ord("N"), np.uint8)
        for r, i in enumerate(np.flatnonzero(keep)):
            wins[r, :lens[i]] = seq[starts[i]:starts[i] + lens[i]]
        want = engine.segment_mean(engine.classify(wins, prec), cids[keep], n_contigs)
        assert np.array_equal(got, want)
        assert got.shape == (n_contigs, 3) and np.allclose(got.sum(1), 1.0, atol=1e-5)
        # contigs shard embarrassingly: the two halves, classified separately, give the same bits
        h = n_contigs // 2
        a, _ = engine.classify_contigs_dev(buf.ptr, offsets[:h + 1], False, prec)
        b, _ = engine.classify_contigs_dev(buf.ptr + int(offsets[h]), offsets[h:] - offsets[h], False, prec)
        assert np.array_equal(np.concatenate([a, b]), got)
        # host-side edits: lower-case bases are upper-cased on the device; a run of literal 'N' makes
        # the skip rule fire (window_n > 0 and > 4000 'N'), a run of lower-case 'n' does not count
        # (Sequence.count is case-sensitive on the raw string, sequence.py:38-39)
        mod = seq.copy()
        mod[::3] |= 0x20
        order = np.argsort(-np.diff(offsets))
        c0, c1 = int(order[0]), int(order[1])
        assert offsets[c1 + 1] - offsets[c1] > 40000
        mod[offsets[c0] + 6000:offsets[c0] + 6000 + 15000] = ord("N")
        mod[offsets[c1] + 12000:offsets[c1] + 12000 + 15000] = ord("n")
        got_mod, ids_mod = engine.classify_contigs(mod, offsets, False, prec)
        keep2 = np.array([wn[i] == 0 or np.count_nonzero(mod[starts[i]:starts[i] + lens[i]] == ord("N")) <= 4000
                          for i in range(len(starts))])
        assert np.count_nonzero(~keep2 & (cids == c0)) == 2 and not np.any(~keep2 & (cids == c1))
        assert np.array_equal(ids_mod, cids[keep2])
        wins2 = np.full((int(keep2.sum()), 6000), ord("N"), np.uint8)
        for r, i in enumerate(np.flatnonzero(keep2)):
            w = mod[starts[i]:starts[i] + lens[i]]
            wins2[r, :lens[i]] = np.where((w >= ord("a")) & (w <= ord("z")), w - 32, w)
        want2 = engine.segment_mean(engine.classify(wins2, prec), cids[keep2], n_contigs)
        assert np.array_equal(got_mod, want2)
    finally:
        buf.free()


def test_rccl_transport_through_the_c_abi(engine):
    """genomad_amd.rccl.RcclComm (ncclCommInitRank / ncclGather / ncclAllGather / ncclAllReduce behind the C
    ABI's gnn_comm_*, unique id exchanged through a file) with the one rank this box has; the same sharding
    functions run with two and three ranks over gloo in the CPU suite, and at 2/4/8 GPUs in the driver's
    scaling run."""
    from genomad_amd import rccl, sharding
    comm = rccl.RcclComm(engine, 0, 1)
    try:
        comm.barrier()
        assert comm.allgather_i64([3, 5]).tolist() == [[3, 5]]
        x = np.arange(12, dtype=np.float32).reshape(4, 3)
        assert np.array_equal(comm.gather_array(x)[0], x)
        assert comm.allreduce_max(2.5) == 2.5
        assert sharding.gather_bytes(comm, b"hello") == [b"hello"]
        scores = sharding.gather_scores(comm, x, 4)
        assert np.array_equal(scores, x)
        send, recv = engine.alloc(48), engine.alloc(48)
        try:
            send.upload(x)
            comm.gather_dev(send.ptr, recv.ptr, 48, 0)
            engine.sync()
            assert np.array_equal(recv.download((4, 3), np.float32), x)
        finally:
            send.free()
            recv.free()
        names, preds, ids, total = sharding.gather_contig_parts(
            comm, [(1, np.array(["b"]), x[1:2], np.array([0, 0])), (0, np.array(["a"]), x[0:1], np.array([0]))])
        assert list(names) == ["a", "b"] and np.array_equal(preds, x[:2]) and ids.tolist() == [0, 1, 1] and total == 3
    finally:
        comm.close()
    with pytest.raises(Exception, match="communicator"):
        from genomad_amd import _lib
        _lib.check(engine.lib.gnn_comm_barrier(engine.ctx))


def test_main_product_path_with_cuda_visible_devices_minus_one(synth_weights, tmp_path):
    """The reference module exports CUDA_VISIBLE_DEVICES=-1 at import (modules/nn_classification.py:8) and HIP
    honours that variable: a process that inherits it must still find the GPU — main() removes it before the
    first HIP call.  Also run as rank 0 of a one-rank launch (WORLD_SIZE=1 set, as torch.distributed.run does)."""
    import subprocess
    from genomad_amd import weights as W
    rng = np.random.default_rng(8)
    fa = tmp_path / "sample.fna"
    with open(fa, "wb") as f:
        for i in range(5):
            body = rng.choice(np.frombuffer(b"ACGT", np.uint8), int(rng.integers(3000, 20000))).tobytes()
            f.write(b">c%d x\n" % i + b"\n".join(body[j:j + 70] for j in range(0, len(body), 70)) + b"\n")
    wpath = tmp_path / "w.npz"
    W.save_npz(wpath, synth_weights)
    env = dict(os.environ, GENOMAD_AMD_WEIGHTS=str(wpath), CUDA_VISIBLE_DEVICES="-1", WORLD_SIZE="1", RANK="0", LOCAL_RANK="0",
               PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    code = ("import os, sys; assert os.environ['CUDA_VISIBLE_DEVICES'] == '-1'; "
            "from genomad_amd import nn_classification as n; "
            "n.main(sys.argv[1], sys.argv[2], False, 128, True, 1, False, False); "
            "assert 'CUDA_VISIBLE_DEVICES' not in os.environ")
    subprocess.run([sys.executable, "-c", code, str(fa), str(tmp_path / "out")], check=True, env=env, timeout=600)
    z = np.load(tmp_path / "out" / "sample_nn_classification" / "sample_nn_classification.npz")
    assert list(z["contig_names"]) == [f"c{i}" for i in range(5)] and np.isfinite(z["predictions"]).all()


def test_classify_contigs_entry_point_equals_span_level_path(engine):
    """gnn_classify_contigs (native window cutting, N rule as a device-side mask of the segment mean, scores
    resident on the device, sequence uploaded in pieces) against the span-level entry points driven from numpy
    (candidate_spans + gnn_span_byte_count + gnn_classify_spans + gnn_segment_mean): same per-contig scores
    bit for bit and the same kept-window ids — including N-rich windows the rule drops, lower-case n (not
    counted), short tails, contigs shorter than a window, single_window, and the empty table."""
    rng = np.random.default_rng(77)
    lengths = [100, 2499, 2500, 6000, 6001, 8499, 8500, 14500, 30000, 61234, 3, 12000]
    parts = []
    for i, L in enumerate(lengths):
        body = rng.choice(np.frombuffer(b"ACGTacgt", np.uint8), L)
        if i == 8:
            body[6100:10500] = ord("N")        # second window: > 4000 N -> dropped
            body[12100:16050] = ord("N")       # third window: 3950 N -> kept
        if i == 9:
            body[6000:11000] = ord("n")        # lower-case n is not counted by the rule (sequence.py:38-39)
            body[0:5000] = ord("N")            # window 0 is never dropped
        parts.append(body)
    seq = np.concatenate(parts)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    buf = engine.alloc(len(seq))
    try:
        buf.upload(seq)
        for single in (False, True):
            for prec in (DEFAULT_PRECISION, "f32"):
                want, want_ids = engine.classify_contigs_spans(buf.ptr, offsets, single, prec)
                got_dev, ids_dev = engine.classify_contigs_dev(buf.ptr, offsets, single, prec)
                got_host, ids_host = engine.classify_contigs(seq, offsets, single, prec)
                assert np.array_equal(ids_dev, want_ids) and np.array_equal(ids_host, want_ids)
                assert np.array_equal(got_dev, want) and np.array_equal(got_host, want), (single, prec)
        assert len(want_ids) == len(lengths)                          # single window: one per contig
        full, full_ids = engine.classify_contigs(seq, offsets, False, DEFAULT_PRECISION)
        assert len(full_ids) == sum(len(sequence.window_spans(n)) for n in lengths) - 1      # one dropped
        # a sub-table that starts in the middle of the buffer, and the empty table
        sub, sub_ids = engine.classify_contigs(seq, offsets[7:], False, DEFAULT_PRECISION)
        assert np.array_equal(sub, full[7:]) and np.array_equal(sub_ids, full_ids[full_ids >= 7] - 7)
        empty, e_ids = engine.classify_contigs(seq, offsets[:1], False, DEFAULT_PRECISION)
        assert empty.shape == (0, 3) and len(e_ids) == 0
        with pytest.raises(Exception, match="offsets"):
            engine.classify_contigs(seq, np.array([0, 50, 40, 60]), False, DEFAULT_PRECISION)
    finally:
        buf.free()


# ------------------------------------------------------------------ downstream consumers
def test_downstream_consumers_match_the_reference_functions(engine, golden_dir, tmp_path):
    """branch_attention / score_batch_correction on the device vs the outputs of the REFERENCE's own
    numpy functions (tests/golden/consumers_golden.npz, generated by running them in place) — the one
    floating-point part of the reference that can execute here, so this parity is pinned.  f64: 1e-12."""
    from genomad_amd import consumers
    g = np.load(os.path.join(golden_dir, "consumers_golden.npz"))
    for t, key in ((2, "branch_attention_t2"), (1, "branch_attention_t1")):
        got = consumers.branch_attention(engine, g["w"], g["b1"], g["b2"], temperature=t)
        assert np.abs(got - g[key]).max() < 1e-12
    wfile = tmp_path / "score_calibration_weights.npz"
    np.savez(wfile, **{k[len("weights__"):]: g[k] for k in g.files if k.startswith("weights__")})
    for ci, comp in enumerate(g["compositions"]):
        for classifier in ("nn", "marker", "aggregated", "something_else"):
            got = consumers.score_batch_correction(engine, g["b2"], comp, classifier, wfile)
            assert np.abs(got - g[f"calibrated_{ci}_{classifier}"]).max() < 1e-12, (ci, classifier)
    assert consumers.branch_attention(engine, np.zeros(0), np.zeros((0, 3)), np.zeros((0, 3))).shape == (0, 3)


def _calibrated_weights(seed, n_cal=64):
    """synthetic.synth_weights(seed) with the output bias re-centred for THAT seed: the constant of synth_weights is tuned
    for seed 42, other seeds saturate one class (score std 0: a vacuous test).  The mean logits over a few windows come from
    the device's exact-f32 features (debug tap) and the dense head in numpy."""
    from genomad_amd.engine import NNEngine
    w = synthetic.synth_weights(seed=seed)
    bases = synthetic.synth_windows(100_000, n_cal)
    with NNEngine(0, w) as e:
        _, t = e.debug_forward(bases, "f32", taps=("feat",))
    f = t["feat"].astype(np.float64)

    def bn(x, p):
        return w[f"{p}_bn_gamma"] * (x - w[f"{p}_bn_mean"]) / np.sqrt(w[f"{p}_bn_var"] + 1e-3) + w[f"{p}_bn_beta"]
    h1 = np.maximum(bn(f @ w["enc_dense_kernel"] + w["enc_dense_bias"], "enc"), 0)
    h2 = np.maximum(bn(h1 @ w["head_dense_kernel"] + w["head_dense_bias"], "head"), 0)
    logits = h2 @ w["out_dense_kernel"]
    w["out_dense_bias"] = (-logits.mean(axis=0)).astype(np.float32)
    return w


def test_second_weight_set_and_engine(synth_weights):
    """Nothing is specialised to the seed-42 weights: a second engine with other weights (other patch
    positions -> other step buckets, larger conv gains) still matches the oracle; two engines coexist.  And a third,
    NON-DEGENERATE weight set (seed 43, output bias calibrated so that all three class scores vary): the default arithmetic
    holds the tolerance with margin on 4096 windows, the opt-in fast modes stay in its neighbourhood."""
    from genomad_amd._lib import DEFAULT_PRECISION
    from genomad_amd.engine import NNEngine
    w2 = synthetic.synth_weights(seed=7)
    w2["conv2_kernel"] = w2["conv2_kernel"] * 1.5          # different dynamic range
    p = w2["iglooA_patches"].copy()
    p[:300, :, 0] = np.sort(np.random.default_rng(1).integers(5880, 5997, (300, 4)), axis=1)   # crowd the last step
    w2["iglooA_patches"] = p
    bases = synthetic.synth_windows(40, 24)
    want = igloo_oracle.classify_windows(bases, w2, np.float32)
    with NNEngine(0, w2) as e2:
        got = e2.classify(bases, "bf16x3")
        got6 = e2.classify(bases, "f16c6")
        got16 = e2.classify(bases, "f16x3")
        exact = e2.classify(bases, "f32")
    assert np.abs(exact - want).max() <= 2e-5
    assert np.abs(got16 - want).max() <= 2e-5
    assert np.abs(got - want).max() <= SCORE_TOL
    assert np.abs(got6 - want).max() <= SCORE_TOL
    assert not np.array_equal(got, np.zeros_like(got))
    w3 = _calibrated_weights(43)
    big = synthetic.synth_windows(200_000, 4096)
    with NNEngine(0, w3) as e3:
        exact = e3.classify(big, "f32")
        assert exact.std(axis=0).min() > 0.05, exact.std(axis=0)          # every class score varies: the check is not vacuous
        err = {prec: float(np.abs(e3.classify(big, prec) - exact).max()) for prec in ("f16x3", "f16x3tc", "bf16x3", "f16c6")}
    print("seed-43 weights (calibrated), 4096 windows, max |dscore| vs the exact-f32 path:", err)
    assert DEFAULT_PRECISION == "f16x3tc" and err["f16x3tc"] <= SCORE_TOL / 4 and err["f16x3"] <= SCORE_TOL / 4
    assert err["bf16x3"] <= SCORE_TOL
    assert err["f16c6"] <= 2 * SCORE_TOL


@pytest.mark.parametrize("prec", ["f16c6", "f16x3", "f16x3tc", "f16x3tk", "bf16x3"])
def test_padding_skip_is_bit_identical(engine, prec, request):
    """All four streaming kernels (f16c6 of gnn_fused_c6.hip; f16x3 / bf16x3 of gnn_fused_x3.hip; f16x3tc of gnn_fused_tc.hip; f16x3tk of
    gnn_fused_tk.hip) copy the yp rows and pair products of a window's all-N tail from an all-N window instead of
    computing them (the padding of a contig's last window, nn_classification.py:72).  With the skip switched off the
    scores AND the intermediates must be the same bits: windows of every length class (empty, shorter than a step,
    ending exactly on / one base around a step boundary, on both sides of a change of the step count - L = k FT - 15 | L + 1, for the
    96-row steps of tc / tk and the 128-row steps of x3 / c6, up to where the copy disappears -, N runs inside, IUPAC codes and lower
    case in the tail, full).  Every length: tests/test_window_lengths_gpu.py."""
    need_tables(request, prec)
    from genomad_amd import _lib
    rng = np.random.default_rng(11)
    def win(n, tail=b"N"):
        body = bytes(rng.choice(list(b"ACGT"), n).tolist())
        return (body + tail * 6000)[:6000]
    lens = [0, 1, 3, 81, 82, 100, 112, 113, 114, 127, 128, 129, 177, 178, 2500, 2559, 2560, 2561, 4000, 5873, 5874, 5937, 5938, 5984, 5996, 5997, 6000]
    wins = [win(n) for n in lens]
    wins.append(win(3000, b"n"))                      # lower-case n: not ACGT either
    wins.append(win(3000, b"R"))                      # IUPAC code
    w = bytearray(win(6000)); w[1000:5200] = b"N" * 4200; wins.append(bytes(w))       # N run inside, bases after it
    w = bytearray(win(2000)); w[500:700] = b"N" * 200; wins.append(bytes(w))
    bases = np.frombuffer(b"".join(wins), np.uint8).reshape(len(wins), 6000).copy()
    taps = ("m_a", "m_b", "yp_a", "yp_b", "feat")
    try:
        _lib.check(engine.lib.gnn_debug_set_pad_skip(engine.ctx, 0))
        full, tfull = engine.debug_forward(bases, prec, taps=taps)
        _lib.check(engine.lib.gnn_debug_set_pad_skip(engine.ctx, 1))
        skip, tskip = engine.debug_forward(bases, prec, taps=taps)
    finally:
        _lib.check(engine.lib.gnn_debug_set_pad_skip(engine.ctx, 1))
    assert np.isfinite(full).all()
    for k in taps:
        assert np.array_equal(tfull[k], tskip[k]), k
    assert np.array_equal(full, skip)
    exact = engine.classify(bases, "f32")
    assert np.abs(skip - exact).max() <= SCORE_TOL


def test_a_misaligned_window_buffer_gives_the_same_scores(engine):
    """the streaming kernels fetch bases as aligned dwords.  A device buffer a caller offsets by 1, 2 or 3 bytes goes
    through one aligned staging copy and the SAME kernel: bit-identical scores for every fused arithmetic (until round 5 the round-1
    kernel served such buffers: another kernel, several times slower, other bits, no message; f16c6 refused them).  Reference shape:
    nn_classification.py:316-317 - any batch at any offset gives the same scores."""
    n = 300                                        # more than one round of workgroups, not a multiple of anything
    buf = engine.alloc(n * 6000 + 8)
    out = engine.alloc(n * 12)
    try:
        engine.synth_windows_dev(0, n, buf.ptr)
        engine.sync()
        host = buf.download((n * 6000,), np.uint8)
        fused = [p_ for p_ in FUSED if p_ != "f16x3tk" or engine.build_kmer_tables()]
        want = {prec: engine.classify(host.reshape(n, 6000), prec) for prec in fused}
        for shift in (1, 2, 3):
            buf.upload(np.concatenate([np.zeros(shift, np.uint8), host, np.zeros(8 - shift, np.uint8)]))
            for prec in fused:
                engine.classify_dev(buf.ptr + shift, n, out.ptr, prec)
                engine.sync()
                assert np.array_equal(out.download((n, 3), np.float32), want[prec]), (shift, prec)
    finally:
        buf.free()
        out.free()


def test_asynchronous_classification_is_bit_identical(engine):
    """gnn_classify_dev_async leaves the last back end of a call on the second stream, beside the next call's front end
    (two alternating workspaces).  Many small calls (one launch each), mixed sizes, interleaved with synchronous calls and a
    debug forward: after gnn_classify_flush + sync the scores are the bits the synchronous entry point produces."""
    n = 6 * 1024 + 300
    bases = engine.alloc(n * 6000)
    a = engine.alloc(n * 12)
    b = engine.alloc(n * 12)
    try:
        engine.synth_windows_dev(4242, n, bases.ptr)
        engine.classify_dev(bases.ptr, n, a.ptr, "f16c6")
        engine.sync()
        want = a.download((n, 3), np.float32)
        cuts = [0, 1024, 1030, 2048, 3072, 3073, 5000, 6144, n]
        tb = synthetic.synth_windows(7, 4)
        mid = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            engine.classify_dev_async(bases.ptr + lo * 6000, hi - lo, b.ptr + lo * 12, "f16c6")
            if lo == 2048:          # a tapped forward in between reads ITS workspace, whatever is pending
                mid = [engine.debug_forward(tb, "f16c6"), engine.debug_forward(tb, "f16c6")]
        engine.flush()
        engine.sync()
        got = b.download((n, 3), np.float32)
        s3, t3 = engine.debug_forward(tb, "f16c6")       # nothing pending any more: the reference for the two in between

        def rows(x, y):
            return np.nonzero((x != y).reshape(len(x), -1).any(axis=1))[0].tolist()
        report = []
        for i, (s, t) in enumerate(mid):
            if not np.array_equal(s, s3):
                report.append(f"forward {i + 1} of 2 beside pending calls: score rows {rows(s, s3)} differ by {np.abs(s - s3).max():.2e}")
            for k in t:
                if not np.array_equal(t[k], t3[k]):
                    report.append(f"forward {i + 1}: tap {k} windows {rows(t[k], t3[k])}, {int((t[k] != t3[k]).sum())} of "
                                  f"{t[k].size} values, max {np.abs(t[k] - t3[k]).max():.2e}")
        bad = rows(got, want)
        if bad:
            report.append(f"asynchronous scores: {len(bad)} rows differ, first {bad[:12]} last {bad[-3:]}, max "
                          f"{np.abs(got - want)[bad].max():.2e}, NaN rows {int(np.isnan(got[bad]).any(axis=1).sum())}")
        assert not report, "; ".join(report)
        assert np.isfinite(t3["feat"]).all() and np.abs(t3["feat"]).max() > 0
        # no explicit flush: a download orders the pending back end as well
        engine.classify_dev_async(bases.ptr, 512, b.ptr, "f16x3")
        engine.classify_dev_async(bases.ptr + 512 * 6000, 512, b.ptr + 512 * 12, "f16x3")
        got8 = b.download((1024, 3), np.float32)
        engine.classify_dev(bases.ptr, 1024, a.ptr, "f16x3")
        engine.sync()
        assert np.array_equal(got8, a.download((1024, 3), np.float32))
    finally:
        for buf in (bases, a, b):
            buf.free()


def test_asynchronous_calls_survive_a_growing_workspace(synth_weights):
    """A pending asynchronous back end must be finished before a later, larger call re-allocates the workspaces."""
    from genomad_amd.engine import NNEngine
    with NNEngine(0, synth_weights, chunk=2048) as eng:
        n = 2048
        bases, a, b = eng.alloc(n * 6000), eng.alloc(n * 12), eng.alloc(n * 12)
        eng.synth_windows_dev(99, n, bases.ptr)
        eng.classify_dev_async(bases.ptr, 256, b.ptr, "f16c6")               # small workspaces, back end left pending
        eng.classify_dev_async(bases.ptr + 256 * 6000, n - 256, b.ptr + 256 * 12, "f16c6")   # grows them
        eng.flush()
        eng.sync()
        got = b.download((n, 3), np.float32)
        eng.classify_dev(bases.ptr, n, a.ptr, "f16c6")
        eng.sync()
        assert np.array_equal(got, a.download((n, 3), np.float32))


def test_default_launch_size_follows_the_free_device_memory(synth_weights):
    """the library default of 16 384 windows per launch means 14 GB of workspace (28 GB on the asynchronous
    path); an integrator on a shared or partitioned GPU never asked for that.  With most of the device memory taken the default is
    clamped to a quarter of what is free (and says so), an explicit gnn_set_chunk that cannot be allocated is halved until it
    fits (the failed hipMalloc must not stay behind as HIP's last error), the asynchronous path runs in order when its second
    workspace does not fit - and the scores do not move by a bit (scores do not depend on the launch size)."""
    from genomad_amd import _lib
    from genomad_amd.engine import NNEngine
    n = 12288

    def launches_of(eng, fn):
        eng.profile_enable(True)
        eng.profile_reset()
        fn()
        eng.sync()
        _, l = eng.profile_get(_lib.K_FUSED)
        eng.profile_enable(False)
        return l

    with NNEngine(0, synth_weights) as eng:                      # library default, no gnn_set_chunk
        b, s = eng.alloc(n * 6000), eng.alloc(n * 12)
        eng.synth_windows_dev(5000, n, b.ptr)
        eng.sync()
        hog = eng.alloc(eng.mem_info()[0] - (16 << 30))          # leave 16 GB free: a quarter of it = ~4 k windows of workspace
        try:
            l = launches_of(eng, lambda: eng.classify_dev(b.ptr, n, s.ptr))
            want = s.download((n, 3), np.float32)
            assert 3 <= l <= 48, l                               # 12 288 windows in launches of 256 .. 4 096, not ONE launch of 12 288
            assert np.isfinite(want).all() and want.std(axis=0).min() > 0.05
            # asynchronous path: the second workspace is tried, and whatever happens the scores are the same
            eng.classify_dev_async(b.ptr, n // 2, s.ptr)
            eng.classify_dev_async(b.ptr + (n // 2) * 6000, n // 2, s.ptr + (n // 2) * 12)
            eng.flush()
            eng.sync()
            assert np.array_equal(s.download((n, 3), np.float32), want)
        finally:
            hog.free()
        # explicit size: no clamp, halve-and-retry on allocation failure: 12 288 windows x 0.86 MB = 10.6 GB do not fit into the 4 GB
        # left free plus the ~4 GB the clamped workspace gives back; 6 144 windows (5.3 GB) do
        _lib.check(eng.lib.gnn_set_chunk(eng.ctx, 16384))
        hog = eng.alloc(eng.mem_info()[0] - (4 << 30))
        try:
            l = launches_of(eng, lambda: eng.classify_dev(b.ptr, n, s.ptr))
            assert l >= 2
            assert np.array_equal(s.download((n, 3), np.float32), want)
        finally:
            hog.free()
        # with the memory back and the launch size the halving left behind: one more pass, the same bits
        eng.classify_dev(b.ptr, n, s.ptr)
        eng.sync()
        assert np.array_equal(s.download((n, 3), np.float32), want)
    with NNEngine(0, synth_weights, chunk=2048) as ref:          # an engine that never saw a short device
        rb, rs = ref.alloc(n * 6000), ref.alloc(n * 12)
        ref.synth_windows_dev(5000, n, rb.ptr)
        ref.classify_dev(rb.ptr, n, rs.ptr)
        ref.sync()
        assert np.array_equal(rs.download((n, 3), np.float32), want)


def test_bench_command_line_prints_one_complete_json_line(tmp_path):
    """The driver's command, at a size that takes seconds: `python bench.py --gpus 1 --steps K --warmup W --full` prints exactly one
    JSON line on stdout with the contract's fields, goes through RCCL at N = 1 (rccl_ranks), checks EVERY timed window against
    the exact-f32 path (parity.ok) and every step bit for bit against the synchronous entry point, and exits 0; the fast opt-in
    arithmetic is allowed to fail that check but must then say so and exit non-zero, never print a clean line.  The plain command
    prints the headline fields and writes, with --dump-outputs, the scores of the last step: the same bits as the --full run's."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--windows-per-step", "2048", "--cpu-sample", "0"]
    dumps = {}
    for name, extra in (("plain", []), ("full", ["--full"])):
        dumps[name] = tmp_path / name
        r = subprocess.run(cmd + extra + ["--dump-outputs", str(dumps[name])], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [x for x in r.stdout.splitlines() if x.strip()]
        assert len(lines) == 1, r.stdout
        d = json.loads(lines[0])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"):
            assert key in d, key
        assert d["steps"] == 3 and d["value"] > 0 and d["ms_per_step"] > 0
    plain, full = (np.load(dumps[n] / "scores.npy") for n in ("plain", "full"))
    assert plain.shape == (2048, 3) and plain.dtype == np.float32 and np.array_equal(plain, full)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "rccl_ranks", "parity", "steps_verified"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["rccl_ranks"] == 1 and d["steps"] == 3 and d["config"]["precision"] == DEFAULT_PRECISION
    assert d["parity"]["ok"] and d["parity"]["windows"] == 3 * 2048 and d["parity"]["max_abs_dscore_all"] <= SCORE_TOL / 2
    assert d["steps_verified"]["mismatching_windows_all_ranks"] == 0
    assert d["roofline"]["bound"] == "mfma" and 0 < d["roofline"]["frac"] < 1 / d["roofline"]["mfma_passes"]
    assert d["value"] > 50_000


def test_fresh_process_call_mix_is_bit_identical_24_times():
    """The round-2 mismatch only ever showed up in the first launches of FRESH processes (profiles/history/r03_pair_row_race.md: a
    data race on the conv1 pair rows inside the f16c6 kernel that a wave delayed by first-touch latencies exposed; fixed by
    ordering the pair rows with a barrier).  One process = one sample: 40 fresh processes run the call mix of
    scripts/async_hunt.py (synchronous reference, asynchronous calls of mixed sizes, tapped host forwards in between, two
    rounds) — 8 with the f16c6 kernel it was seen in, 16 with the default arithmetic's kernel (round 3 ran 40 per suite and
    1 170 in total without a miss; the default's kernel changed in round 4, so it gets the larger share)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bad = []
    for i0 in range(0, 24, 3):                              # three at a time: each other's first-touch traffic is part of the test
        procs = []
        for i in range(i0, i0 + 3):
            prec = "f16c6" if i % 3 == 0 else DEFAULT_PRECISION
            procs.append((i, prec, subprocess.Popen([sys.executable, os.path.join(root, "scripts", "async_hunt.py"), "2", prec],
                                                    stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
        for i, prec, pr in procs:
            out, err = pr.communicate(timeout=300)
            last = (out.strip().splitlines() or ["<no output>"])[-1]
            if pr.returncode != 0 or not last.startswith("OK"):
                bad.append((i, prec, last[:600], err[-300:]))
    assert not bad, bad


def test_time_split_small_batches_are_bit_identical(engine):
    """Launches smaller than the chip (the reference's call shape: one predict per 128 windows, nn_classification.py:316-317) deal
    every window's 47 steps to up to 4 workgroups with one warm-up step each (gnn_fused_x3.hip).  Scores AND the spilled
    intermediates (pair products behind m, pooled y @ w_v rows) must equal the one-workgroup launch bit for bit, for every batch
    size on both sides of the thresholds, for padded / N-run / all-N / empty windows (padding skip on and off), and for the
    fallback arithmetic; and the split launch must actually be faster at 128 windows."""
    import time
    from genomad_amd import _lib
    wins = synthetic.synth_windows(3000, 130)
    wins[7] = _pad(b"")                                    # all N: the padding skip leaves one step
    wins[8] = _pad(b"ACGT" * 40)                           # 160 bases: 2 steps
    wins[9] = _pad(b"ACGT" * 700)                          # 2800 bases
    wins[10, 3000:3300] = ord("N")
    try:
        for prec in ("f16x3", "f16x3tc", "f16x3tk", "bf16x3"):
            if prec == "f16x3tk" and not engine.build_kmer_tables():
                continue
            for n in (1, 2, 40, 64, 65, 86, 128, 130):
                for skip in (1, 0):
                    _lib.check(engine.lib.gnn_debug_set_pad_skip(engine.ctx, skip))
                    _lib.check(engine.lib.gnn_debug_set_time_split(engine.ctx, 0))
                    want, wt = engine.debug_forward(wins[:n], prec, taps=("m_a", "m_b", "yp_a", "yp_b"))
                    _lib.check(engine.lib.gnn_debug_set_time_split(engine.ctx, 1))
                    got, gt = engine.debug_forward(wins[:n], prec, taps=("m_a", "m_b", "yp_a", "yp_b"))
                    assert np.array_equal(got, want), (prec, n, skip)
                    for k in wt:
                        assert np.array_equal(gt[k], wt[k]), (prec, n, skip, k)
                if n > 40 and prec not in ("f16x3", "f16x3tk"):
                    break                                  # the fallback: the small sizes are enough
        _lib.check(engine.lib.gnn_debug_set_pad_skip(engine.ctx, 1))
        # the point of it: one call of 128 windows through the host-buffer entry point
        import ctypes
        ms, split = {}, ctypes.c_int()
        for on in (0, 1):
            _lib.check(engine.lib.gnn_debug_set_time_split(engine.ctx, on))
            engine.classify(wins[:128])
            _lib.check(engine.lib.gnn_debug_last_split(engine.ctx, ctypes.byref(split)))
            # that the split happened is checked structurally (a wall-clock bound on a 1 ms launch fails on a shared
            # or throttled GPU without any defect): 128 windows on 256 CUs = 2 workgroups per window, 1 with the switch off
            assert split.value == (max(1, min(4, engine.device_info()["cus"] // 128)) if on else 1), (on, split.value)
            t = time.perf_counter()
            for _ in range(20):
                engine.classify(wins[:128])
            ms[on] = (time.perf_counter() - t) / 20 * 1e3
        print(f"gnn_classify of 128 windows: {ms[0]:.3f} ms one workgroup per window, {ms[1]:.3f} ms time split (informational)")
    finally:
        _lib.check(engine.lib.gnn_debug_set_time_split(engine.ctx, 1))
        _lib.check(engine.lib.gnn_debug_set_pad_skip(engine.ctx, 1))


@pytest.mark.parametrize("prec", ["f16x3tc", "f16x3tk"])
def test_toomcook_kernel_is_bit_identical_under_delay_injection(engine, tmp_path, prec):
    """The default kernel orders its LDS producers and consumers with 18 bare s_barriers per step (tests/test_kernel_schedule.py
    models the schedule).  libgenomad_nn_hip_jitter.so is the same library with every wave sleeping a pseudo-random 0..2 000
    cycles behind every barrier (3.5x the run time): scores, pair products and pooled y @ w_v rows of 600 / 128 / 40 windows
    (padded and all-N ones included, time split included) must be the bits the normal library produces - the method that made
    round 2's pair-row race deterministic (profiles/history/r03_pair_row_race.md), applied to the new kernel."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    jitter = os.path.join(root, "genomad_amd", "csrc", "libgenomad_nn_hip_jitter.so")
    if not os.path.exists(jitter):
        pytest.skip("libgenomad_nn_hip_jitter.so not built (genomad_amd/csrc/build.sh builds it)")
    script = os.path.join(root, "scripts", "tc_jitter_check.py")
    if prec == "f16x3tk":
        engine.drop_kmer_tables()          # the subprocesses build their own (one 156 GB set fits beside the session engine, two do not)
    ref = str(tmp_path / "ref.npz")
    env = {k: v for k, v in os.environ.items() if k != "GENOMAD_AMD_LIB"}
    r = subprocess.run([sys.executable, script, "ref", ref, prec], env=env, capture_output=True, text=True, timeout=300, cwd=root)
    if r.returncode == 77:
        pytest.skip("the device cannot hold the k-mer tables")
    assert r.returncode == 0, r.stderr[-1500:]
    for _ in range(2):
        r = subprocess.run([sys.executable, script, "cmp", ref, prec], env=dict(env, GENOMAD_AMD_LIB=jitter), capture_output=True, text=True,
                           timeout=300, cwd=root)
        assert r.returncode == 0 and "OK:" in r.stdout, (r.stdout[-800:], r.stderr[-800:])


# ------------------------------------------------------------------ f16x3tk: conv2 and head A read from k-mer tables in HBM (round 6)
_DIG = {65: 0, 67: 1, 71: 2, 84: 3}


def test_kmer_table_rows_are_the_exact_paths_activations(kmer_tables):
    """The 14-mer table holds x2[t] = LeakyReLU(conv2(x1))[t] (igloo.py:65-67) for the 14 bases t-10 .. t+3, head A's table the pair product
    of (entry, 9-mer at its position) (igloo.py:192-204 folded): rows fetched through the test aid against the exact-f32 path's x2
    tap at the positions of a synthetic window (f64 accumulation, rounded once: within 4e-6 of the f32 FMA chain)."""
    import ctypes
    from genomad_amd import _lib
    eng = kmer_tables
    wins = synthetic.synth_windows(11, 1)
    wins[0, 3000:3020] = ord("N")
    _, t = eng.debug_forward(wins, "f32", taps=("x2",))
    row = np.empty(128, np.float32)
    worst = 0.0
    for pos in (10, 11, 12, 13, 97, 1000, 2999 - 4, 3020 + 10, 5995, 5996):
        code = 0
        for b in wins[0, pos - 10:pos + 4]:
            code = code * 4 + _DIG[int(b)]
        _lib.check(eng.lib.gnn_debug_kmer_table_row(eng.ctx, 0, ctypes.c_uint64(code), row.ctypes.data))
        worst = max(worst, float(np.abs(row - t["x2"][0, pos]).max()))
    assert worst <= 4e-6, worst
    # the all-N-token row = x2 deep inside an N run
    _lib.check(eng.lib.gnn_debug_kmer_table_row(eng.ctx, 0, ctypes.c_uint64(1 << 28), row.ctypes.data))
    alln = np.frombuffer(b"N" * 6000, np.uint8).reshape(1, 6000)
    _, tn = eng.debug_forward(alln, "f32", taps=("x2",))
    assert np.abs(row - tn["x2"][0, 3000]).max() <= 4e-6
    with pytest.raises(_lib.GnnError, match="out of range"):
        _lib.check(eng.lib.gnn_debug_kmer_table_row(eng.ctx, 0, ctypes.c_uint64((1 << 28) + 1), row.ctypes.data))


def test_kmer_tables_rows_no_table_holds(kmer_tables, synth_weights):
    """What the 14-mer table cannot index - the first ten positions of a window (absent tokens), k-mers that mix ACGT with other bytes
    (single Ns, N-run edges at every alignment, IUPAC codes, lower case), the window's last positions - goes through conv2's tap
    tables (<= 6 row reads per position) and, for head A's entries, a per-entry dot product: every stage within the default
    arithmetic's tolerances of the fp64 oracle, scores within 1e-4 / 2 of it, and the same bits whatever the batch."""
    eng = kmer_tables
    rng = np.random.default_rng(17)
    base = synthetic.synth_windows(900, 12).copy()
    base[0, :1] = ord("N")                               # N at the very first base
    base[1, 5:6] = ord("N")
    base[2, 9:14] = ord("N")
    base[3, 5996:] = ord("N")                            # the last token
    for k, a in enumerate(range(1000, 1000 + 40 * 97, 97)):          # N runs of every length 1 .. 40 at every alignment mod 4 and mod 96
        base[4, a:a + k + 1] = ord("N")
    base[5, rng.integers(0, 6000, 300)] = ord("N")       # 5 % scattered N: most 14-mers of the window are mixed
    base[6, rng.integers(0, 6000, 60)] = rng.choice(list(b"RYKMSWBDHVN"), 60)
    base[7, 1200:2400] += 32                             # a lower-case (soft-masked) stretch
    base[8, 0:3] = ord("N")
    base[9, 2000:] = ord("N")                            # a contig's last window: padding
    base[10, :] = ord("N")
    base[11, 95:97] = ord("N")                           # across the first step boundary
    want, t64 = igloo_oracle.forward(sequence_oracle.tokenize_closed_form(base), synth_weights, np.float64, return_taps=True)
    got, taps = eng.debug_forward(base, "f16x3tk")
    for mine, ref, tol in (("m_a", "mA", 1e-4), ("m_b", "mB", 2.5e-4), ("yp_a", "ypA", 1e-4), ("yp_b", "ypB", 2.5e-4), ("feat", "f", 1.25e-4)):
        err = np.abs(taps[mine] - t64[ref]).max()
        assert err <= tol, f"{mine}: {err:.3e}"
    assert np.abs(got - want).max() <= SCORE_TOL / 2
    assert np.array_equal(eng.classify(base[3:9], "f16x3tk"), got[3:9])
    assert np.abs(got - eng.classify(base, "f16x3tc")).max() <= 2e-5


def test_kmer_tables_that_do_not_fit_leave_the_default_arithmetic(synth_weights):
    """A device that cannot hold the tables behind the reserve asked for answers GNN_ERR_NOMEM with nothing allocated (the Python side:
    False), F16X3TK then answers GNN_ERR_STATE, F16X3TC keeps serving; dropping built tables returns their memory."""
    from genomad_amd._lib import GnnError
    from genomad_amd.engine import NNEngine
    with NNEngine(0, synth_weights) as eng:
        free0 = eng.mem_info()[0]
        assert eng.build_kmer_tables(reserve_bytes=1 << 50) is False
        assert not eng.has_kmer_tables() and abs(eng.mem_info()[0] - free0) < (64 << 20)
        b = synthetic.synth_windows(0, 4)
        with pytest.raises(GnnError, match="k-mer tables"):
            eng.classify(b, "f16x3tk")
        ref = eng.classify(b, "f16x3tc")
        if eng.build_kmer_tables(reserve_bytes=0):          # a second set beside the session engine's only fits a large device
            assert eng.has_kmer_tables() and eng.mem_info()[0] < free0 - (140 << 30)
            assert np.abs(eng.classify(b, "f16x3tk") - ref).max() <= 2e-5
            eng.drop_kmer_tables()
            assert not eng.has_kmer_tables() and eng.mem_info()[0] > free0 - (1 << 30)


def test_config3_1m_windows_through_the_kmer_tables(kmer_tables, golden_dir):
    """BASELINE configs 3/4 with the arithmetic bench.py times on a device that holds the tables: run-to-run bit identity, 8 contiguous
    shards == one pass, and every 64th of the 2^20 windows against the outputs of the reference's own graph within half the tolerance."""
    eng = kmer_tables
    n = 1 << 20
    one = _classify_resident(eng, 0, n, "f16x3tk")
    assert hashlib.sha256(one.tobytes()).hexdigest() == hashlib.sha256(_classify_resident(eng, 0, n, "f16x3tk").tobytes()).hexdigest()
    assert np.array_equal(one, _classify_resident(eng, 0, n, "f16x3tk", shards=8))
    assert np.isfinite(one).all() and np.abs(one.sum(1) - 1.0).max() < 1e-5
    assert np.array_equal(one[777_000:777_512], _classify_resident(eng, 777_000, 512, "f16x3tk"))
    g = np.load(os.path.join(golden_dir, "config3_strided_golden.npz"))
    idx = g["indices"]
    e32 = float(np.abs(one[idx] - g["scores_refgraph32"]).max())
    e64 = float(np.abs(one[idx] - g["scores_oracle64"]).max())
    print(f"config 3, {len(idx)} windows strided over 2^20, f16x3tk: max |dscore| vs reference graph {e32:.3e}, vs fp64 oracle {e64:.3e}")
    assert e32 <= SCORE_TOL / 2 and e64 <= SCORE_TOL / 2


def test_main_promotes_the_default_arithmetic_to_the_kmer_tables(kmer_tables, synth_weights, tmp_path, monkeypatch):
    """main() (nn_classification.py:21-30) on an engine that holds the tables classifies with f16x3tk (GENOMAD_AMD_KMER_TABLES=auto),
    with the default arithmetic under GENOMAD_AMD_KMER_TABLES=0: the per-contig scores agree to 2e-5, both are within 1e-4 of the
    oracle chain, and the explicit GENOMAD_AMD_PRECISION=f16x3tk gives the bits of the promoted run."""
    from genomad_amd import nn_classification as nnc
    from genomad_amd import weights as W
    rng = np.random.default_rng(21)
    recs = [("k1", "".join(rng.choice(list("ACGT"), 30000))), ("k2", "NN" + "".join(rng.choice(list("ACGTN"), 14000, p=[.24, .24, .24, .24, .04]))),
            ("k3", "".join(rng.choice(list("acgt"), 700)))]
    fa = tmp_path / "k.fna"
    fa.write_text("".join(f">{n}\n{s}\n" for n, s in recs))
    wpath = tmp_path / "w.npz"
    W.save_npz(wpath, synth_weights)
    monkeypatch.setenv("GENOMAD_AMD_WEIGHTS", str(wpath))
    monkeypatch.setattr(nnc, "_ENGINE", kmer_tables)
    seen = []
    real = nnc.classify_contigs_safely
    monkeypatch.setattr(nnc, "classify_contigs_safely", lambda eng, sq, off, sw, prec, console=None: (seen.append(prec), real(eng, sq, off, sw, prec, console))[1])
    preds = {}
    for tag, env in (("auto", {}), ("off", {"GENOMAD_AMD_KMER_TABLES": "0"}), ("explicit", {"GENOMAD_AMD_PRECISION": "f16x3tk"})):
        for k in ("GENOMAD_AMD_KMER_TABLES", "GENOMAD_AMD_PRECISION"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out = tmp_path / tag
        nnc.main(fa, out, False, 128, True, 1, False, False)
        preds[tag] = np.load(out / "k_nn_classification" / "k_nn_classification.npz")["predictions"]
    assert seen == ["f16x3tk", "f16x3tc", "f16x3tk"], seen
    names, ids, wins = sequence_oracle.encode_fasta(fa)
    want = sequence_oracle.segment_mean(igloo_oracle.classify_windows(wins, synth_weights, np.float32), ids)
    for tag in preds:
        assert np.abs(preds[tag] - want).max() <= SCORE_TOL, tag
    assert np.array_equal(preds["auto"], preds["explicit"])
    assert 0 < np.abs(preds["auto"] - preds["off"]).max() <= 2e-5


def test_crowded_steps_take_the_overflow_loops(engine, synth_weights):
    """A weight set whose random patches are concentrated in the first 600 positions: ~1 300 entries per 96-row step instead of ~134, so
    head B's passes beyond the third (pass_rest) and head A's entries beyond one per helper thread (the loop behind E in gnn_fused_tk.hip)
    run - neither ever does with uniformly drawn patches.  Both Toom-Cook kernels against the exact-f32 path, which has no step structure."""
    from genomad_amd.engine import NNEngine
    w = dict(synth_weights)
    rng = np.random.default_rng(31)
    for head in ("iglooA", "iglooB"):
        p = np.sort(rng.integers(0, 600, size=w[f"{head}_patches"].shape).astype(np.int32), axis=1)
        p[:40, :, 0] = np.sort(rng.integers(0, 12, size=(40, p.shape[1])), axis=1)      # a crowd at the window start: head A's x1-table path as well
        w[f"{head}_patches"] = p
    bases = synthetic.synth_windows(321, 6).copy()
    bases[1, 40:60] = ord("N")
    bases[2, 300:] = ord("N")
    engine.drop_kmer_tables()                      # room for this engine's own tables
    with NNEngine(0, w) as e2:
        ref, rt = e2.debug_forward(bases, "f32", taps=("m_a", "m_b", "feat"))
        precs = ["f16x3tc"] + (["f16x3tk"] if e2.build_kmer_tables() else [])
        for prec in precs:
            got, t = e2.debug_forward(bases, prec, taps=("m_a", "m_b", "feat"))
            assert np.abs(t["m_a"] - rt["m_a"]).max() <= 2e-5, prec
            assert np.abs(t["m_b"] - rt["m_b"]).max() <= 2e-4, prec
            assert np.abs(got - ref).max() <= SCORE_TOL / 2, (prec, float(np.abs(got - ref).max()))
            assert np.array_equal(e2.classify(bases, prec), got)
