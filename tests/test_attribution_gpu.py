"""Attention contribution maps on the MI355X (gnn_attribute, gnn_attribute_dev, gnn_attribute_contigs): parity with the fp64
reference maps, completeness on the device's own numbers, scores bit for bit those of classify(), the bins as sequential f32 sums
of the bin = 1 map, block tails and batch invariance, the contig path against its definitions under two launch sizes, the error
paths, and main() end to end with GENOMAD_AMD_ATTRIBUTION_BIN."""
import os
from pathlib import Path

import numpy as np
import pytest

from genomad_amd import _lib, sequence
from tests import attribution_ref as R
from tests.conftest import need_tables
from tests.test_embeddings_gpu import _setup_main

pytestmark = pytest.mark.gpu

ARITH = ["f32", "f16x3", "bf16x3", "f16x3tc", "f16x3tk"]
TOL = 1e-4                                  # the project's score and embedding tolerance
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _softmax(x):
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


@pytest.mark.parametrize("prec", ARITH)
def test_maps_match_the_fp64_reference_and_are_complete(engine, prec, request):
    """Parity on the decided windows: max |d contrib| <= 1e-4 max(1, max |contrib_ref|) per window, bias and logits in the same form.
    Completeness on the device's own numbers, every window: |sum contrib + bias - logits| <= 1e-4 max(1, sum |contrib|),
    softmax(logits) within 1e-6 of the scores, the scores those of classify() bit for bit.
    Decided: every pre-activation of both hidden layers of the oracle is farther from zero than 1e-4 (attribution_ref.decided: a
    superset of the windows decided under the margin 1e-4 max(1, max |h1|), which leaves out 8 of these 32); at most 2 may not be."""
    need_tables(request, prec)
    bases, ref = R.reference_32()
    contrib, bias, logits, scores = engine.attribute(bases, 1, prec)
    assert contrib.shape == (32, 2, 749, 3) and contrib.dtype == np.float32
    assert all(a.shape == (32, 3) and a.dtype == np.float32 for a in (bias, logits, scores))
    assert np.array_equal(scores, engine.classify(bases, prec))
    c64 = contrib.astype(np.float64)
    gap = np.abs(c64.sum(axis=(1, 2)) + bias - logits) / np.maximum(1.0, np.abs(c64).sum(axis=(1, 2)))          # per (window, class)
    soft = np.abs(_softmax(logits.astype(np.float64)) - scores).max()
    ok = R.decided(ref)
    rel = lambda got, want: (np.abs(got.astype(np.float64) - want).reshape(32, -1).max(axis=1)                         # noqa: E731
                             / np.maximum(1.0, np.abs(want).reshape(32, -1).max(axis=1)))
    e_c, e_b, e_l = rel(contrib, ref["contrib"]), rel(bias, ref["bias"]), rel(logits, ref["logits"])
    print(f"\nattribution {prec}: {int((~ok).sum())} undecided windows ({int((~R.decided(ref, scaled=True)).sum())} under the scaled margin); on the decided ones max rel |d contrib| = {e_c[ok].max():.3e}, "
          f"|d bias| = {e_b[ok].max():.3e}, |d logits| = {e_l[ok].max():.3e}; on all 32: {e_c.max():.3e} / {e_b.max():.3e} / {e_l.max():.3e}; "
          f"completeness {gap.max():.3e}, |softmax(logits) - scores| = {soft:.3e}")
    # the plain margin compares seven windows the scaled one would leave out; their closest units (1.3e-4 .. 5.9e-4) lie inside the
    # project's h1 bound of these windows (6.5e-4): an arithmetic that flipped one would fail below without being wrong
    assert (~ok).sum() <= 2
    assert gap.max() <= TOL, f"{prec}: {gap.max():.3e}"
    assert soft <= 1e-6
    assert e_c[ok].max() <= TOL and e_b[ok].max() <= TOL and e_l[ok].max() <= TOL, (prec, e_c[ok].max(), e_b[ok].max(), e_l[ok].max())


def test_bins_are_the_sequential_sums_of_the_bin_1_map(engine):
    bases, _ = R.reference_32()
    bases = bases[:9]
    one, bias, logits, scores = engine.attribute(bases, 1)
    for bin_, nb in ((8, 94), (100, 8), (748, 2), (749, 1)):
        got, b2, l2, s2 = engine.attribute(bases, bin_)
        assert got.shape == (9, 2, nb, 3)
        assert np.array_equal(got, R.binned(one, bin_)), bin_
        assert np.array_equal(b2, bias) and np.array_equal(l2, logits) and np.array_equal(s2, scores)


def test_block_tails_batch_invariance_and_the_dev_path(engine):
    bases = engine.synth_windows(0, 300)
    full = engine.attribute(bases, 8)
    for n in (1, 7, 9, 32):
        for a, b in zip(engine.attribute(bases[:n], 8), full):
            assert np.array_equal(a, b[:n]), n
    n, nb = 300, 94
    db, dc = engine.alloc(n * _lib.WINDOW), engine.alloc(n * 2 * nb * 3 * 4)
    d3 = [engine.alloc(n * 3 * 4) for _ in range(3)]
    try:
        db.upload(bases)
        engine.attribute_dev(db.ptr, n, 8, dc.ptr, bias_ptr=d3[0].ptr, logits_ptr=d3[1].ptr, scores_ptr=d3[2].ptr)
        engine.sync()
        assert np.array_equal(dc.download((n, 2, nb, 3), np.float32), full[0])
        for d, want in zip(d3, full[1:]):
            assert np.array_equal(d.download((n, 3), np.float32), want)
        dc.upload(np.zeros(n * 2 * nb * 3, np.float32))
        engine.attribute_dev(db.ptr, 33, 8, dc.ptr)                       # the optional outputs may be NULL
        engine.sync()
        got = dc.download((n, 2, nb, 3), np.float32)
        assert np.array_equal(got[:33], full[0][:33]) and not got[33:].any()
    finally:
        for d in [db, dc] + d3:
            d.free()


# ---- contig path --------------------------------------------------------------------------------------------------------------
def _small_contigs():
    """a contig shorter than a window, one with a 2500-base tail, an empty record, one whose middle window is all N (dropped by the N
    rule), and a five-window contig that straddles the slabs of a small launch size: 11 windows"""
    rng = np.random.default_rng(31)
    acgt = lambda k: "".join(rng.choice(list("ACGT"), k))          # noqa: E731
    recs = [acgt(2000), acgt(8500), "", acgt(6000) + "N" * 6000 + acgt(3000), acgt(29000)]
    seq = np.frombuffer("".join(recs).encode(), dtype=np.uint8).copy()
    return seq, np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)


def test_contig_path_is_its_definitions_under_two_launch_sizes(synth_weights, engine):
    from genomad_amd.engine import AttributionResult, NNEngine
    seq, offsets = _small_contigs()
    starts, lens, ids, _ = sequence.candidate_spans(offsets)
    wins = sequence.materialize_spans(seq, starts, lens)
    assert len(starts) == 11 and list(lens[1:3]) == [6000, 2500] and (wins[4] == ord("N")).all()
    results = []
    with NNEngine(0, synth_weights, chunk=2) as e2:                      # slabs of 8 windows: the last contig straddles them
        assert ids[7] == ids[8]
        for chunk, bin_ in ((2, 8), (3, 8), (2, 1)):
            e2.lib.gnn_set_chunk(e2.ctx, chunk)
            res = e2.attribute_contigs(seq, offsets, bin_, False, "f16x3tc")
            results.append(res)
            assert tuple(res.asdict()) == AttributionResult.FIELDS and res.bin == bin_
            contrib, bias, logits, scores = e2.attribute(wins, bin_, "f16x3tc")
            assert np.array_equal(res.contrib, contrib) and np.array_equal(res.bias, bias) and np.array_equal(res.logits, logits)
            scan = e2.scan_contigs(seq, offsets, 6000, False, "f16x3tc")
            assert np.array_equal(res.window_scores, scan.scores) and np.array_equal(res.window_scores, scores)
            assert np.array_equal(res.kept, scan.kept) and res.kept.dtype == np.bool_ and not res.kept[4] and res.kept.sum() == 10
            for k in ("win_offsets", "starts", "lens"):
                assert np.array_equal(getattr(res, k), getattr(scan, k)) and getattr(res, k).dtype == getattr(scan, k).dtype, k
            cs, kept_ids = e2.classify_contigs(seq, offsets, False, "f16x3tc")
            assert np.array_equal(res.contig_scores, cs) and np.array_equal(ids[res.kept], kept_ids)
            assert not res.contig_scores[2].any()                        # the empty record
        dev = e2.alloc(seq.nbytes)
        try:
            dev.upload(seq)
            on_dev = e2.attribute_contigs_dev(dev.ptr, offsets, 8, False, "f16x3tc")
        finally:
            dev.free()
    for k in AttributionResult.FIELDS:
        assert np.array_equal(getattr(results[0], k), getattr(results[1], k)), k          # two launch sizes
        assert np.array_equal(getattr(results[0], k), getattr(on_dev, k)), k              # wherever the sequence lives
    whole = engine.attribute_contigs(seq, offsets, 8, False, "f16x3tc")                   # and the default launch size
    assert np.array_equal(whole.contrib, results[0].contrib) and np.array_equal(whole.bias, results[0].bias)
    assert np.array_equal(results[2].contrib.shape, (11, 2, 749, 3)) and np.array_equal(R.binned(results[2].contrib, 8), whole.contrib)
    single = engine.attribute_contigs(seq, offsets, 8, True, "f16x3tc")
    assert len(single.contrib) == 4 and np.array_equal(single.contrib, whole.contrib[[0, 1, 3, 6]])


def test_attribution_errors_leave_the_ctx_usable(engine):
    bases, _ = R.reference_32()
    seq, offsets = _small_contigs()
    with pytest.raises(_lib.GnnError, match="f16c6"):
        engine.attribute(bases[:2], 1, "f16c6")
    with pytest.raises(_lib.GnnError, match="f16c6"):
        engine.attribute_contigs(seq, offsets, 8, False, "f16c6")
    for bad in (0, 750):
        with pytest.raises(_lib.GnnError, match=r"\[1, 749\]"):
            engine.attribute(bases[:2], bad)
        with pytest.raises(_lib.GnnError, match=r"\[1, 749\]"):
            engine.attribute_contigs(seq, offsets, bad)
    contrib = np.zeros((11, 2, 94, 3), np.float32)
    call = lambda cap: engine.lib.gnn_attribute_contigs(                                   # noqa: E731
        engine.ctx, seq.ctypes.data, 1, seq.nbytes, offsets.ctypes.data, len(offsets) - 1, 8, 0, _lib.PRECISIONS["f16x3tc"],
        contrib.ctypes.data, cap, None, None, None, None, None)
    assert call(10) == _lib.ERR_ARG and b"11" in engine.lib.gnn_last_error() and not contrib.any()
    assert call(11) == 0                                                # every optional output may be NULL
    assert np.array_equal(contrib, engine.attribute_contigs(seq, offsets, 8).contrib)
    empty = engine.attribute_contigs(np.zeros(0, np.uint8), np.array([0, 0, 0]), 8)
    assert empty.contrib.shape == (0, 2, 94, 3) and not empty.contig_scores.any() and len(empty.win_offsets) == 3


# ---- main() -------------------------------------------------------------------------------------------------------------------
def test_main_writes_the_attribution_map_only_when_asked(engine, synth_weights, tmp_path, monkeypatch):
    from genomad_amd.engine import AttributionResult
    nnc = _setup_main(tmp_path, monkeypatch, engine, synth_weights)
    fa = Path(ROOT) / "tests" / "golden" / "fasta_fixture.fna.gz"
    for k in ("GENOMAD_AMD_STRAND", "GENOMAD_AMD_SCAN_STRIDE", "GENOMAD_AMD_EMBEDDINGS", "GENOMAD_AMD_OCCLUSION_BLOCK",
              "GENOMAD_AMD_ATTRIBUTION_BIN", "GENOMAD_AMD_FRONT_END"):
        monkeypatch.delenv(k, raising=False)
    nnc.main(fa, tmp_path / "off", False, 128, False, 1, False, False)
    monkeypatch.setenv("GENOMAD_AMD_ATTRIBUTION_BIN", "8")
    nnc.main(fa, tmp_path / "on", False, 128, False, 1, False, False)
    prefix = sequence.prefix_of(fa)
    d_off, d_on = tmp_path / "off" / f"{prefix}_nn_classification", tmp_path / "on" / f"{prefix}_nn_classification"
    files = lambda d: sorted(str(p.relative_to(d)) for p in d.rglob("*"))      # noqa: E731
    assert files(d_on) == sorted(files(d_off) + [f"{prefix}_nn_attribution.npz"])
    for rel in (f"{prefix}_nn_classification.npz", f"{prefix}_encoded_sequences/{prefix}_seq_window_id.npz"):
        a, b = np.load(d_off / rel), np.load(d_on / rel)
        assert sorted(a.files) == sorted(b.files) and all(a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]) for k in a.files)
    assert (d_off / f"{prefix}_nn_classification.tsv").read_bytes() == (d_on / f"{prefix}_nn_classification.tsv").read_bytes()
    names, seq, off = sequence.read_fasta_packed(fa, True)
    want = engine.attribute_contigs(seq, off, 8, False, "f16x3tc").asdict()
    z = np.load(d_on / f"{prefix}_nn_attribution.npz")
    assert sorted(z.files) == sorted(("contig_names",) + AttributionResult.FIELDS) and list(z["contig_names"]) == list(names)
    assert int(z["bin"]) == 8 and z["contrib"].shape == (len(want["starts"]), 2, 94, 3)
    for k in AttributionResult.FIELDS[1:]:
        assert z[k].dtype == want[k].dtype and np.array_equal(z[k], want[k]), k
    assert np.array_equal(z["contig_scores"], np.load(d_on / f"{prefix}_nn_classification.npz")["predictions"])
