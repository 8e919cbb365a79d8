"""Interval embeddings on the MI355X: the fold kernels on rows of the test's choosing, the pass against the
fold of embed(), the fp64 oracle, invariance under the launch size / where seq lives / call order, the ties to embed_contigs and
classify_contigs, the strand modes, the errors, embed_regions and main() with GENOMAD_AMD_REGION_EMBEDDINGS.

The coherence bound (COH_TOL = 1e-5 absolute against the float64 definition, intervals of at most 64 kept members), derived:
with eps = 2^-24 (float32 rounding to nearest) and n kept members,

- the squared norm of a row is 4 products and 3 additions in a lane, 6 butterfly levels inside a wave and one addition between the
  two waves: all terms are non-negative, so its relative error is at most (1 + 3 + 6 + 1) eps = 11 eps; rsqrt halves that and adds
  its own error of at most 1 ulp = 2 eps, the product with the element one more eps: a unit row is off by at most
  (5.5 + 2 + 1) eps < 9 eps of its own length 1;
- the n unit rows are added one after the other: addition i rounds a partial sum of length at most i, so the sum is off by at most
  (1 + 2 + ... + n) eps = n (n + 1) / 2 eps; together with the rows' own errors |dU| <= (9 n + n (n + 1) / 2) eps, and after the
  division by n the coherence is off by (9 + (n + 1) / 2) eps;
- the final norm (11 eps as above, halved by the square root, plus the root's and the division's rounding) adds at most 8 eps of
  a value <= 1.

Together (17 + (n + 1) / 2) eps: 49.5 eps = 3.0e-6 at n = 64.  The issue's own estimate is (n + 12) eps = 4.6e-6; the tolerance is
about twice the larger of the two.  It was written down before the kernel ran."""
import functools

import numpy as np
import pytest

from genomad_amd import _lib, sequence
from oracle import igloo_oracle, sequence_oracle
from tests.conftest import need_tables
from tests.test_embeddings_gpu import EMB_TOL, _contigs, _fasta, _setup_main

pytestmark = pytest.mark.gpu

STRIDE = 2000
COH_TOL = 1e-5
INTERVALS = [(1, 0, 9000), (1, 9000, 9000), (1, 9000, 20000), (1, 26000, 33000), (2, 0, 19000), (3, 0, 100), (5, 0, 9000),
             (5, 9000, 18000), (6, 0, 1000), (6, 1000, 31000), (6, 31000, 31500), (6, 31500, 70000), (9, 0, 13000)]
MEMBERS = [3, 0, 6, 3, 8, 1, 3, 4, 0, 14, 1, 18, 5]
KEPT = [3, 0, 6, 3, 7, 1, 3, 3, 0, 14, 1, 18, 4]


@functools.lru_cache(maxsize=None)
def _fixture():
    """the shared contigs at stride 2000, the interval list, its member ranges, the N rule's mask and the materialised windows"""
    seq, offsets = _contigs()
    contig, start, end = (np.array(x, dtype=np.int64) for x in zip(*INTERVALS))
    starts, lens, ids, window_n, win_off, _ = sequence.scan_spans(offsets, STRIDE)
    n_count = np.array([np.count_nonzero(seq[a:a + l] == ord("N")) for a, l in zip(starts, lens)])
    kept = (window_n == 0) | (n_count <= sequence.MAX_N)
    w_lo, w_hi = sequence.interval_windows(offsets, STRIDE, contig, start, end)
    wins = sequence.materialize_spans(seq, starts, lens)
    return dict(seq=seq, offsets=offsets, contig=contig, start=start, end=end, starts=starts, lens=lens, kept=kept, w_lo=w_lo,
                w_hi=w_hi, wins=wins)


def _iv(fx):
    return fx["contig"], fx["start"], fx["end"]


def _same(got, want, coherence=True):
    """embedding, scores and count bit for bit; coherence within the derived bound of the float64 definition"""
    assert np.array_equal(got["count"], want["count"])
    assert np.array_equal(got["embedding"], want["embedding"])
    assert np.array_equal(got["scores"], want["scores"])
    if coherence:
        d = np.abs(got["coherence"].astype(np.float64) - want["coherence"]).max()
        assert d <= COH_TOL, d


def _as_dict(r):
    return {k: getattr(r, k) for k in ("count", "embedding", "scores", "coherence")}


def test_the_fixture_is_what_the_issue_counted():
    """in numpy, before anything is asked of the device: an empty interval, intervals without a member, a gap, masked members, a
    one-window interval, and one that crosses two slab boundaries at 4 windows per launch"""
    fx = _fixture()
    assert len(fx["starts"]) == 75 and int(fx["kept"].sum()) == 72
    assert list(fx["w_hi"] - fx["w_lo"]) == MEMBERS
    assert [int(fx["kept"][a:b].sum()) for a, b in zip(fx["w_lo"], fx["w_hi"])] == KEPT
    inside = np.zeros(75, bool)
    for a, b in zip(fx["w_lo"], fx["w_hi"]):
        inside[a:b] = True
    assert int((fx["kept"] & ~inside).sum()) == 9
    assert (fx["w_lo"][11], fx["w_hi"][11]) == (47, 65) and 47 < 48 and 64 < 65        # global windows 47-64: slabs of 16 cut it twice
    assert max(KEPT) <= 64                                                             # the coherence bound's premise


def test_fold_on_chosen_rows(engine):
    fx = _fixture()
    rng = np.random.default_rng(31)
    rows = rng.standard_normal((75, 512)).astype(np.float32) * np.exp2(rng.integers(-3, 4, size=(75, 1))).astype(np.float32)
    scores = rng.random((75, 3), dtype=np.float32)
    want = sequence.interval_embeddings(rows, scores, fx["kept"], fx["w_lo"], fx["w_hi"])
    live = want["count"] > 0
    spread = want["coherence"][live].max() - want["coherence"][live].min()
    print(f"\ncoherence of signed random rows: {np.round(want['coherence'], 3)}")
    assert spread > 0.3, spread
    got = engine.fold_intervals(rows, fx["kept"], fx["w_lo"], fx["w_hi"], scores)
    print(f"max |coherence - float64| = {np.abs(got['coherence'] - want['coherence']).max():.3e}")
    _same(got, want)
    assert got["coherence"].dtype == np.float32 and not got["coherence"][~live].any() and not got["embedding"][~live].any()
    for per_call in (5, 16):                       # slices: every output, coherence included, bit for bit
        part = engine.fold_intervals(rows, fx["kept"], fx["w_lo"], fx["w_hi"], scores, rows_per_call=per_call)
        for k in ("count", "embedding", "scores", "coherence"):
            assert np.array_equal(part[k], got[k]), (per_call, k)
    none = engine.fold_intervals(rows, fx["kept"], fx["w_lo"], fx["w_hi"])                # without scores
    assert np.array_equal(none["embedding"], got["embedding"]) and np.array_equal(none["coherence"], got["coherence"])
    assert not none["scores"].any()


def test_fold_zero_and_non_finite_rows_add_nothing_to_u(engine):
    fx = _fixture()
    rng = np.random.default_rng(32)
    rows = rng.standard_normal((75, 512)).astype(np.float32)
    base = engine.fold_intervals(rows, fx["kept"], fx["w_lo"], fx["w_hi"])
    # interval 9 is windows 25 .. 38, all kept: a zero row, a row with an inf and a row with a NaN among them
    lo = int(fx["w_lo"][9])
    odd = rows.copy()
    odd[lo + 1] = 0.0
    odd[lo + 4, 7] = np.inf
    odd[lo + 9, 500] = np.nan
    want = sequence.interval_embeddings(odd, None, fx["kept"], fx["w_lo"], fx["w_hi"])
    got = engine.fold_intervals(odd, fx["kept"], fx["w_lo"], fx["w_hi"])
    assert np.array_equal(got["count"], base["count"])                                  # kept decides the count, not the row
    assert np.abs(got["coherence"].astype(np.float64) - want["coherence"]).max() <= COH_TOL
    assert np.isfinite(got["coherence"]).all()
    assert np.array_equal(got["embedding"], want["embedding"], equal_nan=True)
    others = np.arange(len(fx["w_lo"])) != 9
    assert np.array_equal(got["embedding"][others], base["embedding"][others])
    # U of interval 9 is the sum over the 11 ordinary rows alone
    keep = fx["kept"].copy()
    keep[[lo + 1, lo + 4, lo + 9]] = False
    u11 = sequence.interval_embeddings(rows, None, keep, fx["w_lo"], fx["w_hi"])["coherence"][9] * 11
    assert abs(float(got["coherence"][9]) * 14 - u11) <= 14 * COH_TOL
    same = np.tile(rows[:1], (75, 1))                                                  # identical rows: coherence 1
    one = engine.fold_intervals(same, fx["kept"], fx["w_lo"], fx["w_hi"])
    assert np.abs(one["coherence"][one["count"] > 0] - 1.0).max() <= COH_TOL


@pytest.mark.parametrize("prec", ["f32", "bf16x3", "f16x3tc", "f16x3tk"])
def test_the_pass_equals_the_fold_of_embed(engine, prec, request):
    need_tables(request, prec)
    fx = _fixture()
    rows, scores = engine.embed(fx["wins"], prec, with_scores=True)
    want = sequence.interval_embeddings(rows, scores, fx["kept"], fx["w_lo"], fx["w_hi"])
    got = engine.embed_intervals(fx["seq"], fx["offsets"], STRIDE, *_iv(fx), precision=prec)
    print(f"\n{prec}: coherence {np.round(got.coherence, 4)}; max |d| to float64 {np.abs(got.coherence - want['coherence']).max():.3e}")
    _same(_as_dict(got), want)
    assert np.array_equal(got.w_lo, fx["w_lo"]) and np.array_equal(got.w_hi, fx["w_hi"])
    assert list(got.count) == KEPT and got.stride == STRIDE and got.strand == "forward"
    assert got.embedding[got.count > 0].any(axis=1).all()


@pytest.fixture(scope="module")
def oracle_rows(synth_weights):
    """fp64 oracle h1 of the fixture's 75 windows"""
    tokens = sequence_oracle.tokenize_closed_form(_fixture()["wins"])
    return np.concatenate([igloo_oracle.forward(tokens[a:a + 16], synth_weights, np.float64, literal=False, return_taps=True)[1]["h1"]
                           for a in range(0, len(tokens), 16)])


def test_interval_means_match_the_fp64_oracle(engine, oracle_rows):
    fx = _fixture()
    got = engine.embed_intervals(fx["seq"], fx["offsets"], STRIDE, *_iv(fx))
    worst = 0.0
    for i, (a, b) in enumerate(zip(fx["w_lo"], fx["w_hi"])):
        sel = np.arange(a, b)[fx["kept"][a:b]]
        if not len(sel):
            assert not got.embedding[i].any()
            continue
        h1 = oracle_rows[sel]
        err = np.abs(got.embedding[i].astype(np.float64) - h1.mean(axis=0)).max() / max(1.0, np.abs(h1).max())
        worst = max(worst, err)
    print(f"\ninterval means vs fp64 oracle: max |d| / max(1, max|h1|) = {worst:.3e}")
    assert worst <= EMB_TOL, worst


def test_results_do_not_depend_on_launch_size_residence_or_call_order(synth_weights, engine):
    from genomad_amd.engine import NNEngine
    fx = _fixture()
    args = (fx["offsets"], STRIDE, *_iv(fx))
    ref = _as_dict(engine.embed_intervals(fx["seq"], *args))
    with NNEngine(0, synth_weights, chunk=4) as e2:              # slabs of 16 windows: interval 11 crosses two boundaries
        runs = [_as_dict(e2.embed_intervals(fx["seq"], *args))]
        for chunk in (64, 13):
            e2.lib.gnn_set_chunk(e2.ctx, chunk)
            runs.append(_as_dict(e2.embed_intervals(fx["seq"], *args)))
        runs.append(_as_dict(e2.embed_intervals(fx["seq"], *args, strand="both")))
    both = _as_dict(engine.embed_intervals(fx["seq"], *args, strand="both"))
    for r in runs[:3]:
        for k, v in ref.items():
            assert np.array_equal(r[k], v), k
    for k, v in both.items():
        assert np.array_equal(runs[3][k], v), k
    dev = engine.alloc(fx["seq"].nbytes)
    try:
        dev.upload(fx["seq"])
        on_dev = _as_dict(engine.embed_intervals_dev(dev.ptr, *args))
    finally:
        dev.free()
    engine.scan_contigs(fx["seq"], fx["offsets"], 3000)          # an unrelated call in between: another window table
    after = _as_dict(engine.embed_intervals(fx["seq"], *args))
    for r in (on_dev, after):
        for k, v in ref.items():
            assert np.array_equal(r[k], v), k


def test_whole_contigs_at_stride_6000_are_embed_contigs_and_classify_contigs(engine):
    fx = _fixture()
    seq, offsets = fx["seq"], fx["offsets"]
    n = len(offsets) - 1
    got = engine.embed_intervals(seq, offsets, 6000, np.arange(n), np.zeros(n, np.int64), np.diff(offsets))
    scores, emb, ids = engine.embed_contigs(seq, offsets)
    assert np.array_equal(got.embedding, emb)
    assert np.array_equal(got.scores, engine.classify_contigs(seq, offsets)[0]) and np.array_equal(got.scores, scores)
    assert np.array_equal(got.count, np.bincount(ids, minlength=n))
    fwd = engine.embed_intervals(seq, offsets, 6000, np.arange(n), np.zeros(n, np.int64), np.diff(offsets), strand="forward")
    for k, v in _as_dict(got).items():
        assert np.array_equal(getattr(fwd, k), v), k
    s_both, ids_b, e_both, _, _ = engine._classify_contigs(seq, offsets, False, _lib.DEFAULT_PRECISION, embed=True, strand="both")
    both = engine.embed_intervals(seq, offsets, 6000, np.arange(n), np.zeros(n, np.int64), np.diff(offsets), strand="both")
    assert np.array_equal(both.embedding, e_both) and np.array_equal(both.scores, s_both)


def test_strand_modes_against_the_numpy_definition(engine):
    fx = _fixture()
    n = len(fx["starts"])
    rows_f, sc_f = engine.embed(fx["wins"], with_scores=True)
    bufs = [engine.alloc(fx["seq"].nbytes), engine.alloc(n * _lib.WINDOW), engine.alloc(n * 512 * 4), engine.alloc(n * 3 * 4)]
    try:
        bufs[0].upload(fx["seq"])
        engine.revcomp_spans_dev(bufs[0].ptr, fx["starts"], fx["lens"], bufs[1].ptr)
        engine.embed_dev(bufs[1].ptr, n, bufs[2].ptr, scores_ptr=bufs[3].ptr)
        engine.sync()
        rows_r, sc_r = bufs[2].download((n, 512), np.float32), bufs[3].download((n, 3), np.float32)
    finally:
        for b in bufs:
            b.free()
    assert not np.array_equal(rows_r, rows_f)
    args = (fx["seq"], fx["offsets"], STRIDE, *_iv(fx))
    rev = engine.embed_intervals(*args, strand="reverse")
    _same(_as_dict(rev), sequence.interval_embeddings(rows_r, sc_r, fx["kept"], fx["w_lo"], fx["w_hi"]))
    both = engine.embed_intervals(*args, strand="both")
    _same(_as_dict(both), sequence.interval_embeddings(rows_f, sequence.strand_mean(sc_f, sc_r), fx["kept"], fx["w_lo"], fx["w_hi"],
                                                       rows_rev=rows_r))
    assert both.strand == "both" and list(both.count) == KEPT and list(rev.count) == KEPT
    none = engine.embed_intervals(*args)
    fwd = engine.embed_intervals(*args, strand="forward")
    for k, v in _as_dict(none).items():
        assert np.array_equal(getattr(fwd, k), v), k


def test_errors(engine):
    fx = _fixture()
    args = (fx["seq"], fx["offsets"], STRIDE)
    with pytest.raises(_lib.GnnError, match="F16C6"):
        engine.embed_intervals(*args, *_iv(fx), precision="f16c6")
    start = fx["start"].copy()
    start[7] = 8000                                               # reaches back into interval 6
    with pytest.raises(_lib.GnnError, match=r"error -1: gnn_embed_intervals: interval 7 .*overlaps interval 6"):
        engine.embed_intervals(*args, fx["contig"], start, fx["end"])
    end = fx["end"].copy()
    end[12] = 13001
    with pytest.raises(_lib.GnnError, match=r"interval 12 .*beyond its contig of 13000"):
        engine.embed_intervals(*args, fx["contig"], fx["start"], end)
    with pytest.raises(_lib.GnnError, match="strand 7"):
        engine.embed_intervals(*args, *_iv(fx), strand=7)
    with pytest.raises(_lib.GnnError, match=r"stride 6001"):
        engine.embed_intervals(fx["seq"], fx["offsets"], 6001, *_iv(fx))
    empty = engine.embed_intervals(*args, [], [], [])
    assert empty.embedding.shape == (0, 512) and empty.count.shape == (0,)
    rows = np.ones((4, 512), np.float32)
    with pytest.raises(_lib.GnnError, match=r"gnn_interval_fold_dev: interval 1 "):
        engine.fold_intervals(rows, np.ones(4, bool), [0, 1], [2, 3])               # ranges that overlap


# ---- embed_regions and main() -------------------------------------------------------------------------------------------------
MAIN_SWITCHES = ("GENOMAD_AMD_EMBEDDINGS", "GENOMAD_AMD_SCAN_STRIDE", "GENOMAD_AMD_STRAND", "GENOMAD_AMD_REGION_PENALTY",
                 "GENOMAD_AMD_REGION_EMBEDDINGS", "GENOMAD_AMD_PRECISION", "GENOMAD_AMD_FRONT_END")


def _files(d):
    return sorted(str(p.relative_to(d)) for p in d.rglob("*") if p.is_file())


def test_embed_regions_and_main_write_the_regions_rows(engine, synth_weights, tmp_path, monkeypatch):
    nnc = _setup_main(tmp_path, monkeypatch, engine, synth_weights)
    for k in MAIN_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    fa = tmp_path / "m.fna"
    _fasta(fa)
    names, seq, off = sequence.read_fasta_packed(fa)
    scan, reg = engine.scan_regions(seq, off, STRIDE, 0.05, precision="f16x3tc")
    want = engine.embed_regions(seq, off, reg, precision="f16x3tc")
    direct = engine.embed_intervals(seq, off, STRIDE, reg.region_contig, reg.start, reg.end, precision="f16x3tc")
    assert len(want.count) == len(reg.start) > len(names) and np.array_equal(want.embedding, direct.embedding)
    assert np.array_equal(want.contig, reg.region_contig) and np.array_equal(want.start, reg.start) and want.stride == STRIDE
    assert int(want.count.sum()) <= int(scan.kept.sum()) and want.count.max() <= 64
    with pytest.raises(ValueError, match="no base coordinates"):
        engine.embed_regions(seq, off, engine.call_regions(scan.track, scan.bin_offsets, 0.05))
    monkeypatch.setenv("GENOMAD_AMD_SCAN_STRIDE", str(STRIDE))
    monkeypatch.setenv("GENOMAD_AMD_REGION_PENALTY", "0.05")
    nnc.main(fa, tmp_path / "off", False, 128, False, 1, False, False)
    monkeypatch.setenv("GENOMAD_AMD_REGION_EMBEDDINGS", "1")
    nnc.main(fa, tmp_path / "on", False, 128, False, 1, False, False)
    d_off, d_on = tmp_path / "off" / "m_nn_classification", tmp_path / "on" / "m_nn_classification"
    assert _files(d_on) == sorted(_files(d_off) + ["m_nn_region_embeddings.npz"])
    for rel in _files(d_off):                                       # every other file: what a run without the switch writes
        if rel.endswith(".npz"):
            a, b = np.load(d_off / rel), np.load(d_on / rel)
            assert sorted(a.files) == sorted(b.files), rel
            assert all(a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f") for k in a.files), rel
        elif rel.endswith(".tsv"):
            assert (d_off / rel).read_bytes() == (d_on / rel).read_bytes(), rel
    z, rz = np.load(d_on / "m_nn_region_embeddings.npz"), np.load(d_on / "m_nn_regions.npz")
    assert sorted(z.files) == sorted(["contig_names", "contig", "start", "end", "state", "embedding", "count", "coherence", "scores",
                                      "stride", "penalty", "strand"])
    assert list(z["contig_names"]) == list(names)
    for mine, theirs in (("contig", "region_contig"), ("start", "start"), ("end", "end"), ("state", "region_state")):
        assert np.array_equal(z[mine], rz[theirs]) and np.array_equal(z[mine], getattr(reg, theirs))
    assert np.array_equal(z["embedding"], want.embedding) and z["embedding"].dtype == np.float32
    assert np.array_equal(z["count"], want.count) and np.array_equal(z["coherence"], want.coherence)
    assert np.array_equal(z["scores"], want.scores)
    assert (int(z["stride"]), float(z["penalty"]), str(z["strand"])) == (STRIDE, 0.05, "forward")
    print(f"\ncoherence of the {len(z['count'])} regions of the test contigs: {np.round(z['coherence'], 3)}; members {z['count']}")


def test_main_region_embeddings_provirus_pass_and_resume(engine, synth_weights, tmp_path, monkeypatch):
    import json
    nnc = _setup_main(tmp_path, monkeypatch, engine, synth_weights)
    for k in MAIN_SWITCHES:
        monkeypatch.delenv(k, raising=False)
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
    calls = []
    real = type(engine).embed_intervals
    monkeypatch.setattr(type(engine), "embed_intervals", lambda self, *a, **k: calls.append(1) or real(self, *a, **k))
    run = lambda: nnc.main(fa, out, False, 128, False, 1, False, False)       # noqa: E731
    d = out / "v_nn_classification"
    monkeypatch.setenv("GENOMAD_AMD_SCAN_STRIDE", "3000")
    monkeypatch.setenv("GENOMAD_AMD_REGION_PENALTY", "0.05")
    run()                                                           # regions, no embeddings of them ...
    assert not calls and not (d / "v_nn_region_embeddings.npz").exists()
    monkeypatch.setenv("GENOMAD_AMD_REGION_EMBEDDINGS", "1")
    run()                                                           # ... then asked for them: both stages run again
    assert len(calls) == 2
    z, pz = np.load(d / "v_nn_region_embeddings.npz"), np.load(d / "v_provirus_nn_region_embeddings.npz")
    prz = np.load(d / "v_provirus_nn_regions.npz")
    assert list(pz["provirus_names"]) == ["k1|provirus_1_9000", "k2|provirus_5_3000"]
    assert np.array_equal(pz["start"], prz["start"]) and pz["embedding"].shape == (len(prz["start"]), 512)
    first = z["embedding"].copy()
    run()
    assert len(calls) == 2                                          # same request, everything there: nothing runs
    for env, value in (("GENOMAD_AMD_REGION_PENALTY", "0"), ("GENOMAD_AMD_STRAND", "both"), ("GENOMAD_AMD_SCAN_STRIDE", "2000")):
        n = len(calls)
        monkeypatch.setenv(env, value)
        run()
        assert len(calls) == n + 2, env
        z = np.load(d / "v_nn_region_embeddings.npz")
        assert (int(z["stride"]), float(z["penalty"]), str(z["strand"])) == (
            nnc.scan_stride_requested(), nnc.region_penalty_requested(), nnc.strand_requested()), env
        assert np.array_equal(z["start"], np.load(d / "v_nn_regions.npz")["start"])
    assert z["embedding"].shape != first.shape or not np.array_equal(z["embedding"], first)
    n = len(calls)
    monkeypatch.delenv("GENOMAD_AMD_REGION_EMBEDDINGS")
    run()                                                           # no request: the files go, the regions stay
    assert len(calls) == n and not (d / "v_nn_region_embeddings.npz").exists() and not (d / "v_provirus_nn_region_embeddings.npz").exists()
    assert (d / "v_nn_regions.npz").exists()
