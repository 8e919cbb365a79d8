"""The interval fold at its limits on the MI355X: the inputs of tests/interval_limits_data.py - ranges of
every length against every position of the 8-row batch, runs of empty ranges on slab edges, poison in rows no sum may see, 2000
dependent steps, rows from all-subnormal to FLT_MAX, the second strand on rows of the test's choosing - and the pass over a 2 Mbp
contig at stride 1000.  Count, embedding and scores are compared bit for bit with the numpy definition (the sums are sequential f32
sums in both), the coherence with the float64 definition within ``coh_tol(n)``, the bound derived in interval_limits_data before
the device was run; tests/test_interval_limits_host.py shows what that tolerance can and cannot hide.

On the kernel before the row-scale rule (a unit row only when the plain f32 squared norm was in (0, FLT_MAX]) test_scales failed and
nothing else here did.  It returned the coherence 0 for "huge" and for "subnormal" (float64: 0.2088), 0.6 for "five_scales" (1.0:
the members at 2^-140 and 2^120 had no unit row), 0.5 for "opposite_0_100" and "opposite_-100_0" (0: one of the two rows was
dropped) and 0 for the one-hot rows 2^-149, 2^-126, 2^64 and 2^127 (1); "opposite_60_-60" (0) and the one-hot rows 2^-64, 2^-63,
1 and 2^63 (1) were right."""
import functools

import numpy as np
import pytest

from genomad_amd import _lib, sequence
from tests import interval_limits_data as lim

pytestmark = pytest.mark.gpu


def _fold(engine, fx, **kw):
    kw.setdefault("scores", fx["scores"])
    return engine.fold_intervals(fx["rows"], fx["kept"], fx["w_lo"], fx["w_hi"], **kw)


def _coherence(got, want, what, strands=1):
    """max |coherence - float64| over the intervals, printed, each within coh_tol of its own count"""
    d = np.abs(np.asarray(got["coherence"], np.float64) - want["coherence"])
    tol = np.array([lim.coh_tol(int(n), strands) for n in want["count"]])
    at = int(np.argmax(d / tol))
    print(f"{what}: max |coherence - float64| = {d.max():.3e}; nearest the bound at count {int(want['count'][at])}: "
          f"{d[at]:.3e} of coh_tol = {tol[at]:.3e}")
    assert np.isfinite(np.asarray(got["coherence"])).all() and (d <= tol).all(), (what, at, d[at], tol[at])
    return float(d.max())


def _same(got, want, what, strands=1, equal_nan=False):
    """count, embedding and scores bit for bit, coherence (float32) within the derived bound of the float64 definition"""
    assert np.array_equal(got["count"], want["count"]), what
    assert np.array_equal(got["embedding"], want["embedding"], equal_nan=equal_nan), what
    assert np.array_equal(got["scores"], want["scores"]), what
    assert np.asarray(got["coherence"]).dtype == np.float32
    return _coherence(got, want, what, strands)


def _identical(got, ref, what):
    for k in lim.KEYS:
        assert np.array_equal(got[k], ref[k], equal_nan=True), (what, k)


@functools.lru_cache(maxsize=None)
def _cuts_definition():
    return lim.definition(lim.cuts())


@pytest.fixture(scope="module")
def cuts_on_device(engine):
    """the unsliced fold of ``cuts``: the reference of the slices and of the empty runs"""
    return _fold(engine, lim.cuts())


def test_cuts(engine, cuts_on_device):
    print()
    fx, want = lim.cuts(), _cuts_definition()
    _same(cuts_on_device, want, "cuts")
    dead = want["count"] == 0
    assert dead.sum() >= 2 and not cuts_on_device["embedding"][dead].any() and not cuts_on_device["coherence"][dead].any()
    none = _fold(engine, fx, scores=None)
    for per_call in (1, 7, 8, 9, 64):
        _identical(_fold(engine, fx, rows_per_call=per_call), cuts_on_device, per_call)
        part = _fold(engine, fx, scores=None, rows_per_call=per_call)
        _identical(part, none, per_call)
    for k in ("count", "embedding", "coherence"):
        assert np.array_equal(none[k], cuts_on_device[k]), k
    assert not none["scores"].any()


@pytest.mark.parametrize("per_call", [None, 8, 1])
def test_empty_runs(engine, cuts_on_device, per_call):
    wide = lim.with_empty_runs(lim.cuts())
    got = _fold(engine, wide, rows_per_call=per_call)
    for k in lim.KEYS:
        assert np.array_equal(got[k][wide["index"]], cuts_on_device[k]), k
        assert not np.delete(got[k], wide["index"], axis=0).any(), k         # exact zeros, count 0


def test_poison_in_rows_no_sum_may_see(engine):
    print()
    fx = lim.cuts()
    bad, clean = lim.poisoned(fx), lim.poison_free(fx)
    ref = _fold(engine, clean)
    _same(ref, lim.definition(clean), "poison_free")
    for per_call in (None, 1, 8):
        got = _fold(engine, bad, rows_per_call=per_call)
        assert all(np.isfinite(got[k]).all() for k in lim.KEYS), per_call
        for k in lim.KEYS:
            assert np.array_equal(got[k], ref[k]), (per_call, k)


@pytest.mark.parametrize("length", lim.ODD_LAST_ROW)
def test_a_zero_an_inf_and_a_nan_in_the_last_row_of_a_range(engine, cuts_on_device, length):
    """the kept-row cases of test_fold_zero_and_non_finite_rows_add_nothing_to_u where the batch ends: the last row of a range of
    length 9 is the row the clamped prefetch repeats, that of a range of length 16 the last of a full batch"""
    print()
    fx = lim.cuts()
    i = length                                                       # range i has length i
    last = int(fx["w_hi"][i]) - 1
    assert fx["w_hi"][i] - fx["w_lo"][i] == length and fx["kept"][last]
    others = np.arange(lim.N_RANGES) != i
    for what in ("zero", "inf", "nan"):
        odd = dict(fx, rows=fx["rows"].copy())
        if what == "zero":
            odd["rows"][last] = 0.0
        else:
            odd["rows"][last, 77] = np.inf if what == "inf" else np.nan
        want = lim.definition(odd)
        for per_call in (None, 8):
            got = _fold(engine, odd, rows_per_call=per_call)
            _same(got, want, f"length {length}, {what} in the last row, rows_per_call {per_call}", equal_nan=True)
            assert np.array_equal(got["count"], cuts_on_device["count"])
            for k in lim.KEYS:
                assert np.array_equal(got[k][others], cuts_on_device[k][others]), (what, k)
        # U is the sum over the other kept members alone
        keep = fx["kept"].copy()
        keep[last] = False
        fewer = lim.definition(dict(fx, kept=keep))
        n = int(want["count"][i])
        assert abs(float(got["coherence"][i]) * n - fewer["coherence"][i] * (n - 1)) <= n * lim.coh_tol(n)


@pytest.mark.parametrize("kind,n,thirds", [(kind, n, thirds) for kind, n, thirds, _ in lim.long_ranges()])
def test_long_ranges(engine, kind, n, thirds):
    print()
    fx = next(f for k, m, t, f in lim.long_ranges() if (k, m, t) == (kind, n, thirds))
    want = lim.definition(fx)
    got = _fold(engine, fx)
    _same(got, want, f"{kind}, {int(want['count'][0])} kept of {n}")
    _identical(_fold(engine, fx, rows_per_call=52), got, 52)


def test_scales(engine):
    print()
    fx = lim.scaled()
    want = lim.definition(fx)
    got = _fold(engine, fx)
    coh = lambda name: float(got["coherence"][lim.interval(fx, name)])       # noqa: E731
    for name in ("huge", "subnormal", "five_scales", *(f"opposite_{a}_{b}" for a, b in lim.OPPOSITE),
                 *(f"one_hot_{k}_{s}" for k in lim.ONE_HOT_K for s in "+-")):
        i = lim.interval(fx, name)
        print(f"{name}: coherence {coh(name):.7f}, float64 {want['coherence'][i]:.7f}, unscaled twin {coh(fx['twin_of'][name]):.7f}")
    _same(got, want, "scaled", equal_nan=True)
    assert not np.isfinite(got["embedding"][lim.interval(fx, "huge")]).all()         # S overflows there; U does not
    for name, twin in fx["twin_of"].items():
        n = int(want["count"][lim.interval(fx, name)])
        assert abs(coh(name) - coh(twin)) <= lim.coh_tol(n), (name, coh(name), coh(twin))
    assert abs(coh("five_scales") - 1) < 1e-3
    for a, b in lim.OPPOSITE:
        assert coh(f"opposite_{a}_{b}") <= lim.coh_tol(2)
    for k in lim.ONE_HOT_K:
        assert abs(coh(f"one_hot_{k}_+") - 1) <= lim.coh_tol(1) and abs(coh(f"one_hot_{k}_-") - 1) <= lim.coh_tol(1)
    _identical(_fold(engine, fx, rows_per_call=5), got, 5)


@pytest.mark.parametrize("kind", lim.BOTH_KINDS)
def test_both_strands(engine, kind):
    print()
    fx = lim.both_strands(kind)
    want = lim.definition(fx, fx["rows_rev"])
    got = _fold(engine, fx, rows_rev=fx["rows_rev"])
    _same(got, want, f"both strands, {kind}", strands=2)
    live = want["count"] > 0
    if kind == "negated":                                            # S_f + S_r is exactly zero, U_f + U_r cancels
        assert not got["embedding"].any() and (got["coherence"] <= [lim.coh_tol(int(n), 2) for n in want["count"]]).all()
    else:
        assert got["embedding"][live].any(axis=1).all() and (got["coherence"][live] > 0.05).all()
    one = _fold(engine, fx)
    assert np.array_equal(one["count"], got["count"]) and np.array_equal(one["scores"], got["scores"])
    _identical(_fold(engine, fx, rows_rev=fx["rows_rev"], rows_per_call=7), got, 7)


# ---- the pass on the example of the kernel's own comment: a 2 Mbp contig at stride 1000 ---------------------------------------------
STRIDE = 1000
LENGTH = 2_004_417
N_RUNS = ((300_250, 6_500), (1_111_111, 9_000), (1_750_003, 5_200))     # (start, length) of runs of N: windows they fill are masked
SPLITS = (0, 654_321, 1_333_777, LENGTH)                                 # no window centre: centres are k * 1000 + 3000 (+ the tail's)


@functools.lru_cache(maxsize=None)
def _long_contig():
    rng = np.random.default_rng(505)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, LENGTH)].copy()
    for a, n in N_RUNS:
        seq[a:a + n] = ord("N")
    offsets = np.array([0, LENGTH], np.int64)
    starts, lens, _, window_n, _, _ = sequence.scan_spans(offsets, STRIDE)
    n_count = np.array([np.count_nonzero(seq[a:a + n] == ord("N")) for a, n in zip(starts, lens)])
    kept = (window_n == 0) | (n_count <= sequence.MAX_N)
    assert len(starts) >= 2000 and 5 <= int((~kept).sum()) <= 20
    assert all(s % STRIDE != 3000 % STRIDE for s in SPLITS[1:-1])
    return dict(seq=seq, offsets=offsets, starts=starts, lens=lens, kept=kept)


def _interval_lists():
    zero = np.zeros(1, np.int64)
    return (zero, zero, np.array([LENGTH])), (np.zeros(3, np.int64), np.array(SPLITS[:-1]), np.array(SPLITS[1:]))


def _reverse_rows(engine, fx):
    """rows and scores of the reverse windows, the way test_strand_modes_against_the_numpy_definition makes them"""
    n = len(fx["starts"])
    bufs = [engine.alloc(fx["seq"].nbytes), engine.alloc(n * _lib.WINDOW), engine.alloc(n * 512 * 4), engine.alloc(n * 3 * 4)]
    try:
        bufs[0].upload(fx["seq"])
        engine.revcomp_spans_dev(bufs[0].ptr, fx["starts"], fx["lens"], bufs[1].ptr)
        engine.embed_dev(bufs[1].ptr, n, bufs[2].ptr, scores_ptr=bufs[3].ptr)
        engine.sync()
        return bufs[2].download((n, 512), np.float32), bufs[3].download((n, 3), np.float32)
    finally:
        for b in bufs:
            b.free()


def test_the_pass_over_a_2_mbp_contig_at_stride_1000(engine, synth_weights):
    from genomad_amd.engine import NNEngine
    print()
    fx = _long_contig()
    wins = sequence.materialize_spans(fx["seq"], fx["starts"], fx["lens"])
    rows, scores = engine.embed(wins, with_scores=True)
    rows_r, scores_r = _reverse_rows(engine, fx)
    assert not np.array_equal(rows_r, rows)
    mixed = sequence.strand_mean(scores, scores_r)
    with NNEngine(0, synth_weights, chunk=13) as e2:                 # slabs of 52 windows (26 per strand under both): no multiple of 8
        for contig, start, end in _interval_lists():
            w_lo, w_hi = sequence.interval_windows(fx["offsets"], STRIDE, contig, start, end)
            assert w_lo[0] == 0 and w_hi[-1] == len(fx["starts"]) and ((w_lo[1:] % 8 != 0) & (w_lo[1:] % 52 != 0)).all()
            want = sequence.interval_embeddings(rows, scores, fx["kept"], w_lo, w_hi)
            got = e2.embed_intervals(fx["seq"], fx["offsets"], STRIDE, contig, start, end)
            assert np.array_equal(got.w_lo, w_lo) and np.array_equal(got.w_hi, w_hi) and int(got.count.sum()) == int(fx["kept"].sum())
            _same({k: getattr(got, k) for k in lim.KEYS}, want, f"the pass, {len(contig)} intervals, members {list(got.count)}")
            want = sequence.interval_embeddings(rows, mixed, fx["kept"], w_lo, w_hi, rows_rev=rows_r)
            got = e2.embed_intervals(fx["seq"], fx["offsets"], STRIDE, contig, start, end, strand="both")
            _same({k: getattr(got, k) for k in lim.KEYS}, want, f"the pass under both, {len(contig)} intervals", strands=2)
