"""Label transfer on the MI355X at the limits tests/test_votes_gpu.py stays away from (inputs and their CPU-side conditions:
tests/votes_limits_data.py, tests/embedding_limits_data.py, tests/linkage_limits_data.py, tests/test_votes_limits_host.py).  What each
group pins in gnn_votes.hip:

  two slabs, rectangle   vt_run with q0 > 0: `query_dev + q0 * D` and `query_host + q0 * D`, the output offsets `q0 * n_classes` of both
                         entry points, and d_query, v.key and the landing buffer v.d_out reused by a last slab of 70 rows
  two slabs, self form   `qfrag = w.bfrag.get() + q0 / 32 * BLK_U4`, `qvalid = w.bvalid.get() + q0`, `a.self_off = q0`
  self form, splits      own[nb] (`rel = col - self0`, `+ 4 * half`) when the own column lies in another base range than most of the
                         tile's columns, on the LDS path and straight to memory, against the fold of match's edges - not against itself
  dead tiles and steps   lok[] all false in a tile, `__ballot(vote != 0) == 0` in every wave for whole steps at threshold -1, an invalid
                         row 0 and an invalid last row on both sides
  row scales             nn_prepare_kernel's per-row power of two under the vote; rows from all-subnormal to FLT_MAX, heavy rows
  threshold edges        `s >= a.threshold` at pairs of exactly 1, +0 and -1; +0 against -0; thresholds beyond every value
  wide labels            vt_label_kernel compares the int64 before it narrows it

"The fold" is tests/votes_data.fold_edges over NNEngine.match's edges of the same rows: exact, no tolerance.  The float64 comparisons
use thresholds chosen on the CPU to keep 2e-5 clear of every float64 cosine (tests/test_votes_limits_host.py asserts it).

Measured on an MI355X (profiles/votes/README.md, "At the limits"): the rectangle of 262 214 queries x 33 base rows 0.6 - 0.7 ms on the
device and 0.44 s in the call; the self form of 262 214 rows 286 ms (16 classes, LDS) and 291 ms (17 classes, memory), 0.75 s per test;
weight / 2^32 within 2.6e-7 per voter and nearest_sim within 7.7e-7 of float64 on the extreme and heavy rows; the opposite rows 77 and
150 of dead_tiles at -1.00000012 on the device; every other test below 0.05 s."""
import time

import numpy as np
import pytest

from genomad_amd import _lib, sequence
from genomad_amd._lib import GnnError
from tests import embedding_limits_data as lim
from tests import votes_data as V
from tests import votes_limits_data as L
from tests.linkage_data import device_values
from tests.votes_limits_data import bits, differing, identical

pytestmark = pytest.mark.gpu

FIELDS = sequence.VOTE_FIELDS


def restore(engine):
    engine.set_neighbour_split(0)
    engine.set_vote_lds(16)


def from_match(engine, q, b, label, n_classes, t, leave_one_out=False):
    """the four arrays folded from the device's own edges"""
    a, col, sim = engine.match(q, b, t).edges()
    return V.fold_edges(a, col, sim, label, len(q), n_classes, leave_one_out)


def on_device(engine, q, b, label, n_classes, t):
    """the four arrays through gnn_vote_dev"""
    nq = len(q)
    cells = nq * n_classes
    bufs = [engine.alloc(max(q.nbytes, 8)), engine.alloc(max(8 * len(label), 8))] + [engine.alloc(8 * cells) for _ in range(3)] + [engine.alloc(4 * cells)]
    base = None if b is None else engine.alloc(b.nbytes)
    try:
        bufs[0].upload(q)
        bufs[1].upload(label)
        if base is not None:
            base.upload(b)
        engine.vote_dev(bufs[0].ptr, nq, None if base is None else base.ptr, 0 if b is None else len(b), bufs[1].ptr, n_classes, t,
                        *(x.ptr for x in bufs[2:]))
        engine.sync()
        return [bufs[2 + i].download((nq, n_classes), np.int64) for i in range(3)] + [bufs[5].download((nq, n_classes), np.float32)]
    finally:
        for x in bufs + ([] if base is None else [base]):
            x.free()


def timed_vote(engine, what, *args):
    """engine.vote with profiling on: prints the device time of the passes and the wall time of the call"""
    engine.profile_enable(True)
    try:
        t0 = time.perf_counter()
        res = engine.vote(*args)
        wall = time.perf_counter() - t0
        ms = engine.vote_pass_ms()
    finally:
        engine.profile_enable(False)
    print(f"\n{what}: device passes {np.round(ms, 3).tolist()} ms, sum {ms.sum():.1f} ms; the call {wall:.2f} s wall")
    return res


# ---- two query slabs ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def big():
    """the 262 214 tiled rows, 537 MB of host memory: built once, freed when the module is done"""
    holder = [L.big_queries()]
    yield holder[0]
    holder.clear()


@pytest.fixture(scope="module")
def period_votes(engine):
    """the device's answer on the 333 rows of the period against the 33-row base, with the library's own split and path"""
    restore(engine)
    p, base = V.query()[0], V.base(33)
    return {(nc, t): engine.vote(p, base, V.labels(33, nc), nc, t) for nc, t in ((3, V.T_MID), (3, -1.0), (17, V.T_MID))}


@pytest.mark.parametrize("entry", ("host", "device"))
@pytest.mark.parametrize("n_classes,t", ((3, V.T_MID), (3, -1.0), (17, V.T_MID)))
def test_two_query_slabs_of_the_rectangle(engine, big, period_votes, entry, n_classes, t):
    """row i of the 262 214 is row i % 333 of the period, in all four arrays, bit for bit: 3 classes on the LDS path, 17 straight to
    memory; a 70-row call gives afterwards what it gave before"""
    try:
        restore(engine)
        base, label = V.base(33), V.labels(33, n_classes)
        idx = L.slab_index()
        small = engine.vote(big[:70], base, label, n_classes, t)
        want = period_votes[(n_classes, t)]
        assert identical(small, [getattr(want, f)[:70] for f in FIELDS])
        if entry == "host":
            got = timed_vote(engine, f"rectangle 262214 x 33, {n_classes} classes, t {t}", big, base, label, n_classes, t)
            got = [getattr(got, f) for f in FIELDS]
        else:
            got = on_device(engine, big, base, label, n_classes, t)
        for f, g in zip(FIELDS, got):
            w = getattr(want, f)[idx]
            assert g.dtype == w.dtype and np.array_equal(bits(g), bits(w)), (f, np.argwhere(bits(g) != bits(w))[:5].tolist())
        assert (got[0][L.QSLAB:] > 0).any() and (got[0][idx == 225] == 0).all()      # the last slab has votes; an invalid row has none
        assert identical(engine.vote(big[:70], base, label, n_classes, t), small)
    finally:
        restore(engine)


@pytest.mark.parametrize("n_classes,with_dead_row", ((16, False), (17, False), (16, True)))
def test_two_query_slabs_of_the_self_form(engine, big, n_classes, with_dead_row):
    """the 262 214 rows among themselves at 0.9, against the period's own edges with their multiplicities (tiled_self_votes; the host
    test checks it against the definition).  16 classes: the LDS path; 17: straight to memory.  With a dead row: row i < 64 is zeroed,
    so that the flags of row i and of row 262144 + i differ - in the planted rows as they are, rows 0..69 and the last slab's are
    all valid, and a flag read without the slab's offset would not show."""
    try:
        restore(engine)
        p = V.query()[0]
        label = L.self_labels(n_classes)
        idx = L.slab_index()
        a, b, sim = engine.match(p, p, V.T_HIGH).edges()
        dead = [L.dead_first_copy(label, V.T_HIGH)] if with_dead_row else []
        want = L.tiled_self_votes(a, b, sim, label, len(big), L.PERIOD, n_classes, dead=dead)
        assert want[0][L.QSLAB:].sum() > 0 and (want[0][idx == 225] == 0).all()
        assert all(want[0][L.QSLAB + i].sum() > 0 for i in dead)
        keep = big[dead].copy()
        try:
            big[dead] = 0
            got = timed_vote(engine, f"self form 262214, {n_classes} classes, t {V.T_HIGH}", big, None, label[idx], n_classes, V.T_HIGH)
        finally:
            big[dead] = keep
        assert identical(got, want), differing(got, want)
    finally:
        restore(engine)


# ---- the self form under every split and on both paths -----------------------------------------------------------------------------

@pytest.mark.parametrize("n_classes", (16, 17))
@pytest.mark.parametrize("t", (V.T_HIGH, -1.0))
def test_the_self_form_is_the_fold_under_every_split_and_on_both_paths(engine, n_classes, t):
    p = V.query()[0]
    label = L.self_labels(n_classes)
    ok = V.valid(p)
    try:
        restore(engine)
        want = from_match(engine, p, p, label, n_classes, t, leave_one_out=True)
        assert want[0][5, n_classes - 1] == 0 and want[0].sum() > 0
        full = engine.vote(p, p, label, n_classes, t)
        for split in (32, 64, 100, 333, 0):
            for lds in (16, 0):
                engine.set_neighbour_split(split)
                engine.set_vote_lds(lds)
                got = engine.vote(p, None, label, n_classes, t)
                assert identical(got, want), (split, lds, differing(got, want))
                if t == -1.0:
                    own = np.flatnonzero(ok & (label >= 0))
                    diag = np.zeros_like(full.count)
                    diag[own, label[own]] = 1
                    assert np.array_equal(got.count, full.count - diag), (split, lds)
    finally:
        restore(engine)


# ---- dead tiles and dead steps -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dead_values(engine):
    """(the median of the device's own cosines among the live rows of dead_tiles, the cosines)"""
    restore(engine)
    r, _, dead, _ = L.dead_case(False)
    s = device_values(engine, r)
    live = np.setdiff1d(np.arange(600), dead)
    assert np.isnan(s[dead]).all() and np.isnan(s[:, dead]).all() and not np.isnan(s[np.ix_(live, live)]).any()
    return float(np.median(s[np.ix_(live, live)])), s


@pytest.mark.parametrize("unlabelled_head", (False, True))
def test_tiles_without_a_valid_row_and_steps_without_a_voter(engine, dead_values, unlabelled_head):
    """at -1 every live labelled pair votes, so the counts are the class sizes - but for a pair of exactly opposite rows (row 77 is
    minus row 150): its float64 cosine is -1, the threshold itself, and the device's float32 may lie an ulp below it.  Such a
    pair is told from the device's own value, and must be one of those."""
    r, label, dead, voters = L.dead_case(unlabelled_head)
    dead_median, s = dead_values
    live = np.setdiff1d(np.arange(600), dead)
    sizes = np.bincount(label[voters], minlength=5)
    below = np.zeros((600, 5), np.int64)                         # per row and class: its voters whose device cosine is below -1
    with np.errstate(invalid="ignore"):
        lo_i, lo_j = np.nonzero(s < -1.0)
    opposite = {(77, 150), (150, 77)}
    assert set(zip(lo_i.tolist(), lo_j.tolist())) <= opposite and (np.abs(s[lo_i, lo_j] + 1.0) <= V.GAP).all()
    assert all(np.array_equal(r[i], -r[j]) for i, j in opposite)
    at = np.isin(lo_j, voters)
    np.add.at(below, (lo_i[at], label[lo_j[at]]), 1)
    print(f"\n{len(lo_i)} of the 2 opposite pairs lie below -1 on the device: {s[lo_i, lo_j].tolist()}")
    try:
        for t in (-1.0, dead_median):
            restore(engine)
            want = {False: from_match(engine, r, r, label, 5, t), True: from_match(engine, r, r, label, 5, t, leave_one_out=True)}
            for split in (0, 32, 256):
                for lds in (16, 0):
                    engine.set_neighbour_split(split)
                    engine.set_vote_lds(lds)
                    for self_form in (False, True):
                        got = engine.vote(r, None if self_form else r, label, 5, t)
                        assert identical(got, want[self_form]), (t, split, lds, self_form, differing(got, want[self_form]))
                        assert (got.count[dead] == 0).all() and (got.weight[dead] == 0).all() and (got.nearest[dead] == -1).all()
                        assert np.isnan(got.nearest_sim[dead]).all() and not got.query_valid[dead].any()
                        assert np.isin(got.nearest[got.nearest >= 0], voters).all()
                        if t == -1.0:
                            own = np.zeros((len(live), 5), np.int64)
                            if self_form:
                                at = np.flatnonzero(label[live] >= 0)
                                own[at, label[live][at]] = 1
                            want_count = sizes - own - below[live]
                            assert np.array_equal(got.count[live], want_count), (split, lds, self_form, live[(got.count[live] != want_count).any(axis=1)])
            assert 0 < want[False][0].sum() and (t == -1.0 or want[False][0].sum() < len(live) * len(voters))
    finally:
        restore(engine)


# ---- row scales --------------------------------------------------------------------------------------------------------------------

def test_a_power_of_two_per_row_changes_no_bit_of_the_votes(engine):
    try:
        restore(engine)
        q, b = lim.signed_rows(333, 8), lim.signed_rows(300, 9)
        label = (np.arange(300) % 4 - 1).astype(np.int64)
        q2, b2 = lim.power_of_two_scaled(q, 3), lim.power_of_two_scaled(b, 4)
        for t in (0.05, -1.0):
            first = engine.vote(q, b, label, 4, t)
            assert identical(first, from_match(engine, q, b, label, 4, t)) and first.count.sum() > 0
            assert t > 0 or (first.count.sum() == 333 * (label >= 0).sum() and (first.weight < 0).any())      # negative similarities vote at -1
            assert identical(engine.vote(q2, b2, label, 4, t), first), t
        own = (np.arange(333) % 4 - 1).astype(np.int64)
        assert identical(engine.vote(q2, None, own, 4, -1.0), engine.vote(q, None, own, 4, -1.0))
    finally:
        restore(engine)


@pytest.mark.parametrize("which", ("extreme", "heavy"))
def test_rows_from_all_subnormal_to_flt_max_and_heavy_tails(engine, which):
    try:
        restore(engine)
        q, b, label, nc, s, thresholds = L.scale_case(which)
        self_form = b is None
        for t in thresholds:
            got = engine.vote(q, b, label, nc, t)
            want = from_match(engine, q, q if self_form else b, label, nc, t, leave_one_out=self_form)
            assert identical(got, want), (t, differing(got, want))
            assert got.query_valid.all() and (got.count > 0).mean() > 0.5
            werr, nerr = L.against_float64(got, s, label, nc, t, self_form)
            print(f"\n{which}, t {t:.6f}: max |weight / 2^32 - float64 sum| per voter = {werr:.3e}, max |nearest_sim - float64| = {nerr:.3e}")
    finally:
        restore(engine)


# ---- threshold edges ---------------------------------------------------------------------------------------------------------------

def test_thresholds_at_beside_and_beyond_the_exact_values_of_one_hot_rows(engine):
    r, label, s = L.one_hot_case()
    try:
        restore(engine)
        dev = device_values(engine, r)
        assert set(bits(dev).ravel().tolist()) == {int(bits(np.float32(x))) for x in (1.0, 0.0, -1.0)}      # exactly 1, +0 and -1
        assert np.array_equal(dev.astype(np.float64), s)
        for lds in (16, 0):
            engine.set_vote_lds(lds)
            got = {}
            for k, t in enumerate(L.EDGE_THRESHOLDS):
                for self_form in (False, True):
                    res = got[(k, self_form)] = engine.vote(r, None if self_form else r, label, 4, t)
                    want = sequence.class_votes(r, None if self_form else r, label, 4, t)
                    assert identical(res, want), (t, self_form, lds, differing(res, want))
                    assert identical(res, from_match(engine, r, r, label, 4, t, leave_one_out=self_form)), (t, self_form, lds)
                    assert (bits(res.nearest_sim[res.nearest_sim == 0]) == 0).all()
            for self_form in (False, True):
                assert identical(got[(2, self_form)], got[(3, self_form)])                     # +0.0 and -0.0
                assert got[(6, self_form)].count.sum() == 0 and (got[(6, self_form)].nearest == -1).all()       # FLT_MAX: all empty
                assert np.isnan(got[(6, self_form)].nearest_sim).all() and got[(1, self_form)].count.sum() == 0
                assert identical(got[(4, self_form)], got[(7, self_form)]) and identical(got[(4, self_form)], got[(5, self_form)])
                counts = [int(got[(k, self_form)].count.sum()) for k in (0, 2, 4)]
                assert 0 < counts[0] < counts[1] < counts[2], counts                           # the ties at 1, at 0 and at -1 vote
            assert (got[(2, True)].nearest_sim == 0).any()
    finally:
        restore(engine)


# ---- labels beyond int32 -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wide", L.WIDE_LABELS)
def test_a_label_beyond_int32_is_refused_before_an_output_is_touched(engine, wide):
    try:
        restore(engine)
        q, b = V.query()[0][:70], V.base(33)
        wrong = V.labels(33, 3).copy()
        wrong[20] = wide
        assert wrong.dtype == np.int64 and int(wrong[20]) == wide
        with pytest.raises(ValueError, match=r"a label is outside \[-1, 3\)"):
            engine.vote(q, b, wrong, 3, 0.5)                        # the host refuses first: the library is called directly below
        out = [np.full((70, 3), 7, np.int64) for _ in range(3)] + [np.full((70, 3), 7, np.float32)]
        for base, nb in ((b, 33), (None, 0)):                       # the rectangle and the self form (33 rows among themselves)
            nq = 70 if base is not None else 33
            rc = engine.lib.gnn_vote(engine.ctx, q.ctypes.data, nq, None if base is None else base.ctypes.data, nb, wrong.ctypes.data, 3, 0.5,
                                     *(a.ctypes.data for a in out))
            assert rc == _lib.ERR_ARG and b"gnn_vote: a label is outside [-1, 3)" in engine.lib.gnn_last_error()
            assert all((a == 7).all() for a in out)
        bufs = [engine.alloc(q.nbytes), engine.alloc(b.nbytes), engine.alloc(8 * 33)] + [engine.alloc(8 * 210) for _ in range(4)]
        try:
            for buf, arr in zip(bufs, (q, b, wrong, out[0], out[1], out[2], np.full((70, 3), 7, np.int64))):
                buf.upload(arr)
            with pytest.raises(GnnError, match=r"gnn_vote_dev: a label is outside \[-1, 3\)"):
                engine.vote_dev(bufs[0].ptr, 70, bufs[1].ptr, 33, bufs[2].ptr, 3, 0.5, *(x.ptr for x in bufs[3:]))
            with pytest.raises(GnnError, match=r"gnn_vote_dev: a label is outside \[-1, 3\)"):
                engine.vote_dev(bufs[0].ptr, 33, None, 0, bufs[2].ptr, 3, 0.5, *(x.ptr for x in bufs[3:]))
            engine.sync()
            assert all((x.download((70, 3), np.int64) == 7).all() for x in bufs[3:])
        finally:
            for buf in bufs:
                buf.free()
        good = V.labels(33, 3)                                      # and the call works afterwards
        assert identical(engine.vote(q, b, good, 3, 0.5), from_match(engine, q, b, good, 3, 0.5))
    finally:
        restore(engine)
