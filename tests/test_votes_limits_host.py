"""What tests/test_votes_limits_gpu.py leans on, without a GPU: every generator of tests/votes_limits_data.py runs (each asserts its own
conditions), the helper that spells out the self form on a tiled array agrees with the definition on a 700-row tiling, the thresholds
of the float64 comparisons keep their gap, and each comparison function of the device tests passes on values that stand in for the
device's - float32 roundings of the float64 cosines - and fails on a wrong one."""
import numpy as np
import pytest

from genomad_amd import sequence
from tests import embedding_limits_data as lim
from tests import votes_data as V
from tests import votes_limits_data as L


def test_the_slab_border_falls_inside_a_period():
    idx = L.slab_index()
    assert len(idx) == 262214 and idx[L.QSLAB] == 73 and idx[-1] == (262214 - 1) % 333
    ok = V.valid(V.query()[0])
    assert np.flatnonzero(~ok).tolist() == [225, 285] and ok[idx[L.QSLAB:]].all()   # the last slab holds rows 73..142: all valid
    # the generator itself on a small tiling: np.take gives row i % 333, bit for bit
    p = V.query()[0]
    small = np.take(p, np.arange(700) % 333, axis=0)
    assert small.dtype == np.float32 and np.array_equal(small[333:666].view(np.uint32), p.view(np.uint32))


@pytest.mark.parametrize("n_classes", (16, 17))
@pytest.mark.parametrize("t", (V.T_HIGH, -1.0))
def test_the_tiled_self_form_is_the_definition_on_700_rows(n_classes, t):
    """700 = 2 * 333 + 34: rows 0..33 stand three times, the others twice.  The similarity matrix is float32, built from sims64 and
    tiled, so every copy of a pair has one value - as on the device."""
    s, ok = L.period_sims32()
    label = L.self_labels(n_classes)
    assert (label == n_classes - 1).sum() == 1
    idx = np.arange(700) % 333
    rows = np.take(V.query()[0], idx, axis=0)
    want = sequence.class_votes(rows, None, label[idx], n_classes, t, sims=s[np.ix_(idx, idx)])
    a, b, sim = L.edges_of(s, ok, ok, t)
    assert (a == b).sum() == ok.sum()                                           # the own pairs are edges: the helper takes them out
    got = L.tiled_self_votes(a, b, sim, label, 700, 333, n_classes)
    assert L.identical(got, want), L.differing(got, want)
    assert want[0][5, n_classes - 1] == 2 and want[2][5, n_classes - 1] == 338   # row 5 hears its two copies
    assert want[2][338, n_classes - 1] == 5
    # one period is the plain self form, and a helper that forgets the row itself is noticed
    one = L.tiled_self_votes(a, b, sim, label, 333, 333, n_classes)
    assert L.identical(one, sequence.class_votes(V.query()[0], None, label, n_classes, t, sims=s))
    assert L.identical(one, V.fold_edges(a, b, sim, label, 333, n_classes, leave_one_out=True))
    assert not L.identical(one, V.fold_edges(a, b, sim, label, 333, n_classes))
    # a first copy made invalid (the device test's second case): the definition on the tiling with that row zeroed
    i = L.dead_first_copy(label, t)
    rows[i] = 0
    want = sequence.class_votes(rows, None, label[idx], n_classes, t, sims=s[np.ix_(idx, idx)])
    got = L.tiled_self_votes(a, b, sim, label, 700, 333, n_classes, dead=[i])
    assert L.identical(got, want), L.differing(got, want)
    assert want[0][i].sum() == 0 and want[0][i + 333].sum() > 0 and (want[2] != i).all()


def test_the_self_form_labels_and_the_fold_with_leave_one_out():
    s, ok = L.period_sims32()
    for nc in (16, 17):
        label = L.self_labels(nc)
        for t in (V.T_HIGH, -1.0):
            a, b, sim = L.edges_of(s, ok, ok, t)
            fold = V.fold_edges(a, b, sim, label, 333, nc, leave_one_out=True)
            assert L.identical(fold, sequence.class_votes(V.query()[0], None, label, nc, t, sims=s)), (nc, t)
            assert L.identical(fold, V.loop_votes(s, ok, ok, label, nc, t, leave_one_out=True)), (nc, t)
        full = V.fold_edges(a, b, sim, label, 333, nc)
        diag = np.zeros_like(full[0])
        own = np.flatnonzero(ok & (label >= 0))
        diag[own, label[own]] = 1
        assert np.array_equal(full[0] - diag, fold[0])


@pytest.mark.parametrize("unlabelled_head", (False, True))
def test_dead_tiles_and_steps_without_a_voter(unlabelled_head):
    r, label, dead, voters = L.dead_case(unlabelled_head)
    ok = V.valid(r)
    assert len(voters) == (int((label[512:599] >= 0).sum()) if unlabelled_head else int((ok & (np.arange(600) % 5 > 0)).sum())) > 50
    lab = np.where(ok, label, -1)
    for c0 in (0, 256):                                                          # whole 256-column steps without a voter
        assert (lab[c0:c0 + 256] == -1).all() == (unlabelled_head or c0 == 256)
    # the fold against the definition on exact values: the rows are integers, so float64 cosines of the valid rows stand in
    s = np.zeros((600, 600))
    at = np.flatnonzero(ok)
    s[np.ix_(at, at)] = L.sims64(r[ok], r[ok])
    s32 = s.astype(np.float32)
    med = float(np.median(s32[np.ix_(at, at)]))
    for t in (med, -1.0):                                                        # the last one: every live labelled pair votes
        a, b, sim = L.edges_of(s32, ok, ok, t)
        for self_form in (False, True):
            fold = V.fold_edges(a, b, sim, label, 600, 4, leave_one_out=self_form)
            want = sequence.class_votes(r, None if self_form else r, label, 4, t, sims=s32)
            assert L.identical(fold, want), (t, self_form)
            assert (fold[0][dead] == 0).all() and (fold[2][dead] == -1).all() and np.isnan(fold[3][dead]).all()
            assert np.isin(fold[2][fold[2] >= 0], voters).all()
    sizes = np.bincount(label[voters], minlength=4)
    assert (fold[0][at] == sizes - np.eye(4, dtype=np.int64)[label[at]] * (label[at] >= 0)[:, None]).all()


def test_the_row_scale_inputs_keep_their_gap():
    q, b = lim.signed_rows(333, 8), lim.signed_rows(300, 9)
    assert not np.array_equal(lim.power_of_two_scaled(q, 3), q) and lim.power_of_two_scaled(b, 4).shape == (300, 512)
    for which in ("extreme", "heavy"):
        q, b, label, nc, s, thresholds = L.scale_case(which)
        self_form = b is None
        assert len(thresholds) == 2 and thresholds[0] > 0 > thresholds[1]
        off = s[~np.eye(len(s), dtype=bool)] if self_form else s
        for t in thresholds:
            assert t == float(np.float32(t)) and np.abs(off - t).min() > 2 * V.GAP and 0.02 < abs(t) < 0.08, (which, t)
            # the definition on float32 roundings of its own cosines passes the device's comparison ...
            stand_in = sequence.class_votes(q, b, label, nc, t, sims=s.astype(np.float32))
            werr, nerr = L.against_float64(stand_in, s, label, nc, t, self_form)
            assert werr <= 2.0 ** -24 and nerr <= 2.0 ** -24 and (stand_in[0] > 0).mean() > 0.5, (which, t, werr, nerr)
            # ... and a vote too many does not
            wrong = [x.copy() for x in stand_in]
            wrong[0][3, 1] += 1
            with pytest.raises(AssertionError):
                L.against_float64(wrong, s, label, nc, t, self_form)


def test_one_hot_rows_at_the_threshold_edges():
    r, label, s = L.one_hot_case()
    assert L.EDGE_THRESHOLDS[1] > 1 and L.EDGE_THRESHOLDS[5] < -1 and np.signbit(L.EDGE_THRESHOLDS[3]) and not np.signbit(L.EDGE_THRESHOLDS[2])
    ok = np.ones(16, bool)
    results = {}
    for t in map(str, L.EDGE_THRESHOLDS):
        for self_form in (False, True):
            want = sequence.class_votes(r, None if self_form else r, label, 4, float(t))
            a, b, sim = L.edges_of(s.astype(np.float32), ok, ok, float(t))
            assert L.identical(want, V.fold_edges(a, b, sim, label, 16, 4, leave_one_out=self_form)), (t, self_form)
            assert (L.bits(want[3][want[3] == 0]) == 0).all()                    # a zero is +0
            results[(t, self_form)] = want
    for self_form in (False, True):
        assert L.identical(results[('0.0', self_form)], results[('-0.0', self_form)])
        assert results[(str(L.FLT_MAX), self_form)][0].sum() == 0 == results[(str(L.EDGE_THRESHOLDS[1]), self_form)][0].sum()
        assert L.identical(results[('-1.0', self_form)], results[(str(-L.FLT_MAX), self_form)])
        assert L.identical(results[('-1.0', self_form)], results[(str(L.EDGE_THRESHOLDS[5]), self_form)])
        counts = [int(results[(t, self_form)][0].sum()) for t in ('1.0', '0.0', '-1.0')]
        assert 0 < counts[0] < counts[1] < counts[2]                             # the ties at 1, at 0 and at -1 all vote
    assert (results[('0.0', True)][3] == 0).any()


def test_wide_labels_are_refused_by_the_definition():
    r, label, _ = L.one_hot_case()
    assert [int(np.int64(v).astype(np.int32)) for v in L.WIDE_LABELS] == [1, -2 ** 31, -1, -2]
    for v in L.WIDE_LABELS:
        wrong = label.copy()
        wrong[2] = v
        with pytest.raises(ValueError, match=r"a label is outside \[-1, 3\)"):
            sequence.class_votes(r, r, wrong, 3, 0.5)
