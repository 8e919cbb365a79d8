"""Label transfer on the MI355X: the four vote arrays against the device's own pairs (the edges NNEngine.match returns for the same
rows, folded on the host: exact, no tolerance), against the float64 definition on inputs that keep 1e-5 clear of the threshold
(tests/test_votes_host.py asserts the gap), bit identity under the split of the base, both paths, the host and the device entry
points and a permutation of the base, the self form, the masks, the edges of the interface, and embed_contigs -> vote end to end.
333 queries are six 64-row tiles, off every boundary; 7, 33 and 300 base rows lie below a 32-column block, across one and across
the 256-column step; 3, 16, 17 and 40 classes on both sides of the LDS limit."""
import numpy as np
import pytest

from genomad_amd import _lib, sequence, synthetic
from genomad_amd._lib import GnnError
from tests import votes_data as V
from tests.kmeans_data import signed_init, signed_rows

pytestmark = pytest.mark.gpu

SPLITS = (32, 100, 333, 0)
FIELDS = sequence.VOTE_FIELDS


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def identical(got, want):
    """every array bit for bit; ``got`` / ``want``: a VoteResult or the four arrays"""
    g = [getattr(got, f) for f in FIELDS] if hasattr(got, "nearest_sim") else got
    w = [getattr(want, f) for f in FIELDS] if hasattr(want, "nearest_sim") else want
    return all(a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b)) for a, b in zip(g, w))


def from_match(engine, q, b, label, n_classes, t, leave_one_out=False):
    """the four arrays folded from the device's own edges"""
    m = engine.match(q, b, t)
    a, col, sim = m.edges()
    return V.fold_edges(a, col, sim, label, len(q), n_classes, leave_one_out)


@pytest.fixture(scope="module")
def found(engine):
    """the device's answer on every (base, classes, threshold), computed once with the library's own split and path"""
    engine.set_neighbour_split(0)
    engine.set_vote_lds(16)
    q = V.query()[0]
    return {(nb, nc, t): engine.vote(q, V.base(nb), V.labels(nb, nc), nc, t) for nb in V.BASES for nc in V.CLASSES for t in V.GAPPED}


@pytest.mark.parametrize("n_base", V.BASES)
@pytest.mark.parametrize("n_classes", V.CLASSES)
def test_votes_are_the_fold_of_the_devices_own_pairs(engine, found, n_base, n_classes):
    """count, weight, nearest and nearest_sim from match's edges of the same rows: equal, no tolerance - at 0.9, at 0.8 and at -1,
    where every valid labelled pair votes and the counts are the class sizes"""
    q, b, label = V.query()[0], V.base(n_base), V.labels(n_base, n_classes)
    q_ok, b_ok = V.valid(q), V.valid(b)
    for t in V.GAPPED:
        res = found[(n_base, n_classes, t)]
        assert identical(res, from_match(engine, q, b, label, n_classes, t)), t
        assert np.array_equal(res.query_valid, q_ok) and res.n_classes == n_classes and res.threshold == float(np.float32(t))
    sizes = np.bincount(label[b_ok & (label >= 0)], minlength=n_classes)
    res = found[(n_base, n_classes, -1.0)]
    assert (res.count[q_ok] == sizes).all() and (res.count[~q_ok] == 0).all() and sizes[-1] == 0 and sizes.sum() > 0


def test_tied_rows_vote_at_the_threshold_and_the_smaller_index_is_nearest(engine):
    """cosines that are exact multiples of 1 / 256 on the device too: 900 pairs tie with the threshold, 21 identical rows tie as the
    nearest - against match's edges and against the definition, exactly, on both paths"""
    r, s, threshold, label = V.tie_case()
    engine.set_neighbour_split(0)
    try:
        for lds in (16, 0):
            engine.set_vote_lds(lds)
            res = engine.vote(r, r, label, 5, threshold)
            assert identical(res, from_match(engine, r, r, label, 5, threshold)), lds
            assert identical(res, sequence.class_votes(r, r, label, 5, threshold)), lds
            own = engine.vote(r, None, label, 5, threshold)
            assert identical(own, sequence.class_votes(r, None, label, 5, threshold)), lds
    finally:
        engine.set_vote_lds(16)
    above = engine.vote(r, r, label, 5, float(np.nextafter(np.float32(threshold), np.float32(2))))
    assert res.count.sum() - above.count.sum() == int((s[:, label >= 0] == threshold).sum()) > 0


@pytest.mark.parametrize("n_base", V.BASES)
def test_votes_equal_the_float64_definition_where_it_is_well_defined(found, n_base):
    """count exactly (no pair is within 1e-5 of the threshold, the device's f32 value is within 1e-5 of the float64 cosine);
    |weight / 2^32 - the float64 sum| <= 1e-5 per voter (the same bound, plus 2^-33 of rounding per voter); nearest wherever the
    definition's top two of the class are more than 2e-5 apart, nearest_sim within 1e-5"""
    s, q_ok, b_ok = V.cosines(n_base)
    q, b = V.query()[0], V.base(n_base)
    worst = 0.0
    for nc in V.CLASSES:
        label = V.labels(n_base, nc)
        for t in V.GAPPED:
            res = found[(n_base, nc, t)]
            count, weight, nearest, nearest_sim = sequence.class_votes(q, b, label, nc, t)
            assert np.array_equal(res.count, count), (nc, t)
            err = np.abs(res.similarity_sum() - weight.astype(np.float64) / V.UNIT)
            worst = max(worst, float((err / np.maximum(count, 1)).max()))
            assert (err <= V.GAP * count).all(), (nc, t)
            thr = float(np.float32(t))
            clear = np.zeros(count.shape, bool)
            for c in range(nc):
                cols = np.flatnonzero((label == c) & b_ok)
                if len(cols):
                    v = np.where((s[:, cols] >= thr) & q_ok[:, None], s[:, cols], -np.inf)
                    top = np.sort(np.concatenate([v, np.full((len(v), 1), -np.inf)], axis=1), axis=1)[:, -2:]
                    clear[:, c] = (count[:, c] > 0) & (top[:, 1] - np.where(np.isfinite(top[:, 0]), top[:, 0], -9.0) > V.NEAREST_GAP)
            assert clear.sum() >= 0.95 * (count > 0).sum() and np.array_equal(res.nearest[clear], nearest[clear]), (nc, t)
            assert np.array_equal(res.nearest < 0, count == 0) and np.array_equal(np.isnan(res.nearest_sim), count == 0)
            assert np.abs(res.nearest_sim[count > 0].astype(np.float64) - nearest_sim[count > 0]).max(initial=0) <= V.GAP
    print(f"\nn_base {n_base}: max |weight / 2^32 - float64 sum| per voter = {worst:.3e}")


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


@pytest.mark.parametrize("n_classes", (3, 16))
def test_no_bit_depends_on_the_split_the_path_or_the_entry_point(engine, found, n_classes):
    q, b, label = V.query()[0], V.base(300), V.labels(300, n_classes)
    try:
        for t in (V.T_MID, -1.0):
            first = found[(300, n_classes, t)]
            for split in SPLITS:
                for lds in (16, 0):
                    engine.set_neighbour_split(split)
                    engine.set_vote_lds(lds)
                    assert identical(engine.vote(q, b, label, n_classes, t), first), (t, split, lds)
            engine.set_neighbour_split(100)
            assert identical(on_device(engine, q, b, label, n_classes, t), first), t
            # two calls in a row on one ctx, a larger one between them: nothing is left over in the workspace
            engine.vote(q, b, V.labels(300, 40), 40, -1.0)
            assert identical(engine.vote(q, b, label, n_classes, t), first), t
            assert identical(engine.vote(q, None, V.labels(300, n_classes)[np.arange(333) % 300], n_classes, t),
                             on_device(engine, q, None, V.labels(300, n_classes)[np.arange(333) % 300], n_classes, t))
    finally:
        engine.set_neighbour_split(0)
        engine.set_vote_lds(16)
    with pytest.raises(GnnError, match=r"gnn_debug_set_vote_lds: 17 classes is outside \[0, 16\]"):
        engine.set_vote_lds(17)


@pytest.mark.parametrize("n_classes", (3, 40))
def test_a_permutation_of_the_base_with_its_labels_changes_no_sum(engine, found, n_classes):
    q, b, label = V.query()[0], V.base(300), V.labels(300, n_classes)
    s, q_ok, b_ok = V.cosines(300)
    perm = np.random.default_rng(3).permutation(300)             # new row k is old row perm[k]
    for t in (V.T_MID, -1.0):
        first = found[(300, n_classes, t)]
        got = engine.vote(q, np.ascontiguousarray(b[perm]), label[perm], n_classes, t)
        assert np.array_equal(got.count, first.count) and np.array_equal(got.weight, first.weight)
        assert np.array_equal(bits(got.nearest_sim), bits(first.nearest_sim))
        # the maximum is unique where no other voter of the class has the nearest's f32 value: match's edges tell
        m = engine.match(q, b, t)
        a, col, sim = m.edges()
        keep = label[col] >= 0
        a, c, sim = a[keep], label[col[keep]], sim[keep]
        at_max = np.zeros(first.count.shape, np.int64)
        np.add.at(at_max, (a, c), bits(sim) == bits(first.nearest_sim[a, c]))
        unique = at_max == 1
        assert unique.sum() >= 0.9 * (first.count > 0).sum()
        assert np.array_equal(perm[got.nearest[unique]], first.nearest[unique])


def test_the_self_form_leaves_the_row_itself_out(engine):
    q = V.query()[0]
    label = V.labels(300, 16)[np.arange(333) % 300].copy()
    label[5] = 15                                               # a row alone in its class
    assert (label == 15).sum() == 1 and V.valid(q)[5]
    engine.set_neighbour_split(0)
    for t in (V.T_HIGH, -1.0):
        res = engine.vote(q, None, label, 16, t)
        assert identical(res, from_match(engine, q, q, label, 16, t, leave_one_out=True)), t
        assert res.count[5, 15] == 0 and res.nearest[5, 15] == -1 and np.isnan(res.nearest_sim[5, 15])
    ok = V.valid(q)
    assert (np.delete(res.count[:, 15], 5)[np.delete(ok, 5)] == 1).all()          # everybody else hears that row at -1
    full = engine.vote(q, q, label, 16, -1.0)
    own = np.flatnonzero(ok & (label >= 0))
    diag = np.zeros_like(full.count)
    diag[own, label[own]] = 1
    assert np.array_equal(full.count - diag, res.count)
    two = engine.vote(q[:2], None, np.array([0, 0]), 1, -1.0)    # two rows: each hears the other
    assert list(two.count[:, 0]) == [1, 1] and list(two.nearest[:, 0]) == [1, 0]


def test_masks_invalid_rows_unlabelled_rows_and_padded_columns(engine):
    q, b, label = V.query()[0], V.base(33), V.labels(33, 16)
    engine.set_neighbour_split(0)
    res = engine.vote(q, b, label, 16, -1.0)
    bad = ~V.valid(q)
    assert bad.sum() == 2 and (res.count[bad] == 0).all() and (res.weight[bad] == 0).all() and (res.nearest[bad] == -1).all()
    assert np.isnan(res.nearest_sim[bad]).all()
    # a zero, NaN or -1-labelled base row changes nothing: the call on the base without them, the indices mapped back
    keep = np.flatnonzero(V.valid(b) & (label >= 0))
    assert len(keep) < 33 - 2
    less = engine.vote(q, np.ascontiguousarray(b[keep]), label[keep], 16, -1.0)
    assert np.array_equal(less.count, res.count) and np.array_equal(less.weight, res.weight)
    assert np.array_equal(bits(less.nearest_sim), bits(res.nearest_sim))
    assert np.array_equal(np.where(less.nearest >= 0, keep[less.nearest], -1), res.nearest)
    # negative similarities do not lose against padded columns (zero fragments: their 0 would beat every negative value)
    sq, sb = signed_rows(333), signed_init(33)
    sl = (np.arange(33) % 4 - 1).astype(np.int64)
    for nc, lds in ((3, 16), (3, 0), (17, 16)):
        engine.set_vote_lds(lds)
        neg = engine.vote(sq, sb, np.minimum(sl, nc - 2), nc, -1.0)
        assert identical(neg, from_match(engine, sq, sb, np.minimum(sl, nc - 2), nc, -1.0))
        assert (neg.nearest_sim[:, :2] < 0).all() and (neg.weight[:, :2] < 0).all() and (neg.nearest[:, :2] < 33).all()
        assert (neg.count.sum(axis=1) == (sl >= 0).sum()).all()
    engine.set_vote_lds(16)


def test_edges_of_the_interface(engine):
    q, b = V.query()[0][:70], V.base(33)
    label = V.labels(33, 3)
    engine.set_neighbour_split(0)
    for bad in (3, -2):
        wrong = label.copy()
        wrong[20] = bad
        with pytest.raises(ValueError, match=r"a label is outside \[-1, 3\)"):
            engine.vote(q, b, wrong, 3, 0.5)
        out = [np.full((70, 3), 7, np.int64) for _ in range(3)] + [np.full((70, 3), 7, np.float32)]
        rc = engine.lib.gnn_vote(engine.ctx, q.ctypes.data, 70, b.ctypes.data, 33, wrong.ctypes.data, 3, 0.5, *(a.ctypes.data for a in out))
        assert rc == _lib.ERR_ARG and b"gnn_vote: a label is outside [-1, 3)" in engine.lib.gnn_last_error()
        assert all((a == 7).all() for a in out)                 # the outputs are untouched
        bufs = [engine.alloc(q.nbytes), engine.alloc(b.nbytes), engine.alloc(8 * 33)] + [engine.alloc(8 * 210) for _ in range(4)]
        try:
            for buf, arr in zip(bufs, (q, b, wrong, out[0], out[1], out[2], np.full((70, 3), 7, np.int64))):
                buf.upload(arr)
            with pytest.raises(GnnError, match=r"gnn_vote_dev: a label is outside \[-1, 3\)"):
                engine.vote_dev(bufs[0].ptr, 70, bufs[1].ptr, 33, bufs[2].ptr, 3, 0.5, *(x.ptr for x in bufs[3:]))
            engine.sync()
            assert all((x.download((70, 3), np.int64) == 7).all() for x in bufs[3:])
        finally:
            for buf in bufs:
                buf.free()
    for nc in (0, 1025):
        with pytest.raises(ValueError, match=r"n_classes .*\[1, 1024\]"):
            engine.vote(q, b, label, nc, 0.5)
    with pytest.raises(ValueError, match="finite float"):
        engine.vote(q, b, label, 3, float("nan"))
    with pytest.raises(ValueError, match="one integer per base row"):
        engine.vote(q, b, label[:5], 3, 0.5)
    with pytest.raises(ValueError, match="one integer per base row"):
        engine.vote(q, None, label, 3, 0.5)
    with pytest.raises(GnnError, match=r"gnn_vote_dev: n_classes 0 is outside \[1, 1024\]"):
        engine.vote_dev(0, 4, 0, 4, 0, 0, 0.5, 0, 0, 0, 0)
    with pytest.raises(GnnError, match="bad argument to gnn_vote_dev"):
        engine.vote_dev(0, 4, 0, 4, 0, 3, 0.5, 0, 0, 0, 0)
    one = engine.vote(q, b[:1], label[:1], 3, -1.0)             # n_base = 1
    assert identical(one, from_match(engine, q, b[:1], label[:1], 3, -1.0)) and one.count.sum() == V.valid(q).sum()
    single = engine.vote(q[3:4], b, label, 1024, -1.0)          # n_query = 1, the most classes
    assert identical(single, from_match(engine, q[3:4], b, label, 1024, -1.0)) and single.count.shape == (1, 1024)
    empty = engine.vote(q, b[:0], label[:0], 3, -1.0)           # no base row: every class is empty
    assert (empty.count == 0).all() and (empty.nearest == -1).all() and np.isnan(empty.nearest_sim).all()
    assert engine.vote(q[:0], b, label, 3, 0.5).count.shape == (0, 3)
    assert engine.vote(q[:1], None, label[:1], 3, -1.0).count.sum() == 0       # alone with itself
    engine.profile_enable(True)
    try:
        engine.vote(q, b, label, 3, 0.5)
        ms = engine.vote_pass_ms()
        assert len(ms) == 3 and (ms >= 0).all() and ms[1] > 0   # labels, votes, finish
    finally:
        engine.profile_enable(False)


def test_embed_contigs_to_vote_end_to_end(engine):
    rng = np.random.default_rng(5)
    windows = synthetic.synth_windows(900, 30)
    contigs = [windows[a:a + n].reshape(-1)[:int(rng.integers((n - 1) * 6000 + 3000, n * 6000 + 1))]
               for a, n in zip(range(0, 24, 2), [1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 2])]
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in contigs])]).astype(np.int64)
    seq = np.concatenate(contigs)
    engine.set_neighbour_split(0)
    before, _ = engine.classify_contigs(seq, offsets)
    _, emb, _ = engine.embed_contigs(seq, offsets)
    idx0, sim0 = engine.neighbours(emb, None, 3)
    picked = np.array([0, 2, 3, 5, 7, 8, 10])                    # the labelled subset of the same contigs
    label = np.array([0, 1, 2, 0, 1, 2, 3], dtype=np.int64)
    res = engine.vote(emb, np.ascontiguousarray(emb[picked]), label, 5, 0.999)
    idx1, sim1 = engine.neighbours(emb, None, 3)                 # the searches share the fragment buffers
    after, _ = engine.classify_contigs(seq, offsets)
    got, _, _ = res.predict("nearest")
    assert np.array_equal(got[picked], label) and (res.count[picked, label] >= 1).all() and (res.nearest[picked, label] == np.arange(7)).all()
    assert (res.count[:, 4] == 0).all() and res.query_valid.all()
    table = res.table(list("abcdefghijkl"), ["v", "p", "c", "h", "x"], [f"ref{i}" for i in range(7)], rule="nearest")
    assert table[0]["label"] == "v" and table[0]["nearest"] == "ref0" and table[10]["label"] == "h"
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    assert np.array_equal(idx0, idx1) and np.array_equal(sim0.view(np.uint32), sim1.view(np.uint32))
