"""Matches against a reference on the MI355X: indptr and col against the numpy definition (sequence.threshold_matches) - exactly, on
planted rows whose fp64 similarities keep 9.7e-4 from both thresholds (asserted here) and on integer rows whose dots are exact with many
ties at the threshold -, sim within the neighbour search's 1e-5 of fp64 and bit for bit the value neighbours returns, independence of
how the base is split over workgroups, the device entry points with sentinels behind the outputs, the square match against the graph,
GraphResult.extend against the graph of the concatenation, the full rectangle, the edges of the interface, the errors, and
embed_contigs -> match end to end.  133 query rows are three 64-row tiles, the last with 5 rows; 333 base rows are two 256-column steps."""
import numpy as np
import pytest

from genomad_amd import sequence, synthetic
from genomad_amd._lib import GnnError, check
from genomad_amd.engine import NNEngine
from tests.clusters_data import THRESHOLDS, planted
from tests.neighbours_data import rows, sims64

pytestmark = pytest.mark.gpu

SPLITS = (32, 100, 333, 4096, 0)
SHAPES = {"133x333": (slice(0, 133), slice(0, 333)), "333x133": (slice(0, 333), slice(0, 133))}
EDGES = {0.8: 488, 0.9: 482}


def csr(res):
    return res.indptr, res.col, res.sim


def same_bits(got, want):
    """(indptr, col, sim) of the right dtypes, equal bit for bit"""
    return (got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.float32 and len(got) == len(want) == 3
            and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            and np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)))


def check_shape(res, nq, nb):
    """what every result must be, whatever its matches: a CSR by query row with ascending columns among the valid rows"""
    assert res.indptr.dtype == np.int64 and res.indptr.shape == (nq + 1,) and res.indptr[0] == 0 and (np.diff(res.indptr) >= 0).all()
    assert res.col.dtype == np.int32 and res.sim.dtype == np.float32 and len(res.col) == len(res.sim) == res.indptr[-1] == res.n_edges
    a, b, _ = res.edges()
    assert (b >= 0).all() and (b < max(nb, 1)).all()
    assert ((np.diff(b) > 0) | (np.diff(a) > 0)).all()            # within a row the columns ascend
    assert res.query_valid[a].all() and res.base_valid[b].all() and res.n_query == nq and res.n_base == nb
    assert res.query_valid.shape == (nq,) and res.base_valid.shape == (nb,)


@pytest.fixture(scope="module")
def data():
    """the planted rows and the definition's answers for both shapes at both thresholds, computed once"""
    r, _ = planted()
    want = {(s, t): sequence.threshold_matches(r[q], r[b], t) for s, (q, b) in SHAPES.items() for t in THRESHOLDS}
    return {"rows": r, "want": want}


@pytest.fixture(scope="module")
def found(engine, data):
    """the device's answers, computed once with the library's own split"""
    engine.set_neighbour_split(0)
    r = data["rows"]
    return {(s, t): engine.match(r[q], r[b], t) for s, (q, b) in SHAPES.items() for t in THRESHOLDS}


def test_the_definition_alone_decides_every_planted_pair(data):
    r = data["rows"]
    s64 = sims64(r[:133], r)
    for t in THRESHOLDS:
        margin = np.abs(s64 - float(np.float32(t))).min()
        print(f"\nplanted 133 x 333 at {t}: fp64 margin {margin:.3e}")
        assert margin >= 9.7e-4
        for s in SHAPES:
            assert len(data["want"][(s, t)][1]) == EDGES[t]


@pytest.mark.parametrize("threshold", THRESHOLDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_planted_rows_equal_the_definition(data, found, shape, threshold):
    res, (indptr, col, sim64) = found[(shape, threshold)], data["want"][(shape, threshold)]
    q, b = SHAPES[shape]
    check_shape(res, q.stop, b.stop)
    assert np.array_equal(res.indptr, indptr) and np.array_equal(res.col, col) and res.n_edges == EDGES[threshold]
    err = np.abs(res.sim.astype(np.float64) - sim64).max()
    print(f"\nplanted {shape} at {threshold}: {res.n_edges} matches, max |sim - fp64| = {err:.3e}")
    assert err <= 1e-5
    assert res.threshold == float(np.float32(threshold)) and res.metric == "cosine" and res.query_valid.all() and res.base_valid.all()


@pytest.mark.parametrize("threshold", THRESHOLDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_results_do_not_depend_on_the_split_and_the_device_path_agrees(engine, data, found, shape, threshold):
    q, b = (data["rows"][s] for s in SHAPES[shape])
    first = csr(found[(shape, threshold)])
    nq, nb, total = len(q), len(b), found[(shape, threshold)].n_edges
    try:
        for split in SPLITS:
            engine.set_neighbour_split(split)
            assert same_bits(csr(engine.match(q, b, threshold)), first), split
        engine.set_neighbour_split(100)
        cap = total + 64
        bufs = [engine.alloc(q.nbytes), engine.alloc(b.nbytes), engine.alloc(8 * (nq + 1)), engine.alloc(4 * cap), engine.alloc(4 * cap)]
        try:
            bufs[0].upload(q)
            bufs[1].upload(b)
            bufs[3].upload(np.full(cap, -7, np.int32))
            bufs[4].upload(np.full(cap, -7.0, np.float32))
            assert engine.match_count_dev(bufs[0].ptr, nq, bufs[1].ptr, nb, threshold, bufs[2].ptr) == total
            engine.match_fill_dev(bufs[0].ptr, nq, bufs[1].ptr, nb, threshold, bufs[3].ptr, bufs[4].ptr, cap)
            engine.sync()
            col, sim = bufs[3].download((cap,), np.int32), bufs[4].download((cap,), np.float32)
            assert same_bits((bufs[2].download((nq + 1,), np.int64), col[:total], sim[:total]), first)
            assert (col[total:] == -7).all() and (sim[total:] == -7.0).all()          # nothing behind the last match was touched
        finally:
            for buf in bufs:
                buf.free()
    finally:
        engine.set_neighbour_split(0)


@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_the_square_match_holds_the_graph_the_diagonal_and_the_transposes_index_set(engine, data, threshold):
    r = data["rows"]
    n = len(r)
    engine.set_neighbour_split(0)
    res, g = engine.match(r, r, threshold), engine.graph(r, threshold)
    check_shape(res, n, n)
    a, b, s = res.edges()
    up = b > a
    counts = np.bincount(a[up], minlength=n)
    assert same_bits((np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), res.col[up], s[up]), csr(g))
    diag = a[b == a]
    assert np.array_equal(diag, np.arange(n))                     # (i, i) for every row: all are valid
    lo = b < a
    assert np.array_equal(np.stack([b[lo], a[lo]])[:, np.lexsort((a[lo], b[lo]))], np.stack([a[up], b[up]]))
    t_ptr, t_col, _ = res.transpose()
    assert np.array_equal(t_ptr, res.indptr) and np.array_equal(t_col, res.col)      # the index set is symmetric


@pytest.mark.parametrize("split", (0, 32))
@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_extend_is_the_graph_of_the_concatenation_bit_for_bit(engine, data, threshold, split):
    r = data["rows"]
    try:
        engine.set_neighbour_split(split)
        old, cross, new = engine.graph(r[:200], threshold), engine.match(r[:200], r[200:], threshold), engine.graph(r[200:], threshold)
        both = old.extend(cross, new)
        whole = engine.graph(r, threshold)
        assert same_bits(csr(both), csr(whole)) and cross.n_edges > 0
        assert both.n == 333 and both.n_edges == whole.n_edges and np.array_equal(both.valid, whole.valid)
        assert both.threshold == whole.threshold and both.metric == whole.metric
        assert np.array_equal(both.components(), engine.cluster(r, threshold).label)
    finally:
        engine.set_neighbour_split(0)


def test_the_values_are_those_neighbours_returns(engine):
    """pins the orientation (query i, base row j), the >=, and that both searches compute the same f32"""
    q, b = rows(70, 9), rows(64, 10)
    engine.set_neighbour_split(0)
    idx, sim = engine.neighbours(q, b, 64)
    assert (idx >= 0).all()
    s = np.full((70, 64), np.nan, np.float32)
    np.put_along_axis(s, idx, sim, axis=1)                             # s[i, j]: query i, base row j
    threshold = np.sort(s.reshape(-1))[s.size // 2]                    # one of the returned f32 values: a tie exactly at the threshold
    assert threshold.dtype == np.float32 and (s == threshold).any()
    res = engine.match(q, b, threshold)
    check_shape(res, 70, 64)
    a, c, got = res.edges()
    assert np.array_equal(np.stack([a, c]), np.stack(np.nonzero(s >= threshold)))
    assert np.array_equal(got.view(np.uint32), s[a, c].view(np.uint32))
    assert res.n_edges == int((s >= threshold).sum()) and (got == threshold).any()
    idx1, sim1 = engine.neighbours(q, b, 1)
    keep = sim1[:, 0] >= threshold
    best_idx, best_sim = res.best()
    assert keep.any()
    assert np.array_equal(best_idx, np.where(keep, idx1[:, 0], -1))
    assert np.array_equal(best_sim[keep].view(np.uint32), sim1[keep, 0].view(np.uint32)) and np.isnan(best_sim[~keep]).all()
    high = np.sort(sim1[:, 0])[35]                                     # the median of the best values: half the queries have no match
    keep = sim1[:, 0] >= high
    best_idx, best_sim = engine.match(q, b, high).best()
    assert keep.any() and not keep.all() and best_sim.dtype == np.float32
    assert np.array_equal(best_idx, np.where(keep, idx1[:, 0], -1))
    assert np.array_equal(best_sim[keep].view(np.uint32), sim1[keep, 0].view(np.uint32)) and np.isnan(best_sim[~keep]).all()


def test_integer_dots_with_ties_at_the_threshold_equal_numpy(engine):
    rng = np.random.default_rng(12)
    q = rng.integers(0, 8, (70, 512)).astype(np.float32)               # every dot is an integer below 512 * 49 < 2^24: exact on the device
    b = rng.integers(0, 8, (300, 512)).astype(np.float32)
    b[40:60] = q[10]
    b[299] = q[69]
    dots = q.astype(np.float64) @ b.astype(np.float64).T
    threshold = float(np.median(dots))
    assert (dots == threshold).sum() > 10 and 0.3 < (dots >= threshold).mean() < 0.7
    hit = dots >= threshold
    want_ptr, (want_a, want_b) = np.concatenate([[0], np.cumsum(hit.sum(axis=1))]), np.nonzero(hit)
    try:
        for split in (0, 32):
            engine.set_neighbour_split(split)
            res = engine.match(q, b, threshold, "dot")
            check_shape(res, 70, 300)
            assert np.array_equal(res.indptr, want_ptr) and np.array_equal(res.col, want_b), split
            assert np.array_equal(res.sim.astype(np.float64), dots[want_a, want_b]), split
    finally:
        engine.set_neighbour_split(0)


@pytest.mark.parametrize("shape", ((1, 1), (1, 257), (64, 256), (65, 33), (133, 333)))
def test_full_rectangle_of_equal_rows(engine, shape):
    nq, nb = shape
    one = rows(1, 4)
    q, b = np.tile(one, (nq, 1)), np.tile(one, (nb, 1))
    try:
        for split in (0, 32):
            engine.set_neighbour_split(split)
            res = engine.match(q, b, 0.99)
            check_shape(res, nq, nb)
            assert np.array_equal(res.indptr, np.arange(nq + 1, dtype=np.int64) * nb), split
            assert np.array_equal(res.col.reshape(nq, nb), np.tile(np.arange(nb, dtype=np.int32), (nq, 1))), split
            assert (res.sim.view(np.uint32) == res.sim.view(np.uint32)[0]).all() and abs(float(res.sim[0]) - 1.0) <= 1e-5
            assert np.array_equal(res.hits(), np.full(nq, nb)) and np.array_equal(res.base_hits(), np.full(nb, nq))
    finally:
        engine.set_neighbour_split(0)


def test_edges_of_the_interface(engine, data):
    engine.set_neighbour_split(0)
    q = np.tile(rows(1, 4), (70, 1))
    b = q.copy()
    q[1] = 0
    q[3, 100] = np.nan
    q[65, 511] = np.inf
    b[2] = 0
    b[64, 7] = -np.inf
    b[69, 0] = np.nan
    for metric in ("cosine", "dot"):
        got = engine.match(q, b, 0.5, metric)
        check_shape(got, 70, 70)
        indptr, col, _ = sequence.threshold_matches(q, b, 0.5, metric)
        assert np.array_equal(got.indptr, indptr) and np.array_equal(got.col, col), metric
        assert (got.hits()[[1, 3, 65]] == 0).all() and (got.base_hits()[[2, 64, 69]] == 0).all()
        # a zero row is valid under dot, and 0 < 0.5 matches nobody
        assert list(np.flatnonzero(~got.query_valid)) == ([1, 3, 65] if metric == "cosine" else [3, 65])
        assert list(np.flatnonzero(~got.base_valid)) == ([2, 64, 69] if metric == "cosine" else [64, 69])
        assert got.n_edges == 67 * 67
    zero = engine.match(q, b, -0.5, "dot")                             # under dot the zero rows take part: 0 >= -0.5
    assert zero.hits()[1] == 68 and zero.base_hits()[2] == 68 and zero.n_edges == 68 * 68
    empty = (np.zeros(0, np.int32), np.zeros(0, np.float32))
    for nq, nb in ((0, 70), (70, 0), (0, 0)):
        got = engine.match(q[:nq], b[:nb], 0.5)
        assert same_bits(csr(got), (np.zeros(nq + 1, np.int64),) + empty) and (got.n_query, got.n_base, got.n_edges) == (nq, nb, 0)
        assert list(got.best()[0]) == [-1] * nq and len(got.base_hits()) == nb
    p = data["rows"]
    got = engine.match(p[:133], p, 1.5)                                # above every similarity: no match, no fill launch
    check_shape(got, 133, 333)
    assert got.n_edges == 0 and (got.indptr == 0).all()
    bufs = [engine.alloc(p.nbytes), engine.alloc(8 * 134)]
    try:
        bufs[0].upload(p)
        for nq, nb in ((133, 333), (133, 0), (0, 333)):
            bufs[1].upload(np.full(134, 7, np.int64))
            assert engine.match_count_dev(bufs[0].ptr, nq, bufs[0].ptr, nb, 1.5, bufs[1].ptr) == 0
            engine.match_fill_dev(bufs[0].ptr, nq, bufs[0].ptr, nb, 1.5, None, None, 0)      # a total of 0 accepts null outputs
            engine.sync()
            out = bufs[1].download((134,), np.int64)
            assert (out[:nq + 1] == 0).all() and (out[nq + 1:] == 7).all()
    finally:
        for buf in bufs:
            buf.free()


def test_errors(engine, data):
    p = data["rows"]
    q, n = p[:133], len(p)
    engine.set_neighbour_split(0)
    with pytest.raises(GnnError, match=r"gnn_match_count: threshold nan is outside .* finite"):
        engine.match(q, p, float("nan"))
    with pytest.raises(GnnError, match=r"gnn_match_count: metric 9 is outside \[0, 1\]"):
        engine.match(q, p, 0.5, 9)
    with pytest.raises(GnnError, match=r"gnn_match_count_dev: n_query -1 is outside \[0, 2\^31\)"):
        engine.match_count_dev(0, -1, 0, 3, 0.5, 0)
    with pytest.raises(GnnError, match=r"gnn_match_fill_dev: n_base 2147483648 is outside \[0, 2\^31\)"):
        engine.match_fill_dev(0, 3, 0, 1 << 31, 0.5, 0, 0, 0)
    total = engine.match(q, p, 0.8).n_edges
    g_total = engine.graph(p, 0.8).n_edges
    cap = max(total, g_total)
    bufs = [engine.alloc(p.nbytes), engine.alloc(8 * (n + 1)), engine.alloc(4 * cap), engine.alloc(4 * cap)]
    try:
        bufs[0].upload(p)
        rows_ptr, ind, col, sim = (x.ptr for x in bufs)
        with NNEngine(0) as fresh:                                     # an engine that never counted
            with pytest.raises(GnnError, match=r"error -3: gnn_match_fill_dev: no gnn_match_count\* of the same \(n_query, n_base, threshold, "
                                               r"metric\) = \(133, 333, "):
                fresh.match_fill_dev(rows_ptr, 133, rows_ptr, n, 0.8, col, sim, cap)
            with pytest.raises(GnnError, match=r"error -3: gnn_match_fill: no gnn_match_count of the same"):
                check(fresh.lib.gnn_match_fill(fresh.ctx, 133, n, 0.8, 0, None, None, cap))
        # a fill belongs to the last count of either kind
        assert engine.match_count_dev(rows_ptr, n, rows_ptr, n, 0.8, ind) > g_total
        with pytest.raises(GnnError, match=r"error -3: gnn_graph_fill_dev: no gnn_graph_count\* of the same"):
            engine.graph_fill_dev(rows_ptr, n, 0.8, col, sim, cap)
        assert engine.graph_count_dev(rows_ptr, n, 0.8, ind) == g_total
        with pytest.raises(GnnError, match=r"error -3: gnn_match_fill_dev: no gnn_match_count\* of the same"):
            engine.match_fill_dev(rows_ptr, n, rows_ptr, n, 0.8, col, sim, cap)
        assert engine.match_count_dev(rows_ptr, 133, rows_ptr, n, 0.8, ind) == total
        with pytest.raises(GnnError, match=r"error -3: gnn_match_fill_dev: no gnn_match_count\* of the same"):
            engine.match_fill_dev(rows_ptr, 133, rows_ptr, n, 0.9, col, sim, cap)               # another threshold
        with pytest.raises(GnnError, match=r"error -3: gnn_match_fill_dev"):
            engine.match_fill_dev(rows_ptr, 132, rows_ptr, n, 0.8, col, sim, cap)               # another n_query
        with pytest.raises(GnnError, match=r"error -3: gnn_match_fill_dev"):
            engine.match_fill_dev(rows_ptr, 133, rows_ptr, n - 1, 0.8, col, sim, cap)           # another n_base
        with pytest.raises(GnnError, match=r"error -3: gnn_match_fill_dev"):
            engine.match_fill_dev(rows_ptr, 133, rows_ptr, n, 0.8, col, sim, cap, "dot")        # another metric
        with pytest.raises(GnnError, match=rf"error -1: gnn_match_fill_dev: capacity {total - 1} is below the {total} edges"):
            engine.match_fill_dev(rows_ptr, 133, rows_ptr, n, 0.8, col, sim, total - 1)
        engine.match_fill_dev(rows_ptr, 133, rows_ptr, n, 0.8, col, sim, total)                 # the count still stands
        engine.sync()
        want = engine.match(q, p, 0.8)
        assert same_bits((bufs[1].download((134,), np.int64), bufs[2].download((total,), np.int32), bufs[3].download((total,), np.float32)),
                         csr(want))
        # the host fill reads the base rows its count uploaded: another host search replaces them
        engine.neighbours(p[:5], None, 2)
        with pytest.raises(GnnError, match=r"error -3: gnn_match_fill: .*another search has replaced the rows"):
            check(engine.lib.gnn_match_fill(engine.ctx, 133, n, 0.8, 0, None, None, total))
    finally:
        for buf in bufs:
            buf.free()
    with pytest.raises(ValueError, match=rf"{total} matches at the threshold 0\.8, more than max_edges = {total - 1}"):
        engine.match(q, p, 0.8, max_edges=total - 1)
    assert same_bits(csr(engine.match(q, p, 0.8, max_edges=total)), csr(want))                 # the next call on the same engine works
    assert engine.graph(p, 0.8).n_edges == g_total                                             # and so does the graph


def test_embed_contigs_to_match_end_to_end(engine):
    rng = np.random.default_rng(5)
    windows = synthetic.synth_windows(900, 30)
    contigs = [windows[a:a + n].reshape(-1)[:int(rng.integers((n - 1) * 6000 + 3000, n * 6000 + 1))]
               for a, n in zip(range(0, 24, 2), [1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 2])]
    contigs[9] = contigs[4].copy()                            # byte-identical to contig 4
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in contigs])]).astype(np.int64)
    seq = np.concatenate(contigs)
    engine.set_neighbour_split(0)
    before, _ = engine.classify_contigs(seq, offsets)
    _, emb, _ = engine.embed_contigs(seq, offsets)
    ref = np.concatenate([emb, emb[4:5]])                     # the reference: those embeddings plus a byte-identical copy of contig 4's
    idx0, sim0 = engine.neighbours(emb, None, 3)
    res = engine.match(emb, ref, 0.999)
    idx1, sim1 = engine.neighbours(emb, None, 3)              # the searches share the fragment buffers
    after, _ = engine.classify_contigs(seq, offsets)
    check_shape(res, 12, 13)
    for i in (4, 9):                                          # itself, its twin among the contigs, and the copy
        assert {4, 9, 12} <= set(res.col[res.indptr[i]:res.indptr[i + 1]].tolist())
    assert all(i in res.col[res.indptr[i]:res.indptr[i + 1]] for i in range(12))
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    assert np.array_equal(idx0, idx1) and np.array_equal(sim0.view(np.uint32), sim1.view(np.uint32))
