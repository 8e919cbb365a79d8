"""The similarity graph among encoder embeddings on the MI355X: indptr and col against the numpy definition (sequence.threshold_graph) -
exactly, on planted rows whose fp64 similarities keep 1e-4 from the threshold (tests/test_clusters_host.py asserts it) and on integer
rows whose dots are exact with many ties at the threshold -, sim within the neighbour search's 1e-5 of fp64 and bit for bit the value
neighbours returns, independence of how the base is split over workgroups, the device entry points with sentinels behind the outputs,
placement across waves, column blocks, steps and parts, the complete graph, the edges of the interface, the errors, and embed_contigs
-> graph end to end.  333 rows are six 64-row tiles and two 256-column steps, off every boundary."""
import numpy as np
import pytest

from genomad_amd import sequence, synthetic
from genomad_amd._lib import GnnError, check
from genomad_amd.engine import NNEngine
from tests.clusters_data import THRESHOLDS, planted
from tests.neighbours_data import rows

pytestmark = pytest.mark.gpu

SPLITS = (32, 100, 333, 4096, 0)


def csr(res):
    return res.indptr, res.col, res.sim


def same_bits(got, want):
    """(indptr, col, sim) of the right dtypes, equal bit for bit"""
    return (got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.float32 and len(got) == len(want) == 3
            and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            and np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)))


def check_shape(res, n):
    """what every result must be, whatever its edges: a CSR over the upper triangle with ascending columns"""
    assert res.indptr.dtype == np.int64 and res.indptr.shape == (n + 1,) and res.indptr[0] == 0 and (np.diff(res.indptr) >= 0).all()
    assert res.col.dtype == np.int32 and res.sim.dtype == np.float32 and len(res.col) == len(res.sim) == res.indptr[-1] == res.n_edges
    a, b, _ = res.edges()
    assert (a < b).all() and (b < n).all()
    assert ((np.diff(b) > 0) | (np.diff(a) > 0)).all()            # within a row the columns ascend
    assert res.valid[a].all() and res.valid[b].all() and res.n == n


@pytest.fixture(scope="module")
def data():
    """the planted rows and the definition's answer at both thresholds, computed once"""
    r, _ = planted()
    return {"rows": r, "want": {t: sequence.threshold_graph(r, t) for t in THRESHOLDS}}


@pytest.fixture(scope="module")
def found(engine, data):
    """the device's answer at both thresholds, computed once with the library's own split"""
    engine.set_neighbour_split(0)
    return {t: engine.graph(data["rows"], t) for t in THRESHOLDS}


@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_planted_rows_equal_the_definition(data, found, threshold):
    res, (indptr, col, sim64) = found[threshold], data["want"][threshold]
    check_shape(res, 333)
    assert np.array_equal(res.indptr, indptr) and np.array_equal(res.col, col)
    err = np.abs(res.sim.astype(np.float64) - sim64).max()
    print(f"\nplanted at {threshold}: {res.n_edges} edges, max |sim - fp64| = {err:.3e}")
    assert err <= 1e-5
    assert res.threshold == float(np.float32(threshold)) and res.metric == "cosine" and res.valid.all()
    assert res.n_edges >= 5 * 66 + 23 + 1                         # the five families' cliques, the chain's links, the pair


@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_results_do_not_depend_on_the_split_and_the_device_path_agrees(engine, data, found, threshold):
    r, first = data["rows"], csr(found[threshold])
    n, total = len(r), found[threshold].n_edges
    try:
        for split in SPLITS:
            engine.set_neighbour_split(split)
            assert same_bits(csr(engine.graph(r, threshold)), first), split
        engine.set_neighbour_split(100)
        cap = total + 64
        bufs = [engine.alloc(r.nbytes), engine.alloc(8 * (n + 1)), engine.alloc(4 * cap), engine.alloc(4 * cap)]
        try:
            bufs[0].upload(r)
            bufs[2].upload(np.full(cap, -7, np.int32))
            bufs[3].upload(np.full(cap, -7.0, np.float32))
            assert engine.graph_count_dev(bufs[0].ptr, n, threshold, bufs[1].ptr) == total
            engine.graph_fill_dev(bufs[0].ptr, n, threshold, bufs[2].ptr, bufs[3].ptr, cap)
            engine.sync()
            col, sim = bufs[2].download((cap,), np.int32), bufs[3].download((cap,), np.float32)
            assert same_bits((bufs[1].download((n + 1,), np.int64), col[:total], sim[:total]), first)
            assert (col[total:] == -7).all() and (sim[total:] == -7.0).all()          # nothing behind the last edge was touched
        finally:
            for buf in bufs:
                buf.free()
    finally:
        engine.set_neighbour_split(0)


def test_integer_dots_with_ties_at_the_threshold_equal_the_definition(engine):
    rng = np.random.default_rng(11)
    base = rng.integers(0, 8, (200, 512)).astype(np.float32)          # every dot is an integer below 512 * 49 < 2^24: exact on the device
    base[40:60] = base[10]
    base[150] = base[3]
    base[199] = base[3]
    dots = base.astype(np.float64) @ base.astype(np.float64).T
    iu = np.triu_indices(200, 1)
    threshold = float(np.median(dots[iu]))                             # the median pair's dot: about half of the 19 900 pairs are edges
    assert (dots[iu] == threshold).sum() > 10 and 0.3 < (dots[iu] >= threshold).mean() < 0.7
    upper = np.triu(dots >= threshold, 1)
    want_ptr, (want_a, want_b) = np.concatenate([[0], np.cumsum(upper.sum(axis=1))]), np.nonzero(upper)
    try:
        for split in (0, 32):
            engine.set_neighbour_split(split)
            res = engine.graph(base, threshold, "dot")
            check_shape(res, 200)
            assert np.array_equal(res.indptr, want_ptr) and np.array_equal(res.col, want_b), split
            assert np.array_equal(res.sim.astype(np.float64), dots[want_a, want_b]), split
    finally:
        engine.set_neighbour_split(0)


def test_the_values_are_those_neighbours_returns(engine):
    """pins the orientation (query i, base row j, i < j), the >=, and that both searches compute the same f32"""
    r = rows(65, 9)
    engine.set_neighbour_split(0)
    idx, sim = engine.neighbours(r, None, 64)
    assert (idx >= 0).all()
    s = np.full((65, 65), np.nan, np.float32)
    np.put_along_axis(s, idx, sim, axis=1)                             # s[i, j]: query i, base row j
    upper = s[np.triu_indices(65, 1)]
    threshold = np.sort(upper)[len(upper) // 2]                        # one of the returned f32 values: a tie exactly at the threshold
    assert threshold.dtype == np.float32 and (upper == threshold).any()
    res = engine.graph(r, threshold)
    check_shape(res, 65)
    a, b, got = res.edges()
    assert np.array_equal(got.view(np.uint32), s[a, b].view(np.uint32))
    assert res.n_edges == int((upper >= threshold).sum())
    want = np.triu(s >= threshold, 1)
    assert np.array_equal(np.stack([a, b]), np.stack(np.nonzero(want)))


def test_placement_across_waves_column_blocks_steps_and_parts(engine):
    """300 equal rows among 333: a copy's segment is exactly the later copies, in order - its edges lie in all four waves, both
    column blocks, two steps and, under the split of 32, up to eleven parts"""
    r = rows(333, 13)
    copies = np.sort(np.random.default_rng(14).permutation(333)[:300])
    r[copies] = r[copies[0]]
    try:
        for split in (0, 32):
            engine.set_neighbour_split(split)
            res = engine.graph(r, 0.99)
            check_shape(res, 333)
            assert res.n_edges == 300 * 299 // 2 == 44850
            for k, i in enumerate(copies):
                assert np.array_equal(res.col[res.indptr[i]:res.indptr[i + 1]], copies[k + 1:]), (split, i)
            others = np.setdiff1d(np.arange(333), copies)
            assert (np.diff(res.indptr)[others] == 0).all()
            a, b, s = res.edges()
            assert (s.view(np.uint32) == s.view(np.uint32)[0]).all() and abs(float(s[0]) - 1.0) <= 1e-5      # one pair of rows, one value
            cl = engine.cluster(r, 0.99)
            assert np.array_equal(res.degree(), cl.degree) and np.array_equal(res.components(), cl.label), split
    finally:
        engine.set_neighbour_split(0)


def test_complete_graph(engine, data):
    r = data["rows"]
    n = len(r)
    engine.set_neighbour_split(0)
    res = engine.graph(r, -1.0)
    check_shape(res, n)
    i = np.arange(n + 1, dtype=np.int64)
    assert np.array_equal(res.indptr, i * (2 * n - i - 1) // 2) and res.n_edges == n * (n - 1) // 2
    for k in range(n):
        assert np.array_equal(res.col[res.indptr[k]:res.indptr[k + 1]], np.arange(k + 1, n)), k


def test_edges_of_the_interface(engine, data):
    engine.set_neighbour_split(0)
    r = np.tile(rows(1, 4), (70, 1))
    r[1] = 0
    r[3, 100] = np.nan
    r[65, 511] = np.inf
    for metric in ("cosine", "dot"):
        got = engine.graph(r, 0.5, metric)
        check_shape(got, 70)
        indptr, col, _ = sequence.threshold_graph(r, 0.5, metric)
        assert np.array_equal(got.indptr, indptr) and np.array_equal(got.col, col), metric
        bad = [3, 65] + ([1] if metric == "cosine" else [])          # a zero row is valid under dot, and 0 < 0.5 joins nobody
        assert (np.diff(got.indptr)[[1, 3, 65]] == 0).all() and not np.isin(got.col, [1, 3, 65]).any()
        assert list(np.flatnonzero(~got.valid)) == sorted(bad) and got.n_edges == 67 * 66 // 2
        cl = engine.cluster(r, 0.5, metric)
        assert np.array_equal(got.degree(), cl.degree) and np.array_equal(got.components(), cl.label), metric
    got = engine.graph(r[:0], 0.5)
    assert same_bits(csr(got), (np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))) and got.n == 0 and got.n_edges == 0
    got = engine.graph(r[:1], 0.5)
    assert list(got.indptr) == [0, 0] and got.n_edges == 0 and list(got.components()) == [0]
    p = data["rows"]
    got = engine.graph(p, 1.5)                                         # above every similarity, the twins' included: no edge, no fill launch
    check_shape(got, len(p))
    assert got.n_edges == 0 and (got.indptr == 0).all() and np.array_equal(got.components(), np.arange(len(p)))
    buf, ptr = engine.alloc(p.nbytes), engine.alloc(8 * (len(p) + 1))
    try:
        buf.upload(p)
        assert engine.graph_count_dev(buf.ptr, len(p), 1.5, ptr.ptr) == 0
        engine.graph_fill_dev(buf.ptr, len(p), 1.5, None, None, 0)     # a total of 0 accepts null outputs
        engine.sync()
        assert (ptr.download((len(p) + 1,), np.int64) == 0).all()
    finally:
        buf.free()
        ptr.free()


def test_errors(engine, data):
    p = data["rows"]
    n = len(p)
    engine.set_neighbour_split(0)
    with pytest.raises(GnnError, match=r"gnn_graph_count: threshold nan is outside .* finite"):
        engine.graph(p, float("nan"))
    with pytest.raises(GnnError, match=r"gnn_graph_count: threshold inf is outside .* finite"):
        engine.graph(p, float("inf"))
    with pytest.raises(GnnError, match=r"gnn_graph_count: metric 9 is outside \[0, 1\]"):
        engine.graph(p, 0.5, 9)
    with pytest.raises(GnnError, match=r"gnn_graph_count_dev: -1 rows is outside \[0, 2\^31\)"):
        engine.graph_count_dev(0, -1, 0.5, 0)
    with pytest.raises(GnnError, match=r"gnn_graph_fill_dev: -1 rows is outside \[0, 2\^31\)"):
        engine.graph_fill_dev(0, -1, 0.5, 0, 0, 0)
    with pytest.raises(GnnError, match=r"gnn_graph_fill_dev: threshold nan is outside .* finite"):
        engine.graph_fill_dev(0, 3, float("nan"), 0, 0, 0)
    total = engine.graph(p, 0.8).n_edges
    bufs = [engine.alloc(p.nbytes), engine.alloc(8 * (n + 1)), engine.alloc(4 * total), engine.alloc(4 * total)]
    try:
        bufs[0].upload(p)
        with NNEngine(0) as fresh:                                     # an engine that never counted
            with pytest.raises(GnnError, match=r"error -3: gnn_graph_fill_dev: no gnn_graph_count\* of the same \(n, threshold, metric\)"):
                fresh.graph_fill_dev(bufs[0].ptr, n, 0.8, bufs[2].ptr, bufs[3].ptr, total)
            with pytest.raises(GnnError, match=r"error -3: gnn_graph_fill: no gnn_graph_count of the same"):
                check(fresh.lib.gnn_graph_fill(fresh.ctx, n, 0.8, 0, None, None, total))
        assert engine.graph_count_dev(bufs[0].ptr, n, 0.8, bufs[1].ptr) == total
        with pytest.raises(GnnError, match=r"error -3: gnn_graph_fill_dev: no gnn_graph_count\* of the same"):
            engine.graph_fill_dev(bufs[0].ptr, n, 0.9, bufs[2].ptr, bufs[3].ptr, total)          # another threshold
        with pytest.raises(GnnError, match=r"error -3: gnn_graph_fill_dev"):
            engine.graph_fill_dev(bufs[0].ptr, n - 1, 0.8, bufs[2].ptr, bufs[3].ptr, total)      # another n
        with pytest.raises(GnnError, match=r"error -3: gnn_graph_fill_dev"):
            engine.graph_fill_dev(bufs[0].ptr, n, 0.8, bufs[2].ptr, bufs[3].ptr, total, "dot")   # another metric
        with pytest.raises(GnnError, match=rf"error -1: gnn_graph_fill_dev: capacity {total - 1} is below the {total} edges"):
            engine.graph_fill_dev(bufs[0].ptr, n, 0.8, bufs[2].ptr, bufs[3].ptr, total - 1)
        engine.graph_fill_dev(bufs[0].ptr, n, 0.8, bufs[2].ptr, bufs[3].ptr, total)              # the count still stands
        engine.sync()
        want = engine.graph(p, 0.8)
        assert same_bits((bufs[1].download((n + 1,), np.int64), bufs[2].download((total,), np.int32), bufs[3].download((total,), np.float32)),
                         csr(want))
        # the host fill reads the rows its count uploaded: another host search replaces them
        engine.neighbours(p[:5], None, 2)
        with pytest.raises(GnnError, match=r"error -3: gnn_graph_fill: .*another search has replaced the rows"):
            check(engine.lib.gnn_graph_fill(engine.ctx, n, 0.8, 0, None, None, total))
    finally:
        for buf in bufs:
            buf.free()
    with pytest.raises(ValueError, match=rf"{total} edges at the threshold 0\.8, more than max_edges = {total - 1}"):
        engine.graph(p, 0.8, max_edges=total - 1)
    assert same_bits(csr(engine.graph(p, 0.8, max_edges=total)), csr(want))                     # the next call on the same engine works


def test_embed_contigs_to_graph_end_to_end(engine):
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
    idx0, sim0 = engine.neighbours(emb, None, 3)
    res = engine.graph(emb, 0.999)
    idx1, sim1 = engine.neighbours(emb, None, 3)              # the searches share the fragment buffers
    after, _ = engine.classify_contigs(seq, offsets)
    check_shape(res, 12)
    assert 9 in res.col[res.indptr[4]:res.indptr[5]]
    cl = engine.cluster(emb, 0.999)
    assert np.array_equal(res.degree(), cl.degree) and np.array_equal(res.components(), cl.label)
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    assert np.array_equal(idx0, idx1) and np.array_equal(sim0.view(np.uint32), sim1.view(np.uint32))
