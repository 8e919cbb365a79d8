"""Clusters among encoder embeddings on the MI355X: the four arrays against the numpy definition (sequence.threshold_clusters) - exactly,
on planted rows whose fp64 similarities keep 1e-4 from the threshold (tests/test_clusters_host.py asserts it; the device's f32 values
are within 1e-5) and on integer rows whose dots are exact with many ties at the threshold -, independence of how the base is split
over workgroups, the device's own values (the edges of cluster are those of the similarities neighbours returns, for i < j), many
joins of one tree at once, the edges of the interface, and embed_contigs -> cluster end to end.  333 rows are six 64-row tiles and two
256-column steps, off every boundary, and tiles 1 to 5 each begin inside a step."""
import numpy as np
import pytest

from genomad_amd import sequence, synthetic
from genomad_amd._lib import GnnError
from tests.clusters_data import THRESHOLDS, components, device_edges, planted
from tests.neighbours_data import rows

pytestmark = pytest.mark.gpu

FIELDS = sequence.CLUSTER_FIELDS


def arrays(res):
    return [getattr(res, k) for k in FIELDS]


def same(got, want):
    return len(got) == len(want) == 4 and all(a.dtype == np.int64 and a.shape == b.shape and np.array_equal(a, b) for a, b in zip(got, want))


@pytest.fixture(scope="module")
def data():
    """the planted rows and the definition's answer at both thresholds, computed once"""
    r, groups = planted()
    return {"rows": r, "groups": groups, "want": {t: sequence.threshold_clusters(r, t) for t in THRESHOLDS}}


@pytest.fixture(scope="module")
def found(engine, data):
    """the device's answer at both thresholds, computed once with the library's own split"""
    engine.set_neighbour_split(0)
    return {t: engine.cluster(data["rows"], t) for t in THRESHOLDS}


@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_planted_clusters_equal_the_definition(data, found, threshold):
    res, want = found[threshold], data["want"][threshold]
    for k, a, b in zip(FIELDS, arrays(res), want):
        assert a.dtype == np.int64 and np.array_equal(a, b), (k, np.flatnonzero(a != b)[:10])
    assert res.threshold == float(np.float32(threshold)) and res.metric == "cosine"
    assert res.n_edges == int(want[1].sum()) // 2 and res.n_clusters == int((want[0] == np.arange(len(want[0]))).sum())
    big = [c for c in res.table() if c["size"] > 1]
    assert sorted(c["size"] for c in big) == [2] + [12] * 5 + [24]
    assert [c["edges"] < c["size"] * (c["size"] - 1) // 2 for c in big] == [c["size"] == 24 for c in big]    # the chain alone is no clique


@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_results_do_not_depend_on_the_split_and_the_device_path_agrees(engine, data, found, threshold):
    r, first = data["rows"], arrays(found[threshold])
    try:
        for split in (32, 100, 333, 4096, 0):
            engine.set_neighbour_split(split)
            assert same(arrays(engine.cluster(r, threshold)), first), split
        engine.set_neighbour_split(100)
        bufs = [engine.alloc(r.nbytes)] + [engine.alloc(8 * len(r)) for _ in range(4)]
        try:
            bufs[0].upload(r)
            engine.cluster_dev(bufs[0].ptr, len(r), threshold, *(b.ptr for b in bufs[1:]))
            engine.sync()
            assert same([b.download((len(r),), np.int64) for b in bufs[1:]], first)
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
    upper = dots[np.triu_indices(200, 1)]
    threshold = float(np.median(upper))                                # the median pair's dot: about half of the 19 900 pairs are edges
    assert (upper == threshold).sum() > 10 and 0.3 < (upper >= threshold).mean() < 0.7
    want = sequence.threshold_clusters(base, threshold, "dot")
    assert same(want, components(dots >= threshold))
    try:
        for split in (0, 32):
            engine.set_neighbour_split(split)
            assert same(arrays(engine.cluster(base, threshold, "dot")), want), split
    finally:
        engine.set_neighbour_split(0)


def test_the_edges_are_those_of_the_similarities_neighbours_returns(engine):
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
    want = components(device_edges(s, threshold))
    res = engine.cluster(r, threshold)
    for k, a, b in zip(FIELDS, arrays(res), want):
        assert np.array_equal(a, b), (k, np.flatnonzero(a != b)[:10])
    assert res.n_edges == int((upper >= threshold).sum())


def test_many_joins_of_one_tree_at_once(engine):
    r = rows(333, 13)
    copies = np.sort(np.random.default_rng(14).permutation(333)[:300])
    r[copies] = r[copies[0]]
    want = sequence.threshold_clusters(r, 0.99)
    try:
        for split in (0, 32):
            engine.set_neighbour_split(split)
            got = engine.cluster(r, 0.99)
            assert (got.label[copies] == copies[0]).all() and (got.rep[copies] == copies[0]).all()
            assert (got.degree[copies] == 299).all() and (got.size[copies] == 300).all()
            assert same(arrays(got), want), split
            assert got.n_clusters == 34 and got.n_edges == 300 * 299 // 2
    finally:
        engine.set_neighbour_split(0)


def test_edges_of_the_interface(engine, data):
    engine.set_neighbour_split(0)
    r = np.tile(rows(1, 4), (70, 1))
    r[1] = 0
    r[3, 100] = np.nan
    r[65, 511] = np.inf
    bad = np.isin(np.arange(70), [1, 3, 65])
    for metric in ("cosine", "dot"):
        got = engine.cluster(r, 0.5, metric)
        assert same(arrays(got), sequence.threshold_clusters(r, 0.5, metric)), metric
        invalid = bad & ~((np.arange(70) == 1) & (metric == "dot"))      # a zero row is valid under dot, and 0 < 0.5 joins nobody
        assert (got.label[invalid] == -1).all() and (got.degree[invalid] == 0).all() and (got.size[invalid] == 0).all()
        assert (got.rep[invalid] == -1).all() and (got.label[~bad] == 0).all() and (got.size[~bad] == 67).all()
    got = engine.cluster(r[:0], 0.5)
    assert all(a.dtype == np.int64 and a.shape == (0,) for a in arrays(got)) and got.n_clusters == 0 and got.n_edges == 0
    assert [list(a) for a in arrays(engine.cluster(r[:1], 0.5))] == [[0], [0], [1], [0]]
    p = data["rows"]
    got = engine.cluster(p, 1.5)                                       # above every similarity, the twins' included: all singletons
    assert same(arrays(got), sequence.threshold_clusters(p, 1.5)) and got.n_clusters == len(p) and got.n_edges == 0
    got = engine.cluster(p, -1.0)                                      # one cluster of all rows
    assert same(arrays(got), sequence.threshold_clusters(p, -1.0)) and got.n_clusters == 1 and (got.degree == len(p) - 1).all()
    assert (got.rep == 0).all()
    with pytest.raises(GnnError, match=r"gnn_cluster: threshold nan is outside .* finite"):
        engine.cluster(p, float("nan"))
    with pytest.raises(GnnError, match=r"gnn_cluster: threshold inf is outside .* finite"):
        engine.cluster(p, float("inf"))
    with pytest.raises(GnnError, match=r"gnn_cluster: metric 9 is outside \[0, 1\]"):
        engine.cluster(p, 0.5, 9)
    with pytest.raises(GnnError, match=r"gnn_cluster_dev: -1 rows is outside \[0, 2\^31\)"):
        engine.cluster_dev(0, -1, 0.5, 0, 0, 0, 0)


def test_embed_contigs_to_clusters_end_to_end(engine):
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
    res = engine.cluster(emb, 0.999)
    idx1, sim1 = engine.neighbours(emb, None, 3)              # the searches share the fragment buffers
    after, _ = engine.classify_contigs(seq, offsets)
    assert res.label[4] == res.label[9] == 4 and res.size[4] == res.size[9] >= 2 and res.degree[4] >= 1 and res.degree[9] >= 1
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    assert np.array_equal(idx0, idx1) and np.array_equal(sim0.view(np.uint32), sim1.view(np.uint32))
