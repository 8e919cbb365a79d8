"""Density clusters among encoder embeddings on the MI355X: the six arrays against the numpy definition (sequence.density_clusters) -
exactly, on planted rows whose fp64 similarities keep 1e-4 from the threshold and whose border rows' best and second-best core
neighbours keep 1e-4 from each other (tests/test_density_host.py asserts both; the device's f32 values are within 1e-5) and on 0/1
integer rows whose dots are exact, with hundreds of ties at the threshold and between anchors -, independence of how the base is split
over workgroups, the device's own values (edges, anchors and a border row's similarity are those of the similarities neighbours
returns, for i < j), the identities with cluster, many joins of one tree at once, the edges of the interface, and embed_contigs ->
density end to end.  333 rows are six 64-row tiles and two 256-column steps, off every boundary."""
import numpy as np
import pytest

from genomad_amd import sequence, synthetic
from genomad_amd._lib import GnnError
from tests.clusters_data import device_edges
from tests.density_data import T, dbscan, integer_case, planted, second_gap
from tests.neighbours_data import rows

pytestmark = pytest.mark.gpu

FIELDS = sequence.DENSITY_FIELDS
MIN_POINTS = (1, 3, 6, 11)
SPLITS = (32, 100, 333, 4096, 0)


def arrays(res):
    return [getattr(res, k) for k in FIELDS]


def check(got, want, sim_tol, what=""):
    """the five integer arrays equal; ``sim``: float32, NaN where ``want`` has NaN, within ``sim_tol`` elsewhere"""
    assert len(got) == len(want) == 6
    for k, a, b in zip(FIELDS, got, want):
        if k == "sim":
            assert a.dtype == np.float32 and a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)), (what, k)
            err = np.abs(a.astype(np.float64) - b)[~np.isnan(b)]
            assert (err <= sim_tol).all(), (what, k, err.max())
        else:
            assert a.dtype == (np.uint8 if k == "kind" else np.int64) and a.shape == b.shape, (what, k)
            assert np.array_equal(a, b), (what, k, np.flatnonzero(a != b)[:10])


def identical(got, first):
    """bit for bit, ``sim`` included"""
    return len(got) == len(first) == 6 and all(a.dtype == b.dtype and a.shape == b.shape and
                                               np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                                              b.view(np.uint32) if b.dtype == np.float32 else b) for a, b in zip(got, first))


@pytest.fixture(scope="module")
def data():
    """the planted rows and the definition's answer at every min_points, computed once"""
    r, groups = planted()
    return {"rows": r, "groups": groups, "want": {m: sequence.density_clusters(r, T, m) for m in MIN_POINTS}}


@pytest.fixture(scope="module")
def found(engine, data):
    """the device's answer at every min_points, computed once with the library's own split"""
    engine.set_neighbour_split(0)
    return {m: engine.density(data["rows"], T, m) for m in MIN_POINTS}


@pytest.mark.parametrize("min_points", MIN_POINTS)
def test_planted_density_clusters_equal_the_definition(data, found, min_points):
    res, want = found[min_points], data["want"][min_points]
    check(arrays(res), want, 1e-5, min_points)
    assert res.threshold == float(np.float32(T)) and res.min_points == min_points and res.metric == "cosine"
    kind = want[5]
    assert (res.n_core, res.n_border, res.n_noise) == (int((kind == 3).sum()), int((kind == 2).sum()), int((kind == 1).sum()))
    assert res.n_clusters == int((want[0] == np.arange(len(kind))).sum()) and len(res.table()) == res.n_clusters
    if min_points == 6:                                       # the bridges hang on to B, A, B and do not merge the two families
        g = data["groups"]
        assert (res.kind[g["bridges"]] == 2).all() and res.label[g["familyA"][0]] != res.label[g["familyB"][0]]
        assert np.array_equal(res.anchor[g["bridges"]], [g["familyB"][0], g["familyA"][1], g["familyB"][2]])
        assert res.kind[g["hanger"][1]] == 1 and res.n_clusters == 4


@pytest.mark.parametrize("min_points", MIN_POINTS)
def test_results_do_not_depend_on_the_split_and_the_device_path_agrees(engine, data, found, min_points):
    r, first = data["rows"], arrays(found[min_points])
    n = len(r)
    try:
        for split in SPLITS:
            engine.set_neighbour_split(split)
            assert identical(arrays(engine.density(r, T, min_points)), first), split
        engine.set_neighbour_split(100)
        bufs = [engine.alloc(r.nbytes)] + [engine.alloc(8 * n) for _ in range(4)] + [engine.alloc(4 * n), engine.alloc(n)]
        try:
            bufs[0].upload(r)
            engine.density_dev(bufs[0].ptr, n, T, min_points, *(b.ptr for b in bufs[1:]))
            engine.sync()
            got = [b.download((n,), t) for b, t in zip(bufs[1:], [np.int64] * 4 + [np.float32, np.uint8])]
            assert identical(got, first)
        finally:
            for buf in bufs:
                buf.free()
    finally:
        engine.set_neighbour_split(0)


def test_integer_dots_with_ties_at_the_threshold_and_between_anchors(engine):
    r, dots, threshold, min_points = integer_case()            # every dot is an integer below 512: exact on the device
    adj = dots >= threshold
    adj[np.arange(len(r)), np.arange(len(r))] = False
    want = sequence.density_clusters(r, threshold, min_points, "dot")
    brute = dbscan(adj, dots, min_points)
    for k, a, b in zip(FIELDS, want, brute):
        assert np.array_equal(a, b, equal_nan=(k == "sim")), k
    assert (dots[np.triu_indices(len(r), 1)] == threshold).sum() >= 10
    assert (second_gap(adj, dots, brute) == 0).sum() >= 10    # borders whose two best anchors tie: the smaller index must win
    try:
        for split in (0, 32):
            engine.set_neighbour_split(split)
            check(arrays(engine.density(r, threshold, min_points, "dot")), want, 0.0, split)
    finally:
        engine.set_neighbour_split(0)


def test_edges_anchors_and_similarities_are_those_neighbours_returns(engine):
    """pins the orientation (query i, base row j, i < j), the >=, the anchor's argmax over the device's own f32 and sim's bits"""
    r = rows(65, 9)
    engine.set_neighbour_split(0)
    idx, sim = engine.neighbours(r, None, 64)
    assert (idx >= 0).all()
    s = np.full((65, 65), np.nan, np.float32)
    np.put_along_axis(s, idx, sim, axis=1)                             # s[i, j]: query i, base row j
    iu = np.triu_indices(65, 1)
    upper = s[iu]
    threshold = np.sort(upper)[(3 * len(upper)) // 4]                  # one of the returned f32 values: a tie exactly at the threshold
    assert threshold.dtype == np.float32 and (upper == threshold).any()
    adj = device_edges(s, threshold)
    sym = np.zeros((65, 65), np.float32)
    sym[iu] = upper
    sym = sym + sym.T                                                  # the pair's one value, at (i, j) and (j, i)
    min_points = int(np.median(adj.sum(axis=1))) + 1
    want = dbscan(adj, sym, min_points)
    assert (want[5] == 3).sum() >= 5 and (want[5] == 2).sum() >= 5     # core and border rows both exist
    res = engine.density(r, threshold, min_points)
    check(arrays(res), want, 0.0)
    border = np.flatnonzero(res.kind == 2)
    lo, hi = np.minimum(border, res.anchor[border]), np.maximum(border, res.anchor[border])
    assert np.array_equal(res.sim[border].view(np.uint32), s[lo, hi].view(np.uint32))


@pytest.mark.parametrize("threshold", (T, 0.3))
def test_degree_is_clusters_degree_and_min_points_one_is_its_label(engine, data, threshold):
    r = data["rows"]
    engine.set_neighbour_split(0)
    c = engine.cluster(r, threshold)
    one = engine.density(r, threshold, 1)
    assert np.array_equal(one.label, c.label) and np.array_equal(one.degree, c.degree) and np.array_equal(one.size, c.size)
    assert np.array_equal(one.kind, np.where(c.label >= 0, 3, 0)) and np.isnan(one.sim).all()
    two = engine.density(r, threshold, 2)
    assert np.array_equal(two.degree, c.degree) and np.array_equal(two.kind == 3, c.degree > 0) and two.n_border == 0
    assert np.array_equal(two.label[two.kind == 3], c.label[two.kind == 3]) and np.array_equal(two.kind == 1, c.size == 1)
    assert np.array_equal(engine.density(r, threshold, 7).degree, c.degree)


def test_many_joins_of_one_tree_at_once(engine):
    r = rows(333, 13)
    copies = np.sort(np.random.default_rng(14).permutation(333)[:300])
    r[copies] = r[copies[0]]
    rest = np.setdiff1d(np.arange(333), copies)
    try:
        for split in (0, 32):
            engine.set_neighbour_split(split)
            got = engine.density(r, 0.99, 300)                         # the 300 copies see each other: all core, one cluster
            check(arrays(got), sequence.density_clusters(r, 0.99, 300), 1e-5, split)
            assert (got.kind[copies] == 3).all() and (got.label[copies] == copies[0]).all() and (got.size[copies] == 300).all()
            assert (got.degree[copies] == 299).all() and (got.kind[rest] == 1).all() and got.n_clusters == 1
            got = engine.density(r, 0.99, 301)                         # one more: nothing is core, every row is noise
            assert (got.kind == 1).all() and (got.label == -1).all() and (got.anchor == -1).all() and (got.size == 0).all()
            assert (got.degree[copies] == 299).all() and np.isnan(got.sim).all()
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
        for min_points in (67, 68):                                    # 67 equal rows: all core, or none
            got = engine.density(r, 0.5, min_points, metric)
            check(arrays(got), sequence.density_clusters(r, 0.5, min_points, metric), 1e-5, (metric, min_points))
            invalid = bad & ~((np.arange(70) == 1) & (metric == "dot"))      # a zero row is valid under dot, and 0 < 0.5: noise
            assert (got.kind[invalid] == 0).all() and (got.label[invalid] == -1).all() and (got.anchor[invalid] == -1).all()
            assert (got.degree[invalid] == 0).all() and (got.size[invalid] == 0).all() and np.isnan(got.sim[invalid]).all()
            assert (got.kind[~bad] == (3 if min_points == 67 else 1)).all() and (got.degree[~bad] == 66).all()
            if metric == "dot":
                assert got.kind[1] == 1 and got.label[1] == -1
    got = engine.density(r[:0], 0.5)
    assert [a.dtype for a in arrays(got)] == [np.int64] * 4 + [np.float32, np.uint8] and all(a.shape == (0,) for a in arrays(got))
    assert (got.n_clusters, got.n_core, got.n_border, got.n_noise) == (0, 0, 0, 0) and got.table() == []
    one = engine.density(r[:1], 0.5, 1)                                # one valid row: core at 1, noise at 2
    assert [int(a[0]) for a in arrays(one)[:4]] == [0, 0, 1, 0] and one.kind[0] == 3 and np.isnan(one.sim[0])
    one = engine.density(r[:1], 0.5, 2)
    assert [int(a[0]) for a in arrays(one)[:4]] == [-1, 0, 0, -1] and one.kind[0] == 1 and np.isnan(one.sim[0])
    p = data["rows"]
    got = engine.density(p, 1.5, 1)                                    # above every similarity, the twins' included: all alone
    check(arrays(got), sequence.density_clusters(p, 1.5, 1), 0.0)
    assert got.n_clusters == got.n_core == 331 and (got.degree == 0).all()
    assert engine.density(p, 1.5, 2).n_noise == 331
    got = engine.density(p, -1.0, 331)                                 # one cluster of all valid rows
    check(arrays(got), sequence.density_clusters(p, -1.0, 331), 0.0)
    assert got.n_clusters == 1 and got.n_core == 331 and (got.degree[got.kind == 3] == 330).all()
    assert engine.density(p, -1.0, 332).n_noise == 331
    with pytest.raises(GnnError, match=r"gnn_density: threshold nan is outside .* finite"):
        engine.density(p, float("nan"))
    with pytest.raises(GnnError, match=r"gnn_density: threshold inf is outside .* finite"):
        engine.density(p, float("inf"))
    with pytest.raises(GnnError, match=r"gnn_density: min_points 0 is outside \[1, 2\^31\)"):
        engine.density(p, 0.5, 0)
    with pytest.raises(GnnError, match=r"gnn_density: min_points 2147483648 is outside \[1, 2\^31\)"):
        engine.density(p, 0.5, 1 << 31)
    with pytest.raises(GnnError, match=r"gnn_density: metric 9 is outside \[0, 1\]"):
        engine.density(p, 0.5, 5, 9)
    with pytest.raises(GnnError, match=r"gnn_density_dev: -1 rows is outside \[0, 2\^31\)"):
        engine.density_dev(0, -1, 0.5, 5, 0, 0, 0, 0, 0, 0)
    with pytest.raises(GnnError, match=r"bad argument to gnn_density_dev: the rows and the six outputs are required"):
        engine.density_dev(0, 4, 0.5, 5, 0, 0, 0, 0, 0, 0)


def test_embed_contigs_to_density_end_to_end(engine):
    rng = np.random.default_rng(5)
    windows = synthetic.synth_windows(900, 30)
    contigs = [windows[a:a + n].reshape(-1)[:int(rng.integers((n - 1) * 6000 + 3000, n * 6000 + 1))]
               for a, n in zip(range(0, 24, 2), [1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 2])]
    contigs[9] = contigs[4].copy()                            # byte-identical to contig 4
    contigs[11] = contigs[4].copy()
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in contigs])]).astype(np.int64)
    seq = np.concatenate(contigs)
    engine.set_neighbour_split(0)
    before, _ = engine.classify_contigs(seq, offsets)
    _, emb, _ = engine.embed_contigs(seq, offsets)
    idx0, sim0 = engine.neighbours(emb, None, 3)
    res = engine.density(emb, 0.999, 3)
    idx1, sim1 = engine.neighbours(emb, None, 3)              # the searches share the fragment buffers
    after, _ = engine.classify_contigs(seq, offsets)
    trio = [4, 9, 11]
    assert (res.kind[trio] == 3).all() and (res.label[trio] == 4).all() and (res.size[trio] >= 3).all() and (res.degree[trio] >= 2).all()
    c = engine.cluster(emb, 0.999)
    assert np.array_equal(res.degree, c.degree)
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    assert np.array_equal(idx0, idx1) and np.array_equal(sim0.view(np.uint32), sim1.view(np.uint32))
