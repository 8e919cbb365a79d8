"""The single-linkage tree among encoder embeddings on the MI355X: the tree against the numpy definition (sequence.single_linkage_tree)
- exactly on integer rows whose dots are exact, with many ties -, against a brute-force Kruskal over the device's own f32 values
(indices and bits: orientation, order and the tie rule), its cut against NNEngine.cluster at thresholds that tie with merges, its
weights against fp64, independence of how the base is split over workgroups, many joins at once, the bound on the rounds, the edges of
the interface, and embed_contigs -> linkage end to end.  Second-scale shapes, those of tests/test_clusters_gpu.py: 333 rows are six
64-row tiles and two 256-column steps, off every boundary."""
import numpy as np
import pytest

from genomad_amd import sequence, synthetic
from genomad_amd._lib import GnnError
from tests.clusters_data import THRESHOLDS, planted
from tests.linkage_data import (bits, check_shape, device_values, integer_rows, integer_rows_with_two_invalid, interface_rows, kruskal,
                                many_copies, same)
from tests.neighbours_data import rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def data():
    """the planted rows and the float64 definition's tree, computed once"""
    r, groups = planted()
    return {"rows": r, "groups": groups, "want": sequence.single_linkage_tree(r)}


@pytest.fixture(scope="module")
def found(engine, data):
    """the device's tree of the planted rows, computed once with the library's own split"""
    engine.set_neighbour_split(0)
    return engine.linkage(data["rows"])


@pytest.mark.parametrize("invalid", (False, True))
def test_integer_dots_with_ties_equal_the_definition(engine, invalid):
    base = integer_rows_with_two_invalid() if invalid else integer_rows()
    a, b, sim, valid = sequence.single_linkage_tree(base, "dot")
    assert len(a) == (197 if invalid else 199) and len(np.unique(sim)) < len(sim)
    try:
        for split in (0, 32):
            engine.set_neighbour_split(split)
            res = engine.linkage(base, "dot")
            check_shape(res, 200)
            assert same(res, (a, b, sim)) and np.array_equal(res.valid, valid) and res.metric == "dot", split
            assert res.valid[[5, 77]].tolist() == ([0, 0] if invalid else [1, 1])
    finally:
        engine.set_neighbour_split(0)


@pytest.mark.parametrize("which", ("rows65", "planted"))
def test_the_tree_is_kruskal_over_the_values_neighbours_returns(engine, data, found, which):
    """pins the orientation (query i, base row j, i < j), the order, the tie rule, and that both searches compute the same f32"""
    engine.set_neighbour_split(0)
    r, res = (rows(65, 9), None) if which == "rows65" else (data["rows"], found)
    res = engine.linkage(r) if res is None else res
    check_shape(res, len(r))
    s = device_values(engine, r)
    assert not np.isnan(s[np.triu_indices(len(r), 1)]).any()
    want = kruskal(s)
    assert want[2].dtype == np.float32 and same(res, want), np.flatnonzero((res.a != want[0]) | (res.b != want[1]))[:10]


def test_the_cut_is_cluster(engine, data, found):
    r, res = data["rows"], found
    engine.set_neighbour_split(0)
    ties = [float(res.sim[k]) for k in (0, 78, 200)]                   # thresholds that are merges' own similarities: exact ties
    for t in THRESHOLDS + tuple(ties) + (-1.0, 1.5):
        c = engine.cluster(r, t)
        assert np.array_equal(res.cut(t), c.label), t
        assert res.cluster_counts([t]).tolist() == [c.n_clusters], t


def test_the_weights_are_within_1e_5_of_fp64(data, found):
    """1e-5 is the bound for a pair's value (README, nearest neighbours), and the k-th largest tree weight moves by at most the largest
    perturbation of a pair: #(edges >= t) = n_valid - components(t).  Measured on an MI355X: 5.4e-7."""
    a, b, sim, valid = data["want"]
    assert found.n_edges == 332 == len(a) and int((found.sim >= 0.9).sum()) == 79 and found.n_valid == 333
    err = float(np.abs(np.sort(found.sim).astype(np.float64) - np.sort(sim).astype(np.float64)).max())
    print(f"largest |sorted device weight - sorted fp64 weight| = {err:.3g}")
    assert err <= 1e-5
    assert found.rounds >= 2
    assert np.array_equal(found.matrix()[:, 2], 1.0 - found.sim.astype(np.float64))
    for g in ("family0", "chain", "pair"):                             # every planted group is one cluster at 0.9
        assert len(set(found.cut(0.9)[data["groups"][g]])) == 1


def test_results_do_not_depend_on_the_split_and_the_device_path_agrees(engine, data, found):
    r = data["rows"]
    try:
        for split in (32, 100, 333, 4096, 0):
            engine.set_neighbour_split(split)
            assert same(engine.linkage(r), found), split
        engine.set_neighbour_split(100)
        buf = engine.alloc(r.nbytes)
        try:
            buf.upload(r)
            assert same(engine.linkage_dev(buf.ptr, len(r)), found)
        finally:
            buf.free()
    finally:
        engine.set_neighbour_split(0)


def test_many_joins_at_once(engine):
    r, copies = many_copies()
    a, b, sim, valid = sequence.single_linkage_tree(r)
    try:
        for split in (0, 32):
            engine.set_neighbour_split(split)
            res = engine.linkage(r)
            check_shape(res, 333)
            assert res.n_edges == 332 and np.array_equal(res.a, a) and np.array_equal(res.b, b), split
            assert np.abs(res.sim.astype(np.float64) - sim.astype(np.float64)).max() <= 1e-5
            # 44 850 equal values: the tie rule names the smallest copy as a, the others in ascending order
            assert (res.a[:299] == copies[0]).all() and np.array_equal(res.b[:299], copies[1:]) and len(set(bits(res.sim[:299]))) == 1
    finally:
        engine.set_neighbour_split(0)


def test_edges_of_the_interface(engine, data):
    engine.set_neighbour_split(0)
    r = interface_rows()
    for metric in ("cosine", "dot"):
        res = engine.linkage(r, metric)
        check_shape(res, 70)
        a, b, sim, valid = sequence.single_linkage_tree(r, metric)
        assert np.array_equal(res.valid, valid) and np.array_equal(res.a, a) and np.array_equal(res.b, b), metric
        bad = [3, 65] if metric == "dot" else [1, 3, 65]               # a zero row is valid under dot
        assert res.valid[bad].tolist() == [0] * len(bad) and res.n_valid == 70 - len(bad) == res.n_edges + 1
        assert not np.isin(bad, np.concatenate([res.a, res.b])).any() and (res.cut(0.5)[bad] == -1).all()
        assert (res.a == 0).all()                                      # equal rows: every edge names the smallest one
    res = engine.linkage(r[:0])
    check_shape(res, 0)
    res = engine.linkage(r[:1])
    check_shape(res, 1)
    assert res.valid.tolist() == [1]
    res = engine.linkage(r[:2])                                        # row 1 is zero: two rows, one valid, no edge
    check_shape(res, 2)
    assert res.valid.tolist() == [1, 0] and res.n_edges == 0
    res = engine.linkage(r[4:6])
    check_shape(res, 2)
    assert (res.a.tolist(), res.b.tolist(), res.rounds) == ([0], [1], 1) and abs(float(res.sim[0]) - 1) <= 1e-5
    with pytest.raises(ValueError, match="metric 'l2'"):
        engine.linkage(r, "l2")
    with pytest.raises(GnnError, match=r"gnn_linkage: metric 9 is outside \[0, 1\]"):
        engine.linkage(r, 9)
    with pytest.raises(GnnError, match=r"gnn_linkage_dev: -1 rows is outside \[0, 2\^31\)"):
        engine.linkage_dev(0, -1)


def test_embed_contigs_to_linkage_end_to_end(engine):
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
    res = engine.linkage(emb)
    idx1, sim1 = engine.neighbours(emb, None, 3)              # the searches share the fragment buffers
    after, _ = engine.classify_contigs(seq, offsets)
    check_shape(res, 12)
    assert (res.a[0], res.b[0]) == (4, 9) and res.n_edges == 11 and len(res.table()) == 11
    assert np.array_equal(res.cut(0.999), engine.cluster(emb, 0.999).label)
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    assert np.array_equal(idx0, idx1) and np.array_equal(sim0.view(np.uint32), sim1.view(np.uint32))
