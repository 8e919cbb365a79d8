"""The density-aware linkage tree among encoder embeddings on the MI355X: min_points 1 against NNEngine.linkage bit for bit, the core
similarities against NNEngine.neighbours' own lists, the tree against a brute-force Kruskal over the device's own f32 values and core
(indices and bits), exactly against the numpy definition on integer rows with ties and invalid rows, independence of the split and of
the entry point, its cut against NNEngine.density, its weights against fp64, the bound on the rounds, the edges of the interface, and
embed_contigs -> density_tree -> hdbscan end to end.  The shapes are the family's own (tests/test_linkage_gpu.py)."""
import ctypes as C
import math

import numpy as np
import pytest

from genomad_amd import sequence, synthetic
from genomad_amd._lib import GnnError
from tests.clusters_data import THRESHOLDS, planted
from tests.density_tree_data import last_finite, mutual, same_tree
from tests.linkage_data import (bits, check_shape, device_values, integer_rows, integer_rows_with_two_invalid, interface_rows, kruskal,
                                many_copies, same)
from tests.neighbours_data import rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def data(engine):
    """the planted rows, rows(65, 9) and the device's own pair values of both, computed once and left unchanged"""
    engine.set_neighbour_split(0)
    r, groups = planted()
    r65 = rows(65, 9)
    return {"planted": r, "groups": groups, "rows65": r65, "values": {"planted": device_values(engine, r), "rows65": device_values(engine, r65)}}


@pytest.fixture(scope="module")
def found(engine, data):
    """the device's trees of the planted rows at min_points 5, with the library's own split"""
    engine.set_neighbour_split(0)
    return engine.density_tree(data["planted"], 5)


def check_tree(res, n, m):
    check_shape(res, n)
    assert res.core.dtype == np.float32 and res.core.shape == (n,) and res.min_points == m
    assert np.array_equal(np.isnan(res.core), res.valid == 0) or res.n_valid < 2


@pytest.mark.parametrize("metric", ("cosine", "dot"))
@pytest.mark.parametrize("which", ("planted", "integer"))
def test_min_points_1_is_linkage_bit_for_bit(engine, data, which, metric):
    r = data["planted"] if which == "planted" else integer_rows_with_two_invalid()
    try:
        for split in (0, 32):
            engine.set_neighbour_split(split)
            want = engine.linkage(r, metric)
            res = engine.density_tree(r, 1, metric)
            check_tree(res, len(r), 1)
            assert same(res, want), split              # a, b, the bits of sim, valid and rounds
            assert np.array_equal(res.core[res.valid == 1], np.full(res.n_valid, np.inf, np.float32))
    finally:
        engine.set_neighbour_split(0)


@pytest.mark.parametrize("m", (2, 5, 65))
def test_core_is_the_last_finite_entry_of_the_neighbour_list(engine, data, m):
    engine.set_neighbour_split(0)
    r = data["planted"]
    res = engine.density_tree(r, m)
    check_tree(res, 333, m)
    assert np.array_equal(bits(res.core), bits(last_finite(engine.neighbours(r, None, m - 1)[1])))
    assert np.array_equal(bits(res.core), bits(engine.neighbours(r, None, m - 1)[1][:, -1]))       # 332 partners: no padding here


def test_core_of_nan_padded_lists(engine, data):
    """40 valid rows at min_points 65: every list has 39 entries and 25 NaN; core is the least similar partner there is"""
    engine.set_neighbour_split(0)
    r = data["planted"][:42].copy()
    r[7, 3] = np.nan
    r[30] = 0
    res = engine.density_tree(r, 65)
    check_tree(res, 42, 65)
    sim = engine.neighbours(r, None, 64)[1]
    assert res.n_valid == 40 and np.isnan(sim[:, 39:]).all() and not np.isnan(sim[res.valid == 1][:, :39]).any()
    assert np.array_equal(bits(res.core), bits(last_finite(sim))) and np.isnan(res.core[[7, 30]]).all()
    assert np.array_equal(bits(res.core[res.valid == 1]), bits(sim[res.valid == 1][:, 38]))


@pytest.mark.parametrize("m", (2, 5, 17))
@pytest.mark.parametrize("which", ("rows65", "planted"))
def test_the_tree_is_kruskal_over_the_devices_values_and_core(engine, data, which, m):
    """pins the value min(v(i, j), core_i, core_j) with v of the orientation (query i, base row j, i < j), the order and the tie rule"""
    engine.set_neighbour_split(0)
    r, s = data[which], data["values"][which]
    res = engine.density_tree(r, m)
    check_tree(res, len(r), m)
    assert not np.isnan(s[np.triu_indices(len(r), 1)]).any()
    want = kruskal(mutual(s, res.core))
    assert want[2].dtype == np.float32 and same(res, want), np.flatnonzero((res.a != want[0]) | (res.b != want[1]))[:10]
    assert len(np.unique(res.sim)) < len(res.sim) or m == 2          # mutual reachability ties


def test_integer_dots_with_invalid_rows_equal_the_definition(engine):
    base = integer_rows_with_two_invalid()
    try:
        for m in (2, 5):
            a, b, sim, core, valid = sequence.mutual_reachability_tree(base, m, "dot")
            assert len(a) == 197 and len(np.unique(sim)) < len(sim)
            for split in (0, 32):
                engine.set_neighbour_split(split)
                res = engine.density_tree(base, m, "dot")
                check_tree(res, 200, m)
                assert same(res, (a, b, sim)) and np.array_equal(res.valid, valid) and res.metric == "dot", (m, split)
                assert np.array_equal(bits(res.core), bits(core)) and res.valid[[5, 77]].tolist() == [0, 0]
                assert not np.isin([5, 77], np.concatenate([res.a, res.b])).any()
    finally:
        engine.set_neighbour_split(0)


def test_many_copies_give_one_value_in_index_order(engine):
    r, copies = many_copies()
    engine.set_neighbour_split(0)
    res = engine.density_tree(r, 5)
    check_tree(res, 333, 5)
    assert res.n_edges == 332
    assert (res.a[:299] == copies[0]).all() and np.array_equal(res.b[:299], copies[1:]) and len(set(bits(res.sim[:299]))) == 1
    assert len(set(bits(res.core[copies]))) == 1 and bits(res.core[copies[0]]) == bits(res.sim[0])


def test_results_do_not_depend_on_the_split_and_the_device_path_agrees(engine, data, found):
    r = data["planted"]
    try:
        for split in (32, 64, 0):
            engine.set_neighbour_split(split)
            assert same_tree(engine.density_tree(r, 5), found), split
        engine.set_neighbour_split(64)
        buf = engine.alloc(r.nbytes)
        try:
            buf.upload(r)
            assert same_tree(engine.density_tree_dev(buf.ptr, len(r), 5), found)
        finally:
            buf.free()
    finally:
        engine.set_neighbour_split(0)


def test_the_cut_is_density_at_its_core_rows_integer_dots(engine):
    """values are exact and symmetric: thresholds equal to pair values and to core values tie exactly"""
    base = integer_rows_with_two_invalid()
    engine.set_neighbour_split(0)
    for m in (2, 5):
        res = engine.density_tree(base, m, "dot")
        core = np.unique(res.core[res.valid == 1])
        ts = [float(res.sim[k]) for k in (0, 20, 100, 196)] + [float(core[0]), float(core[len(core) // 2]), float(core[-1])]
        for t in ts + [float(core[-1]) + 1, 0.0]:
            d = engine.density(base, t, m, "dot")
            assert np.array_equal(res.cut(t), np.where(d.kind == 3, d.label, -1)), (m, t)
            assert res.cluster_counts([t]).tolist() == [int(((d.kind == 3) & (d.label == np.arange(200))).sum())], (m, t)


def test_the_cut_is_density_at_its_core_rows_planted(engine, data, found):
    r, s = data["planted"], data["values"]["planted"]
    engine.set_neighbour_split(0)
    off = ~np.eye(len(r), dtype=bool)
    for t in THRESHOLDS:
        assert np.abs(s[off].astype(np.float64) - t).min() > 1e-5, t       # no pair value, in either orientation, near the threshold
        for m, res in ((5, found), (10, engine.density_tree(r, 10))):
            d = engine.density(r, t, m)
            assert np.array_equal(res.cut(t), np.where(d.kind == 3, d.label, -1)), (m, t)
            assert (d.kind == 3).any() and (d.kind != 3).any()


def test_the_weights_are_within_1e_5_of_fp64(data, found):
    """1e-5 is the bound for a pair's value (README, nearest neighbours); a minimum of perturbed values moves by at most the largest
    perturbation, and so does the k-th largest weight of the tree."""
    a, b, sim, core, valid = sequence.mutual_reachability_tree(data["planted"], 5)
    assert found.n_edges == 332 == len(a) and found.n_valid == 333
    err = float(np.abs(np.sort(found.sim).astype(np.float64) - np.sort(sim).astype(np.float64)).max())
    cerr = float(np.abs(found.core.astype(np.float64) - core.astype(np.float64)).max())
    print(f"largest |sorted device weight - sorted fp64 weight| = {err:.3g}, largest |device core - fp64 core| = {cerr:.3g}")
    assert err <= 1e-5 and cerr <= 1e-5
    assert np.array_equal(found.matrix()[:, 2], 1.0 - found.sim.astype(np.float64)) and len(found.table()) == 332
    for g in ("family0", "family3"):                                   # a family of 12 is one cluster of core rows at 0.8
        assert len(set(found.cut(0.8)[data["groups"][g]])) == 1 and found.cut(0.8)[data["groups"][g]][0] >= 0


def test_rounds_and_the_edges_of_the_interface(engine, data, found):
    engine.set_neighbour_split(0)
    assert 1 <= found.rounds <= math.ceil(math.log2(333))
    r = interface_rows()
    for metric in ("cosine", "dot"):
        res = engine.density_tree(r, 3, metric)
        check_tree(res, 70, 3)
        bad = [3, 65] if metric == "dot" else [1, 3, 65]
        assert res.valid[bad].tolist() == [0] * len(bad) and res.n_valid == 70 - len(bad) == res.n_edges + 1
        assert np.isnan(res.core[bad]).all() and (res.cut(0.5)[bad] == -1).all()
    for n in (0, 1):
        res = engine.density_tree(r[:n], 5)
        check_tree(res, n, 5)
        assert res.n_edges == 0 and res.rounds == 0
    assert np.isnan(engine.density_tree(r[:1], 5).core[0])             # one valid row: no partner
    res = engine.density_tree(np.zeros((5, 512), np.float32), 2)       # no row is valid
    check_tree(res, 5, 2)
    assert res.n_valid == 0 and res.n_edges == 0 and np.isnan(res.core).all()
    for m in (0, 66, 2.5, True):
        with pytest.raises(ValueError, match="min_points"):
            engine.density_tree(r, m)
    with pytest.raises(ValueError, match="metric 'l2'"):
        engine.density_tree(r, 5, "l2")
    # the library's own checks come before anything is written
    a, b, sim = np.full(69, 7, np.int64), np.full(69, 7, np.int64), np.full(69, 7, np.float32)
    core, valid = np.full(70, 7, np.float32), np.full(70, 7, np.uint8)
    n_edges, rounds = C.c_int64(7), C.c_int64(7)
    for fn, name in ((engine.lib.gnn_density_tree, "gnn_density_tree"), (engine.lib.gnn_density_tree_dev, "gnn_density_tree_dev")):
        for m, metric, what in ((0, 0, "min_points 0 is outside"), (66, 0, "min_points 66 is outside"), (5, 9, "metric 9 is outside")):
            assert fn(engine.ctx, r.ctypes.data, 70, m, metric, a.ctypes.data, b.ctypes.data, sim.ctypes.data, core.ctypes.data,
                      valid.ctypes.data, C.addressof(n_edges), C.addressof(rounds)) != 0
            assert f"{name}: {what}" in engine.lib.gnn_last_error().decode()
            assert (a == 7).all() and (b == 7).all() and (sim == 7).all() and (core == 7).all() and (valid == 7).all()
            assert (n_edges.value, rounds.value) == (7, 7)
    with pytest.raises(GnnError, match=r"gnn_density_tree_dev: -1 rows is outside \[0, 2\^31\)"):
        engine.density_tree_dev(0, -1)
    small = engine.density_tree(data["rows65"][:9], 3)                 # a small call after the large ones
    check_tree(small, 9, 3)
    assert small.n_edges == 8 and same(small, kruskal(mutual(data["values"]["rows65"][:9, :9], small.core)))


def test_embed_contigs_to_hdbscan_end_to_end(engine):
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
    res = engine.density_tree(emb, 2)
    idx1, sim1 = engine.neighbours(emb, None, 3)              # the searches share the fragment buffers
    after, _ = engine.classify_contigs(seq, offsets)
    check_tree(res, 12, 2)
    assert (res.a[0], res.b[0]) == (4, 9) and res.n_edges == 11
    assert np.array_equal(bits(res.core), bits(sim0[:, 0]))
    got = res.hdbscan(2)
    want = sequence.hdbscan_clusters(res.a, res.b, res.sim, res.valid, 2)
    assert np.array_equal(got["label"], want["label"]) and got["label"][4] == got["label"][9]
    assert np.array_equal(got["lambda_out"], want["lambda_out"]) and got["lambda_out"][4] == got["lambda_out"][9]
    with pytest.raises(ValueError, match="cosine only"):
        engine.density_tree(emb, 2, "dot").hdbscan(2)
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    assert np.array_equal(idx0, idx1) and np.array_equal(sim0.view(np.uint32), sim1.view(np.uint32))
