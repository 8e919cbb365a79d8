"""The single-linkage tree on the MI355X at the limits tests/test_linkage_gpu.py stays away from (inputs and their CPU-side conditions:
tests/linkage_limits_data.py, tests/embedding_limits_data.py, tests/test_linkage_limits_host.py).  What each group pins in
gnn_linkage.hip:

  negative values   the `u & 0x80000000 ? ~u` branch of lk_image under lk_shfl_xor, atomicMax, lk_pick_lo_kernel and lk_pick_hi_kernel
                    where it decides an edge; the host's sort of es[] and lk_value on negative records; +0 for a zero
  forest            valid rows whose every pair is NaN (elements beyond the f16 range under dot): the host's loop ends on the round
                    that adds no edge, never on `edges == capacity`; the outputs past n_edges
  dead tiles        `if (okm == 0) return;` on the first tile, `__all(cc < 0 ...) continue` on whole steps, an invalid row 0 and last row
  rounds            ceil(log2 n_valid) reached with equality, every pick of every round mutual (lk_link_kernel records an edge once, by
                    the smaller root) and tied; a star, where all picks but one are not mutual
  row scales        nn_prepare_kernel's per-row power of two, from all-subnormal rows to FLT_MAX, one-hot rows (values exactly 1, tied)
  small after large the grow-only workspaces shared with the neighbour search

References: the numpy definition (sequence.single_linkage_tree), exact on integer rows under dot, and under cosine the brute-force
Kruskal of tests/linkage_data.py over the device's own f32 values; indices and the bits of sim are compared on every edge.  The one
tolerance is the project's bound of 1e-5 on a pair's cosine value, which the k-th largest tree weight inherits (the argument is in
tests/test_linkage_gpu.py::test_the_weights_are_within_1e_5_of_fp64).

Measured on an MI355X (profiles/linkage/README.md, "At the limits"): sorted weights within 1.5e-7 (signed rows), 7.2e-7 (corners),
2.1e-7 (extreme rows) and 3.6e-7 (heavy rows) of the fp64 definition's; 8 rounds on ruler_path under both metrics, 7 without its last
row, 1 on simplex_star and negative_contest, 4 on corners and on the forest; no test here takes more than 0.2 s on the device."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from genomad_amd import _lib, sequence
from tests import embedding_limits_data as lim
from tests import linkage_limits_data as ld
from tests.embedding_limits_data import VALUE_TOL
from tests.linkage_data import bits, check_shape, device_values, kruskal, same
from tests.neighbours_data import rows

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def fixture_rows(name):
    """the rows of a named input, made once and read-only"""
    r = {"corners": lambda: ld.corners()[0], "simplex_star": lambda: ld.simplex_star()[0],
         "negative_contest": lambda: lim.negative_contest()[0], "ruler_path": ld.ruler_path,
         "dead_tiles": lambda: ld.dead_tiles()[0], "forest_rows": lambda: ld.forest_rows()[0],
         "signed_rows": lambda: lim.signed_rows(333, 8), "extreme_base": lim.extreme_base, "heavy_rows": lambda: lim.heavy_rows(333, 8),
         "rows65": lambda: rows(65, 9)}[name]()
    r.flags.writeable = False
    return r


@functools.lru_cache(maxsize=None)
def definition(name, metric):
    """the numpy definition's (a, b, sim, valid) of a named input, computed once"""
    return sequence.single_linkage_tree(fixture_rows(name), metric)


def exact(res, want):
    """the whole result against a definition's (a, b, sim, valid): every index, the bits of every sim, every flag"""
    a, b, sim, valid = want
    assert res.n_edges == len(a), (res.n_edges, len(a))
    assert same(res, (a, b, sim)), np.flatnonzero((res.a != a) | (res.b != b) | (bits(res.sim) != bits(sim)))[:10]
    assert np.array_equal(res.valid, valid)
    return True


def zeros_are_plus_zero(res):
    return bool((bits(res.sim[res.sim == 0]) == 0).all())


def weight_error(res, want_sim, what):
    err = float(np.abs(np.sort(res.sim).astype(np.float64) - np.sort(want_sim).astype(np.float64)).max())
    print(f"\n{what}: largest |sorted device weight - sorted fp64 weight| = {err:.3g}")
    assert err <= VALUE_TOL
    return err


# ---- negative values ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which,negative", (("corners", 3), ("simplex_star", 332), ("negative_contest", 1)))
def test_negative_contests_under_dot_equal_the_definition(engine, which, negative):
    r, want = fixture_rows(which), definition(which, "dot")
    centre = int(np.argmax(np.bincount(np.concatenate(want[:2])))) if which == "simplex_star" else None
    try:
        for split in (0, 32):
            engine.set_neighbour_split(split)
            res = engine.linkage(r, "dot")
            check_shape(res, len(r))
            assert exact(res, want), split
            # on the device's result itself: the negative edges are that many, negative, and the last ones
            assert res.n_edges == len(r) - 1 and (np.diff(res.sim) <= 0).all()
            assert (res.sim[-negative:] < 0).all() and (res.sim[:-negative] >= 0).all() and int((res.sim < 0).sum()) == negative
            assert zeros_are_plus_zero(res)
            if which == "simplex_star":
                assert res.rounds == 1 and ((res.a == centre) | (res.b == centre)).all()
            if which == "negative_contest":
                assert int((res.sim == 0).sum()) == 2                      # 0 against negative values: +0 is above every one of them
            print(f"\n{which}, split {split}: {res.rounds} rounds")
    finally:
        engine.set_neighbour_split(0)


@pytest.mark.parametrize("which", ("signed_rows", "corners"))
def test_negative_values_under_cosine_are_kruskal_over_the_devices_values(engine, which):
    r = fixture_rows(which)
    try:
        engine.set_neighbour_split(0)
        s = device_values(engine, r)
        upper = s[np.triu_indices(333, 1)]
        assert not np.isnan(upper).any() and 0.3 < (upper < 0).mean() < 0.8          # the running bests start among negative values
        want = kruskal(s)
        assert want[2].dtype == np.float32 and len(want[0]) == 332
        for split in (0, 32, 100):
            engine.set_neighbour_split(split)
            res = engine.linkage(r)
            check_shape(res, 333)
            assert same(res, want) and res.valid.all(), (split, np.flatnonzero((res.a != want[0]) | (res.b != want[1]))[:10])
            assert zeros_are_plus_zero(res)
        weight_error(res, definition(which, "cosine")[2], f"{which}, cosine")
        if which == "corners":
            assert int((res.sim < 0).sum()) == 3 and (res.sim[-3:] < 0).all()
    finally:
        engine.set_neighbour_split(0)


def test_the_cut_at_negative_thresholds_is_cluster(engine):
    engine.set_neighbour_split(0)
    r = fixture_rows("corners")
    res = engine.linkage(r, "dot")
    assert res.n_edges == 332 and (res.sim[-3:] < 0).all() and res.sim[-4] > 0
    thresholds = [float(t) for t in res.sim[-3:]] + [float(res.sim[-1]) - 1.0, 0.0, float(res.sim[-4])]
    counts = []
    for t in thresholds:
        c = engine.cluster(r, t, "dot")
        assert np.array_equal(res.cut(t), c.label), t
        assert np.array_equal(res.cut(t), sequence.threshold_clusters(r, t, "dot")[0]), t
        assert res.cluster_counts([t]).tolist() == [c.n_clusters], t
        counts.append(c.n_clusters)
    assert counts == [3, 2, 1, 1, 4, 4]                                    # a tie on a negative weight is an edge; four groups above
    r = fixture_rows("signed_rows")
    res = engine.linkage(r)
    assert res.n_edges == 332
    for t in [float(res.sim[k]) for k in (0, 166, 331)] + [-1.0]:
        c = engine.cluster(r, t)
        assert np.array_equal(res.cut(t), c.label), t
        assert res.cluster_counts([t]).tolist() == [c.n_clusters], t
    assert c.n_clusters == 1


# ---- a forest ----------------------------------------------------------------------------------------------------------------------

def test_rows_beyond_the_f16_range_are_isolated_rows_of_a_forest_under_dot(engine):
    r, out, keep = ld.forest_rows()
    rest = np.ascontiguousarray(r[keep])
    want = sequence.single_linkage_tree(rest, "dot")
    assert len(want[0]) == 265
    try:
        engine.set_neighbour_split(0)
        s = device_values(engine, r, "dot")
        gone = np.zeros(333, bool)
        gone[out] = True
        assert np.array_equal(np.isnan(s), gone[:, None] | gone[None, :])
        forest = kruskal(s)
        for split in (0, 32):
            engine.set_neighbour_split(split)
            full, part = engine.linkage(r, "dot"), engine.linkage(rest, "dot")
            check_shape(part, 266)
            assert exact(part, want), split
            check_shape(full, 333)
            assert full.n_valid == 333
            assert np.array_equal(full.a, keep[part.a]) and np.array_equal(full.b, keep[part.b]), split
            assert np.array_equal(bits(full.sim), bits(part.sim)), split
            assert full.valid.all() and full.n_edges == 333 - 1 - len(out) == 265 and full.rounds == part.rounds, (split, full.rounds)
            assert not np.isin(out, np.concatenate([full.a, full.b])).any()
            assert same(full, forest), split
            assert int((full.sim < 0).sum()) == 3 and (full.sim[-3:] < 0).all()
            for t in (float(full.sim[100]), float(full.sim[-2])):          # a positive and a negative weight of the tree
                c = engine.cluster(r, t, "dot")
                label = full.cut(t)
                assert np.array_equal(label, c.label) and np.array_equal(label[out], out), (split, t)
                assert full.cluster_counts([t]).tolist() == [c.n_clusters], (split, t)
            assert len(full.table()) == full.n_edges
            print(f"\nforest, split {split}: {full.n_edges} edges in {full.rounds} rounds")
        # the untrimmed outputs of the library: past n_edges they hold -1, -1 and NaN
        a, b, sim = np.full(332, 7, np.int64), np.full(332, 7, np.int64), np.full(332, 7.0, np.float32)
        valid, n_edges, rounds = np.zeros(333, np.uint8), C.c_int64(0), C.c_int64(0)
        _lib.check(engine.lib.gnn_linkage(engine.ctx, r.ctypes.data, 333, _lib.KNN_METRICS["dot"], a.ctypes.data, b.ctypes.data,
                                          sim.ctypes.data, valid.ctypes.data, C.addressof(n_edges), C.addressof(rounds)))
        assert n_edges.value == 265 and rounds.value == full.rounds and valid.all()
        assert np.array_equal(a[:265], full.a) and np.array_equal(b[:265], full.b) and np.array_equal(bits(sim[:265]), bits(full.sim))
        assert (a[265:] == -1).all() and (b[265:] == -1).all() and np.isnan(sim[265:]).all()
    finally:
        engine.set_neighbour_split(0)


# ---- dead tiles and dead steps -----------------------------------------------------------------------------------------------------

def test_tiles_and_steps_without_a_valid_row(engine):
    r, dead = fixture_rows("dead_tiles"), ld.DEAD_ROWS
    want = definition("dead_tiles", "dot")
    assert len(want[0]) == 278 and int(want[3].sum()) == 279
    zero = np.array(r)
    zero[64] = 0                                                           # valid under dot, invalid under cosine
    bad = np.sort(np.append(dead, 64))
    ok = np.ones(600, bool)
    ok[bad] = False
    try:
        engine.set_neighbour_split(0)
        s = device_values(engine, zero)
        assert np.isnan(s[bad]).all() and np.isnan(s[:, bad]).all() and not np.isnan(s[ok][:, ok]).any()
        by_values = kruskal(s, ok)
        assert len(by_values[0]) == 277
        for split in (0, 32, 256):
            engine.set_neighbour_split(split)
            res = engine.linkage(r, "dot")
            check_shape(res, 600)
            assert exact(res, want), split
            assert res.n_valid == 279 and not res.valid[dead].any() and not np.isin(dead, np.concatenate([res.a, res.b])).any()
            for t in (float(res.sim[0]), float(res.sim[139]), float(res.sim[-1])):
                label = res.cut(t)
                assert (label[dead] == -1).all() and (np.delete(label, dead) >= 64).all(), (split, t)
            res = engine.linkage(zero)
            check_shape(res, 600)
            assert same(res, by_values), (split, np.flatnonzero((res.a != by_values[0]) | (res.b != by_values[1]))[:10])
            assert np.array_equal(res.valid.astype(bool), ok) and not np.isin(bad, np.concatenate([res.a, res.b])).any()
            assert (res.cut(0.0)[bad] == -1).all()
    finally:
        engine.set_neighbour_split(0)


# ---- rounds ------------------------------------------------------------------------------------------------------------------------

def test_a_tied_path_needs_every_round_the_bound_allows(engine):
    r = fixture_rows("ruler_path")
    want = definition("ruler_path", "dot")
    assert len(want[0]) == 255 and (want[1] - want[0] == 1).all()
    cut = np.array(r)
    cut[255, 0] = np.nan
    want_cut = sequence.single_linkage_tree(cut, "dot")
    assert len(want_cut[0]) == 254 and want_cut[3].tolist() == [1] * 255 + [0]
    dots = ld.dots64(r)
    try:
        for split in (0, 32):
            engine.set_neighbour_split(split)
            res = engine.linkage(r, "dot")
            check_shape(res, 256)
            assert exact(res, want), split
            assert res.rounds == 8 == math.ceil(math.log2(res.n_valid)), (split, res.rounds)
            assert zeros_are_plus_zero(res)
            res = engine.linkage(cut, "dot")
            check_shape(res, 256)
            assert exact(res, want_cut), split
            # every component picks its best pair under a strict order, so a plain Boruvka takes the same rounds: 7
            assert res.rounds <= 8 and res.rounds == ld.boruvka(dots, want_cut[3])[0], (split, res.rounds)
        engine.set_neighbour_split(0)
        by_values = kruskal(device_values(engine, r))
        for split in (0, 32):
            engine.set_neighbour_split(split)
            res = engine.linkage(r)
            check_shape(res, 256)
            assert same(res, by_values) and res.valid.all() and res.n_edges == 255, split
            assert (res.b - res.a == 1).all() and zeros_are_plus_zero(res)
            print(f"\nruler_path, cosine, split {split}: {res.rounds} rounds")
    finally:
        engine.set_neighbour_split(0)


# ---- row scales (cosine) -----------------------------------------------------------------------------------------------------------

def test_a_power_of_two_per_row_changes_no_bit_of_the_tree(engine):
    engine.set_neighbour_split(0)
    r = fixture_rows("signed_rows")
    first = engine.linkage(r)
    check_shape(first, 333)
    assert first.n_edges == 332
    assert same(engine.linkage(lim.power_of_two_scaled(r, 3)), first)     # 2^-100 .. 2^100 per row, exact: rounds included


@pytest.mark.parametrize("which", ("extreme_base", "heavy_rows"))
def test_rows_from_all_subnormal_to_flt_max_and_heavy_tails(engine, which):
    engine.set_neighbour_split(0)
    r = fixture_rows(which)
    a, b, sim, valid = definition(which, "cosine")
    assert len(a) == 332 and valid.all()
    res = engine.linkage(r)
    check_shape(res, 333)
    s = device_values(engine, r)
    assert not np.isnan(s).any()
    want = kruskal(s)
    assert same(res, want) and res.valid.all(), np.flatnonzero((res.a != want[0]) | (res.b != want[1]))[:10]
    weight_error(res, sim, f"{which}, cosine")
    if which == "extreme_base":                                            # the one-hot pairs: exactly 1.0f, tied, in the order's order
        assert list(zip(res.a[:8].tolist(), res.b[:8].tolist())) == list(ld.ONE_HOT_PAIRS)
        assert (bits(res.sim[:8]) == bits(np.float32(1.0))).all() and res.sim[8] < 1


# ---- a small call after a large one ------------------------------------------------------------------------------------------------

def test_a_small_tree_after_large_ones_is_the_small_tree_alone(engine):
    engine.set_neighbour_split(0)
    small = fixture_rows("rows65")
    idx0, sim0 = engine.neighbours(small, None, 3)
    first = engine.linkage(small)
    check_shape(first, 65)
    assert first.n_edges == 64
    assert engine.linkage(fixture_rows("dead_tiles"), "dot").n_edges == 278
    assert engine.linkage(fixture_rows("forest_rows"), "dot").n_edges == 265
    assert same(engine.linkage(small), first)
    idx1, sim1 = engine.neighbours(small, None, 3)
    assert np.array_equal(idx0, idx1) and np.array_equal(bits(sim0), bits(sim1))
