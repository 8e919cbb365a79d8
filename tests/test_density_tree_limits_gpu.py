"""The density-aware linkage tree on the MI355X at the limits tests/test_density_tree_gpu.py stays away from (inputs and their CPU-side
conditions: tests/density_tree_limits_data.py, tests/linkage_limits_data.py, tests/embedding_limits_data.py,
tests/test_density_tree_limits_host.py).  What each group pins in gnn_linkage.hip, all in the MR = true instantiation:

  negative values   the two fminf of lk_candidates in front of nn_image's sign branch: negative cores, trees whose every weight is a
                    core-clamped negative tie, +0 for a zero in sim and in core
  forest            valid rows whose every pair is NaN (elements beyond the f16 range under dot) have core = NaN although valid = 1
                    (lk_core_kernel: "NaN for a row without one"); `e` is taken before the fminf in lk_candidates, which alone keeps a
                    NaN pair whose ends have a core from becoming an edge; NaN-padded lists in lk_core_kernel (`if (s == s) c = s`)
  dead tiles        `lcore[tid] = r0 + tid < a.n ? a.core[r0 + tid] : NAN`, ncore fetched a step ahead for columns >= b1, the early
                    return of a tile without a valid row and the skipped steps
  rounds            equality with a plain Boruvka over the same values on a tied path - 8, 7, 7 and 6 rounds, not the ruler's own 8
  row scales        nn_prepare_kernel's per-row power of two under core and tree together; rows from all-subnormal to FLT_MAX
  few rows          two and three valid rows at min_points 2, 3 and 65: lists of one or two entries, padded
  small after large the grow-only k.nidx / k.nsim: a small nk, small n call after a large one

References: the numpy definition (sequence.mutual_reachability_tree), exact on integer rows under dot, and otherwise the brute-force
Kruskal of tests/linkage_data.py over min(device value, device core_i, device core_j); in every case core is compared, bit for bit,
with the last finite entry of NNEngine.neighbours' own list.  Every group runs at splits 0 and 32 (dead tiles: 256 too).  The one tolerance is the project's bound of 1e-5 on a pair's cosine,
which a minimum and the k-th largest tree weight inherit (tests/test_density_tree_gpu.py::test_the_weights_are_within_1e_5_of_fp64).

Measured on an MI355X (profiles/density_tree/README.md, "At the limits"): sorted weights and cores within 1.5e-7 (signed rows), 7.2e-7
(corners), 2.1e-7 (extreme rows) and 3.6e-7 (heavy rows) of the fp64 definition's; 8 / 7 rounds on ruler_path at min_points 2 / 3 under
both metrics, 7 / 6 without its last row; 4, 3 and 2 rounds on corners and on the forest at min_points 2, 5 and 65; 1 on simplex_star and
negative_contest; no test here takes more than 0.3 s."""
import ctypes as C
import math

import numpy as np
import pytest

from genomad_amd import _lib, sequence
from tests import density_tree_limits_data as T
from tests import embedding_limits_data as lim
from tests import linkage_limits_data as ld
from tests.density_tree_data import last_finite, mutual, same_tree
from tests.embedding_limits_data import VALUE_TOL
from tests.linkage_data import bits, device_values, same

pytestmark = pytest.mark.gpu

SPLITS = (0, 32)


def restore(engine):
    engine.set_neighbour_split(0)
    engine.set_vote_lds(16)


@pytest.fixture(scope="module")
def values_of(engine):
    """values_of(name, metric): the device's own pair values of a named input, with the library's own split, computed once per
    module and released with it"""
    cache = {}

    def get(name, metric):
        if (name, metric) not in cache:
            engine.set_neighbour_split(0)
            cache[(name, metric)] = device_values(engine, T.fixture_rows(name), metric)
        return cache[(name, metric)]
    yield get
    cache.clear()


def core_is_the_list(engine, res, r, metric):
    """core against the neighbour search's own list of min_points - 1 entries: its last finite entry, bit for bit"""
    if res.min_points >= 2:
        sim = engine.neighbours(r, None, res.min_points - 1, metric)[1]
        assert np.array_equal(bits(res.core), bits(last_finite(sim))), np.flatnonzero(bits(res.core) != bits(last_finite(sim)))[:10]
    return True


def is_kruskal(res, values, valid=None):
    want = T.kruskal_reference(values, res.core, valid)
    assert same(res, want), np.flatnonzero((res.a != want[0]) | (res.b != want[1]) | (bits(res.sim) != bits(want[2])))[:10]
    return True


# ---- negative values ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", T.M_ALL)
@pytest.mark.parametrize("which", ("corners", "simplex_star", "negative_contest"))
def test_negative_values_and_cores_under_dot_equal_the_definition(engine, which, m):
    r, want = T.fixture_rows(which), T.definition(which, m, "dot")
    try:
        for split in SPLITS:
            engine.set_neighbour_split(split)
            res = engine.density_tree(r, m, "dot")
            T.check_tree(res, len(r), m)
            assert T.exact(res, want), split
            assert core_is_the_list(engine, res, r, "dot") and T.zeros_are_plus_zero(res)
            if which == "simplex_star":
                assert (res.sim < 0).all() and (res.core < 0).all() and len(np.unique(res.sim)) < 200
            if which == "negative_contest" and m < 65:
                assert (res.sim == 0).sum() == 2 and (res.core == 0).sum() == 2
            print(f"\n{which}, min_points {m}, split {split}: {res.rounds} rounds, {int((res.sim < 0).sum())} negative weights")
    finally:
        restore(engine)


@pytest.mark.parametrize("m", (2, 5))
@pytest.mark.parametrize("which", ("signed_rows", "corners"))
def test_negative_values_under_cosine_are_kruskal_over_the_devices_values_and_core(engine, values_of, which, m):
    r = T.fixture_rows(which)
    try:
        s = values_of(which, "cosine")
        upper = s[np.triu_indices(333, 1)]
        assert not np.isnan(upper).any() and 0.3 < (upper < 0).mean() < 0.8
        for split in SPLITS:
            engine.set_neighbour_split(split)
            res = engine.density_tree(r, m)
            T.check_tree(res, 333, m)
            assert res.n_edges == 332 and res.valid.all() and is_kruskal(res, s), split
            assert core_is_the_list(engine, res, r, "cosine") and T.zeros_are_plus_zero(res)
        err, cerr = T.errors_against_fp64(res, T.definition(which, m, "cosine"), f"{which}, cosine, min_points {m}")
        assert err <= VALUE_TOL and cerr <= VALUE_TOL
        if which == "corners":
            assert int((res.sim < 0).sum()) == 3 and (res.sim[-3:] < 0).all()
    finally:
        restore(engine)


@pytest.mark.parametrize("which", ("corners", "simplex_star"))
def test_the_cut_at_negative_thresholds_is_density_at_its_core_rows(engine, which):
    """thresholds that are weights of the tree and cores of rows, so that pairs and cores tie with them exactly: on corners the three
    negative weights, on simplex_star every weight and every core is negative"""
    r = T.fixture_rows(which)
    try:
        for split in SPLITS:
            engine.set_neighbour_split(split)
            for m in (2, 5):
                res = engine.density_tree(r, m, "dot")
                core = np.unique(res.core)
                ts = [float(t) for t in res.sim[-3:]] + [float(res.sim[0]), float(res.sim[166]), float(core[0]), float(core[len(core) // 2]),
                                                         float(core[-1]), float(res.sim[-1]) - 1.0, 0.0]
                assert sum(t < 0 for t in ts) >= 4
                for t in ts:
                    d = engine.density(r, t, m, "dot")
                    assert np.array_equal(res.cut(t), np.where(d.kind == 3, d.label, -1)), (split, m, t)
                    assert res.cluster_counts([t]).tolist() == [int(((d.kind == 3) & (d.label == np.arange(333))).sum())], (split, m, t)
    finally:
        restore(engine)


# ---- a forest ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", T.M_ALL)
def test_rows_beyond_the_f16_range_have_no_core_and_no_edge(engine, values_of, m):
    r, out, keep = ld.forest_rows()
    rest = T.fixture_rows("forest_part")
    want = T.definition("forest_part", m, "dot")
    try:
        s = values_of("forest_rows", "dot")
        gone = np.zeros(333, bool)
        gone[out] = True
        assert np.array_equal(np.isnan(s), gone[:, None] | gone[None, :])
        for split in SPLITS:
            engine.set_neighbour_split(split)
            full, part = engine.density_tree(r, m, "dot"), engine.density_tree(rest, m, "dot")
            T.check_tree(part, 266, m)
            assert T.exact(part, want) and core_is_the_list(engine, part, rest, "dot"), split
            T.check_tree(full, 333, m, no_partner=out)                     # valid, and NaN exactly there
            assert full.valid.all() and full.n_valid == 333 and np.array_equal(np.flatnonzero(np.isnan(full.core)), out)
            assert full.n_edges == 265 and full.rounds == part.rounds, (split, full.rounds, part.rounds)
            assert np.array_equal(full.a, keep[part.a]) and np.array_equal(full.b, keep[part.b]), split
            assert np.array_equal(bits(full.sim), bits(part.sim)) and np.array_equal(bits(full.core[keep]), bits(part.core)), split
            assert not np.isin(out, np.concatenate([full.a, full.b])).any()
            assert is_kruskal(full, ld.nan_rows_and_columns(s, out)) and core_is_the_list(engine, full, r, "dot"), split
            for t in (float(full.sim[100]), float(full.sim[-2]), float(np.nanmin(full.core))):
                d = engine.density(r, t, m, "dot")
                label = full.cut(t)
                assert (label[out] == -1).all() and np.array_equal(label, np.where(d.kind == 3, d.label, -1)), (split, t)
            print(f"\nforest, min_points {m}, split {split}: {full.n_edges} edges in {full.rounds} rounds")
        with pytest.raises(ValueError, match="metric 'dot': 1 - sim is a distance under cosine only"):
            full.hdbscan(2)
        with pytest.raises(ValueError, match="265 edges among 333 valid rows: hdbscan needs a spanning tree, not a forest"):
            sequence.hdbscan_clusters(full.a, full.b, full.sim, full.valid, 2)
        # the untrimmed outputs of the library: past n_edges they hold -1, -1 and NaN
        a, b, sim = np.full(332, 7, np.int64), np.full(332, 7, np.int64), np.full(332, 7.0, np.float32)
        core, valid, n_edges, rounds = np.full(333, 7.0, np.float32), np.zeros(333, np.uint8), C.c_int64(0), C.c_int64(0)
        _lib.check(engine.lib.gnn_density_tree(engine.ctx, r.ctypes.data, 333, m, _lib.KNN_METRICS["dot"], a.ctypes.data, b.ctypes.data,
                                               sim.ctypes.data, core.ctypes.data, valid.ctypes.data, C.addressof(n_edges), C.addressof(rounds)))
        assert n_edges.value == 265 and rounds.value == full.rounds and valid.all() and np.array_equal(bits(core), bits(full.core))
        assert np.array_equal(a[:265], full.a) and np.array_equal(b[:265], full.b) and np.array_equal(bits(sim[:265]), bits(full.sim))
        assert (a[265:] == -1).all() and (b[265:] == -1).all() and np.isnan(sim[265:]).all()
    finally:
        restore(engine)


def test_a_forest_whose_connected_rows_have_nan_padded_lists(engine):
    """40 connected rows among 67 without a partner, min_points 65: every list has 39 entries and 25 NaN, or 64 NaN"""
    sub, out, keep = T.forest_40()
    want = T.definition("forest_40_part", 65, "dot")
    try:
        for split in SPLITS:
            engine.set_neighbour_split(split)
            full = engine.density_tree(sub, 65, "dot")
            T.check_tree(full, 107, 65, no_partner=out)
            sim = engine.neighbours(sub, None, 64, "dot")[1]
            assert np.isnan(sim[out]).all() and np.isnan(sim[keep][:, 39:]).all() and not np.isnan(sim[keep][:, :39]).any()
            assert np.array_equal(bits(full.core), bits(last_finite(sim)))
            assert np.array_equal(bits(full.core[keep]), bits(sim[keep][:, 38])) and np.array_equal(bits(full.core[keep]), bits(want[3]))
            assert full.n_edges == 39 and np.array_equal(full.a, keep[want[0]]) and np.array_equal(full.b, keep[want[1]])
            assert np.array_equal(bits(full.sim), bits(want[2])) and full.valid.all()
            part = engine.density_tree(T.fixture_rows("forest_40_part"), 65, "dot")
            T.check_tree(part, 40, 65)
            assert T.exact(part, want) and part.rounds == full.rounds
    finally:
        restore(engine)


# ---- dead tiles and dead steps -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", T.M_ALL)
def test_tiles_and_steps_without_a_valid_row(engine, values_of, m):
    r, dead = T.fixture_rows("dead_tiles"), ld.DEAD_ROWS
    want = T.definition("dead_tiles", m, "dot")
    zero = T.fixture_rows("dead_tiles_zero")
    bad = np.sort(np.append(dead, 64))
    ok = np.ones(600, bool)
    ok[bad] = False
    try:
        s = values_of("dead_tiles_zero", "cosine")
        assert np.isnan(s[bad]).all() and np.isnan(s[:, bad]).all() and not np.isnan(s[ok][:, ok]).any()
        for split in (0, 32, 256):
            engine.set_neighbour_split(split)
            res = engine.density_tree(r, m, "dot")
            T.check_tree(res, 600, m)
            assert T.exact(res, want) and core_is_the_list(engine, res, r, "dot"), split
            assert res.n_valid == 279 and np.isnan(res.core[dead]).all() and not np.isin(dead, np.concatenate([res.a, res.b])).any()
            for t in (float(res.sim[0]), float(res.sim[139]), float(res.sim[-1])):
                assert (res.cut(t)[dead] == -1).all(), (split, t)
            res = engine.density_tree(zero, m)
            T.check_tree(res, 600, m)
            assert np.array_equal(res.valid.astype(bool), ok) and res.n_edges == 277
            assert is_kruskal(res, s, ok) and core_is_the_list(engine, res, zero, "cosine"), split
            assert np.isnan(res.core[bad]).all() and not np.isin(bad, np.concatenate([res.a, res.b])).any()
            assert (res.cut(0.0)[bad] == -1).all()
    finally:
        restore(engine)


# ---- rounds ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", (2, 3))
@pytest.mark.parametrize("which", ("ruler_path", "ruler_cut"))
def test_a_tied_path_takes_the_rounds_of_a_plain_boruvka(engine, values_of, which, m):
    r, want = T.fixture_rows(which), T.definition(which, m, "dot")
    rounds = T.ruler_rounds(which, m)[0]
    assert rounds == {("ruler_path", 2): 8, ("ruler_cut", 2): 7, ("ruler_path", 3): 7, ("ruler_cut", 3): 6}[(which, m)]
    try:
        for split in SPLITS:
            engine.set_neighbour_split(split)
            res = engine.density_tree(r, m, "dot")
            T.check_tree(res, 256, m)
            assert T.exact(res, want) and core_is_the_list(engine, res, r, "dot") and T.zeros_are_plus_zero(res), split
            assert res.rounds == rounds <= math.ceil(math.log2(res.n_valid)), (split, res.rounds)
        s = values_of(which, "cosine")                       # under cosine: the bound, and Kruskal over the device's values and core
        ok = want[4].astype(bool)
        assert np.array_equal(np.isnan(s), ~ok[:, None] | ~ok[None, :])
        for split in SPLITS:
            engine.set_neighbour_split(split)
            res = engine.density_tree(r, m)
            T.check_tree(res, 256, m)
            assert np.array_equal(res.valid.astype(bool), ok) and res.rounds <= 8 and res.n_edges == int(ok.sum()) - 1, (split, res.rounds)
            assert is_kruskal(res, s, ok) and core_is_the_list(engine, res, r, "cosine"), split
            print(f"\n{which}, cosine, min_points {m}, split {split}: {res.rounds} rounds")
    finally:
        restore(engine)


# ---- row scales (cosine) -----------------------------------------------------------------------------------------------------------

def test_a_power_of_two_per_row_changes_no_bit_of_core_or_tree(engine):
    r = T.fixture_rows("signed_rows")
    scaled = lim.power_of_two_scaled(r, 3)                  # 2^-100 .. 2^100 per row, exact
    try:
        for split in SPLITS:
            engine.set_neighbour_split(split)
            first = engine.density_tree(r, 5)
            T.check_tree(first, 333, 5)
            assert first.n_edges == 332 and first.valid.all()
            assert same_tree(engine.density_tree(scaled, 5), first), split                  # rounds included
    finally:
        restore(engine)


@pytest.mark.parametrize("m", (2, 17))
@pytest.mark.parametrize("which", ("extreme_base", "heavy_rows"))
def test_rows_from_all_subnormal_to_flt_max_and_heavy_tails(engine, values_of, which, m):
    r = T.fixture_rows(which)
    want = T.definition(which, m, "cosine")
    try:
        s = values_of(which, "cosine")
        assert not np.isnan(s).any()
        for split in SPLITS:
            engine.set_neighbour_split(split)
            res = engine.density_tree(r, m)
            T.check_tree(res, 333, m)
            assert res.n_edges == 332 and res.valid.all() and is_kruskal(res, s) and core_is_the_list(engine, res, r, "cosine"), split
            err, cerr = T.errors_against_fp64(res, want, f"{which}, cosine, min_points {m}, split {split}")
            assert err <= VALUE_TOL and cerr <= VALUE_TOL
            if which == "extreme_base" and m == 2:       # the one-hot rows with an identical partner: core exactly 1.0f, tied edges
                first = T.one_hot_first_edges()
                ends = sorted({i for p in first for i in p})
                assert (bits(res.core[ends]) == bits(np.float32(1.0))).all() and int((res.core == 1).sum()) == len(ends)
                assert list(zip(res.a[:len(first)].tolist(), res.b[:len(first)].tolist())) == first, split
                assert (bits(res.sim[:len(first)]) == bits(np.float32(1.0))).all() and res.sim[len(first)] < 1
    finally:
        restore(engine)


# ---- few rows ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", ("dot", "cosine"))
@pytest.mark.parametrize("which", T.FEW)
def test_two_and_three_valid_rows(engine, which, metric):
    r, live = T.few_rows(which)
    try:
        for m in (2, 3, 65):
            want = sequence.mutual_reachability_tree(r, m, metric)
            for split in SPLITS:
                engine.set_neighbour_split(split)
                res = engine.density_tree(r, m, metric)
                T.check_tree(res, len(r), m)
                assert T.exact(res, want) and core_is_the_list(engine, res, r, metric), (m, split)
                assert res.n_edges == len(live) - 1 and res.rounds == 1
                if len(live) == 2:
                    assert bits(res.sim[0]) == bits(res.core[res.a[0]]) == bits(res.core[res.b[0]])
                    assert (res.a[0], res.b[0]) == (live[0], live[1])
    finally:
        restore(engine)


# ---- a small call after a large one ------------------------------------------------------------------------------------------------

def test_small_calls_after_a_large_one_are_the_small_calls_alone(engine):
    """the small calls first, with the library's own split; then, at each split, the large call and the small ones behind it"""
    small = T.fixture_rows("rows65")
    try:
        restore(engine)
        idx0, sim0 = engine.neighbours(small, None, 3)
        first = engine.density_tree(small, 2), engine.linkage(small), engine.density_tree(small[:9], 65)
        T.check_tree(first[0], 65, 2)
        T.check_tree(first[2], 9, 65)
        assert first[0].n_edges == 64 and first[2].n_edges == 8
        for split in SPLITS:
            engine.set_neighbour_split(split)
            large = engine.density_tree(T.fixture_rows("dead_tiles"), 65, "dot")           # 600 rows x 64 entries in k.nidx / k.nsim
            assert T.exact(large, T.definition("dead_tiles", 65, "dot")), split
            assert same_tree(engine.density_tree(small, 2), first[0]), split               # 65 rows x 1 entry
            assert same(engine.linkage(small), first[1]), split
            nine = engine.density_tree(small[:9], 65)                                      # 9 rows x 64 entries, 56 of them NaN
            assert same_tree(nine, first[2]) and core_is_the_list(engine, nine, small[:9], "cosine"), split
            idx1, sim1 = engine.neighbours(small, None, 3)
            assert np.array_equal(idx0, idx1) and np.array_equal(bits(sim0), bits(sim1)), split
    finally:
        restore(engine)
