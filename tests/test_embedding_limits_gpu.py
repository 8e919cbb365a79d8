"""The embedding searches on the MI355X at the limits their own tests stay away from (inputs and their CPU-side conditions:
tests/embedding_limits_data.py, tests/test_embedding_limits_host.py).  Which line of which kernel each group pins:

  A  query slabs     nn_search (gnn_neighbours.hip), QSLAB = 16384: `qfrag = w.bfrag + q0 / 32 * BLK_U4`, `self_off = q0` of a later slab
                     (`own = a.self_off + q - b0` in nn_tile_kernel), the outputs at `q0 * k`, `query_dev + q0 * D`, the reuse of d_query,
                     d_idx, d_sim and the partial lists by the second slab.
  B  range cap       SPLIT_MAX = 65280 in nn_split_rows (gnn_nn_frag.h); `uint16_t loff`, `(uint16_t)off` in nn_insert, `eo < off` on
                     offsets beyond 32767, `b0 + loff[row][j]`, `lself` / `own < a.split_rows` in a full range and in a second one.
  C  signs           `es > s || (es == s && eo < off)` of nn_insert and nn_precedes on negative values; the `u >> 31` branch of
                     rp_image / rp_unimage (gnn_representatives.hip) where it decides who represents a row; `s >= a.threshold` with a
                     negative threshold in cl_tile_kernel and rp_tile_kernel; `s + 0.f` (-0 counts as +0).
  D  row scales      nn_prepare_kernel (gnn_nn_frag.h): `frexpf(amax, &ex)`, `ldexpf(x[e], -ex)` before the squares are summed, from
                     all-subnormal rows to FLT_MAX; `x / norm * 256` on one-hot rows (exact) and on rows with a 10^4 dynamic range.
  E  dot range       the unscaled split of nn_prepare_kernel under dot: the relative bound on [2^-7, 65504) that include/genomad_nn.h
                     states, and `s == s` (nn_tile_kernel) / `s >= threshold` (cluster, representatives) for elements beyond the f16 range.

References: fp64 similarities of the f32 rows actually passed (sims64), the numpy definitions of genomad_amd/sequence.py, and for exact
comparisons under cosine the device's own f32 values fed to the brute-force walk and components.  VALUE_TOL, GAP and the 90 % cap on
the exact-order check are those of tests/test_neighbours_gpu.py.

Measured on an MI355X (profiles/neighbours/README.md, "At the limits"): max |sim - fp64| 6.3e-8 .. 7.7e-7 against the bound of 1e-5
(the largest on rows whose largest element is in [2^127, FLT_MAX]; 4.2e-7 on all-subnormal rows, which are valid); qualifying shares
99.9 % / 94.1 % (two slabs, k = 1 / 10), 97.1 % (65350 base rows, k = 1), 100 % / 94.3 % / 95.2 % (signed rows), 100 % / 98.6 % / 98.8 %
(heavy rows); dot: 0.093 and 0.031 of the bound inside the stated range, 9.6 times the bound below it.  The self-search of 16454
rows takes 0.016 s, that of 65350 rows in ranges of 65280 takes 0.042 s; no test here takes more than 0.4 s on the device."""
import time

import numpy as np
import pytest

from genomad_amd import sequence
from tests import embedding_limits_data as lim
from tests.clusters_data import components, device_edges
from tests.embedding_limits_data import CAP, GAP, VALUE_TOL
from tests.neighbours_data import rows, sims64
from tests.representatives_data import walk

pytestmark = pytest.mark.gpu

CLUSTER_FIELDS = sequence.CLUSTER_FIELDS


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_pair(got, want):
    """(idx, sim) bit for bit; NaN padding compares by its bits too"""
    return np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))


def check_values(idx, sim, s64, k, what, own=None):
    """test_similarities_are_the_fp64_cosine_of_the_returned_pairs: shapes, no base row twice, values within VALUE_TOL, ordered"""
    assert idx.dtype == np.int64 and sim.dtype == np.float32 and idx.shape == sim.shape == (len(s64), k)
    assert (idx >= 0).all() and (idx < s64.shape[1]).all()
    assert (np.sort(idx, axis=1)[:, 1:] != np.sort(idx, axis=1)[:, :-1]).all()
    if own is not None:
        assert (idx != np.asarray(own)[:, None]).all()
    err = np.abs(sim.astype(np.float64) - np.take_along_axis(s64, idx, axis=1)).max()
    print(f"\n{what} k={k}: max |sim - fp64 sim of the returned pair| = {err:.3e}")
    assert err <= VALUE_TOL
    assert (np.diff(sim, axis=1) <= 0).all()
    return err


def check_sets(idx, s64, k):
    """test_no_row_is_left_out_and_none_is_let_in"""
    kth = -np.sort(-s64, axis=1)[:, k - 1]
    assert (np.take_along_axis(s64, idx, axis=1) >= kth[:, None] - GAP).all()
    returned = np.zeros(s64.shape, bool)
    np.put_along_axis(returned, idx, True, axis=1)
    assert returned[s64 > kth[:, None] + GAP].all()


def check_order(idx, s64, k, what):
    """test_order_is_the_definitions_where_the_gaps_allow, the definition's order read off the fp64 matrix"""
    ok = lim.qualifies(s64, k)
    print(f"\n{what} k={k}: {ok.mean():.1%} of the rows have every top-{k + 1} gap above {GAP:g}")
    assert ok.mean() >= CAP
    assert np.array_equal(idx[ok], lim.order64(s64, k)[ok])


def neighbours_dev(engine, q, b, k, metric="cosine"):
    """engine.neighbours_dev on rows uploaded here; b = None: the self-search"""
    shape = (len(q), k)
    bufs = [engine.alloc(q.nbytes), engine.alloc(b.nbytes) if b is not None else None, engine.alloc(8 * len(q) * k),
            engine.alloc(4 * len(q) * k)]
    try:
        bufs[0].upload(q)
        if b is not None:
            bufs[1].upload(b)
        engine.neighbours_dev(bufs[0].ptr, len(q), bufs[1].ptr if b is not None else None, 0 if b is None else len(b), bufs[2].ptr,
                              bufs[3].ptr, k, metric)
        engine.sync()
        return bufs[2].download(shape, np.int64), bufs[3].download(shape, np.float32)
    finally:
        for buf in bufs:
            if buf is not None:
                buf.free()


def cluster_arrays(res):
    return [getattr(res, f) for f in CLUSTER_FIELDS]


def same_clusters(got, want):
    return all(a.dtype == np.int64 and np.array_equal(a, b) for a, b in zip(got, want))


def same_representatives(a, b):
    return (all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("rep", "size", "rank")) and a.rounds == b.rounds
            and np.array_equal(bits(a.sim), bits(b.sim)))


def exact_representatives(res, want):
    """rep, size, rank, rounds and the bits of sim against the definition's tuple"""
    rep, sim, size, rank, rounds = want
    for f, a, b in (("rep", res.rep, rep), ("size", res.size, size), ("rank", res.rank, rank)):
        assert a.dtype == np.int64 and np.array_equal(a, b), (f, np.flatnonzero(a != b)[:10])
    assert res.rounds == rounds and res.sim.dtype == np.float32 and np.array_equal(np.isnan(res.sim), np.isnan(sim))
    member = ~np.isnan(sim)
    assert np.array_equal(bits(res.sim)[member], bits(sim)[member])
    return True


# ---- A: query slabs ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def slab_pairs():
    """16454 signed queries - one slab of 16384 and 70 rows - against 333 signed base rows, and their fp64 similarities"""
    q, b = lim.signed_rows(lim.NQ_SLABS, 30), lim.signed_rows(333, 8)
    return q, b, sims64(q, b)


@pytest.fixture(scope="module")
def slab_self():
    """the 16454 rows planted across the slab border, the 198 rows at the two ends and their fp64 similarities to all rows"""
    r, pairs, triple = lim.slab_rows()
    edge = np.concatenate([np.arange(64), np.arange(lim.QSLAB - 64, lim.NQ_SLABS)])
    return r, pairs, triple, edge, lim.self64(r, edge)


@pytest.mark.parametrize("k", (1, 10))
def test_a_second_query_slab_answers_as_the_first(engine, slab_pairs, k):
    q, b, s64 = slab_pairs
    try:
        engine.set_neighbour_split(0)
        idx, sim = engine.neighbours(q, b, k)
        check_values(idx, sim, s64, k, "slabs, 16454 x 333")
        check_sets(idx, s64, k)
        check_order(idx, s64, k, "slabs, 16454 x 333")
        a = lim.QSLAB - 64
        tail = (idx[a:], sim[a:])                             # 134 rows: the last tile of the first slab and all of the second
        assert same_pair(engine.neighbours(q[a:], b, k), tail)
        assert same_pair(neighbours_dev(engine, q[a:], b, k), tail)
        assert same_pair(neighbours_dev(engine, q, b, k), (idx, sim))          # query_dev + q0 * D, idx_dev + q0 * k
    finally:
        engine.set_neighbour_split(0)


def test_a_row_of_a_later_slab_is_not_its_own_neighbour(engine, slab_self):
    r, pairs, triple, edge, own64 = slab_self
    k = 10
    try:
        engine.set_neighbour_split(0)
        t0 = time.perf_counter()
        idx, sim = engine.neighbours(r, None, k)
        print(f"\nself-search of 16454 rows, k={k}: {time.perf_counter() - t0:.3f} s")
        assert idx.shape == sim.shape == (lim.NQ_SLABS, k) and (idx >= 0).all()
        assert (idx != np.arange(lim.NQ_SLABS)[:, None]).all()
        for a, b in pairs:                                    # across the border, both ways
            assert idx[a, 0] == b and idx[b, 0] == a and bits(sim[a, :1]) == bits(sim[b, :1])
            assert abs(float(sim[a, 0]) - 1) <= VALUE_TOL
        for i in triple:                                      # identical rows: the two others first, by index, on one value
            assert list(idx[i, :2]) == [j for j in triple if j != i] and bits(sim[i, :1]) == bits(sim[i, 1:2])
        check_values(idx[edge], sim[edge], own64, k, "slabs, self-search, the rows at both ends", own=edge)
        check_sets(idx[edge], own64, k)
        # the same rows as queries of a search that is no self-search: k + 1 neighbours, the row itself among them
        idx11, sim11 = engine.neighbours(r[edge], r, k + 1)
        is_own = idx11 == edge[:, None]
        assert (is_own.sum(axis=1) == 1).all()
        assert np.array_equal(idx11[~is_own].reshape(-1, k), idx[edge])
        assert np.array_equal(bits(sim11[~is_own].reshape(-1, k)), bits(sim[edge]))
        engine.set_neighbour_split(32)                        # 515 ranges: every range but one holds no row of the tile
        assert same_pair(engine.neighbours(r, None, k), (idx, sim))
    finally:
        engine.set_neighbour_split(0)


# ---- B: the range cap and the 16-bit offsets ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def capped():
    """70 queries of neighbours_data.rows, the base of 65350 rows with its plants, the fp64 similarities (70 x 65350), and for the
    self-search the last 70 rows with the plants and their fp64 similarities (75 x 65350)"""
    q = rows(70, 7)
    base = lim.capped_base(q)
    mine = np.concatenate([np.arange(lim.NB_CAPPED - 70, lim.NB_CAPPED), lim.CAPPED_PLANTS[:3], lim.CAPPED_TIE])
    assert len(set(mine)) == len(mine) == 75 and set(lim.CAPPED_PLANTS) <= set(mine)
    return q, base, sims64(q, base), mine, lim.self64(base, mine)


@pytest.mark.parametrize("k", (1, 10, 64))
def test_a_full_range_of_65280_rows_and_the_first_row_of_the_next(engine, capped, k):
    q, base, s64, _, _ = capped
    try:
        engine.set_neighbour_split(1 << 20)                   # clamps to SPLIT_MAX: two ranges, the first with offsets up to 65279
        idx, sim = engine.neighbours(q, base, k)
        check_values(idx, sim, s64, k, "range cap, 70 x 65350")
        check_sets(idx, s64, k)
        if k == 1:                                            # 97 % of the rows qualify at k = 1, 76 % at k = 10: under the cap
            check_order(idx, s64, k, "range cap, 70 x 65350")
        assert list(idx[:5, 0]) == list(lim.CAPPED_PLANTS) and idx[5, 0] == lim.CAPPED_TIE[0]
        assert (np.abs(sim[:6, 0].astype(np.float64) - 1) <= VALUE_TOL).all()
        if k > 1:                                             # one value at offsets 32769 and 65278: the lower index first
            assert list(idx[5, :2]) == list(lim.CAPPED_TIE) and bits(sim[5, :1]) == bits(sim[5, 1:2])
        for split in (0, 40000, lim.SPLIT_MAX):
            engine.set_neighbour_split(split)
            assert same_pair(engine.neighbours(q, base, k), (idx, sim)), split
    finally:
        engine.set_neighbour_split(0)


def test_the_self_search_over_a_full_range(engine, capped):
    """All 65350 rows, four query slabs against two ranges: 13 T multiply-adds in the three products.  Its wall time on the MI355X,
    the upload of 134 MB included, is in profiles/neighbours/README.md: well under a second, so nothing is cut down."""
    _, base, _, mine, own64 = capped
    k = 3
    try:
        engine.set_neighbour_split(1 << 20)
        t0 = time.perf_counter()
        idx, sim = engine.neighbours(base, None, k)
        print(f"\nself-search of 65350 rows, k={k}, ranges of 65280: {time.perf_counter() - t0:.3f} s")
        assert idx.shape == (lim.NB_CAPPED, k) and (idx >= 0).all() and (idx != np.arange(lim.NB_CAPPED)[:, None]).all()
        check_values(idx[mine], sim[mine], own64, k, "range cap, self-search, the last 70 rows and the plants", own=mine)
        check_sets(idx[mine], own64, k)
        a, b = lim.CAPPED_TIE                                 # the two copies find each other
        assert idx[a, 0] == b and idx[b, 0] == a and bits(sim[a, :1]) == bits(sim[b, :1])
    finally:
        engine.set_neighbour_split(0)


# ---- C: signs ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def signed():
    """signed_rows at the sizes of tests/test_neighbours_gpu.py, the 80-row base whose lists of 64 end in negative values, and the
    fp64 similarities of every case"""
    q, b = lim.signed_rows(70, 7), lim.signed_rows(333, 8)
    few = b[:lim.NEGATIVE_TAIL_BASE]
    return {"pairs": (q, b, sims64(q, b)), "self": (b, None, lim.self64(b)),
            "pairs80": (q, few, sims64(q, few)), "self80": (few, None, lim.self64(few))}


@pytest.mark.parametrize("case", ["pairs", "self"])
@pytest.mark.parametrize("k", (1, 10, 64))
def test_neighbours_of_signed_rows(engine, signed, case, k):
    engine.set_neighbour_split(0)
    q, b, s64 = signed[case]
    idx, sim = engine.neighbours(q, b, k)
    check_values(idx, sim, s64, k, f"signed rows, {case}", own=np.arange(len(q)) if b is None else None)
    check_sets(idx, s64, k)
    if k < 64:
        check_order(idx, s64, k, f"signed rows, {case}")
        ref_idx, _ = sequence.nearest_neighbours(q, b, k)
        ok = lim.qualifies(s64, k)
        assert np.array_equal(idx[ok], ref_idx[ok])
    else:
        # of 333 base rows about 166 are on a query's positive side, so these lists are positive throughout; the 80-row base below
        # is where the lists END in negative values, and there every row must hold them in order
        q, b, s64 = signed[case + "80"]
        try:
            for split in (0, 32):
                engine.set_neighbour_split(split)
                idx, sim = engine.neighbours(q, b, k)
                check_values(idx, sim, s64, k, f"signed rows, {case}, 80 base rows", own=np.arange(len(q)) if b is None else None)
                check_sets(idx, s64, k)
                assert (sim[:, -1] < 0).all() and (sim[:, 0] > 0).all() and ((sim < 0).sum(axis=1) >= 5).all()
                assert (np.diff(sim, axis=1) <= 0).all()
        finally:
            engine.set_neighbour_split(0)


@pytest.mark.parametrize("k", (1, 7, 64))
def test_signed_integer_dots_are_bit_exact(engine, k):
    base = lim.signed_integer_rows(200)
    other = np.random.default_rng(12).integers(-4, 4, (67, 512)).astype(np.float32)
    query = np.concatenate([base[[10, 3, 199]], other])
    try:
        for q, b in ((query, base), (base, None), (query, base[:lim.NEGATIVE_TAIL_BASE])):
            want_idx, want_sim = sequence.nearest_neighbours(q, b, k, "dot")
            for split in (0, 32):
                engine.set_neighbour_split(split)
                idx, sim = engine.neighbours(q, b, k, "dot")
                assert np.array_equal(idx, want_idx), split
                assert np.array_equal(bits(sim), bits(want_sim)), split
        if k == 64:
            assert (want_sim[:, -1] < 0).all()               # the 80-row base: the lists end in negative integers
    finally:
        engine.set_neighbour_split(0)


def test_clusters_and_representatives_of_signed_integer_rows(engine):
    base = lim.signed_integer_rows(200)
    w = np.random.default_rng(3).integers(0, 4, 200)
    try:
        for threshold in lim.integer_thresholds(base):        # a negative and a positive dot, each attained by more than 10 pairs
            want = sequence.threshold_clusters(base, threshold, "dot")
            for split in (0, 32):
                engine.set_neighbour_split(split)
                assert same_clusters(cluster_arrays(engine.cluster(base, threshold, "dot")), want), (threshold, split)
            for weight in (None, w):
                want = sequence.greedy_representatives(base, threshold, weight, "dot")
                for split in (0, 32):
                    engine.set_neighbour_split(split)
                    assert exact_representatives(engine.representatives(base, threshold, weight, "dot"), want), (threshold, split)
    finally:
        engine.set_neighbour_split(0)


@pytest.mark.parametrize("order", ("index", "cab"))
def test_negative_contests_go_to_the_larger_value_and_ties_to_the_smaller_rank(engine, order):
    r, orders = lim.negative_contest()
    weight, winner = orders[order]
    want = sequence.greedy_representatives(r, lim.CONTEST_THRESHOLD, weight, "dot")
    members = np.array(sorted(winner))
    dots = r.astype(np.float64) @ r.astype(np.float64).T
    try:
        for split in (0, 32):
            engine.set_neighbour_split(split)
            res = engine.representatives(r, lim.CONTEST_THRESHOLD, weight, "dot")
            assert exact_representatives(res, want), split
            assert [int(res.rep[m]) for m in members] == [winner[int(m)] for m in members]      # who wins, not only that both agree
            assert np.array_equal(res.sim[members].astype(np.float64), dots[res.rep[members], members])
            zero = members[res.sim[members] == 0]
            assert len(zero) >= 1 and (bits(res.sim[zero]) == 0).all()                            # +0, never -0
            assert (res.sim[members] < 0).sum() >= 8 and list(np.flatnonzero(res.is_rep)) == sorted(lim.CONTEST_REPS)
    finally:
        engine.set_neighbour_split(0)


def test_a_negative_threshold_that_is_one_of_the_devices_own_values(engine):
    """As test_the_values_are_those_neighbours_returns... of the cluster and representative tests, on 65 signed rows with the
    threshold at the 10th percentile of the device's upper-triangle values: a negative f32 with a tie exactly on it."""
    r = lim.signed_rows(65, 9)
    w = np.random.default_rng(10).integers(0, 4, 65).astype(np.float64)
    by_rank = sequence.priority_order(w, 65)
    p = np.ascontiguousarray(r[by_rank])
    engine.set_neighbour_split(0)
    idx, sim = engine.neighbours(p, None, 64)
    assert (idx >= 0).all()
    s = np.full((65, 65), np.nan, np.float32)
    np.put_along_axis(s, idx, sim, axis=1)                    # s[i, j]: query i, base row j, both by rank
    upper = s[np.triu_indices(65, 1)]
    threshold = np.sort(upper)[len(upper) // 10]
    assert threshold.dtype == np.float32 and threshold < 0 and (upper == threshold).any()
    want = components(device_edges(s, threshold))
    res = engine.cluster(p, threshold)
    for f, a, b in zip(CLUSTER_FIELDS, cluster_arrays(res), want):
        assert np.array_equal(a, b), (f, np.flatnonzero(a != b)[:10])
    assert res.n_edges == int((upper >= threshold).sum())
    # the walk at the same threshold and at the 40th percentile, also negative and one of the values: more representatives, and members
    # all of whose candidates are negative
    negative_members = 0
    for thr in (threshold, np.sort(upper)[int(len(upper) * 0.4)]):
        assert thr < 0
        rep_p, sim_p, size_p, _ = walk(s.tolist(), float(thr))
        assert (rep_p != np.arange(65)).sum() > 5 and (rep_p == np.arange(65)).sum() > 1
        negative_members += int((sim_p[~np.isnan(sim_p)] < 0).sum())
        got = engine.representatives(r, thr, w)
        assert np.array_equal(got.rep[by_rank], by_rank[rep_p]) and np.array_equal(got.size[by_rank], size_p)
        assert np.array_equal(bits(got.sim[by_rank]), bits(sim_p))
        assert np.array_equal(got.rank[by_rank], np.arange(65))
    assert negative_members >= 1


# ---- D: row scales (cosine) --------------------------------------------------------------------------------------------------------

def test_a_power_of_two_per_row_changes_no_bit(engine):
    r, q = lim.signed_rows(333, 8), lim.signed_rows(70, 7)
    r2, q2 = lim.power_of_two_scaled(r, 3), lim.power_of_two_scaled(q, 4)          # 2^-100 .. 2^100, exact
    w = np.random.default_rng(5).integers(0, 6, 333).astype(np.float64)
    engine.set_neighbour_split(0)
    pairs, own = engine.neighbours(q, r, 10), engine.neighbours(r, None, 10)
    assert same_pair(engine.neighbours(q2, r2, 10), pairs)
    assert same_pair(engine.neighbours(q2, r, 10), pairs) and same_pair(engine.neighbours(q, r2, 10), pairs)
    assert same_pair(engine.neighbours(r2, None, 10), own)
    threshold = np.sort(own[1][:, 0])[333 // 2]               # one of the device's values: a row's best similarity, the median one
    assert threshold.dtype == np.float32 and 0 < threshold < 1
    first = engine.cluster(r, threshold)
    assert 1 < first.n_clusters < 333
    assert same_clusters(cluster_arrays(engine.cluster(r2, threshold)), cluster_arrays(first))
    first = engine.representatives(r, threshold, w)
    assert 1 < first.n_clusters < 333
    assert same_representatives(engine.representatives(r2, threshold, w), first)


def test_rows_from_all_subnormal_to_flt_max_against_fp64(engine):
    base = lim.extreme_base()
    query = lim.extreme_queries(base)
    kinds = lim.EXTREME_KINDS
    engine.set_neighbour_split(0)
    # every query against the 64 extreme rows alone, k = 64: each of them is a candidate, so a row that came back invalid shows
    idx, sim = engine.neighbours(query, base[:64], 64)
    assert (idx >= 0).all(), (np.flatnonzero((idx < 0).all(axis=1)), sorted(set(range(64)) - set(idx[idx >= 0])))
    s64 = sims64(query, base[:64])
    check_values(idx, sim, s64, 64, "extreme rows, 70 x 64")
    s = np.empty((70, 64), np.float32)
    np.put_along_axis(s, idx, sim, axis=1)
    for name, sl in kinds.items():
        err = np.abs(s[:, sl].astype(np.float64) - s64[:, sl]).max()
        print(f"\nextreme rows, base kind {name}: max |sim - fp64| = {err:.3e}")
    _, pos, sign = lim.one_hot_rows()
    want = np.where(pos[:, None] == pos[None, :], sign[:, None] * sign[None, :], 0).astype(np.float32)
    hot = s[12:28, kinds["one_hot"]]
    assert np.array_equal(hot, want) and set(hot.ravel()) == {-1.0, 0.0, 1.0}                    # exactly +-1.0f or 0
    # each query that is a multiple of a base row finds it first: huge, subnormal, one-hot (the first of its equals), heavy
    assert list(idx[0:6, 0]) == list(range(0, 6)) and list(idx[6:12, 0]) == list(range(16, 22))
    assert list(idx[28:34, 0]) == list(range(48, 54))
    assert (np.abs(sim[:34, 0].astype(np.float64) - 1) <= VALUE_TOL).all()
    # the whole base: the values, the sets, and every extreme row has neighbours and is somebody's neighbour
    for k in (10, 64):
        s64 = sims64(query, base)
        idx, sim = engine.neighbours(query, base, k)
        check_values(idx, sim, s64, k, "extreme rows, 70 x 333")
        check_sets(idx, s64, k)
        own64 = lim.self64(base)
        idx, sim = engine.neighbours(base, None, k)
        check_values(idx, sim, own64, k, "extreme rows, self-search on 333", own=np.arange(333))
        check_sets(idx, own64, k)


@pytest.mark.parametrize("case", ["pairs", "self"])
@pytest.mark.parametrize("k", (1, 10))
def test_neighbours_of_heavy_rows(engine, case, k):
    engine.set_neighbour_split(0)
    q, b = (lim.heavy_rows(70, 7), lim.heavy_rows(333, 8)) if case == "pairs" else (lim.heavy_rows(333, 8), None)
    s64 = sims64(q, b) if b is not None else lim.self64(q)
    idx, sim = engine.neighbours(q, b, k)
    check_values(idx, sim, s64, k, f"heavy rows, {case}", own=np.arange(len(q)) if b is None else None)
    check_sets(idx, s64, k)
    check_order(idx, s64, k, f"heavy rows, {case}")
    ref_idx, _ = sequence.nearest_neighbours(q, b, k)
    ok = lim.qualifies(s64, k)
    assert np.array_equal(idx[ok], ref_idx[ok])


# ---- E: the dot metric's range -----------------------------------------------------------------------------------------------------

def dot_ratio(engine, q, b, k=64):
    """max over the returned pairs of |f32 dot - fp64 dot| / (VALUE_TOL * sum |x_i y_i|)"""
    idx, sim = engine.neighbours(q, b, k, "dot")
    assert (idx >= 0).all() and np.isfinite(sim).all()
    err = np.abs(sim.astype(np.float64) - np.take_along_axis(sims64(q, b, "dot"), idx, axis=1))
    return float((err / np.take_along_axis(lim.dot_bound(q, b), idx, axis=1)).max())


def test_dot_of_rows_inside_the_stated_range(engine):
    """The bound VALUE_TOL * sum |x_i y_i| per pair.  include/genomad_nn.h states it for 2^-7 <= |element| < 65504: asserted on heavy
    rows whose largest element is 6e4 and on rows at the lower end of that range.  Four binades below it the error of the
    f16-subnormal limbs, absolute, is past the bound (12 times, in the host test's emulation): printed here, not asserted."""
    engine.set_neighbour_split(0)
    heavy = dot_ratio(engine, lim.dot_range_rows(70, 71), lim.dot_range_rows(333, 72))
    small = dot_ratio(engine, lim.small_dot_rows(70, 81), lim.small_dot_rows(333, 82))
    below = dot_ratio(engine, lim.signed_rows(70, 7) * np.float32(2.0 ** -14), lim.signed_rows(333, 8) * np.float32(2.0 ** -14))
    print(f"\ndot: max |sim - fp64 dot| / (1e-5 sum |x y|): {heavy:.3f} heavy rows up to 6e4, {small:.3f} elements of 2^-7 .. 2^-3, "
          f"{below:.3f} elements below 2^-9 (outside the stated range)")
    assert heavy <= 1 and small <= 1


def test_rows_beyond_the_f16_range_are_never_returned_under_dot(engine):
    base = lim.out_of_range_base()
    out = list(lim.OUT_OF_RANGE)
    keep = np.delete(np.arange(333), out)
    rest = np.ascontiguousarray(base[keep])
    query = np.random.default_rng(62).integers(-4, 4, (70, 512)).astype(np.float32)
    engine.set_neighbour_split(0)
    for k in (10, 64):
        idx, sim = engine.neighbours(query, base, k, "dot")
        assert not np.isin(idx, out).any() and (idx >= 0).all() and not np.isnan(sim).any()
        idx_r, sim_r = engine.neighbours(query, rest, k, "dot")
        assert np.array_equal(idx, keep[idx_r]) and np.array_equal(bits(sim), bits(sim_r))
        want_idx, want_sim = sequence.nearest_neighbours(query, rest, k, "dot")            # and both are the definition's
        assert np.array_equal(idx_r, want_idx) and np.array_equal(bits(sim_r), bits(want_sim))
        idx, sim = engine.neighbours(base, None, k, "dot")
        assert not np.isin(idx, out).any() and np.array_equal(np.isnan(sim), idx < 0)    # no NaN before a row's padding
        assert (idx[out] == -1).all() and (idx[keep] >= 0).all()                          # as queries they have nobody
        idx_r, sim_r = engine.neighbours(rest, None, k, "dot")
        assert np.array_equal(idx[keep], keep[idx_r]) and np.array_equal(bits(sim[keep]), bits(sim_r))
    dots = rest.astype(np.float64) @ rest.astype(np.float64).T
    threshold = float(np.sort(dots[np.triu_indices(331, 1)])[int(331 * 330 / 2 * 0.98)])
    full, part = engine.cluster(base, threshold, "dot"), engine.cluster(rest, threshold, "dot")
    assert 1 < part.n_clusters < 331
    assert np.array_equal(full.label[out], out) and np.array_equal(full.rep[out], out)    # singletons
    assert (full.degree[out] == 0).all() and (full.size[out] == 1).all()
    assert np.array_equal(full.label[keep], keep[part.label]) and np.array_equal(full.rep[keep], keep[part.rep])
    assert np.array_equal(full.degree[keep], part.degree) and np.array_equal(full.size[keep], part.size)
    full, part = engine.representatives(base, threshold, None, "dot"), engine.representatives(rest, threshold, None, "dot")
    assert 1 < part.n_clusters < 331 and full.rounds == part.rounds
    assert np.array_equal(full.rep[out], out) and (full.size[out] == 1).all() and np.isnan(full.sim[out]).all()
    assert np.array_equal(full.rep[keep], keep[part.rep]) and np.array_equal(full.size[keep], part.size)
    assert np.array_equal(bits(full.sim[keep]), bits(part.sim))
