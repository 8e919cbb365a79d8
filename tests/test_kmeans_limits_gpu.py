"""Spherical k-means on the MI355X at the limits tests/test_kmeans_gpu.py stays away from (the oracle, the inputs and their CPU-side
conditions: tests/moments_limits_data.py, tests/test_kmeans_limits_host.py; the images q of the rows are harvested by one-row calls of
the principal-component sums: tests/test_pca_limits_gpu.py, group A).  Which line of gnn_kmeans.hip each group pins:

  B  sums           km_update_kernel: `q = (long long)((float)hi[e] * 16777216.f) + (long long)((float)lo[e] * 16777216.f)` of general
                    rows into `ls[((l - w0) * 8 + e) * 64 + lane]` and `a.S + l * D + lane * 8 + e`, the flush's `e = (i >> 6) & 7`,
                    km_finish_kernel: every centroid element within one f32 of f32(S / |S|) of the exact integer sums, sizes exact.
  C  launch shapes  km_update_kernel<true> with per_block > 64: `i0 = blockIdx.x * per_block`, `i = i0 + wave; i < i1; i += 4`.
  D  windows        LDS_K = 16 and LDS_K_MAX = 128: k = 15, 16, 17, 32, 127, 128, 129 - a window not full, full, one group past it,
                    two, the last LDS size, the first size straight to memory -: `w0 += LDS_K`, `l < w0 || l >= w0 + LDS_K`,
                    `min(a.k - w0, LDS_K) * D`, `w0 + tid < a.k && tid < LDS_K`, `k <= m.lds_k`.
  E  two ranges     k = 65535 > SPLIT_MAX = 65280: nn_tile_grid's cap, `a.col_off + cg[nb]` and nn_tile_range's column offset in the
                    key, the row-side `atomicMax(a.key + r0 + tid, lkey[tid])` from workgroups of two ranges, the winner on either
                    side of the border and never the smaller column by default.
  F  stops          km_run: `changed == 0` before `iterations == max_iter`, at max_iter = the definition's own count and one less.
  G  extremes       one group of +-e_7: a sum of 2^32 per row, an exactly zero sum that keeps the init row.

The statement on the centroids, derived.  The sums are exact integers, equal to the oracle's.  km_finish_kernel sums 512 squares below
2^126 in float64 (relative error below 512 x 2^-53 = 6e-14, the square root and the division 2^-53 each) and rounds v / norm to f32
once: its float64 quotient is within 1e-13 of the exact one, an f32 is 6e-8 of its value wide, so the result is the correctly rounded
f32 or - where the exact quotient lies within 1e-13 of the middle of two f32, two in a million - its neighbour.  The oracle's float64
is as close.  The compiler may contract `ss += v * v`, so bit equality is not asserted: one f32 at the most, and the count is printed.

Measured on an MI355X (256 CUs).  Centroid elements that differ from the oracle's f32: 0 of 1 561 088 over all cases of B, C and D
(so 0 differ by one f32).  Times: E 1.2 s (kmeans with the uploads of 2 x 134 MB 0.17 s, the reference search 0.06 s, centroids
0.02 s, kmeans again in 2048 ranges of 32 columns 0.72 s), C (33 869 rows, 69 MB, 100 per-group harvests) 0.04 s, no other test above
0.01 s; this file and tests/test_pca_limits_gpu.py together 3.9 s.

Mutations, each applied to a scratch copy and run once (tests of this file that fail):
  km_update_kernel<true> starts at `i0 + wave + 4` when per_block > 64     C
  the key's column taken relative to its range (`cg[nb] - t.b0`)           E
  `iterations == max_iter` tested before `changed == 0`                    F at k = 7 and 33, E
  `col_off` dropped from the key (`(unsigned)cg[nb]`)                      none, and none can: cg is the absolute column here, col_off
                                                                           is non-zero only in the farthest-first traversal, and
                                                                           km_far_kernel reads the key's upper word alone
  the SPLIT_MAX cap lifted in nn_tile_grid                                 none: one range of 65 536 columns over fragments padded to
                                                                           65 536 gives the same labels; the cap serves the 16-bit
                                                                           offsets of the neighbour lists, which end at 65 534 here
  the flush bound `LDS_K - 1`                                              not run: for k = 17 the flush loop would then pass the end of
                                                                           S (only its `if (ls[i])` keeps it from writing there)
No test found a fault in the kernels."""
import time

import numpy as np
import pytest

from tests import moments_limits_data as md
from tests.embedding_limits_data import SPLIT_MAX
from tests.kmeans_data import defined, init_rows, planted
from tests.test_kmeans_gpu import bits, identical, is_neighbours
from tests.test_pca_limits_gpu import harvest_q, restore

pytestmark = pytest.mark.gpu

D = 512
WINDOW_KS = (15, 16, 17, 32, 127, 128, 129)


@pytest.fixture(scope="module")
def harvested(engine):
    return harvest_q(engine)


@pytest.fixture(autouse=True)
def settings_restored(engine):
    """every test of this file, however it ends, leaves the three test aids at the library's choice"""
    try:
        yield
    finally:
        restore(engine)


def one_ulp(what, got, want):
    """every element within one f32 of the oracle's; prints how many are not equal"""
    d = md.ulp_distance(got, want)
    print(f"\n{what}: {int((d != 0).sum())} of {d.size} centroid elements differ from the oracle's f32, by at most {int(d.max())} f32")
    return got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all() and d.max() <= 1


# ---- B: sums to the bit on general rows ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", (7, 33))
def test_b_centroids_of_general_rows_are_the_exact_sums_rounded_once(engine, harvested, k):
    """km_update_kernel's q of hi and lo into the LDS window and straight to memory; km_finish_kernel"""
    q, _ = harvested
    r, keep, _ = md.harvest_rows()
    i = np.arange(len(r))
    label = np.where(i % 10 == 4, -1, i % k)
    want = md.centroid_oracle(md.sum_oracle(q, label, k))
    want_size = np.bincount(label[keep & (label >= 0)], minlength=k)
    try:
        first = None
        for lds in (128, 16, 0):
            engine.set_kmeans_lds(lds)
            cent, size = engine.centroids(r, label, k)
            assert np.array_equal(size, want_size) and one_ulp(f"centroids, k {k}, lds {lds}", cent, want)
            first = cent if first is None else first
            assert np.array_equal(bits(cent), bits(first)), lds
    finally:
        restore(engine)


@pytest.mark.parametrize("k", (7, 33))
def test_b_the_centroids_kmeans_returns_are_the_sums_by_its_last_labels(engine, harvested, k):
    """km_run's update inside the iteration: the labels it held at its last update are the returned ones when it converged, else those
    of a run with one update less"""
    q, _ = harvested
    r, keep, _ = md.harvest_rows()
    init = np.ascontiguousarray(r[keep][:k])
    restore(engine)
    max_iter = 3
    res = engine.kmeans(r, k, init, max_iter)
    assert 1 <= res.iterations <= max_iter and (res.label[~keep] == -1).all() and res.size.sum() == 600
    last = res.label if res.converged else engine.kmeans(r, k, init, max_iter - 1).label
    S = md.sum_oracle(q, last, k)
    members = S.any(axis=1)
    print(f"\nk {k}: {res.iterations} updates, converged {res.converged}, {int(members.sum())} groups with members at the last update")
    assert members.sum() >= k // 2
    assert one_ulp(f"kmeans, k {k}", res.centroids[members], md.centroid_oracle(S)[members])
    assert is_neighbours(engine, r, res)


# ---- C: the library's own launch shapes ------------------------------------------------------------------------------------------------

def test_c_more_than_64_rows_per_workgroup_of_the_update(engine):
    """km_update_kernel<true> with per_block > 64: `i0 = blockIdx.x * per_block`, `i1`, the waves' stride of 4 from i0 + wave"""
    cus = engine.device_info()["cus"]
    r, keep = md.launch_rows(cus)
    n = len(r)
    assert n > 64 * 2 * cus                                                # per_block = ceil(n / (2 cus)) > 64
    t0 = time.perf_counter()
    restore(engine)
    i = np.arange(n)
    S100 = np.stack([engine.pca_moments_fixed(r[i % 100 == g])[1] for g in range(100)])       # S is order-free: a group's rows alone
    S5 = np.stack([S100[c::5].sum(axis=0) for c in range(5)])
    try:
        for k, S in ((5, S5), (100, S100)):
            label = i % k
            want = md.centroid_oracle(S)
            engine.set_kmeans_lds(128)
            cent, size = engine.centroids(r, label, k)
            assert np.array_equal(size, np.bincount(label[keep], minlength=k)) and one_ulp(f"{n} rows, k {k}", cent, want)
            engine.set_kmeans_lds(0)
            c0, s0 = engine.centroids(r, label, k)
            assert np.array_equal(bits(c0), bits(cent)) and np.array_equal(s0, size), k
    finally:
        restore(engine)
    print(f"\n{n} rows at {cus} CUs: {time.perf_counter() - t0:.2f} s")


# ---- D: window and threshold edges -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", WINDOW_KS)
def test_d_the_edges_of_the_lds_windows(engine, harvested, k):
    """km_update_kernel's windows: `w0 += LDS_K`, `l >= w0 + LDS_K`, the flush bound `min(a.k - w0, LDS_K)`, `k <= m.lds_k`"""
    q, _ = harvested
    r, keep, _ = md.harvest_rows()
    i = np.arange(len(r))
    try:
        for groups in (k - 1, k):                                          # the last group empty; every group with members
            label = i % groups
            want = md.centroid_oracle(md.sum_oracle(q, label, k))
            want_size = np.bincount(label[keep], minlength=k)
            first = None
            for lds in (128, 16, 0):
                engine.set_kmeans_lds(lds)
                cent, size = engine.centroids(r, label, k)
                assert np.array_equal(size, want_size), (groups, lds)
                assert one_ulp(f"k {k}, {groups} groups with members, lds {lds}", cent, want)
                first = cent if first is None else first
                assert np.array_equal(bits(cent), bits(first)), (groups, lds)
            assert groups == k or (not first[k - 1].any() and want_size[k - 1] == 0)
    finally:
        restore(engine)


def test_d_the_iteration_on_both_sides_of_the_lds_threshold(engine):
    """km_update's `k <= m.lds_k` inside km_run: k = 128 goes through LDS, k = 129 straight to memory; each against its other path"""
    r, keep, _ = md.harvest_rows()
    valid = np.ascontiguousarray(r[keep])
    try:
        for k in (128, 129):
            engine.set_kmeans_lds(128)
            res = engine.kmeans(r, k, valid[:k], 2)
            assert res.iterations >= 1 and res.size.sum() == 600 and is_neighbours(engine, r, res)
            engine.set_kmeans_lds(0)
            assert identical(engine.kmeans(r, k, valid[:k], 2), res), k
    finally:
        restore(engine)


# ---- E: two forced centroid ranges -----------------------------------------------------------------------------------------------------

def test_e_more_centroids_than_one_range_holds(engine):
    """k = 65535 > SPLIT_MAX: two ranges whatever the split; `a.col_off + cg[nb]` with the range's offset, atomicMax across workgroups"""
    r, source = md.range_rows()
    n, k = md.RANGE_N, md.RANGE_K
    assert k > SPLIT_MAX
    t0 = time.perf_counter()
    try:
        restore(engine)
        init = r[:k]
        res = engine.kmeans(r, k, init, 1)
        t1 = time.perf_counter()
        assert np.array_equal(res.label[:k], np.arange(k))
        assert np.array_equal(res.label, source)                           # every copy carries its source's index: both sides of the border
        assert set(source[k:]) == set(md.RANGE_SOURCES) and max(md.RANGE_SOURCES) > SPLIT_MAX > min(md.RANGE_SOURCES)
        assert np.array_equal(res.size, np.bincount(source, minlength=k)) and set(res.size) == {1, 9, 10}
        assert res.iterations == 1 and res.converged and (res.init_rows == -1).all()
        assert (res.sim > 1 - 1e-5).all()
        assert is_neighbours(engine, r, res)                               # five query slabs of the reference, two base ranges
        t2 = time.perf_counter()
        cent, size = engine.centroids(r, res.label, k)
        assert np.array_equal(bits(cent), bits(res.centroids)) and np.array_equal(size, res.size)
        t3 = time.perf_counter()
        engine.set_neighbour_split(32)
        again = engine.kmeans(r, k, init, 1)
        assert np.array_equal(again.label, res.label) and np.array_equal(bits(again.sim), bits(res.sim))
        assert np.array_equal(bits(again.centroids), bits(res.centroids))
        t4 = time.perf_counter()
    finally:
        restore(engine)
    print(f"\n{n} rows, k {k}: kmeans {t1 - t0:.2f} s, neighbours {t2 - t1:.2f} s, centroids {t3 - t2:.2f} s, kmeans in ranges of 32 "
          f"{t4 - t3:.2f} s")


# ---- F: stops --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", (7, 33))
def test_f_the_iteration_stops_where_the_definition_does(engine, k):
    """km_run: `if (changed == 0) { converged }` stands before `if (iterations == max_iter) break`"""
    r, _ = planted()
    init = init_rows("first", k)
    it = defined(k, "first")[0][4]
    restore(engine)
    for max_iter, converged in ((it, True), (it - 1, False)):
        res = engine.kmeans(r, k, init, max_iter)
        assert res.iterations == max_iter and res.converged == converged, max_iter
        label, sim, cent, size, iterations, conv, picks = defined(k, "first", max_iter)[0]
        assert (iterations, conv) == (max_iter, converged)
        assert np.array_equal(res.label, label) and np.array_equal(res.size, size) and np.array_equal(res.init_rows, picks)
        assert is_neighbours(engine, r, res)


# ---- G: saturation and extremes --------------------------------------------------------------------------------------------------------

def test_g_one_group_of_an_axis_and_its_negative(engine):
    """km_update_kernel with q = +-2^32 per row; km_finish_kernel's `!(ss > 0.0)` on a sum that cancels exactly: the init row is kept"""
    restore(engine)
    for plus, minus, s7 in ((300, 212, 1), (212, 300, -1), (256, 256, 1)):
        want = np.zeros(D, np.float32)                                     # +0 everywhere else: 0 / norm
        want[7] = s7
        r, sign = md.axis_rows(plus, minus)
        res = engine.kmeans(r, 1)
        assert list(res.init_rows) == [0] and sign[0] == 1 and list(res.size) == [512] and (res.label == 0).all()
        assert res.iterations == 1 and res.converged
        assert np.array_equal(bits(res.centroids[0]), bits(want)), (plus, minus)      # 256 of each: the sum is zero, the init row +e_7 stays
        assert np.array_equal(np.sign(res.sim), sign * want[7]) and (np.abs(res.sim) == 1).all()
        cent, size = engine.centroids(r, np.zeros(512, np.int64), 1)
        assert list(size) == [512] and np.array_equal(bits(cent[0]), bits(want if plus != minus else np.zeros(D, np.float32)))
