"""The similarity graph on the MI355X at the limits tests/test_graph_gpu.py stays away from (inputs, helpers and their CPU-side
conditions: tests/graph_limits_data.py, tests/test_graph_limits_host.py).  Which line of which kernel each group pins:

  A  signs           gr_tile_kernel (gnn_graph.hip): `s >= a.threshold` on negative values and with a negative, a zero and a tied
                     threshold; `a.sim[at] = acc[mb][nb][r] * a.scale` on negative values and on an exact zero, which must be the +0
                     that gnn_neighbours returns; the values of NN_PRODUCTS (gnn_nn_frag.h) bit for bit those of nn_tile_kernel on
                     six tiles, two steps and, under the split of 32, eleven parts.
  B  sizes, scan     nn_tile_range / nn_step_column (gnn_nn_frag.h) with n on and beside the 32-column block, the 64-row tile and the
                     256-column step: `t.b1 > t.r0 + 1`, `min(blk, last_blk)`, `col < t.b1`; nn_scan_kernel with n * splits at 1023,
                     1024 and 1026: `per = (m + SCAN_THREADS - 1) / SCAN_THREADS`, `min(m, threadIdx.x * per)`, the runs of two.
  C  row scales      nn_prepare_kernel (gnn_neighbours.hip) as the graph reaches it: `frexpf(amax, &ex)` / `ldexpf(x[e], -ex)` from
                     all-subnormal rows to FLT_MAX, one-hot rows, heavy tails; under dot `a NaN fails >=` in gr_tile_kernel for rows
                     beyond the f16 range, which stay valid and are never an edge.
  D  two ranges      SPLIT_MAX = 65280 in nn_tile_grid: `cnt[(r0 + tid) * a.splits + blockIdx.y]` written by a second range, the early
                     exit `t.b1 > t.r0 + 1` of range 0 for the tile at row 65280, `t.c0 = max(t.b0, t.r0)` in that tile,
                     `a.off[i]` / `a.off[i + 1]` of a row whose segment continues from part 0 into part 1, gr_indptr_kernel's
                     `off[i * splits]`, the scan over 130 700 counters.
  E  count / fill    gr_fill (gnn_graph.hip): `nn_prepare` again before the fill, `gr_args` reading the workspace's split of the COUNT
                     and the fragment buffers as they are now; `host_rows` in gr_check_fill and nn_upload_rows; `if (at < end)` of
                     gr_tile_kernel<true> with rows that changed since the count, both ways.

References: fp64 similarities of the f32 rows actually passed, exact where every dot is an integer, otherwise the band rule
(graph_limits_data.band_rule) with VALUE_TOL = 1e-5 on the values and GAP = 2e-5 around the threshold; the device's own values from
gnn_neighbours where the threshold is one of them.  gnn_neighbours returns at most 64 neighbours, so the 333 x 333 values are put
together from searches against base rows 0..63, 64..127, ...: a pair's value depends on its two rows only.

Out of scope, on record: a total beyond 2^31 edges (the offsets are int64 for it, but it needs 17 GB of output), the error for more
than 65535 ranges (over 2 M rows at the smallest split), and any change to the scan itself.

Measured on an MI355X (profiles/graph/README.md, "At the limits"): max |sim - fp64| 1.5e-7 on signed rows (40110 / 27568 / 15119
edges at -0.05 / 0.0 / 0.05 with 10 / 12 / 9 pairs in the band: the device's counts are fp64's), 2.0e-7 on the extreme base at 0.05
(13356 edges, 14 in the band; 1.5e-7 at rows up to FLT_MAX, 1.5e-7 at all-subnormal rows, 3.6e-8 at one-hot rows, 1.1e-7 at heavy
rows) and exactly 1.0f on its 12 edges at 0.5, 3.4e-7 on heavy rows (1297 / 266 edges, none in the band), 4.8e-7 on the 701 entries at
the 75 sampled rows of the 65350 (2 in the band; 690 edges have their column in the second range), all against the bound of 1e-5.
The graph of 65350 rows at 0.55 has 325103 edges and takes 0.13 s, the upload of 134 MB included; group D as a whole takes 1.1 s,
no other test more than 0.02 s, the file 2.2 s.  With changed rows the fill wrote 602 of 602 counted entries (sparse count, dense
fill) and 602 of 55278 (dense count, sparse fill), none outside its row's segment.  No test found a fault in the kernels."""
import ctypes as C
import time

import numpy as np
import pytest

from genomad_amd import _lib
from genomad_amd._lib import GnnError, check
from genomad_amd.engine import NNEngine
from tests import embedding_limits_data as lim
from tests import graph_limits_data as gd
from tests.clusters_data import planted
from tests.embedding_limits_data import VALUE_TOL
from tests.graph_limits_data import same_bits
from tests.neighbours_data import rows
from tests.test_embedding_limits_gpu import bits, neighbours_dev
from tests.test_graph_gpu import check_shape, csr

pytestmark = pytest.mark.gpu

COSINE = _lib.KNN_METRICS["cosine"]


def device_values(engine, r, metric="cosine"):
    """s[i, j] = the f32 gnn_neighbours returns for query i and base row j, for every pair of the rows: one search per 64 base rows"""
    n = len(r)
    s = np.full((n, n), np.nan, np.float32)
    for c0 in range(0, n, 64):
        b = np.ascontiguousarray(r[c0:c0 + 64])
        idx, sim = engine.neighbours(r, b, len(b), metric)
        assert (idx >= 0).all()
        part = np.empty((n, len(b)), np.float32)
        np.put_along_axis(part, idx, sim, axis=1)
        s[:, c0:c0 + len(b)] = part
    assert not np.isnan(s).any()
    return s


def split_free(engine, r, t, first, splits, metric="cosine"):
    for split in splits:
        engine.set_neighbour_split(split)
        assert same_bits(csr(engine.graph(r, t, metric)), first), split


# ---- A: signs ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def signed():
    r = gd.signed_base()
    return r, gd.upper64(r)


@pytest.fixture(scope="module")
def integers():
    return gd.integer_base()


@pytest.mark.parametrize("t", gd.SIGN_THRESHOLDS)
def test_a_signed_rows_at_a_negative_a_zero_and_a_positive_threshold(engine, signed, t):
    r, s64 = signed
    try:
        engine.set_neighbour_split(0)
        res = engine.graph(r, t)
        check_shape(res, 333)
        err = gd.check_band(csr(res), s64, t)
        edges, band = gd.band_counts(s64, t)
        print(f"\nsigned rows at {t}: {res.n_edges} edges (fp64: {edges}, {band} in the band), max |sim - fp64| = {err:.3e}")
        assert abs(res.n_edges - edges) <= band and res.valid.all()
        assert (res.sim >= np.float32(t)).all()                       # at 0.0 and above, no negative value passes `s >= a.threshold`
        if t < 0:
            assert (res.sim < 0).sum() > 10000                       # the pairs of [-0.05 + GAP, -GAP): negative values in the output
        split_free(engine, r, t, csr(res), gd.SPLITS)
    finally:
        engine.set_neighbour_split(0)


def test_a_the_values_are_those_neighbours_returns_on_six_tiles(engine, signed):
    """test_the_values_are_those_neighbours_returns of tests/test_graph_gpu.py carried from 65 rows to 333, with a negative threshold"""
    r, _ = signed
    try:
        for split in (0, 32):
            engine.set_neighbour_split(split)
            s = device_values(engine, r)
            upper = s[np.triu_indices(333, 1)]
            threshold = np.sort(upper)[len(upper) // 10]              # one of the device's values: a tie exactly on the threshold
            assert threshold.dtype == np.float32 and threshold < 0 and (upper == threshold).any()
            res = engine.graph(r, threshold)
            check_shape(res, 333)
            a, b, got = res.edges()
            want = np.triu(s >= threshold, 1)
            assert res.n_edges == int((upper >= threshold).sum()) and np.array_equal(np.stack([a, b]), np.stack(np.nonzero(want))), split
            assert np.array_equal(bits(got), bits(s[a, b])), split
            assert (got == threshold).any() and (got < 0).any()
    finally:
        engine.set_neighbour_split(0)


def test_a_signed_integer_dots_with_ties_and_zeros(engine, integers):
    r, dots = integers
    neg, pos = lim.integer_thresholds(r)
    try:
        engine.set_neighbour_split(0)
        s = device_values(engine, r, "dot")
        for t, ties in ((neg, 132), (pos, 107)):
            for split in (0, 32):
                engine.set_neighbour_split(split)
                res = engine.graph(r, t, "dot")
                check_shape(res, gd.N_INTEGER)
                gd.check_exact(csr(res), dots, t)
                a, b, got = res.edges()
                assert int((dots[a, b] == t).sum()) == ties, (t, split)
                assert np.array_equal(bits(got), bits(s[a, b])), (t, split)
                zero = dots[a, b] == 0
                assert zero.sum() == (107 if t < 0 else 0)
                assert (bits(got[zero]) == 0).all() and (bits(s[a, b][zero]) == 0).all()          # +0.0f, as neighbours returns it
    finally:
        engine.set_neighbour_split(0)


# ---- B: sizes and the scan ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", gd.PREFIXES)
def test_b_block_tile_and_step_borders(engine, integers, n):
    r, dots = integers
    r, dots = np.ascontiguousarray(r[:n]), dots[:n, :n]
    try:
        for t in lim.integer_thresholds(integers[0]):
            for split in gd.PREFIX_SPLITS:
                engine.set_neighbour_split(split)
                res = engine.graph(r, t, "dot")
                check_shape(res, n)
                edges = gd.check_exact(csr(res), dots, t)
                assert (edges > 0) == (n >= 31 or t < 0), (t, split)
    finally:
        engine.set_neighbour_split(0)


@pytest.mark.parametrize("n, split, total", gd.SCAN_CASES)
def test_b_counters_near_the_scans_1024_threads(engine, integers, n, split, total):
    r, dots = integers
    r, dots = np.ascontiguousarray(r[:n]), dots[:n, :n]
    split_rows = (split + 31) // 32 * 32                              # what nn_tile_grid makes of the debug split
    assert n * ((n + split_rows - 1) // split_rows) == total == gd.counters(n, split)
    assert (total < gd.SCAN_THREADS, total == gd.SCAN_THREADS, total > gd.SCAN_THREADS) == (total == 1023, total == 1024, total == 1026)
    try:
        for t in lim.integer_thresholds(integers[0]):
            engine.set_neighbour_split(0)
            first = csr(engine.graph(r, t, "dot"))
            engine.set_neighbour_split(split)
            got = csr(engine.graph(r, t, "dot"))
            assert gd.check_exact(got, dots, t) > 0 and same_bits(got, first), t
    finally:
        engine.set_neighbour_split(0)


# ---- C: row scales -----------------------------------------------------------------------------------------------------------------

def test_c_a_power_of_two_per_row_changes_no_bit(engine, signed):
    r, _ = signed
    r2 = lim.power_of_two_scaled(r, 3)                                # 2^-100 .. 2^100, exact
    try:
        engine.set_neighbour_split(0)
        own = engine.neighbours(r, None, 10)
        threshold = np.sort(own[1][:, 0])[333 // 2]                   # one of the device's values, as test_a_power_of_two_per_row_changes_no_bit picks it
        assert threshold.dtype == np.float32 and 0 < threshold < 1
        first = engine.graph(r, threshold)
        check_shape(first, 333)
        assert 333 // 4 <= first.n_edges < 333 * 332 // 2 and (first.sim == threshold).any()
        for split in (0, 32):
            engine.set_neighbour_split(split)
            assert same_bits(csr(engine.graph(r2, threshold)), csr(first)), split
    finally:
        engine.set_neighbour_split(0)


def kind_errors(res, s64):
    """the largest |sim - fp64| among the edges that touch each kind of extreme row, and among the others"""
    a, b, s = res.edges()
    err = np.abs(s.astype(np.float64) - s64[a, b])
    out, rest = {}, np.ones(len(a), bool)
    for name, sl in lim.EXTREME_KINDS.items():
        hit = ((a >= sl.start) & (a < sl.stop)) | ((b >= sl.start) & (b < sl.stop))
        out[name] = (int(hit.sum()), float(err[hit].max()) if hit.any() else 0.0)
        rest &= ~hit
    out["ordinary"] = (int(rest.sum()), float(err[rest].max()) if rest.any() else 0.0)
    return out


@pytest.mark.parametrize("t", (0.05, 0.5))
def test_c_rows_from_all_subnormal_to_flt_max(engine, t):
    base = lim.extreme_base()
    s64 = gd.upper64(base)
    try:
        engine.set_neighbour_split(0)
        res = engine.graph(base, t)
        check_shape(res, 333)
        assert res.valid.all()                                        # the all-subnormal rows too
        err = gd.check_band(csr(res), s64, t)
        edges, band = gd.band_counts(s64, t)
        print(f"\nextreme rows at {t}: {res.n_edges} edges (fp64: {edges}, {band} in the band), max |sim - fp64| = {err:.3e}")
        kinds = kind_errors(res, s64)
        for name, (count, e) in kinds.items():
            print(f"extreme rows at {t}, edges at {name} rows: {count}, max |sim - fp64| = {e:.3e}")
        assert abs(res.n_edges - edges) <= band
        if t == 0.05:
            assert all(kinds[name][0] > 0 for name in ("huge", "subnormal", "heavy", "ordinary"))
        else:
            _, pos, sign = lim.one_hot_rows()
            hot = lim.EXTREME_KINDS["one_hot"]
            a, b, s = res.edges()
            inside = (a >= hot.start) & (a < hot.stop) & (b >= hot.start) & (b < hot.stop)
            want = np.triu((pos[:, None] == pos[None, :]) & (sign[:, None] == sign[None, :]), 1)
            got = np.zeros((16, 16), bool)
            got[a[inside] - hot.start, b[inside] - hot.start] = True
            assert np.array_equal(got, want) and inside.sum() == 12
            assert (bits(s[inside]) == bits(np.float32(1.0))).all()                                # exactly 1.0f
        split_free(engine, base, t, csr(res), (32,))
    finally:
        engine.set_neighbour_split(0)


@pytest.mark.parametrize("t", (0.05, 0.2))
def test_c_heavy_rows(engine, t):
    r = lim.heavy_rows(333, 8)
    s64 = gd.upper64(r)
    try:
        engine.set_neighbour_split(0)
        res = engine.graph(r, t)
        check_shape(res, 333)
        err = gd.check_band(csr(res), s64, t)
        edges, band = gd.band_counts(s64, t)
        print(f"\nheavy rows at {t}: {res.n_edges} edges (fp64: {edges}, {band} in the band), max |sim - fp64| = {err:.3e}")
        assert band == 0 and res.n_edges == edges and res.valid.all()
        split_free(engine, r, t, csr(res), (32,))
    finally:
        engine.set_neighbour_split(0)


def test_c_rows_beyond_the_f16_range_are_valid_and_never_an_edge_under_dot(engine):
    base = lim.out_of_range_base()
    out = list(lim.OUT_OF_RANGE)
    keep = np.delete(np.arange(333), out)
    rest = np.ascontiguousarray(base[keep])
    dots = rest.astype(np.float64) @ rest.astype(np.float64).T
    threshold = float(np.sort(dots[np.triu_indices(331, 1)])[int(331 * 330 / 2 * 0.98)])
    try:
        for split in (0, 32):
            engine.set_neighbour_split(split)
            full, part = engine.graph(base, threshold, "dot"), engine.graph(rest, threshold, "dot")
            check_shape(full, 333)
            check_shape(part, 331)
            assert full.valid[out].all() and full.valid.all()
            assert (np.diff(full.indptr)[out] == 0).all() and not np.isin(full.col, out).any()      # they own nothing, nobody's partner
            assert not np.isnan(full.sim).any()
            assert same_bits(gd.renumbered(csr(full), keep, 333), csr(part)), split
            assert gd.check_exact(csr(part), dots, threshold) > 1000
            cl = engine.cluster(base, threshold, "dot")
            assert np.array_equal(full.degree(), cl.degree) and np.array_equal(full.components(), cl.label), split
            assert (cl.degree[out] == 0).all() and np.array_equal(cl.label[out], out)
    finally:
        engine.set_neighbour_split(0)


# ---- D: two ranges -----------------------------------------------------------------------------------------------------------------

def test_d_a_full_range_of_65280_columns_and_a_second_one(engine):
    """65350 rows under the split 1 << 20, which clamps to 65280: two ranges.  2.1 G pairs in two passes; the wall time is printed."""
    base, pairs = gd.two_range_base()
    mine = gd.two_range_mine()
    s64 = lim.self64(base, mine)
    n, t = lim.NB_CAPPED, gd.TWO_RANGE_THRESHOLD
    try:
        engine.set_neighbour_split(1 << 20)
        t0 = time.perf_counter()
        res = engine.graph(base, t)
        print(f"\n65350 rows at {t}, ranges of 65280: {res.n_edges} edges, {time.perf_counter() - t0:.3f} s")
        check_shape(res, n)
        got = csr(res)
        for i, j in pairs:                                            # every planted pair is an edge, at 1
            seg = res.col[res.indptr[i]:res.indptr[i + 1]]
            k = int(np.searchsorted(seg, j))
            assert k < len(seg) and seg[k] == j, (i, j)
            assert abs(float(res.sim[res.indptr[i] + k]) - 1) <= VALUE_TOL, (i, j)
        chain = list(gd.COPIES) + [n - 1]
        seg = res.col[res.indptr[gd.COPIES_OF]:res.indptr[gd.COPIES_OF + 1]]
        assert [int(c) for c in seg if c in chain] == chain          # from part 0 into part 1, the columns still ascending
        mask, val = gd.touching(got, mine, n)
        gd.band_rule(mask, s64, t)
        err = gd.value_rule(mask, val, s64)
        entries, band, unordered, second = gd.touching_counts(s64, mine, t)
        print(f"65350 rows, the 75 sampled rows: {int(mask.sum())} entries (fp64: {entries}, {band} in the band; {unordered} pairs, "
              f"{second} with the column in the second range), max |sim - fp64| = {err:.3e}")
        assert abs(int(mask.sum()) - entries) <= band
        second_range = int((res.col >= lim.SPLIT_MAX).sum())           # every such column is one of the last 70 rows: all sampled
        print(f"65350 rows: {second_range} edges have their column in the second range")
        assert abs(second_range - second) <= band
        cl = engine.cluster(base, t)                                  # the same rows, the same split
        assert res.n_edges == cl.n_edges
        assert np.array_equal(res.degree(), cl.degree) and np.array_equal(res.components(), cl.label)
        split_free(engine, base, t, got, gd.TWO_RANGE_SPLITS)
    finally:
        engine.set_neighbour_split(0)


# ---- E: the count / fill contract --------------------------------------------------------------------------------------------------

SENTINEL = -7


class Outputs:
    """rows, indptr, col and sim on the device; col and sim of ``cap`` elements, filled with the sentinel"""

    def __init__(self, engine, r, cap):
        self.engine, self.n, self.cap = engine, len(r), cap
        self.bufs = [engine.alloc(r.nbytes), engine.alloc(8 * (len(r) + 1)), engine.alloc(4 * cap), engine.alloc(4 * cap)]
        self.rows, self.indptr, self.col, self.sim = self.bufs
        self.rows.upload(r)
        self.reset()

    def reset(self):
        self.col.upload(np.full(self.cap, SENTINEL, np.int32))
        self.sim.upload(np.full(self.cap, float(SENTINEL), np.float32))

    def count(self, t):
        return self.engine.graph_count_dev(self.rows.ptr, self.n, t, self.indptr.ptr)

    def fill(self, t):
        self.engine.graph_fill_dev(self.rows.ptr, self.n, t, self.col.ptr, self.sim.ptr, self.cap)
        self.engine.sync()
        return (self.indptr.download((self.n + 1,), np.int64), self.col.download((self.cap,), np.int32),
                self.sim.download((self.cap,), np.float32))

    def free(self):
        for buf in self.bufs:
            buf.free()


def filled(out, total, want):
    """the first ``total`` entries are ``want`` bit for bit and nothing behind the last edge was touched"""
    indptr, col, sim = out
    return (same_bits((indptr, col[:total], sim[:total]), want) and (col[total:] == SENTINEL).all()
            and (sim[total:] == float(SENTINEL)).all())


@pytest.fixture(scope="module")
def contract(engine):
    """the planted rows, the device's graph of them at 0.8 under the library's own split, and the rows of the searches in between"""
    p, _ = planted()
    engine.set_neighbour_split(0)
    return p, 0.8, csr(engine.graph(p, 0.8)), rows(70, 3), rows(1000, 4)


@pytest.mark.parametrize("which", ("session", "fresh"))
def test_e_other_searches_a_changed_split_and_a_second_fill_between_count_and_fill(engine, contract, which):
    """On the session's engine the fragment buffers are as large as the suite made them; on a fresh one the cluster search of 1000
    rows grows them between the count and the fill."""
    p, t, want, other70, other1000 = contract
    total = len(want[1])
    eng = engine if which == "session" else NNEngine(0)
    out = None
    try:
        out = Outputs(eng, p, total + 64)
        eng.set_neighbour_split(32)
        assert out.count(t) == total
        eng.set_neighbour_split(4096)
        idx, _ = neighbours_dev(eng, other70, None, 10)
        assert (idx >= 0).all()
        assert eng.cluster(other1000, t).n_clusters > 1
        assert filled(out.fill(t), total, want)
        out.reset()
        assert filled(out.fill(t), total, want)                       # the count still stands: a second fill gives the same bits
    finally:
        if out is not None:
            out.free()
        eng.set_neighbour_split(0)
        if which == "fresh":
            eng.close()


def test_e_the_host_fill_survives_a_device_pointer_search_and_refuses_after_a_host_search(engine, contract):
    p, t, want, other70, other1000 = contract
    n, total = len(p), len(want[1])
    indptr, nnz = np.empty(n + 1, np.int64), C.c_int64(0)
    col, sim = np.full(total + 64, SENTINEL, np.int32), np.full(total + 64, float(SENTINEL), np.float32)
    try:
        engine.set_neighbour_split(0)
        check(engine.lib.gnn_graph_count(engine.ctx, p.ctypes.data, n, t, COSINE, indptr.ctypes.data, C.addressof(nnz)))
        assert nnz.value == total
        idx, _ = neighbours_dev(engine, other70, None, 10)            # device pointers: the uploaded rows stay, the fragments do not
        assert (idx >= 0).all()
        check(engine.lib.gnn_graph_fill(engine.ctx, n, t, COSINE, col.ctypes.data, sim.ctypes.data, total + 64))
        assert filled((indptr, col, sim), total, want)
        engine.cluster(other1000, t)                                  # host pointers: the uploaded rows are replaced
        assert engine.lib.gnn_graph_fill(engine.ctx, n, t, COSINE, col.ctypes.data, sim.ctypes.data, total + 64) == _lib.ERR_STATE
        with pytest.raises(GnnError, match=r"error -3: gnn_graph_fill: .*another search has replaced the rows"):
            check(engine.lib.gnn_graph_fill(engine.ctx, n, t, COSINE, col.ctypes.data, sim.ctypes.data, total + 64))
        assert filled((indptr, col, sim), total, want)                # the refused fill wrote nothing
        assert same_bits(csr(engine.graph(p, t)), want)               # and a fresh graph is right
    finally:
        engine.set_neighbour_split(0)


def written_inside_the_segments(out, total, n):
    """Garbage is allowed, an overrun is not: nothing at or behind the counted total, col and sim written together, and every col
    written inside row i's counted segment is a column in (i, n).  Returns how many entries were written."""
    indptr, col, sim = out
    assert indptr[-1] == total and (col[total:] == SENTINEL).all() and (sim[total:] == float(SENTINEL)).all()
    wrote = col[:total] != SENTINEL
    assert np.array_equal(wrote, sim[:total] != float(SENTINEL))
    row = np.repeat(np.arange(n), np.diff(indptr))
    assert ((col[:total][wrote] > row[wrote]) & (col[:total][wrote] < n)).all()
    return int(wrote.sum())


def test_e_rows_that_changed_since_the_count_give_garbage_inside_the_segments(engine, contract):
    """col and sim have room for the complete graph and 64 more, so even a broken guard stays inside the allocation."""
    p, t, want, _, _ = contract
    n, total = len(p), len(want[1])
    dense = gd.complete_rows(p)
    full = n * (n - 1) // 2
    out = None
    try:
        engine.set_neighbour_split(0)
        out = Outputs(engine, p, full + 64)
        assert out.count(t) == total                                  # a sparse count ...
        out.rows.upload(dense)
        wrote = written_inside_the_segments(out.fill(t), total, n)   # ... and a dense fill: call and synchronise succeed
        print(f"\nsparse count, dense fill: {wrote} of {total} counted entries written")
        assert wrote > 0
        out.reset()
        assert out.count(t) == full                                   # a dense count ...
        out.rows.upload(p)
        wrote = written_inside_the_segments(out.fill(t), full, n)    # ... and a sparse fill
        print(f"dense count, sparse fill: {wrote} of {full} counted entries written")
        assert 0 < wrote < full                                       # it leaves sentinels
        out.reset()
        assert out.count(t) == total                                  # afterwards the same engine counts and fills as ever
        assert filled(out.fill(t), total, want)
        assert same_bits(csr(engine.graph(p, t)), want)
    finally:
        if out is not None:
            out.free()
        engine.set_neighbour_split(0)
