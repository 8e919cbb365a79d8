"""Matches against a reference on the MI355X at the limits tests/test_match_gpu.py stays away from (inputs, helpers and their CPU-side
conditions: tests/match_limits_data.py, tests/test_match_limits_host.py).  Which line of which kernel each group pins:

  A  signs           gr_tile_kernel<., true> (gnn_graph.hip): `rok && cg[nb] >= 0 && s >= a.threshold` on negative values and with a
                     negative, a zero and a tied threshold; `a.sim[at] = acc[mb][nb][r] * a.scale` on negative values and on an
                     exact zero, which must be +0; the values bit for bit those of nn_tile_kernel on three query tiles and two steps.
  B  borders, scan   nn_tile_range(..., upper = false) / nn_step_column with n_query and n_base on and beside the 32-column block, the
                     64-row tile and the 256-column step, with rows that differ; nn_scan_kernel with n_query * splits at 1023, 1024
                     and 1026.
  C  slabs           gr_prepare: ALL query rows into qfrag / qvalid at once, 16454 of them, where nn_search works in slabs of 16384;
                     the neighbour search and a small match on the same engine afterwards.
  D  two ranges      SPLIT_MAX = 65280 over the base: `cnt[(r0 + tid) * a.splits + blockIdx.y]` written by a second range, `a.off[i]`
                     / `a.off[i + 1]` of a row whose segment continues from part 0 into part 1.
  E  row scales      nn_prepare_kernel on either side, from all-subnormal rows to FLT_MAX; under dot `a NaN fails >=` for rows beyond
                     the f16 range, as query and as base.
  F  count / fill    `if (at < end)` of gr_tile_kernel<true, true> with query or base rows that changed since the count, both ways.
  G  host side       MatchResult.transpose on a rectangle; GraphResult.extend with invalid rows in all three pieces.

References: fp64 similarities of the f32 rows actually passed, exact where every dot is an integer, otherwise the band rule
(graph_limits_data.band_rule) with VALUE_TOL = 1e-5 on the values and GAP = 2e-5 around the threshold; the device's own values from
gnn_neighbours where the threshold is one of them.

Measured on an MI355X: the signed rows 133 x 333 (and 333 x 133) have 32309 / 22350 / 12200 matches at -0.05 / 0.0 / 0.05 with 9 / 9 /
5 pairs in the band - the device's counts are fp64's - and max |sim - fp64| 7.7e-7 (the pairs (i, i)); 16454 x 333 at 0.1 has 601990
matches in 0.027 s, its 200 sampled rows 7314 (5 in the band) at 3.6e-7; 333 x 16454 the same 601990 (507 in the band); 75 x 65350 at
0.34 has 1824 matches (1 in the band; 57 in the second range, 47 query rows with matches in both ranges) at 4.2e-7 in 0.12 s; extreme
queries x extreme base 2760 matches at 0.05 and 58 at 0.5.  With changed rows the fill wrote 403 (dense queries) and 94 (dense base) of
the 488 counted entries and 488 of 44289 (dense count, sparse fill), none outside its row's segment.  Group D takes 0.9 s, the two
slab tests 0.2 s and 0.3 s, no other test more than 0.02 s, the file 2.6 s.  No test found a fault in the kernels."""
import time

import numpy as np
import pytest

from genomad_amd import sequence
from tests import embedding_limits_data as lim
from tests import graph_limits_data as gd
from tests import match_limits_data as md
from tests.clusters_data import planted
from tests.embedding_limits_data import GAP, VALUE_TOL
from tests.neighbours_data import sims64
from tests.test_embedding_limits_gpu import bits, same_pair
from tests.test_match_gpu import check_shape, csr

pytestmark = pytest.mark.gpu

same_bits = md.same_bits


def device_values(engine, q, b, metric="cosine"):
    """s[i, j] = the f32 gnn_neighbours returns for query i and base row j, for every pair: one search per 64 base rows"""
    s = np.full((len(q), len(b)), np.nan, np.float32)
    for c0 in range(0, len(b), 64):
        part = np.ascontiguousarray(b[c0:c0 + 64])
        idx, sim = engine.neighbours(q, part, len(part), metric)
        assert (idx >= 0).all()
        out = np.empty((len(q), len(part)), np.float32)
        np.put_along_axis(out, idx, sim, axis=1)
        s[:, c0:c0 + len(part)] = out
    assert not np.isnan(s).any()
    return s


def report(what, res, s64, t, err):
    matches, band = md.band_counts(s64, t)
    print(f"\n{what} at {t}: {res.n_edges} matches (fp64: {matches}, {band} in the band), max |sim - fp64| = {err:.3e}")
    assert abs(res.n_edges - matches) <= band
    return matches, band


def split_free(engine, q, b, t, first, splits, metric="cosine"):
    for split in splits:
        engine.set_neighbour_split(split)
        assert same_bits(csr(engine.match(q, b, t, metric)), first), split


# ---- A: signs ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("t", gd.SIGN_THRESHOLDS)
@pytest.mark.parametrize("nq, nb", md.SHAPES)
def test_a_signed_rows_at_a_negative_a_zero_and_a_positive_threshold(engine, nq, nb, t):
    q, b, s64 = md.signed_sides(nq, nb)
    assert md.band_is_narrow(s64, t)
    try:
        engine.set_neighbour_split(0)
        res = engine.match(q, b, t)
        check_shape(res, nq, nb)
        err = md.check_band(csr(res), s64, t)
        report(f"signed rows {nq} x {nb}", res, s64, t, err)
        assert res.query_valid.all() and res.base_valid.all() and (res.sim >= np.float32(t)).all()
        if t < 0:
            assert (res.sim < 0).sum() > 5000                        # negative values in the output
        split_free(engine, q, b, t, csr(res), gd.SPLITS)
    finally:
        engine.set_neighbour_split(0)


def test_a_the_values_are_those_neighbours_returns_on_three_tiles_and_two_steps(engine):
    q, b, _ = md.signed_sides(133, 333)
    try:
        for split in (0, 32):
            engine.set_neighbour_split(split)
            s = device_values(engine, q, b)
            threshold = np.sort(s.reshape(-1))[s.size // 10]          # one of the device's values: a tie exactly on the threshold
            assert threshold.dtype == np.float32 and threshold < 0 and (s == threshold).any()
            res = engine.match(q, b, threshold)
            check_shape(res, 133, 333)
            a, c, got = res.edges()
            assert np.array_equal(np.stack([a, c]), np.stack(np.nonzero(s >= threshold))), split
            assert np.array_equal(bits(got), bits(s[a, c])), split
            assert (got == threshold).any() and (got < 0).sum() > 5000
    finally:
        engine.set_neighbour_split(0)


def test_a_signed_integer_dots_with_ties_zeros_and_the_negated_row(engine):
    q, b, dots = md.integer_sides()
    neg, pos = lim.integer_thresholds(lim.signed_integer_rows(gd.N_INTEGER))
    copies = [0, 19, 210]                                             # row 3 and its copies among the base rows
    try:
        for t in (neg, pos):
            for split in (0, 32):
                engine.set_neighbour_split(split)
                res = engine.match(q, b, t, "dot")
                check_shape(res, len(q), len(b))
                matches = md.check_exact(csr(res), dots, t)
                a, c, got = res.edges()
                assert (dots[a, c] == t).sum() > 10, (t, split)       # ties on the threshold match
                zero = dots[a, c] == 0
                assert zero.sum() == ((dots == 0).sum() if t < 0 else 0) and (bits(got[zero]) == 0).all()      # +0
                # the negated row: -dots[3, 3] lies far below the negative threshold, so it matches none of row 3's copies
                assert -dots[3, 0] < neg
                mine = res.col[res.indptr[77]:res.indptr[77 + 1]]
                assert not np.isin(copies, mine).any() and (1 in mine) == (dots[77, 1] >= t)
                assert np.isin(copies, res.col[res.indptr[3]:res.indptr[4]]).all()
        print(f"\ninteger rows 133 x 211 at {pos}: {matches} matches, exact")
    finally:
        engine.set_neighbour_split(0)


# ---- B: borders and the scan -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", gd.PREFIXES)
@pytest.mark.parametrize("side", ("query", "base"))
def test_b_block_tile_and_step_borders(engine, side, n):
    nq, nb = (n, gd.N_INTEGER) if side == "query" else (70, n)
    q, b, dots = md.integer_prefix(nq, nb)
    try:
        for t in lim.integer_thresholds(lim.signed_integer_rows(gd.N_INTEGER)):
            for split in gd.PREFIX_SPLITS:
                engine.set_neighbour_split(split)
                res = engine.match(q, b, t, "dot")
                check_shape(res, nq, nb)
                assert md.check_exact(csr(res), dots, t) > 0, (t, split)
    finally:
        engine.set_neighbour_split(0)


@pytest.mark.parametrize("nq, split, total", md.SCAN_CASES)
def test_b_counters_near_the_scans_1024_threads(engine, nq, split, total):
    q, b, dots = md.integer_prefix(nq, md.SCAN_BASE)
    split_rows = (split + 31) // 32 * 32
    assert nq * ((md.SCAN_BASE + split_rows - 1) // split_rows) == total == md.counters(nq, md.SCAN_BASE, split)
    assert (total < gd.SCAN_THREADS, total == gd.SCAN_THREADS, total > gd.SCAN_THREADS) == (total == 1023, total == 1024, total == 1026)
    try:
        for t in lim.integer_thresholds(lim.signed_integer_rows(gd.N_INTEGER)):
            engine.set_neighbour_split(0)
            first = csr(engine.match(q, b, t, "dot"))
            engine.set_neighbour_split(split)
            got = csr(engine.match(q, b, t, "dot"))
            assert md.check_exact(got, dots, t) > 0 and same_bits(got, first), t
    finally:
        engine.set_neighbour_split(0)


# ---- C: more query rows than a slab of the neighbour search ------------------------------------------------------------------------------

def listed_values_agree(res, idx, sim, t):
    """every pair gnn_neighbours lists is a match iff its value reaches the threshold, and then with the same bits"""
    val = np.full((res.n_query, res.n_base), np.nan, np.float32)
    a, c, s = res.edges()
    val[a, c] = s
    got = np.take_along_axis(val, idx, axis=1)
    hit = sim >= np.float32(t)
    assert np.array_equal(~np.isnan(got), hit) and np.array_equal(bits(got[hit]), bits(sim[hit]))
    return int(hit.sum())


def test_c_all_query_rows_at_once_where_the_neighbour_search_works_in_slabs(engine):
    q, pairs, triple = md.slab_queries()
    base = np.ascontiguousarray(q[:md.SLAB_BASE])
    q70 = np.ascontiguousarray(q[:70])
    t = md.SLAB_THRESHOLD
    mine = md.slab_sample()
    s64 = sims64(q[mine], base)
    assert md.band_is_narrow(s64, t)
    try:
        engine.set_neighbour_split(0)
        near70 = engine.neighbours(q70, base, 10)
        match70 = csr(engine.match(q70, base, t))
        t0 = time.perf_counter()
        res = engine.match(q, base, t)
        seconds = time.perf_counter() - t0
        check_shape(res, lim.NQ_SLABS, md.SLAB_BASE)
        got = csr(res)
        mask, val = md.rows_of(got, mine, md.SLAB_BASE)
        md.band_rule(mask, s64, t)
        err = md.value_rule(mask, val, s64)
        matches, band = md.band_counts(s64, t)
        print(f"\n16454 x 333 at {t}: {res.n_edges} matches, {seconds:.3f} s; the {len(mine)} sampled rows: {int(mask.sum())} (fp64: {matches}, "
              f"{band} in the band), max |sim - fp64| = {err:.3e}")
        assert abs(int(mask.sum()) - matches) <= band
        for i, j in ((lim.QSLAB, 5), (triple[1], triple[0]), (triple[2], triple[0])):      # the planted multiples and copies, at 1
            k = int(np.flatnonzero(mine == i)[0])
            assert mask[k, j] and abs(float(val[k, j]) - 1) <= VALUE_TOL, (i, j)
        idx, sim = engine.neighbours(q, base, 64)                     # two slabs
        assert listed_values_agree(res, idx, sim, t) > 100000
        # the same engine afterwards: the buffers hold 16454 prepared rows
        assert same_pair(engine.neighbours(q70, base, 10), near70)
        again = engine.match(q70, base, t)
        assert same_bits(csr(again), match70)
        assert same_bits(match70, (got[0][:71], got[1][:got[0][70]], got[2][:got[0][70]]))
        split_free(engine, q, base, t, got, (32,))
    finally:
        engine.set_neighbour_split(0)


def test_c_the_mirror_more_base_rows_than_a_slab(engine):
    b, _, triple = md.slab_queries()
    q = np.ascontiguousarray(b[:md.SLAB_BASE])
    t = md.SLAB_THRESHOLD
    s64 = sims64(q, b)
    assert md.band_is_narrow(s64, t)
    try:
        engine.set_neighbour_split(0)
        res = engine.match(q, b, t)
        check_shape(res, md.SLAB_BASE, lim.NQ_SLABS)
        err = md.check_band(csr(res), s64, t)
        report("333 x 16454", res, s64, t, err)
        seg = res.col[res.indptr[triple[0]]:res.indptr[triple[0] + 1]]
        assert np.isin([triple[0], triple[1], triple[2]], seg).all() and lim.QSLAB in res.col[res.indptr[5]:res.indptr[6]]
        split_free(engine, q, b, t, csr(res), (32, 4096))
    finally:
        engine.set_neighbour_split(0)


# ---- D: two ranges ---------------------------------------------------------------------------------------------------------------------

def test_d_a_full_range_of_65280_base_rows_and_a_second_one(engine):
    """75 queries against 65350 base rows under the split 1 << 20, which clamps to 65280: two ranges, two counters per query row"""
    q, base = md.two_range_sides()
    s64 = sims64(q, base)
    t = md.TWO_RANGE_THRESHOLD
    assert md.band_is_narrow(s64, t) and md.counters(75, lim.NB_CAPPED, 1 << 20) == 150
    try:
        engine.set_neighbour_split(1 << 20)
        t0 = time.perf_counter()
        res = engine.match(q, base, t)
        seconds = time.perf_counter() - t0
        check_shape(res, 75, lim.NB_CAPPED)
        got = csr(res)
        err = md.check_band(got, s64, t)
        report(f"75 x 65350, ranges of 65280, {seconds:.3f} s,", res, s64, t, err)
        mask, val = md.dense(got, 75, lim.NB_CAPPED)
        for i, at in enumerate(lim.CAPPED_PLANTS):
            for row in (i, 70 + i):
                assert mask[row, at] and abs(float(val[row, at]) - 1) <= VALUE_TOL, (row, at)
        for at in lim.CAPPED_TIE:
            assert mask[5, at] and abs(float(val[5, at]) - 1) <= VALUE_TOL
        second = mask[:, lim.SPLIT_MAX:].sum()
        both = mask[:, :lim.SPLIT_MAX].any(axis=1) & mask[:, lim.SPLIT_MAX:].any(axis=1)
        print(f"75 x 65350: {int(second)} matches in the second range, {int(both.sum())} query rows with matches in both")
        assert both[3] and both[4] and both.sum() >= 40
        for i in np.flatnonzero(both):                                # from part 0 into part 1, the columns still ascending
            seg = res.col[res.indptr[i]:res.indptr[i + 1]]
            assert (np.diff(seg) > 0).all() and seg[0] < lim.SPLIT_MAX <= seg[-1]
        split_free(engine, q, base, t, got, gd.TWO_RANGE_SPLITS)
    finally:
        engine.set_neighbour_split(0)


# ---- E: row scales ---------------------------------------------------------------------------------------------------------------------

def test_e_a_power_of_two_per_row_on_either_side_changes_no_bit(engine):
    q, b, _ = md.signed_sides(133, 333)
    q2, b2 = lim.power_of_two_scaled(q, 3), lim.power_of_two_scaled(b, 4)
    try:
        engine.set_neighbour_split(0)
        best = engine.neighbours(q, b, 10)[1][:, 5]
        threshold = np.sort(best)[len(best) // 2]                     # one of the device's values
        assert threshold.dtype == np.float32 and 0 < threshold < 1
        first = engine.match(q, b, threshold)
        check_shape(first, 133, 333)
        assert first.n_edges > 400 and (first.sim == threshold).any()
        for split in (0, 32):
            engine.set_neighbour_split(split)
            for what, (x, y) in {"queries": (q2, b), "base": (q, b2), "both": (q2, b2)}.items():
                assert same_bits(csr(engine.match(x, y, threshold)), csr(first)), (what, split)
    finally:
        engine.set_neighbour_split(0)


@pytest.mark.parametrize("t", (0.05, 0.5))
def test_e_rows_from_all_subnormal_to_flt_max(engine, t):
    base = lim.extreme_base()
    q = lim.extreme_queries(base)
    s64 = sims64(q, base)
    assert md.band_is_narrow(s64, t)
    try:
        engine.set_neighbour_split(0)
        res = engine.match(q, base, t)
        check_shape(res, 70, 333)
        assert res.query_valid.all() and res.base_valid.all()        # the all-subnormal rows too
        err = md.check_band(csr(res), s64, t)
        report("extreme queries x extreme base", res, s64, t, err)
        assert res.n_edges > 20
        split_free(engine, q, base, t, csr(res), (32,))
    finally:
        engine.set_neighbour_split(0)


@pytest.mark.parametrize("side", ("base", "query"))
def test_e_rows_beyond_the_f16_range_are_valid_and_never_match_under_dot(engine, side):
    r = lim.out_of_range_base()
    out = list(lim.OUT_OF_RANGE)
    keep = np.delete(np.arange(333), out)
    other = np.ascontiguousarray(np.random.default_rng(62).integers(-4, 4, (70, 512)).astype(np.float32))
    q, b = (other, r) if side == "base" else (r, other)
    keep_q, keep_b = (np.arange(70), keep) if side == "base" else (keep, np.arange(70))
    q0, b0 = np.ascontiguousarray(q[keep_q]), np.ascontiguousarray(b[keep_b])
    dots = q0.astype(np.float64) @ b0.astype(np.float64).T
    threshold = float(np.sort(dots.reshape(-1))[int(dots.size * 0.9)])
    try:
        for split in (0, 32):
            engine.set_neighbour_split(split)
            full, part = engine.match(q, b, threshold, "dot"), engine.match(q0, b0, threshold, "dot")
            check_shape(full, len(q), len(b))
            assert full.query_valid.all() and full.base_valid.all() and not np.isnan(full.sim).any()
            assert ((full.base_hits() if side == "base" else full.hits())[out] == 0).all()
            assert same_bits(md.without_rows(csr(full), keep_q, keep_b, len(q), len(b)), csr(part)), split
            assert md.check_exact(csr(part), dots, threshold) > 2000
    finally:
        engine.set_neighbour_split(0)


# ---- F: the count / fill contract ------------------------------------------------------------------------------------------------------

SENTINEL = -7


class Outputs:
    """query, base, indptr, col and sim on the device; col and sim of ``cap`` elements, filled with the sentinel"""

    def __init__(self, engine, q, b, cap):
        self.engine, self.nq, self.nb, self.cap = engine, len(q), len(b), cap
        self.bufs = [engine.alloc(q.nbytes), engine.alloc(b.nbytes), engine.alloc(8 * (len(q) + 1)), engine.alloc(4 * cap), engine.alloc(4 * cap)]
        self.query, self.base, self.indptr, self.col, self.sim = self.bufs
        self.query.upload(q)
        self.base.upload(b)
        self.reset()

    def reset(self):
        self.col.upload(np.full(self.cap, SENTINEL, np.int32))
        self.sim.upload(np.full(self.cap, float(SENTINEL), np.float32))

    def count(self, t):
        return self.engine.match_count_dev(self.query.ptr, self.nq, self.base.ptr, self.nb, t, self.indptr.ptr)

    def fill(self, t):
        self.engine.match_fill_dev(self.query.ptr, self.nq, self.base.ptr, self.nb, t, self.col.ptr, self.sim.ptr, self.cap)
        self.engine.sync()
        return (self.indptr.download((self.nq + 1,), np.int64), self.col.download((self.cap,), np.int32),
                self.sim.download((self.cap,), np.float32))

    def free(self):
        for buf in self.bufs:
            buf.free()


def filled(out, total, want):
    """the first ``total`` entries are ``want`` bit for bit and nothing behind the last match was touched"""
    indptr, col, sim = out
    return (same_bits((indptr, col[:total], sim[:total]), want) and (col[total:] == SENTINEL).all()
            and (sim[total:] == float(SENTINEL)).all())


def written_inside_the_segments(out, indptr_of_count, nb):
    """Garbage is allowed, an overrun is not: indptr is the count's, nothing at or behind its total is touched, col and sim are written
    together, and every written col is a base row.  Returns (query row, col, sim) of the written entries."""
    indptr, col, sim = out
    total = int(indptr_of_count[-1])
    assert np.array_equal(indptr, indptr_of_count)
    assert (col[total:] == SENTINEL).all() and (sim[total:] == float(SENTINEL)).all()
    wrote = col[:total] != SENTINEL
    assert np.array_equal(wrote, sim[:total] != float(SENTINEL))
    assert ((col[:total][wrote] >= 0) & (col[:total][wrote] < nb)).all()
    row = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    return row[wrote], col[:total][wrote], sim[:total][wrote]


def test_f_rows_that_changed_since_the_count_give_garbage_inside_the_segments(engine):
    """col and sim have room for the complete rectangle and 64 more, so even a broken guard stays inside the allocation."""
    p, _ = planted()
    q, b, t = np.ascontiguousarray(p[:133]), p, 0.8
    nq, nb = len(q), len(b)
    full = nq * nb
    out = None
    try:
        engine.set_neighbour_split(0)
        want = csr(engine.match(q, b, t))
        total = len(want[1])
        assert 0 < total < full // 10
        out = Outputs(engine, q, b, full + 64)
        assert out.count(t) == total
        assert filled(out.fill(t), total, want)                       # device pointers, sentinels behind the total
        busy_q = int(np.argmax(np.diff(want[0])))                     # the rows with the most partners: their copies match the most rows
        busy_b = int(np.argmax(np.bincount(want[1], minlength=nb)))
        for side in ("query", "base"):                                # a sparse count, then one side made dense, then the fill
            out.reset()
            assert out.count(t) == total
            if side == "query":
                out.query.upload(gd.complete_rows(b[busy_b:busy_b + 1], nq))       # 133 copies of one base row
            else:
                out.base.upload(gd.complete_rows(q[busy_q:busy_q + 1], nb))
            row, col, sim = written_inside_the_segments(out.fill(t), want[0], nb)
            print(f"\nsparse count, dense {side} at the fill: {len(row)} of {total} counted entries written")
            assert len(row) >= 10
            out.query.upload(q)
            out.base.upload(b)
            out.reset()
            assert out.count(t) == total and filled(out.fill(t), total, want)      # afterwards the same engine counts and fills as ever
        out.reset()
        out.query.upload(gd.complete_rows(p, nq))                     # the complete rectangle ...
        out.base.upload(gd.complete_rows(p, nb))
        assert out.count(t) == full
        dense_indptr = np.arange(nq + 1, dtype=np.int64) * nb
        out.query.upload(q)                                           # ... and a sparse fill
        out.base.upload(b)
        row, col, sim = written_inside_the_segments(out.fill(t), dense_indptr, nb)
        print(f"dense count, sparse fill: {len(row)} of {full} counted entries written")
        assert 0 < len(row) < full                                    # it leaves sentinels
        s64 = sims64(q, b)
        assert (s64[row, col] >= gd.threshold32(t) - GAP).all()       # every written entry is a true match of the rows as they are now
        assert (np.abs(sim.astype(np.float64) - s64[row, col]) <= VALUE_TOL).all()
        out.reset()
        assert out.count(t) == total and filled(out.fill(t), total, want)
        assert same_bits(csr(engine.match(q, b, t)), want)
    finally:
        if out is not None:
            out.free()
        engine.set_neighbour_split(0)


# ---- G: the transpose and the extension ------------------------------------------------------------------------------------------------

def test_g_the_transpose_of_a_rectangle_is_the_match_the_other_way_round(engine):
    r = lim.signed_integer_rows(gd.N_INTEGER)
    q, b = np.ascontiguousarray(r[:133]), np.ascontiguousarray(r[9:])      # 133 x 333, rows that overlap but are not aligned
    assert b.shape == (333, 512)
    try:
        for t in lim.integer_thresholds(r):
            for split in (0, 32):
                engine.set_neighbour_split(split)
                one, other = engine.match(q, b, t, "dot"), engine.match(b, q, t, "dot")
                assert one.n_edges == other.n_edges > 1000
                t_ptr, t_col, t_sim = one.transpose()
                assert t_ptr.dtype == np.int64 and t_col.dtype == np.int32 and t_sim.dtype == np.float32
                assert same_bits((t_ptr, t_col, t_sim), csr(other)), (t, split)
                assert not np.array_equal(t_ptr[:134], one.indptr)    # a rectangle is not its own transpose
    finally:
        engine.set_neighbour_split(0)


@pytest.mark.parametrize("split", (0, 32))
@pytest.mark.parametrize("metric", ("cosine", "dot"))
def test_g_extend_with_invalid_rows_in_every_piece(engine, metric, split):
    old, new = md.invalid_halves()
    whole_rows = np.ascontiguousarray(np.concatenate([old, new]))
    t = 0.05 if metric == "cosine" else 100.0
    try:
        engine.set_neighbour_split(split)
        a, cross, c = engine.graph(old, t, metric), engine.match(old, new, t, metric), engine.graph(new, t, metric)
        both, whole = a.extend(cross, c), engine.graph(whole_rows, t, metric)
        assert same_bits((both.indptr, both.col, both.sim), (whole.indptr, whole.col, whole.sim)) and cross.n_edges > 500
        assert np.array_equal(both.valid, whole.valid) and np.array_equal(both.valid, sequence.valid_rows(whole_rows, metric))
        assert (~both.valid).sum() == (6 if metric == "cosine" else 4) and both.n == 333 and both.n_edges == whole.n_edges
        bad = np.flatnonzero(~whole.valid)
        assert (np.diff(both.indptr)[bad] == 0).all() and not np.isin(both.col, bad).any()
        assert np.array_equal(cross.query_valid, a.valid) and np.array_equal(cross.base_valid, c.valid)
    finally:
        engine.set_neighbour_split(0)
