"""Region calls on the MI355X at the limits tests/test_regions_gpu.py stays away from (inputs: tests/regions_limits_data.py; what makes a
pass mean something, on the CPU: tests/test_regions_limits_host.py).  Everything is an integer or a byte: every comparison is
np.array_equal with dtype and shape, against sequence.call_regions.  What each group pins in gnn_regions.hip:

  emissions      load_q on the clamp at 0 and at 1, -0.0, subnormals, +-FLT_MAX, one +-inf or NaN among finite values, rint's ties at
                 k + 1/2 - one bin per contig, so qsum and evidence ARE the bin's q and flag, also against exact fractions; owner_of
                 over 8 002 contigs, the last two empty
  ties           dp_state's `a tie stays` and `the lowest s'`, carry_kernel's `lowest s with maximal d`, at every penalty and tile,
                 tile 4096 (TILE_MAX) included; planted ties across a tile seam, against regions written by hand; the host's rint of
                 penalty * 2^20 on penalties between two steps
  size           1 027 blocks (nn_scan_kernel with two counts per thread), 1 024 tiles at the default tile and 262 139 at tile 1
                 in one contig (carry_kernel, carry_back_kernel), a region across seven blocks, and one region of 262 139 bins whose
                 qsum needs the high word of region_emit_kernel's 64-bit atomics
  building block bin_offsets[0] > 0 with bins before and behind that belong to no contig; two calls with no sync between, the second
                 growing every buffer (the pinned CSR image behind `tables_read`, `a buffer that grows is freed first`), both orders
  errors         the count-only call and the call with exactly enough room, guard entries behind every array

Measured on an MI355X (profiles/regions/README.md, "At the limits"): every test passes on gnn_regions.hip as it stands; the slowest
device call is the long track at tile 1 (one thread carries 262 139 tiles), 0.12 s; eleven value-only mutants of the kernels each fail
tests here, five of them (no clamp at 1, no clamp at 0, the low word of the qsum atomics, a truncated penalty, `e[2] >= e[1]` in the
last state) none of tests/test_regions_gpu.py."""
import time

import numpy as np
import pytest

from genomad_amd import _lib, sequence
from tests import regions_limits_data as rd
from tests.test_regions_gpu import KEYS, _assert_equal, _raw_call, _untouched

pytestmark = pytest.mark.gpu

TILE_MAX = 4096


@pytest.fixture
def tiled(engine):
    yield engine
    engine.set_region_tile(256)


@pytest.fixture(scope="module")
def edge():
    """edge_track(), sequence.call_regions on it at penalty 0, and the emissions in exact arithmetic"""
    track, off = rd.edge_track()
    return track, off, sequence.call_regions(track, off, 0), rd.exact_emissions(track)


@pytest.fixture(scope="module")
def long_reference():
    """sequence.call_regions on long_track(), computed once per penalty"""
    return rd.long_reference


def _timed_call(engine, track, off, penalty, what):
    t = time.perf_counter()
    res = engine.call_regions(track, off, penalty)
    print(f"\n{what}: call_regions took {time.perf_counter() - t:.3f} s, {len(res.region_lo)} regions")
    return res


# ---- emissions ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", (1, 256))
def test_every_edge_value_in_every_column_beside_every_other(tiled, edge, tile):
    track, off, (state, regions), (xq, xev) = edge
    tiled.set_region_tile(tile)
    res = _timed_call(tiled, track, off, 0, f"edge track, tile {tile}")
    _assert_equal(res, state, regions)
    # one bin per region: the sums are the emissions themselves, here against exact fractions
    assert res.region_qsum.dtype == np.int64 and np.array_equal(res.region_qsum, xq)
    assert res.region_evidence.dtype == np.int64 and np.array_equal(res.region_evidence, xev.astype(np.int64))
    assert np.array_equal(res.state, xq.argmax(axis=1))                     # penalty 0: the lowest argmax, (0, 0, 0) gives state 0
    # the two trailing empty contigs yield no region
    assert len(res.region_lo) == 8000 and np.array_equal(res.region_contig, np.arange(8000)) and len(off) == 8003
    assert (res.region_lo == 0).all() and (res.region_hi == 1).all()


# ---- ties --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", (1, 4, 7, 256, TILE_MAX))
def test_a_track_dense_in_ties_at_every_penalty(tiled, tile):
    track, off = rd.tie_track()
    tiled.set_region_tile(tile)
    for penalty in (0, 0.25, 0.5, 1, 2, 4096):
        res = tiled.call_regions(track, off, penalty)
        _assert_equal(res, *rd.tie_reference(penalty))
    assert len(res.region_lo) == sum(1 for s in rd.TIE_SIZES if s)          # the largest penalty: one region per contig, 4097 bins too


@pytest.mark.parametrize("T", (4, 7, 256))
@pytest.mark.parametrize("p", (1, 3))
def test_ties_planted_across_a_tile_seam_give_the_regions_written_by_hand(tiled, T, p):
    track, off, state, regions = rd.planted_ties(T, p)
    for tile in (T, 1, TILE_MAX):
        tiled.set_region_tile(tile)
        res = tiled.call_regions(track, off, p)
        _assert_equal(res, state, regions)
        assert np.bincount(res.region_contig).tolist() == [1, 2, 1, 3], tile


def test_a_penalty_between_two_steps_is_rounded_to_the_nearest_ties_to_even(tiled):
    track, off = rd.fine_track()                                             # d in single units: P = 0, 1 and 2 give different paths
    for tile in (7, 256):
        tiled.set_region_tile(tile)
        for penalty, P in rd.FINE_PENALTIES:
            res = tiled.call_regions(track, off, penalty)
            _assert_equal(res, *sequence.call_regions(track, off, penalty))
            _assert_equal(res, *sequence.call_regions(track, off, P * 2.0 ** -20))


# ---- size --------------------------------------------------------------------------------------------------------------------------

LONG_REGIONS = {0: 157949, 0.25: 67483, 4: 832, 4096: 4}                  # of the numpy definition; the longest: 14, 30, 1 579, 262 139 bins


@pytest.mark.parametrize("penalty,tile", ((0, 256), (4, 256), (0.25, TILE_MAX), (4096, 256), (4096, 1)))
def test_more_than_1024_blocks_and_1024_tiles_in_one_contig(tiled, long_reference, penalty, tile):
    track, off = rd.long_track()
    state, regions = long_reference(penalty)
    tiled.set_region_tile(tile)
    res = _timed_call(tiled, track, off, penalty, f"long track, penalty {penalty}, tile {tile}")
    assert len(res.region_lo) == len(regions["lo"]) == LONG_REGIONS[penalty]
    _assert_equal(res, state, regions)
    if penalty == 4096:                                                      # the long contig is one region: the atomics' high word
        q, ev = sequence.region_emissions(track)
        a, b = int(off[rd.LONG_CONTIG]), int(off[rd.LONG_CONTIG + 1])
        want = q[a:b].astype(np.int64).sum(axis=0)
        assert res.region_contig.tolist() == [1, 2, 3, 5] and res.region_hi[1] == b - a == 262139
        assert np.array_equal(res.region_qsum[1], want) and (want > 1 << 32).all() and res.region_evidence[1] == int(ev[a:b].sum())


# ---- the building block ------------------------------------------------------------------------------------------------------------

def test_the_building_block_with_a_first_offset_above_zero_leaves_the_bins_around_alone(tiled):
    track, off = rd.tie_track()
    n = len(track)
    inf = np.full((1, 3), np.inf, np.float32)
    padded = np.concatenate([np.repeat(inf, 5, axis=0), track, np.repeat(inf, 3, axis=0)])      # 5 bins before the base, 3 behind the end
    dt, ds = tiled.alloc(padded.nbytes), tiled.alloc(len(padded))
    try:
        dt.upload(padded)
        for tile, penalty in ((7, 0.25), (256, 1), (TILE_MAX, 0)):
            tiled.set_region_tile(tile)
            ds.upload(np.full(len(padded), 9, np.uint8))
            tiled.region_states_dev(dt.ptr, off + 5, penalty, ds.ptr)
            tiled.sync()
            got = ds.download((len(padded),), np.uint8)
            assert (got[:5] == 9).all() and (got[5 + n:] == 9).all(), (tile, penalty)
            assert np.array_equal(got[5:5 + n], rd.tie_reference(penalty)[0]), (tile, penalty)
    finally:
        dt.free()
        ds.free()


@pytest.mark.parametrize("order", ("small first", "large first"))
def test_two_building_block_calls_with_no_sync_between(synth_weights, order):
    from genomad_amd.engine import NNEngine
    s_track, s_off, s_state, _ = rd.planted_ties(4, 1)
    # more contigs, tiles and bins than the slack of any buffer the small call has sized (a quarter of the need plus 64)
    tie, tie_off = rd.tie_track()
    edge = rd.edge_track()[0][:300]
    l_track = np.concatenate([tie, edge])
    l_off = np.concatenate([tie_off, tie_off[-1] + 1 + np.arange(300)])
    l_state = sequence.call_regions(l_track, l_off, 0.25)[0]
    assert len(l_off) - 1 > 2 * (len(s_off) + 64) and len(l_track) > 2 * (len(s_track) + 64)
    calls = [(s_track, s_off, 1, s_state), (l_track, l_off, 0.25, l_state)]
    if order == "large first":
        calls.reverse()
    with NNEngine(0, synth_weights) as fresh:                                # a ctx that has sized nothing yet
        fresh.set_region_tile(7)
        bufs = []
        try:
            for track, off, penalty, _ in calls:
                dt, ds = fresh.alloc(track.nbytes), fresh.alloc(len(track))
                bufs += [dt, ds]
                dt.upload(track)
                ds.upload(np.full(len(track), 9, np.uint8))
            fresh.sync()
            for i, (track, off, penalty, _) in enumerate(calls):           # back to back: nothing waits for the first
                fresh.region_states_dev(bufs[2 * i].ptr, off, penalty, bufs[2 * i + 1].ptr)
            fresh.sync()
            for i, (track, off, penalty, want) in enumerate(calls):
                assert np.array_equal(bufs[2 * i + 1].download((len(track),), np.uint8), want), (order, i)
        finally:
            for b in bufs:
                b.free()


# ---- errors ------------------------------------------------------------------------------------------------------------------------

def test_the_count_only_call_and_exactly_enough_room_on_8000_regions(engine, edge):
    track, off, (state, regions), _ = edge
    rc, n, st, arrs, msg = _raw_call(engine, track, off, 0, 0, arrays=False)           # the count-only call
    assert rc == 0 and n == 8000 and np.array_equal(st[:8000], state) and (st[8000:] == 77).all()
    rc, n, st, arrs, msg = _raw_call(engine, track, off, 0, 8000)                      # exactly enough
    assert rc == 0 and n == 8000 and _untouched(arrs, 8000) and (st[8000:] == 77).all()
    assert all(np.array_equal(arrs[k][:8000], regions[k]) for k in KEYS)
    rc, n, st, arrs, msg = _raw_call(engine, track, off, 0, 7999)                      # one too few: the count, and nothing written
    assert rc == _lib.ERR_ARG and n == 8000 and "the call has 8000" in msg and _untouched(arrs) and (st[8000:] == 77).all()
