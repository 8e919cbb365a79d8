"""Region calls on the MI355X (gnn_call_regions, gnn_region_states_dev): bit identity with sequence.call_regions on a hand-made track
whose contig sizes sit on every tile seam, invariance under the tile size, the building block, the error paths with guard values
behind the arrays, grow-only buffers across calls, and scan_regions end to end.  Only the last test runs forward passes."""
import ctypes as C

import numpy as np
import pytest

from genomad_amd import _lib, sequence, synthetic

pytestmark = pytest.mark.gpu

T = 7                                                   # the tile size the contig sizes below are cut around
SIZES = (0, 1, 0, 2, T - 1, 0, T, T + 1, 0, 2 * T, 3 * T + 5, 3, 4, 5, 8, 255, 0, 256, 257, 0, 300)     # 3, 4, 5, 8: the seams of tile 4
TILES = (1, 4, 7, 256)
PENALTIES = (0, 0.25, 1, 7.5, 4096)
KEYS = ("contig", "lo", "hi", "state", "evidence", "qsum")


def _track(sizes=SIZES, seed=11):
    """random scores, about 10 % NaN bins, a NaN run across a tile boundary of every tile size, exact ties (0.5 / 0.5 / 0)"""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    track = rng.random((int(off[-1]), 3), dtype=np.float32)
    track[rng.random(len(track)) < 0.1] = np.nan
    last = int(off[-2])                                 # the last contig, 300 bins: tiles of 1, 4, 7 and 256 all have seams in it
    if sizes[-1] == 300:
        track[last + 250:last + 262] = np.nan           # across bin 256 (and multiples of 4 and 7)
        track[last + 20:last + 40] = (0.5, 0.5, 0)
        track[last + 100:last + 130, :2] = 0.5          # ties between the first two classes, the third random
    return track, off


@pytest.fixture(scope="module")
def reference():
    """sequence.call_regions on the one track, once per penalty"""
    track, off = _track()
    return track, off, {p: sequence.call_regions(track, off, p) for p in PENALTIES}


@pytest.fixture
def tiled(engine):
    yield engine
    engine.set_region_tile(256)


def _assert_equal(res, state, regions):
    assert res.state.dtype == np.uint8 and np.array_equal(res.state, state)
    for k in KEYS:
        got = getattr(res, "region_" + k)
        assert got.dtype == regions[k].dtype and got.shape == regions[k].shape and np.array_equal(got, regions[k]), k


@pytest.mark.parametrize("tile", TILES)
def test_states_and_regions_equal_the_numpy_definition(tiled, reference, tile):
    track, off, want = reference
    tiled.set_region_tile(tile)
    for p in PENALTIES:
        res = tiled.call_regions(track, off, p)
        _assert_equal(res, *want[p])
        assert res.penalty == p and np.array_equal(res.bin_offsets, off) and res.start is None
    n_regions = [len(want[p][1]["lo"]) for p in PENALTIES]
    assert n_regions[0] > 150 and n_regions[-1] == sum(1 for s in SIZES if s) and sorted(n_regions, reverse=True) == n_regions


def test_outputs_do_not_depend_on_the_tile_size(tiled):
    track, off = _track(seed=12)
    outs = []
    for tile in TILES:
        tiled.set_region_tile(tile)
        outs.append([tiled.call_regions(track, off, p).asdict() for p in (0.25, 1)])
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert all(np.array_equal(a[k], b[k]) for k in ("state",) + tuple("region_" + k for k in KEYS))
    for bad in (0, 4097, -3):
        with pytest.raises(_lib.GnnError, match=r"\[1, 4096\]"):
            tiled.set_region_tile(bad)


def test_the_building_block_gives_the_states_of_call_regions(tiled, reference):
    track, off, want = reference
    dt, ds = tiled.alloc(track.nbytes), tiled.alloc(len(track))
    try:
        dt.upload(track)
        for tile in (4, 256):
            tiled.set_region_tile(tile)
            for p in (0, 1, 4096):
                ds.upload(np.full(len(track), 9, np.uint8))
                tiled.region_states_dev(dt.ptr, off, p, ds.ptr)
                tiled.sync()
                assert np.array_equal(ds.download((len(track),), np.uint8), want[p][0])
    finally:
        dt.free()
        ds.free()


def _raw_call(engine, track, off, penalty, cap, arrays=True, guard=3):
    """gnn_call_regions on arrays of `cap` regions followed by `guard` guard entries"""
    fill = {"contig": -7, "lo": -7, "hi": -7, "state": 77, "evidence": -7, "qsum": -7}
    arrs = {k: np.full((cap + guard, 3) if k == "qsum" else cap + guard, fill[k], np.uint8 if k == "state" else np.int64) for k in KEYS}
    state = np.full(len(track) + guard, 77, np.uint8)
    n = C.c_int64(-5)
    ptrs = [a.ctypes.data if arrays else None for a in arrs.values()]
    rc = engine.lib.gnn_call_regions(engine.ctx, track.ctypes.data, off.ctypes.data, len(off) - 1, float(penalty), state.ctypes.data, *ptrs,
                                     cap, C.byref(n))
    return rc, n.value, state, arrs, (engine.lib.gnn_last_error() or b"").decode()


def _untouched(arrs, start=0):
    return all((a[start:] == (77 if k == "state" else -7)).all() for k, a in arrs.items())


def test_errors_name_what_is_needed_and_write_nothing_past_a_capacity(engine, reference):
    track, off, want = reference
    state, regions = want[0.25]
    need = len(regions["lo"])
    rc, n, st, arrs, msg = _raw_call(engine, track, off, 0.25, need - 1)             # one region too few
    assert rc == _lib.ERR_ARG and n == need and f"the call has {need}" in msg and f"hold {need - 1} regions" in msg
    assert _untouched(arrs) and (st[len(track):] == 77).all()
    rc, n, st, arrs, msg = _raw_call(engine, track, off, 0.25, 0, arrays=False)      # the count-only call
    assert rc == 0 and n == need and np.array_equal(st[:len(track)], state) and (st[len(track):] == 77).all()
    rc, n, st, arrs, msg = _raw_call(engine, track, off, 0.25, need)                 # exactly enough
    assert rc == 0 and n == need and _untouched(arrs, need) and (st[len(track):] == 77).all()
    assert all(np.array_equal(arrs[k][:need], regions[k]) for k in KEYS)
    for penalty in (-1, 4097, float("nan")):
        rc, n, st, arrs, msg = _raw_call(engine, track, off, penalty, need)
        assert rc == _lib.ERR_ARG and "[0, 4096]" in msg and n == -5 and _untouched(arrs) and (st == 77).all()
    bad = off.copy()
    bad[4] = bad[3] - 1
    rc, n, st, arrs, msg = _raw_call(engine, track, bad, 1, need)
    assert rc == _lib.ERR_ARG and "non-decreasing" in msg and n == -5 and _untouched(arrs) and (st == 77).all()
    some = [a.ctypes.data for a in arrs.values()]
    some[2] = None                                                                   # five of the six arrays
    rc = engine.lib.gnn_call_regions(engine.ctx, track.ctypes.data, off.ctypes.data, len(off) - 1, 1.0, None, *some, need, C.byref(C.c_int64()))
    assert rc == _lib.ERR_ARG and b"together" in engine.lib.gnn_last_error()
    # nothing to do: no contig, or no bin
    empty = np.zeros(3, np.int64)
    for offs in (empty[:1], empty):
        rc, n, st, arrs, msg = _raw_call(engine, track, offs, 1, need)
        assert rc == 0 and n == 0 and _untouched(arrs) and (st == 77).all()
    res = engine.call_regions(np.zeros((0, 3), np.float32), empty, 1)
    assert len(res.state) == 0 and len(res.region_lo) == 0 and res.region_qsum.shape == (0, 3)


def test_a_smaller_then_a_larger_call_on_the_same_ctx_leak_no_state(engine, reference):
    big, off_big, want = reference
    _assert_equal(engine.call_regions(big, off_big, 1), *want[1])
    small, off_small = _track(sizes=(3, 0, 11), seed=2)
    _assert_equal(engine.call_regions(small, off_small, 0.25), *sequence.call_regions(small, off_small, 0.25))
    larger, off_larger = _track(sizes=(700, 0, 5, 1300, 300), seed=3)                # grows every buffer
    _assert_equal(engine.call_regions(larger, off_larger, 0.25), *sequence.call_regions(larger, off_larger, 0.25))
    _assert_equal(engine.call_regions(big, off_big, 0), *want[0])
    # bins below the first offset belong to no contig: not read, and their states stay as they were
    shifted = np.concatenate([np.full((5, 3), np.inf, np.float32), big])
    res = engine.call_regions(shifted, off_big + 5, 1)
    assert (res.state[:5] == 0).all() and np.array_equal(res.state[5:], want[1][0])
    assert all(np.array_equal(getattr(res, "region_" + k), want[1][1][k]) for k in KEYS)


@pytest.mark.parametrize("strand", [None, "both"])
def test_scan_regions_is_the_scan_followed_by_the_numpy_definition(engine, strand):
    seq = synthetic.synth_windows(0, 3).reshape(-1)[:17000].copy()
    offsets = np.array([0, 14000, 17000], np.int64)
    scan, res = engine.scan_regions(seq, offsets, 2000, 0.05, strand=strand)
    plain = engine.scan_contigs(seq, offsets, 2000) if strand is None else engine.scan_contigs_strand(seq, offsets, 2000, strand)
    assert len(scan.scores) == 6 and scan.track.shape == (9, 3)
    for k in scan.FIELDS:
        x, y = getattr(scan, k), getattr(plain, k)
        assert np.array_equal(x, y, equal_nan=isinstance(x, np.ndarray) and x.dtype.kind == "f"), k
    assert np.array_equal(scan.track.view(np.uint32), plain.track.view(np.uint32))
    state, regions = sequence.call_regions(scan.track, scan.bin_offsets, 0.05)
    _assert_equal(res, state, regions)
    table = sequence.region_table(regions, offsets, 2000)
    assert res.stride == 2000 and all(np.array_equal(getattr(res, k), table[k], equal_nan=True) for k in table)
    assert res.end[res.region_contig == 1][-1] == 3000 and res.end[res.region_contig == 0][-1] == 14000
