"""Markov clustering on the MI355X: every output array, iterations, converged, changed and the final matrix of NNEngine.mcl equal
sequence.markov_clusters bit for bit - on the planted cliques (with a selection number that cuts the largest), the equal-weight clique
(ties in the selection), the path, the random graph (supports reach n), invalid rows and weights <= 0, and a column whose support is
exactly the LDS table's capacity and one above it -, for every table size (the default, 64 slots, none: all overflow) and every number of
workgroups; graph_count_dev -> graph_fill_dev -> mcl_dev never leaves the device and agrees; a bad graph leaves the outputs untouched."""
import ctypes as C
import functools

import numpy as np
import pytest

from genomad_amd import _lib, sequence
from genomad_amd._lib import GnnError
from genomad_amd.engine import NNEngine
from tests import mcl_data as D
from tests.clusters_data import planted

pytestmark = pytest.mark.gpu

ARRAYS = (("label", np.int64), ("size", np.int64), ("attractor", np.int64), ("flow", np.uint32), ("is_attractor", np.bool_))


def _masked():
    """the planted graph with four invalid rows - one in the 100-clique, a bridge's end, a singleton, one of the triple - and every
    17th weight zero or negative"""
    indptr, col, sim = D.PLANTED
    sim = sim.copy()
    sim[::17] = 0.0
    sim[5::34] = -0.4
    valid = np.ones(D.PLANTED_N, dtype=bool)
    valid[[0, 130, 217, 220]] = False
    return (indptr, col, sim), valid


def _fan(extra):
    """the fan whose column 0 is summed over exactly the table's 4096 slots (+ extra) in the first iteration"""
    g = D.fan(63, [64 + extra] + [64] * 62)
    assert g[3] == 4096 + extra
    return g[:3]


CASES = {f"planted-{infl}-{sel}": (lambda: D.PLANTED, None, dict(inflation=infl, select=sel))
         for infl in (1.25, 1.5, 2.0, 4.0) for sel in (256, 64)}
CASES.update({f"planted-iter{k}": (lambda: D.PLANTED, None, dict(inflation=2.0, select=64, max_iter=k)) for k in (0, 1, 2, 3)})
CASES.update({
    "clique-256": (lambda: D.CLIQUE, None, dict(select=256)),
    "clique-64": (lambda: D.CLIQUE, None, dict(select=64)),
    "path-1.5": (lambda: D.PATH, None, dict(inflation=1.5)),
    "path-2": (lambda: D.PATH, None, dict(inflation=2.0)),
    "random-2": (lambda: D.RANDOM, None, dict(inflation=2.0, select=1024)),
    "random-3": (lambda: D.RANDOM, None, dict(inflation=3.0, select=100, precision=1 << 20)),
    "masked": (lambda: _masked()[0], lambda: _masked()[1], dict(inflation=2.0)),
    "shuffled": (lambda: D.shuffled_rows(D.PLANTED), None, dict(inflation=1.5, select=64)),
    "fan-at-capacity": (lambda: _fan(0), None, dict(max_iter=2)),
    "fan-above-capacity": (lambda: _fan(1), None, dict(max_iter=2)),
})


@functools.lru_cache(maxsize=None)
def case(name):
    """(graph, valid, knobs, the definition's answer), computed once"""
    graph, valid, kw = CASES[name]
    graph, valid = graph(), None if valid is None else valid()
    return graph, valid, kw, sequence.markov_clusters(*graph, valid, **kw)


def assert_equal(res, want, what):
    for k, dtype in ARRAYS:
        got = getattr(res, k)
        assert got.dtype == dtype and np.array_equal(got, want[k]), (what, k)
    assert res.iterations == want["iterations"] and res.converged == want["converged"], what
    assert res.changed.dtype == np.int64 and np.array_equal(res.changed, want["changed"]), what
    length, idx, val = res.matrix()
    assert length.dtype == np.int64 and idx.dtype == np.int32 and val.dtype == np.uint32
    assert np.array_equal(length, want["length"]) and np.array_equal(idx, want["idx"]) and np.array_equal(val, want["val"]), what


@pytest.fixture
def knobs(engine):
    """the engine's table size and workgroups are the library's own before and after the test"""
    before = engine.set_mcl_lds(-1)
    engine.set_mcl_groups(0)
    yield engine
    engine.set_mcl_lds(before)
    engine.set_mcl_groups(0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_output_equals_the_definition_for_every_table_size_and_grid(knobs, name):
    engine = knobs
    graph, valid, kw, want = case(name)
    capacity = engine.set_mcl_lds(-1)
    assert capacity == 4096
    for slots, groups in ((capacity, 0), (64, 0), (0, 0), (capacity, 1), (capacity, 3), (64, 3)):
        engine.set_mcl_lds(slots)
        engine.set_mcl_groups(groups)
        res = engine.mcl(*graph, valid, **kw)
        assert_equal(res, want, (name, slots, groups))
        over = engine.mcl_overflow()
        assert len(over) == res.iterations + 1
        if slots == 0:                                  # every column that is not empty took the overflow path, in every pass
            assert over[0] == (len(graph[0]) - 1 if valid is None else int(valid.sum()))
    print(f"\n{name}: {want['iterations']} iterations, {len(np.unique(want['label'][want['label'] >= 0]))} clusters")


def test_the_quoted_clusters_come_out_on_the_device(knobs):
    res = knobs.mcl(*D.PLANTED, inflation=2.0)
    assert res.n_clusters == 8 and D.partition(res.label) == D.partition(D.PLANTED_TRUTH) and res.iterations == 16 and res.converged
    table = res.table()
    assert [c["size"] for c in table] == [5, 12, 30, 70, 100, 3, 1, 1] and all(c["attractors"] for c in table)


def test_a_column_at_the_capacity_stays_in_lds_and_one_above_it_overflows(knobs):
    engine = knobs
    for extra in (0, 1):
        res = engine.mcl(*_fan(extra), max_iter=1)
        over = engine.mcl_overflow()
        print(f"\nsupport {4096 + extra}: overflow columns per pass {over.tolist()}")
        assert res.iterations == 1 and over.tolist() == [0, extra]


def test_graph_to_clusters_without_leaving_the_device(knobs):
    engine = knobs
    rows, t = np.ascontiguousarray(planted()[0][:300]), 0.8
    n = len(rows)
    host = engine.graph(rows, t)
    via_graph = host.mcl(engine, inflation=2.0)
    bufs = [engine.alloc(rows.nbytes), engine.alloc(8 * (n + 1))]
    try:
        bufs[0].upload(rows)
        total = engine.graph_count_dev(bufs[0].ptr, n, t, bufs[1].ptr)
        assert total == host.n_edges > 100
        bufs += [engine.alloc(4 * total), engine.alloc(4 * total)] + [engine.alloc(8 * n) for _ in range(3)] + [engine.alloc(4 * n), engine.alloc(n)]
        engine.graph_fill_dev(bufs[0].ptr, n, t, bufs[2].ptr, bufs[3].ptr, total)
        res = engine.mcl_dev(bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, n, total, *(b.ptr for b in bufs[4:]), inflation=2.0)
        got = {k: b.download((n,), np.uint8 if k == "is_attractor" else dtype).astype(dtype) for (k, dtype), b in zip(ARRAYS, bufs[4:])}
        matrix = res.matrix()
    finally:
        for b in bufs:
            b.free()
    indptr, col, _ = sequence.threshold_graph(rows, t)
    assert np.array_equal(indptr, host.indptr) and np.array_equal(col, host.col)
    want = sequence.markov_clusters(indptr, col, host.sim, host.valid, inflation=2.0)
    for k, _ in ARRAYS:
        assert np.array_equal(got[k], want[k]) and np.array_equal(getattr(via_graph, k), want[k]), k
    assert res.label is None and res.iterations == via_graph.iterations == want["iterations"] and res.converged == want["converged"]
    assert np.array_equal(res.changed, want["changed"]) and np.array_equal(via_graph.changed, want["changed"])
    assert all(np.array_equal(a, want[k]) for a, k in zip(matrix, ("length", "idx", "val")))
    assert via_graph.n_clusters < 300                    # the planted families are found


def _raw(engine, indptr, col, sim, fill=0x5A):
    """gnn_mcl itself on outputs filled with a sentinel: (its status, the outputs untouched)"""
    n = len(indptr) - 1
    indptr, col, sim = np.asarray(indptr, np.int64), np.asarray(col, np.int32), np.asarray(sim, np.float32)
    outs = [np.full(n, fill, dtype=d) for d in (np.int64, np.int64, np.int64, np.uint32, np.uint8)]
    changed, iterations, converged = np.full(100, fill, np.int64), C.c_int64(fill), C.c_int(fill)
    rc = engine.lib.gnn_mcl(engine.ctx, indptr.ctypes.data, col.ctypes.data, sim.ctypes.data, None, n, len(col), 8, 256, 10000, 100,
                            *(o.ctypes.data for o in outs), changed.ctypes.data, C.addressof(iterations), C.addressof(converged))
    same = all((o == fill).all() for o in outs) and (changed == fill).all() and iterations.value == fill and converged.value == fill
    return rc, same


def test_a_graph_that_is_none_is_an_error_and_leaves_the_outputs_untouched(knobs):
    engine = knobs
    good = ([0, 2, 3, 3, 3], [1, 2, 3], [0.9, 0.8, 0.7])
    assert _raw(engine, *good)[0] == 0
    bad = {"a column beyond n": ([0, 2, 3, 3, 3], [1, 4, 3], good[2]), "a column at its row": ([0, 2, 3, 3, 3], [1, 2, 1], good[2]),
           "a column below its row": ([0, 0, 3, 3, 3], [0, 2, 3], good[2]), "a negative column": ([0, 2, 3, 3, 3], [-1, 2, 3], good[2]),
           "an infinite similarity": (good[0], good[1], [0.9, np.inf, 0.7]), "a NaN": (good[0], good[1], [np.nan, 0.8, 0.7]),
           "a similarity of 64": (good[0], good[1], [0.9, 0.8, 64.0]), "indptr that falls": ([0, 2, 1, 3, 3], good[1], good[2]),
           "indptr that stops short": ([0, 2, 2, 2, 2], good[1], good[2]), "indptr that starts late": ([1, 2, 3, 3, 3], good[1], good[2])}
    for what, g in bad.items():
        rc, same = _raw(engine, *g)
        assert rc == _lib.ERR_ARG and same, what
        assert b"gnn_mcl" in engine.lib.gnn_last_error()
    with pytest.raises(GnnError, match="error -1"):
        engine.mcl([0, 1, 1], [2], [0.5])
    for kw in (dict(inflation=1.3), dict(inflation=1.0), dict(select=0), dict(select=1025), dict(precision=0), dict(max_iter=10001)):
        with pytest.raises(ValueError):
            engine.mcl(*good, **kw)
    # the library's own range checks come before the ctx is looked at
    for args in ((4, 256, 10000, 100), (33, 256, 10000, 100), (8, 0, 10000, 100), (8, 1025, 10000, 100), (8, 256, 0, 100),
                 (8, 256, (1 << 20) + 1, 100), (8, 256, 10000, -1), (8, 256, 10000, 10001)):
        assert engine.lib.gnn_mcl(None, None, None, None, None, 4, 3, *args, None, None, None, None, None, None, None, None) == _lib.ERR_ARG


def test_the_matrix_belongs_to_the_last_call(knobs):
    engine = knobs
    with NNEngine(0) as fresh:                           # an engine that never clustered
        out = np.zeros(4, np.int32)
        rc = fresh.lib.gnn_mcl_matrix(fresh.ctx, 4, 256, out.ctypes.data, out.ctypes.data, out.ctypes.data)
        assert rc == _lib.ERR_STATE
    first = engine.mcl(*D.PATH)
    second = engine.mcl(*D.CLIQUE)
    with pytest.raises(GnnError):
        first.matrix()
    assert second.matrix()[0].sum() == len(second.matrix()[1])
    assert engine.lib.gnn_mcl_matrix(engine.ctx, 99, 256, None, None, None) == _lib.ERR_STATE       # another n
    assert engine.lib.gnn_mcl_matrix(engine.ctx, 100, 64, None, None, None) == _lib.ERR_STATE       # another select
    rc, _ = _raw(engine, [0, 1, 1], [2], [0.5])          # a call that fails leaves no matrix behind
    assert rc == _lib.ERR_ARG and engine.lib.gnn_mcl_matrix(engine.ctx, 2, 256, None, None, None) == _lib.ERR_STATE


def test_no_rows_and_rows_without_edges(knobs):
    engine = knobs
    res = engine.mcl([0], [], [])
    assert res.iterations == 1 and res.converged and res.changed.tolist() == [0] and len(res.label) == 0 and res.matrix()[0].shape == (0,)
    res = engine.mcl([0, 0, 0, 0], [], [], valid=[True, False, True])
    want = sequence.markov_clusters([0, 0, 0, 0], np.zeros(0, np.int32), np.zeros(0, np.float32), np.array([True, False, True]))
    assert_equal(res, want, "isolated")
    assert res.label.tolist() == [0, -1, 2] and res.flow.tolist() == [1 << 30, 0, 1 << 30] and res.is_attractor.tolist() == [True, False, True]
