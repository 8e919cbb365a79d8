"""Average linkage on the MI355X: every array of NNEngine.average_linkage, rounds, merged_per_round and complete equal
sequence.average_linkage bit for bit - on every fixture of tests/avglink_data.py, for every size of the LDS table (the library's, none,
8, 64 slots), with and without rows taken by single waves, and for every number of workgroups; the 4 200-leaf star takes the
accumulator in global memory at the library's own table size; rows exactly on a class border are filed by the class rule; the host and the device entry points agree; graph_count_dev ->
graph_fill_dev -> average_linkage_dev never leaves the device; the order function is exact where 64 bits are not; bad arguments leave
the outputs untouched."""
import ctypes as C

import numpy as np
import pytest

from genomad_amd import _lib, sequence
from genomad_amd._lib import GnnError
from tests import avglink_data as D
from tests import row_table_data as B
from tests.clusters_data import planted

pytestmark = pytest.mark.gpu

ARRAYS = (("a", np.int64), ("b", np.int64), ("weight", np.uint64), ("size_a", np.int64), ("size_b", np.int64), ("round", np.int64),
          ("sim", np.float64))
RECORDS = (("parent", np.int32), ("weight", np.uint64), ("size_a", np.int32), ("size_b", np.int32), ("round", np.int32))
SLOTS = (-1, 0, 8, 64)                                # -1: the library's own
WAVE_ROWS = (-1, 0)
GROUPS = (0, 1, 3)


def assert_equal(res, want, what):
    for k, dtype in ARRAYS:
        got = getattr(res, k)
        assert got.dtype == dtype and got.shape == want[k].shape and np.array_equal(got, want[k]), (what, k)
    assert res.rounds == want["rounds"] and res.complete == want["complete"], what
    assert res.merged_per_round.dtype == np.int64 and np.array_equal(res.merged_per_round, want["merged_per_round"]), what
    assert np.array_equal(res.valid, want["valid"]) and res.stop == want["stop"], what


@pytest.fixture
def knobs(engine):
    """the engine's table size, wave rows and workgroups are the library's own before and after the test"""
    slots, wave_rows = engine.set_average_linkage_slots(-1), engine.set_average_linkage_wave_rows(-1)
    engine.set_average_linkage_groups(0)
    yield engine
    engine.set_average_linkage_slots(slots)
    engine.set_average_linkage_wave_rows(wave_rows)
    engine.set_average_linkage_groups(0)


def set_knobs(engine, defaults, slots, wave_rows, groups):
    engine.set_average_linkage_slots(defaults[0] if slots < 0 else slots)
    engine.set_average_linkage_wave_rows(defaults[1] if wave_rows < 0 else wave_rows)
    engine.set_average_linkage_groups(groups)


def defaults_of(engine):
    return engine.set_average_linkage_slots(-1), engine.set_average_linkage_wave_rows(-1)


@pytest.mark.parametrize("name", D.NAMES)
def test_every_table_size_wave_rule_and_grid_equals_the_definition(knobs, name):
    engine = knobs
    csr, valid = D.cases()[name]
    want = D.reference(name)
    defaults = defaults_of(engine)
    assert defaults == (4096, 256)
    for slots in SLOTS:
        for wave_rows in WAVE_ROWS:
            for groups in GROUPS:
                set_knobs(engine, defaults, slots, wave_rows, groups)
                assert_equal(engine.average_linkage(*csr, valid), want, (name, slots, wave_rows, groups))


@pytest.mark.parametrize("name", ["sparse0", "tied1", "planted", "masked"])
def test_a_stop_and_a_round_limit(knobs, name):
    engine = knobs
    csr, valid = D.cases()[name]
    for stop, max_rounds in ((0.4, 1 << 20), (2.0 ** -24, 3), (0.25, 2), (63.9, 5)):
        want = D.reference(name, stop, max_rounds)
        for slots in (-1, 8):
            engine.set_average_linkage_slots(4096 if slots < 0 else slots)
            assert_equal(engine.average_linkage(*csr, valid, stop, max_rounds), want, (name, stop, max_rounds, slots))
    assert not D.reference(name, 2.0 ** -24, 3)["complete"] and D.reference(name, 63.9, 5)["rounds"] == 1


def test_the_star_takes_the_accumulator_at_the_librarys_own_table_size(knobs):
    engine = knobs
    want = D.reference("star", max_rounds=4)
    assert want["merged_per_round"].tolist() == [1, 1, 1, 1] and not want["complete"] and want["b"].tolist() == [1, 2, 3, 4]
    for groups in GROUPS:
        engine.set_average_linkage_groups(groups)
        assert_equal(engine.average_linkage(*D.STAR, max_rounds=4), want, ("star", groups))
        classes = engine.average_linkage_classes()
        assert classes[2] == 4 and classes[0] == 4 * D.STAR_LEAVES - 6, classes      # the hub every round; the leaves not yet absorbed


def test_a_row_on_a_class_border_is_filed_by_the_rule(knobs):
    engine = knobs
    assert defaults_of(engine) == (4096, 256)
    for degrees, slots, wave_limit, classes in B.BORDERS:
        csr, degree = B.stars(degrees)
        assert len(degree) == sum(classes) and B.histogram(degree, slots, wave_limit) == classes
        want = sequence.average_linkage(*csr, max_rounds=1)
        engine.set_average_linkage_slots(4096 if slots < 0 else slots)
        for groups in GROUPS:
            engine.set_average_linkage_groups(groups)
            assert_equal(engine.average_linkage(*csr, max_rounds=1), want, (degrees, groups))
            assert engine.average_linkage_classes().tolist() == classes, (degrees, groups)


def dev_call(engine, csr, valid, **kw):
    """average_linkage_dev on uploaded arrays: (the result, the downloaded per-node records)"""
    indptr, col, sim = (np.ascontiguousarray(x, dtype=t) for x, t in zip(csr, (np.int64, np.int32, np.float32)))
    n, nnz = len(indptr) - 1, len(col)
    ins = [indptr, col if nnz else np.zeros(1, np.int32), sim if nnz else np.zeros(1, np.float32)]
    if valid is not None:
        ins.append(np.ascontiguousarray(valid, dtype=np.uint8))
    bufs = [engine.alloc(max(a.nbytes, 8)) for a in ins] + [engine.alloc(max(np.dtype(t).itemsize * n, 8)) for _, t in RECORDS]
    try:
        for b, a in zip(bufs, ins):
            b.upload(a)
        outs = bufs[len(ins):]
        res = engine.average_linkage_dev(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, n, nnz, *(b.ptr for b in outs),
                                         valid_ptr=bufs[3].ptr if valid is not None else None, **kw)
        got = {k: b.download((n,), t) for (k, t), b in zip(RECORDS, outs)}
    finally:
        for b in bufs:
            b.free()
    return res, got


def records_of(want, n):
    """the per-node records of a definition's merge list"""
    rec = {"parent": np.full(n, -1, np.int32), "weight": np.zeros(n, np.uint64), "size_a": np.zeros(n, np.int32), "size_b": np.zeros(n, np.int32),
           "round": np.zeros(n, np.int32)}
    b = want["b"]
    rec["parent"][b] = want["a"]
    for k in ("weight", "size_a", "size_b", "round"):
        rec[k][b] = want[k]
    return rec


@pytest.mark.parametrize("name", ["sparse1", "planted", "masked", "parallel", "empty"])
def test_the_device_entry_point_agrees(knobs, name):
    csr, valid = D.cases()[name]
    want = D.reference(name)
    res, got = dev_call(knobs, csr, valid)
    assert res.a is None and res.valid is None and res.rounds == want["rounds"] and res.complete == want["complete"]
    assert np.array_equal(res.merged_per_round, want["merged_per_round"])
    for k, v in records_of(want, D.n_of(csr)).items():
        assert got[k].dtype == v.dtype and np.array_equal(got[k], v), k


def test_graph_to_average_linkage_without_leaving_the_device(knobs):
    engine = knobs
    big = planted(2048)[0]
    rows, t = np.ascontiguousarray(big), 0.5
    n = len(rows)
    host = engine.graph(rows, t)
    via_graph = host.average_linkage(engine, stop=0.6)
    direct = engine.average_linkage(host.indptr, host.col, host.sim, host.valid, stop=0.6)
    for k, _ in ARRAYS:
        assert np.array_equal(getattr(via_graph, k), getattr(direct, k)), k
    bufs = [engine.alloc(rows.nbytes), engine.alloc(8 * (n + 1))]
    try:
        bufs[0].upload(rows)
        total = engine.graph_count_dev(bufs[0].ptr, n, t, bufs[1].ptr)
        assert total == host.n_edges > 100
        bufs += [engine.alloc(4 * total), engine.alloc(4 * total)]
        outs = [engine.alloc(np.dtype(d).itemsize * n) for _, d in RECORDS]
        bufs += outs
        engine.graph_fill_dev(bufs[0].ptr, n, t, bufs[2].ptr, bufs[3].ptr, total)
        res = engine.average_linkage_dev(bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, n, total, *(b.ptr for b in outs), stop=0.6)
        got = {k: b.download((n,), d) for (k, d), b in zip(RECORDS, outs)}
    finally:
        for b in bufs:
            b.free()
    assert host.valid.all()                                      # the device call had no validity to pass on
    want = {k: getattr(direct, k) for k, _ in ARRAYS}
    for k, v in records_of(want, n).items():
        assert np.array_equal(got[k], v), k
    assert res.rounds == direct.rounds and res.complete and np.array_equal(res.merged_per_round, direct.merged_per_round)
    assert len(direct.a) > 50 and (direct.sim >= 0.6 - 2.0 ** -24).all()


def order_quads():
    """4 096 quadruples (s1, d1, s2, d2): random ones of every width, operands at 2^63 - 1, equal ratios with different terms, and
    products that differ only above bit 64 or only below it"""
    rng = np.random.default_rng(17)
    top = (1 << 63) - 1
    q = []
    for _ in range(3000):
        bits = rng.integers(1, 64, 4)
        q.append([int(rng.integers(0, 1 << 62)) >> (62 - int(b)) if b < 63 else top for b in bits])
    for _ in range(400):                                  # equal ratios: (k x, k y) against (m x, m y)
        x, y, k, m = (int(v) for v in rng.integers(1, 1 << 31, 4))
        q.append([k * x, k * y, m * x, m * y])
    for _ in range(300):                                  # s1 * d2 and s2 * d1 agree in their low 64 bits, not above
        d = int(rng.integers(1, 1 << 20))
        s = int(rng.integers(1, 1 << 40))
        q.append([s + (1 << 62), d << 2, s, d << 2])      # (s + 2^62) * 4 d = s * 4 d + 2^64 * d
    for _ in range(300):                                  # the products agree above bit 64 and differ by one below
        s = int(rng.integers(1 << 62, top))
        q.append([s, top, s - int(rng.integers(0, 2)), top - int(rng.integers(0, 2))])
    q += [[top, top, top, top], [top, 1, top - 1, 1], [top, top, top - 1, top], [top, top - 1, top, top], [0, top, 0, 1], [0, 1, 1, top],
          [1, top, 0, 5], [top, 1, top, 2]]
    while len(q) < 4096:
        q.append([int(v) for v in rng.integers(0, 1 << 63, 4)])
    return q[:4096]


def test_the_order_function_is_exact_in_128_bits(engine):
    quads = order_quads()
    want = np.array([(s1 * d2 > s2 * d1) - (s1 * d2 < s2 * d1) for s1, d1, s2, d2 in quads], dtype=np.int32)
    got = engine.average_linkage_order(np.array(quads, dtype=np.uint64))
    assert got.dtype == np.int32 and np.array_equal(got, want)
    low = np.array([((s1 * d2) & (2 ** 64 - 1) > (s2 * d1) & (2 ** 64 - 1)) - ((s1 * d2) & (2 ** 64 - 1) < (s2 * d1) & (2 ** 64 - 1))
                    for s1, d1, s2, d2 in quads], dtype=np.int32)
    assert (low != want).sum() > 500 and (want == 0).sum() >= 400 and (want == 1).sum() > 500 and (want == -1).sum() > 500


def raw(engine, csr, stop_q, valid=None, max_rounds=50, fill=0x5A):
    """gnn_avglink itself on outputs filled with a sentinel: (its status, the outputs, whether all of them still hold the sentinel)"""
    indptr, col, sim = np.asarray(csr[0], np.int64), np.asarray(csr[1], np.int32), np.asarray(csr[2], np.float32)
    n = len(indptr) - 1
    ok = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    outs = [np.full(n, fill, dtype=d) for _, d in RECORDS]
    merged, rounds, complete = np.full(max(max_rounds, 1), fill, np.int64), C.c_int64(fill), C.c_int(fill)
    rc = engine.lib.gnn_avglink(engine.ctx, indptr.ctypes.data, col.ctypes.data, sim.ctypes.data, None if ok is None else ok.ctypes.data, n,
                                len(col), stop_q, max_rounds, *(o.ctypes.data for o in outs), merged.ctypes.data, C.addressof(rounds),
                                C.addressof(complete))
    same = all((o == np.array(fill, o.dtype)).all() for o in outs) and (merged == fill).all() and rounds.value == fill and complete.value == fill
    return rc, outs, same


def test_bad_arguments_are_errors_and_leave_the_outputs_untouched(knobs):
    engine = knobs
    good = ([0, 2, 3, 3, 3], [1, 2, 3], [0.9, 0.8, 0.7])
    rc, outs, same = raw(engine, good, 1)
    assert rc == 0 and not same and outs[0].tolist() == [-1, 0, 0, 0]
    bad_graphs = {"a column beyond n": ([0, 2, 3, 3, 3], [1, 4, 3], good[2]), "a column at its row": ([0, 2, 3, 3, 3], [1, 2, 1], good[2]),
                  "a NaN": (good[0], good[1], [np.nan, 0.8, 0.7]), "a similarity of 64": (good[0], good[1], [0.9, 0.8, 64.0]),
                  "indptr that falls": ([0, 2, 1, 3, 3], good[1], good[2]), "indptr that stops short": ([0, 2, 2, 2, 2], good[1], good[2])}
    for what, g in bad_graphs.items():
        rc, _, same = raw(engine, g, 1)
        assert rc == _lib.ERR_ARG and same, what
        assert b"gnn_avglink" in engine.lib.gnn_last_error() and b"CSR" in engine.lib.gnn_last_error()
    for what, kw in (("stop_q of 0", dict(stop_q=0)), ("a negative stop_q", dict(stop_q=-5)), ("stop_q of 2^30", dict(stop_q=1 << 30)),
                     ("no round", dict(stop_q=1, max_rounds=0)), ("too many rounds", dict(stop_q=1, max_rounds=(1 << 20) + 1))):
        rc, _, same = raw(engine, good, **kw)
        assert rc == _lib.ERR_ARG and same, what
    assert engine.lib.gnn_avglink(None, None, None, None, None, 4, 3, 0, 10, *([None] * 8)) == _lib.ERR_ARG      # before the ctx
    with pytest.raises(GnnError, match="error -1"):
        engine.average_linkage([0, 1, 1], [2], [0.5])
    for kw in (dict(stop=0.0), dict(stop=64.0), dict(stop=-1.0), dict(stop=float("nan")), dict(max_rounds=0), dict(max_rounds=1.5)):
        with pytest.raises(ValueError):
            engine.average_linkage(*good, **kw)
    for bad in (-2, 4097):
        with pytest.raises(GnnError):
            engine.set_average_linkage_slots(bad)
        with pytest.raises(GnnError):
            engine.set_average_linkage_wave_rows(bad)
