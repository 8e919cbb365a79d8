"""Modularity communities on the MI355X: every array of NNEngine.communities - label, size, level_label, the per-level counters and
both words of qnum - equals sequence.modularity_communities bit for bit: on the three weight kinds at r = 16, 64, 160 and 256, the
searched inputs with a rejected sweep and with a split community, invalid and empty rows, parallel entries, the big-hub star, one
level and one sweep, rows exactly on a class border; for every size of the LDS table, with and without rows taken by single waves, and for every number of
workgroups; the host and the device entry points agree; graph_count_dev -> graph_fill_dev -> communities_dev never leaves the
device; gnn_label_components equals its definition; the gain and score arithmetic is exact in 128 bits at the stated bounds; bad
arguments leave the outputs untouched."""
import ctypes as C

import numpy as np
import pytest

from genomad_amd import _lib, sequence
from genomad_amd._lib import GnnError
from tests import communities_data as D
from tests import row_table_data as B
from tests.clusters_data import planted

pytestmark = pytest.mark.gpu

ROW_ARRAYS = (("label", np.int64), ("size", np.int64), ("level_label", np.int64))
SLOTS = (0, 64, 4096)
WAVE_ROWS = (0, 16, 256)
GROUPS = (1, 3, 0)                                    # 0: the library's own
R_NAMES = {16: 0.25, 64: 1.0, 160: 2.5, 256: 4.0}


def words_of(qnum):
    return np.array([[q & (2 ** 64 - 1), (q >> 64) & (2 ** 64 - 1)] for q in qnum], dtype=np.uint64).reshape(-1, 2)


def assert_equal(res, want, what, rows=True):
    if rows:
        for k, dtype in ROW_ARRAYS:
            got = getattr(res, k)
            assert got.dtype == dtype and got.shape == want[k].shape and np.array_equal(got, want[k]), (what, k)
        assert np.array_equal(res.valid, want["valid"]), what
    for k in sequence.COMM_LEVEL_FIELDS:
        got = getattr(res, k)
        assert got.dtype == np.int64 and np.array_equal(got, want[k]), (what, k, got, want[k])
    assert res.qnum == want["qnum"] and np.array_equal(res.qnum_words, words_of(want["qnum"])), (what, res.qnum, want["qnum"])
    assert (res.levels, res.complete, res.m2, res.resolution) == (want["levels"], want["complete"], want["m2"], want["resolution"]), what
    assert res.modularity == want["modularity"], what


@pytest.fixture
def knobs(engine):
    """the engine's table size, wave rows and workgroups are the library's own before and after the test"""
    slots, wave_rows = engine.set_communities_slots(-1), engine.set_communities_wave_rows(-1)
    engine.set_communities_groups(0)
    yield engine
    engine.set_communities_slots(slots)
    engine.set_communities_wave_rows(wave_rows)
    engine.set_communities_groups(0)


@pytest.mark.parametrize("name", D.RANDOM_NAMES)
def test_the_three_weight_kinds_at_four_resolutions(knobs, name):
    csr, valid = D.cases()[name]
    for resolution in D.RESOLUTIONS:
        assert_equal(knobs.communities(*csr, valid, resolution), D.reference(name, resolution), (name, resolution))
    sweep_knobs(knobs, csr, valid, 2.5, D.reference(name, 2.5), name)


def sweep_knobs(engine, csr, valid, resolution, want, name):
    """every table size, wave rule and grid: each row class is forced on small rows"""
    assert (engine.set_communities_slots(-1), engine.set_communities_wave_rows(-1)) == (4096, 256)
    for slots in SLOTS:
        for wave_rows in WAVE_ROWS:
            for groups in GROUPS:
                engine.set_communities_slots(slots)
                engine.set_communities_wave_rows(wave_rows)
                engine.set_communities_groups(groups)
                assert_equal(engine.communities(*csr, valid, resolution), want, (name, slots, wave_rows, groups))


@pytest.mark.parametrize("name", [n for n in D.NAMES if n not in D.RANDOM_NAMES])
def test_every_table_size_wave_rule_and_grid_equals_the_definition(knobs, name):
    engine = knobs
    csr, valid = D.cases()[name]
    resolution = {"rejected": D.REJECTED["resolution"], "split": D.SPLIT["resolution"]}.get(name, 1.0)
    sweep_knobs(engine, csr, valid, resolution, D.reference(name, resolution), name)


def test_the_searched_inputs_reach_the_rare_paths():
    assert D.reference("rejected", D.REJECTED["resolution"])["rejected"].any()
    assert D.reference("split", D.SPLIT["resolution"])["split"].any()


def test_a_row_on_a_class_border_is_filed_by_the_rule(knobs):
    engine = knobs
    assert (engine.set_communities_slots(-1), engine.set_communities_wave_rows(-1)) == (4096, 256)
    for degrees, slots, wave_limit, classes in B.BORDERS:
        csr, degree = B.stars(degrees)
        assert len(degree) == sum(classes) and B.histogram(degree, slots, wave_limit) == classes
        want = sequence.modularity_communities(*csr, max_levels=1, max_sweeps=1)
        engine.set_communities_slots(4096 if slots < 0 else slots)
        for groups in GROUPS:
            engine.set_communities_groups(groups)
            assert_equal(engine.communities(*csr, max_levels=1, max_sweeps=1), want, (degrees, groups))
            assert engine.communities_classes()[:3].tolist() == classes, (degrees, groups)


def test_the_star_takes_the_accumulator_at_the_librarys_own_table_size(knobs):
    engine = knobs
    want = D.reference("star")
    assert want["levels"] == 2 and want["accepted"].tolist() == [2, 0] and want["nodes"].tolist() == [D.STAR_LEAVES + 1, D.STAR_LEAVES // 2]
    for groups in GROUPS:
        engine.set_communities_groups(groups)
        assert_equal(engine.communities(*D.STAR), want, ("star", groups))
        classes = engine.communities_classes()
        # the hub in each of level 0's three sweeps, and its component in the contraction; at level 1 the workgroup takes it
        assert classes[2] == 3 and classes[5] == 1 and classes[1] == 1 and classes[0] == 3 * D.STAR_LEAVES + D.STAR_LEAVES // 2 - 1, classes
    want = D.reference("bare_star")
    assert want["levels"] == 1 and want["rejected"].tolist() == [1]
    assert_equal(engine.communities(*D.BARE_STAR), want, "bare star")


@pytest.mark.parametrize("name", ["unit1", "random0", "rejected", "masked"])
def test_a_level_limit_and_a_sweep_limit(knobs, name):
    engine = knobs
    csr, valid = D.cases()[name]
    for max_levels, max_sweeps in ((1, 1 << 20), (32, 1), (2, 2)):
        want = D.reference(name, 2.5, max_levels, max_sweeps)
        for slots in (4096, 64):
            engine.set_communities_slots(slots)
            assert_equal(engine.communities(*csr, valid, 2.5, max_levels, max_sweeps), want, (name, max_levels, max_sweeps, slots))
    assert not D.reference(name, 2.5, 1, 1 << 20)["complete"] and not D.reference(name, 2.5, 32, 1)["complete"]


def dev_call(engine, csr, valid, max_levels=32, **kw):
    """communities_dev on uploaded arrays: (the result, the downloaded label, size and level_label)"""
    indptr, col, sim = (np.ascontiguousarray(x, dtype=t) for x, t in zip(csr, (np.int64, np.int32, np.float32)))
    n, nnz = len(indptr) - 1, len(col)
    ins = [indptr, col if nnz else np.zeros(1, np.int32), sim if nnz else np.zeros(1, np.float32)]
    if valid is not None:
        ins.append(np.ascontiguousarray(valid, dtype=np.uint8))
    shapes = ((n,), (n,), (max_levels, n))
    bufs = [engine.alloc(max(a.nbytes, 8)) for a in ins] + [engine.alloc(max(8 * int(np.prod(s)), 8)) for s in shapes]
    try:
        for b, a in zip(bufs, ins):
            b.upload(a)
        outs = bufs[len(ins):]
        res = engine.communities_dev(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, n, nnz, *(b.ptr for b in outs),
                                     valid_ptr=bufs[3].ptr if valid is not None else None, max_levels=max_levels, **kw)
        got = {k: b.download(s, np.int64) for (k, _), s, b in zip(ROW_ARRAYS, shapes, outs)}
    finally:
        for b in bufs:
            b.free()
    got["level_label"] = got["level_label"][:res.levels]
    return res, got


@pytest.mark.parametrize("name", ["quarter1", "split", "planted", "masked", "parallel", "empty"])
def test_the_device_entry_point_agrees(knobs, name):
    csr, valid = D.cases()[name]
    want = D.reference(name, 2.5)
    res, got = dev_call(knobs, csr, valid, resolution=2.5)
    assert res.label is None and res.valid is None
    assert_equal(res, want, name, rows=False)
    for k, _ in ROW_ARRAYS:
        assert np.array_equal(got[k], want[k]), k


def test_graph_to_communities_without_leaving_the_device(knobs):
    engine = knobs
    rows, t = np.ascontiguousarray(planted(2048)[0]), 0.5
    n = len(rows)
    host = engine.graph(rows, t)
    via_graph = host.communities(engine)
    direct = engine.communities(host.indptr, host.col, host.sim, host.valid)
    want = sequence.modularity_communities(host.indptr, host.col, host.sim, host.valid)
    assert_equal(direct, want, "direct")
    assert_equal(via_graph, want, "via the graph")
    bufs = [engine.alloc(rows.nbytes), engine.alloc(8 * (n + 1))]
    try:
        bufs[0].upload(rows)
        total = engine.graph_count_dev(bufs[0].ptr, n, t, bufs[1].ptr)
        assert total == host.n_edges > 100
        bufs += [engine.alloc(4 * total), engine.alloc(4 * total)]
        outs = [engine.alloc(8 * n), engine.alloc(8 * n), engine.alloc(8 * n * 32)]
        bufs += outs
        engine.graph_fill_dev(bufs[0].ptr, n, t, bufs[2].ptr, bufs[3].ptr, total)
        res = engine.communities_dev(bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, n, total, *(b.ptr for b in outs))
        label, size = outs[0].download((n,), np.int64), outs[1].download((n,), np.int64)
        levels = outs[2].download((32, n), np.int64)[:res.levels]
    finally:
        for b in bufs:
            b.free()
    assert host.valid.all()                                      # the device call had no validity to pass on
    assert_equal(res, want, "on the device", rows=False)
    assert np.array_equal(label, want["label"]) and np.array_equal(size, want["size"]) and np.array_equal(levels, want["level_label"])
    assert direct.n_communities == len(direct.table()) > 5 and direct.levels >= 2 and np.array_equal(direct.at_level(-1), direct.label)


def crafted_labellings():
    """(csr, valid, label): a path of 12 whose label 0 sits on three separate stretches, labels that no entry joins, -1 and an
    invalid row in the middle of a stretch"""
    path = D.path(12)
    yield path, None, np.array([0, 0, 1, 1, 0, 0, 0, 2, -1, 0, 0, 5])
    yield path, np.arange(12) != 5, np.array([0, 0, 1, 1, 0, 0, 0, 2, -1, 0, 0, 5])
    csr, valid = D.cases()["masked"]
    n = D.n_of(csr)
    yield csr, valid, np.arange(n) % 3
    yield csr, valid, np.where(np.arange(n) % 7 == 0, -1, np.arange(n) // 50)
    yield D.PARALLEL, None, np.zeros(7, dtype=np.int64)
    yield D.STAR, None, np.arange(D.STAR_LEAVES + 1) % 2
    for name in ("grid", "rejected"):
        csr, valid = D.cases()[name]
        yield csr, valid, D.reference(name)["label"]


def test_label_components_equals_its_definition(knobs):
    engine = knobs
    for k, (csr, valid, label) in enumerate(crafted_labellings()):
        want = sequence.label_components(*csr, label, valid)
        got = engine.label_components(*csr, label, valid)
        assert got.dtype == np.int64 and np.array_equal(got, want), k
        if k == 0:
            assert want.tolist() == [0, 0, 2, 2, 4, 4, 4, 7, -1, 9, 9, 11]      # label 0 has three components
    csr, valid, label = next(crafted_labellings())
    indptr, col, sim = (np.ascontiguousarray(x, dtype=t) for x, t in zip(csr, (np.int64, np.int32, np.float32)))
    ins = [indptr, col, sim, np.ascontiguousarray(label, dtype=np.int64)]
    bufs = [engine.alloc(a.nbytes) for a in ins] + [engine.alloc(8 * 12)]
    try:
        for b, a in zip(bufs, ins):
            b.upload(a)
        engine.label_components_dev(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, 12, len(col), bufs[3].ptr, bufs[4].ptr)
        assert np.array_equal(bufs[4].download((12,), np.int64), sequence.label_components(*csr, label))
    finally:
        for b in bufs:
            b.free()
    graph = engine.graph(np.ascontiguousarray(planted(300)[0]), 0.5)
    label = np.arange(300) % 4
    assert np.array_equal(graph.label_components(engine, label), sequence.label_components(graph.indptr, graph.col, graph.sim, label, graph.valid))


def gain_operands():
    """4 096 rows (64 M2, r, k, w_ic, w_ia, tot_c, tot_a, in, sq low, sq high, prev low, prev high): random ones of every width up to
    the bounds - M2 < 2^58, r <= 256, every weight and total <= M2, sq <= M2^2 - and the corners"""
    rng = np.random.default_rng(23)
    top = (1 << 58) - 1
    wide = lambda hi: int(rng.integers(0, 1 << 62)) % (hi + 1) >> int(rng.integers(0, 58))
    rows = []
    for _ in range(4000):
        m2 = max(1, wide(top))
        r = int(rng.integers(1, 257))
        k = wide(m2)
        inner, sq = wide(m2), (wide(m2) * wide(m2)) if rng.random() < 0.7 else m2 * m2
        prev = 64 * m2 * wide(m2) - r * wide(m2) * wide(m2)
        if rng.random() < 0.2:
            prev = 64 * m2 * inner - r * sq + int(rng.integers(-1, 2))      # next to the new score
        rows.append([64 * m2, r, k, wide(m2), wide(m2), wide(m2), wide(m2), inner, sq, prev])
    for m2, r in ((top, 256), (top, 1), (1, 256), (top, 64)):
        for k, wc, wa, tc, ta in ((m2, m2, 0, m2, 0), (m2, 0, m2, m2, 0), (m2, 0, m2, 0, m2), (m2, m2, 0, 0, m2), (1, 0, 0, 0, 1), (0, 0, 0, 0, 0)):
            for inner, sq, prev in ((m2, m2 * m2, 0), (0, m2 * m2, -r * m2 * m2), (m2, 0, 64 * m2 * m2), (m2, 0, 64 * m2 * m2 - 1),
                                    (0, m2 * m2, -r * m2 * m2 - 1)):
                rows.append([64 * m2, r, k, wc, wa, tc, ta, inner, sq, prev])
    rows = rows[:4096]
    mask = 2 ** 64 - 1
    ops = np.array([row[:8] + [row[8] & mask, row[8] >> 64, row[9] & mask, (row[9] >> 64) & mask] for row in rows], dtype=np.uint64)
    return rows, ops


def test_the_gain_and_the_score_are_exact_in_128_bits(engine):
    rows, ops = gain_operands()
    mask = 2 ** 64 - 1
    want = []
    for m64, r, k, wc, wa, tc, ta, inner, sq, prev in rows:
        d = m64 * (wc - wa) - r * k * (tc + k - ta)
        q = m64 * inner - r * sq
        assert abs(d) < 2 ** 127 and abs(q) < 2 ** 127
        want.append([d & mask, (d >> 64) & mask, q & mask, (q >> 64) & mask, int(q > prev)])
    want = np.array(want, dtype=np.uint64)
    got = engine.communities_gain(ops)
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    negative = want[:, 1] >> np.uint64(63)
    assert negative.sum() > 500 and (1 - negative).sum() > 500 and (want[:, 1] & np.uint64(mask >> 1)).astype(bool).sum() > 1000
    assert want[:, 4].sum() > 500 and (1 - want[:, 4]).sum() > 500


def raw(engine, csr, r, valid=None, max_levels=4, max_sweeps=50, fill=0x5A):
    """gnn_communities itself on outputs filled with a sentinel: (its status, the outputs, whether all of them still hold it)"""
    indptr, col, sim = np.asarray(csr[0], np.int64), np.asarray(csr[1], np.int32), np.asarray(csr[2], np.float32)
    n = len(indptr) - 1
    ok = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    levels_cap = max(min(max_levels, 32), 1)
    outs = [np.full(n, fill, np.int64), np.full(n, fill, np.int64), np.full((levels_cap, n), fill, np.int64), np.full((levels_cap, 7), fill, np.int64),
            np.full((levels_cap, 2), fill, np.uint64)]
    levels, complete, m2 = C.c_int64(fill), C.c_int(fill), C.c_uint64(fill)
    rc = engine.lib.gnn_communities(engine.ctx, indptr.ctypes.data, col.ctypes.data, sim.ctypes.data, None if ok is None else ok.ctypes.data, n,
                                    len(col), r, max_levels, max_sweeps, *(o.ctypes.data for o in outs), C.addressof(levels),
                                    C.addressof(complete), C.addressof(m2))
    same = all((o == np.array(fill, o.dtype)).all() for o in outs) and levels.value == fill and complete.value == fill and m2.value == fill
    return rc, outs, same


def test_bad_arguments_are_errors_and_leave_the_outputs_untouched(knobs):
    engine = knobs
    good = ([0, 2, 3, 3, 3], [1, 2, 3], [0.9, 0.8, 0.7])
    rc, outs, same = raw(engine, good, 64)
    assert rc == 0 and not same and outs[0].tolist() == sequence.modularity_communities(*(np.asarray(x) for x in good))["label"].tolist()
    bad_graphs = {"a column beyond n": ([0, 2, 3, 3, 3], [1, 4, 3], good[2]), "a column at its row": ([0, 2, 3, 3, 3], [1, 2, 1], good[2]),
                  "a NaN": (good[0], good[1], [np.nan, 0.8, 0.7]), "a similarity of 64": (good[0], good[1], [0.9, 0.8, 64.0]),
                  "indptr that falls": ([0, 2, 1, 3, 3], good[1], good[2]), "indptr that stops short": ([0, 2, 2, 2, 2], good[1], good[2])}
    for what, g in bad_graphs.items():
        rc, _, same = raw(engine, g, 64)
        assert rc == _lib.ERR_ARG and same, what
        assert b"gnn_communities" in engine.lib.gnn_last_error() and b"CSR" in engine.lib.gnn_last_error()
    for what, kw in (("r of 0", dict(r=0)), ("r of 257", dict(r=257)), ("a negative r", dict(r=-64)), ("no level", dict(r=64, max_levels=0)),
                     ("too many levels", dict(r=64, max_levels=33)), ("no sweep", dict(r=64, max_sweeps=0)),
                     ("too many sweeps", dict(r=64, max_sweeps=(1 << 20) + 1))):
        rc, _, same = raw(engine, good, **kw)
        assert rc == _lib.ERR_ARG and same, what
    assert engine.lib.gnn_communities(None, None, None, None, None, 4, 3, 0, 1, 1, *([None] * 8)) == _lib.ERR_ARG      # before the ctx
    with pytest.raises(GnnError, match="error -1"):
        engine.communities([0, 1, 1], [2], [0.5])
    with pytest.raises(GnnError, match="error -1"):
        engine.label_components([0, 1, 1], [2], [0.5], [0, 0])
    for kw in (dict(resolution=0.0), dict(resolution=4.5), dict(resolution=0.01), dict(resolution=float("nan")), dict(max_levels=0),
               dict(max_levels=33), dict(max_sweeps=0), dict(max_sweeps=1.5)):
        with pytest.raises(ValueError):
            engine.communities(*good, **kw)
    with pytest.raises(ValueError):
        engine.label_components(*good, [0, 0, -2, 0])
    for bad in (-2, 4097):
        with pytest.raises(GnnError):
            engine.set_communities_slots(bad)
        with pytest.raises(GnnError):
            engine.set_communities_wave_rows(bad)
