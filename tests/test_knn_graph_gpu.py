"""The k-nearest-neighbour graph on the MI355X: every array of ``NNEngine.knn_graph`` against the numpy definition
(``sequence.knn_graph``) over the device's own neighbour lists - exactly, dtype included -, end to end on integer rows whose lists
numpy computes too, a hub row whose segment passes both class limits (and, with the limits lowered, rows of a few hundred entries that
do), independence of the neighbour search's split, of the entry point and of how large the workspaces have grown, the fill's guards
with sentinels behind every output, the consumers on the result, and the similarity's bits against ``NNEngine.graph``."""
import ctypes as C

import numpy as np
import pytest

from genomad_amd import _lib, sequence
from genomad_amd._lib import GnnError, check
from genomad_amd.engine import GraphResult, KNNGraphResult

pytestmark = pytest.mark.gpu

MODES, WEIGHTS, KS = sequence.KNN_GRAPH_MODES, sequence.KNN_GRAPH_WEIGHTS, (1, 2, 15, 63, 64)
ARRAYS = (("indptr", np.int64), ("col", np.int32), ("sim", np.float32), ("mutual", np.uint8), ("valid", bool))
SENTINEL = 0x5A


def mixed_rows(n=1500, seed=12):
    """mixed-sign rows; a zero row, a NaN row, an Inf row; duplicates, one of them scaled"""
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, 512)).astype(np.float32)
    if n > 1000:
        rows[[3, 700, n - 1]] = 0
        rows[64, 7] = np.nan
        rows[999, 500] = -np.inf
        rows[[17, 640, 1300]] = rows[5]
        rows[1001] = 2 * rows[8]
    return rows


def integer_rows(n=200, seed=4):
    """small signed integers in sixteen columns: every dot is exact on the device, with many ties; a zero row is valid under dot"""
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 512), dtype=np.float32)
    rows[:, :16] = rng.integers(-2, 3, (n, 16))
    rows[9] = 0
    return rows


def hub_rows(n, centre=0, seed=2):
    """c + e_i r_i around the centre row c, e_i in [.5, .6]: cos(i, c) = 1 / sqrt(1 + e_i^2) >= .857, cos(i, j) is about the product of
    the two: at k = 1 every row lists the centre"""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal(512)
    c /= np.linalg.norm(c)
    r = rng.standard_normal((n, 512))
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    rows = c + rng.uniform(.5, .6, (n, 1)) * r
    rows[centre] = c
    return rows.astype(np.float32)


def arrays_of(res):
    return {k: getattr(res, k) for k, _ in ARRAYS}


def assert_same(got, want):
    """every array, dtype included, bit for bit"""
    for k, dtype in ARRAYS:
        assert got[k].dtype == dtype == want[k].dtype and got[k].shape == want[k].shape, k
        same = np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)) if k == "sim" else np.array_equal(got[k], want[k])
        assert same, k


def defined(engine, rows, k, mode, weight, metric="cosine", lists=None):
    """the definition over the device's own neighbour lists"""
    lists = engine.neighbours(rows, None, k, metric) if lists is None else lists
    return sequence.knn_graph(rows, k, mode, weight, metric, neighbours=lists)


@pytest.fixture(scope="module")
def mixed(engine):
    """the 1 500 rows and the device's lists for every k, computed once"""
    engine.set_neighbour_split(0)
    rows = mixed_rows()
    return rows, {k: engine.neighbours(rows, None, k) for k in KS}


@pytest.fixture(autouse=True)
def default_knobs(engine):
    yield
    engine.set_neighbour_split(0)
    engine.set_knn_graph_wave_rows(64)
    engine.set_knn_graph_group_rows(2048)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("weight", WEIGHTS)
@pytest.mark.parametrize("mode", MODES)
def test_every_array_equals_the_definition_over_the_devices_lists(engine, mixed, mode, weight, k):
    rows, lists = mixed
    res = engine.knn_graph(rows, k, mode, weight)
    assert isinstance(res, KNNGraphResult) and isinstance(res, GraphResult)
    assert (res.k, res.mode, res.weight, res.metric, res.n, res.n_edges) == (k, mode, weight, "cosine", 1500, len(res.col))
    assert_same(arrays_of(res), defined(engine, rows, k, mode, weight, lists=lists[k]))
    assert 0 < res.n_edges <= res.valid.sum() * k and res.valid.sum() == 1495
    a, b, _ = res.edges()
    assert (a < b).all() and res.valid[a].all() and res.valid[b].all()
    if weight == "jaccard":
        assert ((res.sim > 0) & (res.sim <= 1)).all()
    if mode == "mutual":
        assert (res.mutual == 1).all() and (res.degree() <= k).all()
    else:
        assert (res.degree()[res.valid] >= k).all()


@pytest.mark.parametrize("weight", WEIGHTS)
@pytest.mark.parametrize("mode", MODES)
def test_padded_lists_no_rows_one_row_and_invalid_rows_alone(engine, mode, weight):
    rows = mixed_rows(5, seed=3)
    res = engine.knn_graph(rows, 64, mode, weight)                       # n = 5 at k = 64: the lists are padded, every pair is mutual
    assert_same(arrays_of(res), defined(engine, rows, 64, mode, weight))
    assert res.n_edges == 10 and (res.mutual == 1).all()
    for r in (rows[:0], rows[:1], np.zeros((70, 512), np.float32), np.full((3, 512), np.nan, np.float32)):
        res = engine.knn_graph(r, 7, mode, weight)
        assert_same(arrays_of(res), sequence.knn_graph(r, 7, mode, weight))
        assert res.n_edges == 0 and res.indptr.tolist() == [0] * (len(r) + 1) and res.valid.sum() == (len(r) == 1)


@pytest.mark.parametrize("k", (1, 5, 64))
def test_integer_rows_under_dot_equal_the_definition_with_numpys_own_lists(engine, k):
    rows = integer_rows()
    idx, sim = sequence.nearest_neighbours(rows, None, k, "dot")
    got = engine.neighbours(rows, None, k, "dot")
    assert np.array_equal(got[0], idx) and np.array_equal(got[1].view(np.uint32), sim.view(np.uint32))       # exact values, ties included
    for mode in MODES:
        for weight in WEIGHTS:
            res = engine.knn_graph(rows, k, mode, weight, "dot")
            assert_same(arrays_of(res), sequence.knn_graph(rows, k, mode, weight, "dot"))
            assert res.valid.all() and res.metric == "dot"


# ---- the hub: a segment of unbounded length -----------------------------------------------------------------------------------------------

KNOBS = ((64, 2048), (8, 64), (1, 2), (64, 4096))


def test_the_hub_row_passes_both_class_limits_and_no_bit_depends_on_them(engine):
    n = 2304                                                             # the centre's segment: 2 303 entries, beyond the 2 048 of the LDS class
    rows = hub_rows(n)
    unit = rows.astype(np.float64) / np.linalg.norm(rows.astype(np.float64), axis=1, keepdims=True)
    s = unit @ unit.T
    np.fill_diagonal(s, -2)
    assert (s[1:].argmax(axis=1) == 0).all()                            # on the CPU: every row's nearest row is the centre
    lists = engine.neighbours(rows, None, 1)
    want = {(m, w): sequence.knn_graph(rows, 1, m, w, neighbours=lists) for m in MODES for w in WEIGHTS}
    assert np.diff(want[("union", "similarity")]["indptr"])[0] == n - 1  # and by the definition the centre's in-degree is n - 1
    classes = {}
    for wave, group in KNOBS:
        engine.set_knn_graph_wave_rows(wave)
        engine.set_knn_graph_group_rows(group)
        for (m, w), ref in want.items():
            assert_same(arrays_of(engine.knn_graph(rows, 1, m, w)), ref)
        classes[(wave, group)] = engine.knn_graph_classes().tolist()     # of the last call: mutual, where the centre keeps one edge
        engine.knn_graph(rows, 1, "union", "jaccard")
        classes[(wave, group)] += engine.knn_graph_classes().tolist()
    assert classes[(64, 2048)] == [0, 0, 0, 1] and classes[(64, 4096)] == [0, 0, 1, 0] and classes[(8, 64)] == [0, 0, 0, 1]


@pytest.mark.parametrize("centre", (0, 150))
def test_a_few_hundred_entries_cross_the_lowered_limits(engine, centre):
    """k = 6 around a hub in the middle: the hub's segment (the rows behind it), segments of the family's size and short ones"""
    rows = hub_rows(300, centre, seed=8)
    lists = engine.neighbours(rows, None, 6)
    for m in MODES:
        for w in WEIGHTS:
            ref = sequence.knn_graph(rows, 6, m, w, neighbours=lists)
            found = []
            for wave, group in KNOBS:
                engine.set_knn_graph_wave_rows(wave)
                engine.set_knn_graph_group_rows(group)
                assert_same(arrays_of(engine.knn_graph(rows, 6, m, w)), ref)
                found.append(engine.knn_graph_classes().tolist())
            if m == "union":
                longest = int(np.diff(ref["indptr"]).max())
                beyond = int((np.diff(ref["indptr"]) > 64).sum())       # the hub, and whoever else the family lists that often
                assert longest >= 299 - centre and found[0] == [beyond, 0] and found[1][1] == beyond >= 1 and found[3] == found[0]
                assert found[2] == [int((np.diff(ref["indptr"]) == 2).sum()), int((np.diff(ref["indptr"]) > 2).sum())] and found[2][1] > 100


def test_the_limits_on_the_mixed_rows(engine, mixed):
    rows, lists = mixed
    for m, w in (("union", "jaccard"), ("mutual", "similarity")):
        ref = sequence.knn_graph(rows, 15, m, w, neighbours=lists[15])
        for wave, group in KNOBS[1:3]:
            engine.set_knn_graph_wave_rows(wave)
            engine.set_knn_graph_group_rows(group)
            assert_same(arrays_of(engine.knn_graph(rows, 15, m, w)), ref)
            assert engine.knn_graph_classes().sum() > 100


def test_knobs_outside_their_ranges_are_refused(engine):
    for value in (0, 65, -1):
        with pytest.raises(GnnError, match=rf"gnn_debug_knn_graph_wave_rows: {value} entries is outside \[1, 64\]"):
            engine.set_knn_graph_wave_rows(value)
    for value in (0, 4097):
        with pytest.raises(GnnError, match=rf"gnn_debug_knn_graph_group_rows: {value} entries is outside \[1, 4096\]"):
            engine.set_knn_graph_group_rows(value)


# ---- splits, entry points, grown workspaces -------------------------------------------------------------------------------------------

class Outputs:
    """rows, indptr, col, sim and mutual on the device; the three edge arrays of ``cap`` elements, every byte the sentinel"""

    def __init__(self, engine, r, cap):
        self.engine, self.n, self.cap = engine, len(r), cap
        self.bufs = [engine.alloc(max(r.nbytes, 4)), engine.alloc(8 * (len(r) + 1)), engine.alloc(4 * cap), engine.alloc(4 * cap), engine.alloc(cap)]
        self.rows, self.indptr, self.col, self.sim, self.mutual = self.bufs
        if len(r):
            self.rows.upload(r)
        self.reset()

    def reset(self):
        self.col.upload(np.full(4 * self.cap, SENTINEL, np.uint8))
        self.sim.upload(np.full(4 * self.cap, SENTINEL, np.uint8))
        self.mutual.upload(np.full(self.cap, SENTINEL, np.uint8))

    def count(self, **kw):
        return self.engine.knn_graph_count_dev(self.rows.ptr, self.n, self.indptr.ptr, **kw)

    def fill(self, capacity, **kw):
        self.engine.knn_graph_fill_dev(self.n, self.col.ptr, self.sim.ptr, self.mutual.ptr, capacity, **kw)
        self.engine.sync()
        return self.download()

    def download(self):
        return {"indptr": self.indptr.download((self.n + 1,), np.int64), "col": self.col.download((self.cap,), np.int32),
                "sim": self.sim.download((self.cap,), np.float32), "mutual": self.mutual.download((self.cap,), np.uint8)}

    def free(self):
        for buf in self.bufs:
            buf.free()


def untouched(out, total):
    """nothing behind the last edge was written"""
    return all((out[k][total:].view(np.uint8) == SENTINEL).all() for k in ("col", "sim", "mutual"))


def test_three_splits_both_entry_points_and_a_grown_workspace_give_the_same_bits(engine, mixed):
    rows, lists = mixed
    small = rows[:333]
    kw = dict(k=15, mode="union", weight="jaccard")
    first = arrays_of(engine.knn_graph(small, **kw))
    assert_same(first, defined(engine, small, 15, "union", "jaccard"))
    for split in (32, 100, 4096):
        engine.set_neighbour_split(split)
        assert_same(arrays_of(engine.knn_graph(small, **kw)), first)
    engine.set_neighbour_split(0)
    total = len(first["col"])
    out = Outputs(engine, small, total + 64)
    try:
        assert out.count(**kw) == total
        got = out.fill(total, **kw)                                      # exact capacity: the sentinels behind every array stand
        assert untouched(got, total)
        assert_same(dict({k: got[k][:total] if k != "indptr" else got[k] for k in got}, valid=first["valid"]), first)
        out.reset()
        got = out.fill(total + 64, **kw)                                 # the count still stands: a second fill gives the same bits
        assert untouched(got, total) and np.array_equal(got["col"][:total], first["col"])
        # a larger call grows every workspace; the same call again is what it was, from both entry points
        assert engine.knn_graph(rows, 64, "union", "similarity").n_edges > total
        assert_same(arrays_of(engine.knn_graph(small, **kw)), first)
        out.reset()
        assert out.count(**kw) == total
        got = out.fill(total + 64, **kw)
        assert untouched(got, total)
        assert_same(dict({k: got[k][:total] if k != "indptr" else got[k] for k in got}, valid=first["valid"]), first)
    finally:
        out.free()


def test_the_fills_guards(engine, mixed):
    rows, _ = mixed
    small = rows[:333]
    kw = dict(k=7, mode="union", weight="similarity")
    want = arrays_of(engine.knn_graph(small, **kw))
    total = len(want["col"])
    out = Outputs(engine, small, total + 64)
    try:
        assert out.count(**kw) == total
        with pytest.raises(GnnError, match=rf"error -1: gnn_knn_graph_fill_dev: capacity {total - 1} is below the {total} edges the count found"):
            out.fill(total - 1, **kw)
        for other in (dict(kw, k=8), dict(kw, mode="mutual"), dict(kw, weight="jaccard"), dict(kw, metric="dot")):
            with pytest.raises(GnnError, match=r"error -3: gnn_knn_graph_fill_dev: no gnn_knn_graph_count\* of the same \(n, k, mode, weight, metric\)"):
                out.fill(total + 64, **other)
        with pytest.raises(GnnError, match=r"error -3: gnn_knn_graph_fill: no gnn_knn_graph_count of the same"):      # the host fill wants a host count
            check(engine.lib.gnn_knn_graph_fill(engine.ctx, 333, 7, 0, 0, 0, None, None, None, total))
        engine.sync()
        assert untouched(out.download(), 0)                              # the refused fills wrote nothing
        got = out.fill(total, **kw)
        assert untouched(got, total) and np.array_equal(got["col"][:total], want["col"]) and np.array_equal(got["mutual"][:total], want["mutual"])
        assert np.array_equal(got["sim"][:total].view(np.uint32), want["sim"].view(np.uint32))
        assert out.count(**dict(kw, mode="mutual")) < total              # another count: the old arguments no longer fill
        with pytest.raises(GnnError, match="error -3: gnn_knn_graph_fill_dev"):
            out.fill(total + 64, **kw)
        # mutual may be NULL; a total of 0 needs no output at all
        engine.knn_graph_fill_dev(333, out.col.ptr, out.sim.ptr, None, total + 64, **dict(kw, mode="mutual"))
        engine.sync()
        zero = Outputs(engine, np.zeros((40, 512), np.float32), 1)
        try:
            assert zero.count(**kw) == 0
            engine.knn_graph_fill_dev(40, None, None, None, 0, **kw)
            assert zero.indptr.download((41,), np.int64).tolist() == [0] * 41
        finally:
            zero.free()
    finally:
        out.free()


def test_argument_errors_carry_the_value_and_the_range_before_the_ctx_is_looked_at(engine):
    lib, total = engine.lib, C.c_int64(0)
    for args, said in (((None, None, -1, 3, 0, 0, 0, None, None), r"-1 rows is outside \[0, 2\^31\)"),
                       ((None, None, 4, 0, 0, 0, 0, None, None), r"k 0 is outside \[1, 64\]"),
                       ((None, None, 4, 65, 0, 0, 0, None, None), r"k 65 is outside \[1, 64\]"),
                       ((None, None, 4, 3, 2, 0, 0, None, None), r"mode 2 is outside \[0, 1\]"),
                       ((None, None, 4, 3, 0, -1, 0, None, None), r"weight -1 is outside \[0, 1\]"),
                       ((None, None, 4, 3, 0, 0, 2, None, None), r"metric 2 is outside \[0, 1\]")):
        for fn in ("gnn_knn_graph_count", "gnn_knn_graph_count_dev"):
            assert getattr(lib, fn)(*args) == _lib.ERR_ARG
            with pytest.raises(GnnError, match=f"{fn}: {said}"):
                check(getattr(lib, fn)(*args))
    assert lib.gnn_knn_graph_count(engine.ctx, None, 4, 3, 0, 0, 0, None, C.addressof(total)) == _lib.ERR_ARG      # rows and indptr are required
    rows = mixed_rows(8, seed=1)
    for k in (0, 65):
        with pytest.raises(ValueError, match=rf"k {k} is outside \[1, 64\]"):
            engine.knn_graph(rows, k)
    with pytest.raises(ValueError, match="mode 'both' is outside"):
        engine.knn_graph(rows, 3, mode="both")
    with pytest.raises(ValueError, match="weight 'snn' is outside"):
        engine.knn_graph(rows, 3, weight="snn")
    with pytest.raises(ValueError, match="metric 'l2'"):
        engine.knn_graph(rows, 3, metric="l2")


# ---- the consumers, and the similarity's bits -----------------------------------------------------------------------------------------------

def family_rows(n=240, families=6, seed=6):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((families, 512))
    rows = centres[np.arange(n) % families] + 1.5 * rng.standard_normal((n, 512))
    rows[7] = 0
    return rows.astype(np.float32)


@pytest.mark.parametrize("mode,weight", (("mutual", "jaccard"), ("union", "similarity")))
def test_communities_and_mcl_of_the_result_equal_the_definitions_on_the_same_csr(engine, mode, weight):
    rows = family_rows()
    g = engine.knn_graph(rows, 10, mode, weight)
    comm = g.communities(engine)
    want = sequence.modularity_communities(g.indptr, g.col, g.sim, g.valid)
    assert np.array_equal(comm.label, want["label"]) and np.array_equal(comm.size, want["size"]) and comm.levels == want["levels"]
    mcl = g.mcl(engine)
    want = sequence.markov_clusters(g.indptr, g.col, g.sim, g.valid)
    assert np.array_equal(mcl.label, want["label"]) and np.array_equal(mcl.size, want["size"]) and mcl.iterations == want["iterations"]
    assert len(g.average_linkage(engine).a) > 0 and len(g.label_components(engine, comm.label)) == len(rows)
    label = np.where(np.arange(len(rows)) < 6, np.arange(len(rows)), -1)
    assert g.spread(engine, label, 6).best.shape == (len(rows),)
    assert len(g.symmetric()[1]) == 2 * g.n_edges and (g.components()[g.valid] >= 0).all() and len(g.table()) == g.n_edges


def test_where_j_is_in_the_list_of_i_the_similarity_has_the_bits_of_the_graphs_value(engine):
    rows = mixed_rows(300, seed=13)
    full = engine.graph(rows, -1.0)                                      # every pair of valid rows
    a, b, s = full.edges()
    graph = dict(zip(zip(a.tolist(), b.tolist()), s.view(np.uint32).tolist()))
    for k in (3, 64):
        idx, _ = engine.neighbours(rows, None, k)
        g = engine.knn_graph(rows, k)
        ga, gb, gs = g.edges()
        listed = np.array([j in idx[i] for i, j in zip(ga.tolist(), gb.tolist())])
        assert listed.sum() > len(ga) // 4 and (g.mutual[~listed] == 0).all()
        assert all(graph[(i, j)] == bits for i, j, bits in zip(ga[listed].tolist(), gb[listed].tolist(), gs[listed].view(np.uint32).tolist()))


def test_the_pass_times_are_filed_under_profiling(engine):
    rows = mixed_rows(200, seed=2)
    check(engine.lib.gnn_profile_enable(engine.ctx, 1))
    try:
        engine.knn_graph(rows, 5)
        ms = engine.knn_graph_pass_ms()
        assert ms.shape == (7,) and (ms >= 0).all()                      # [search, lists, count, scan] and the fill's [fill, order, finish]
    finally:
        check(engine.lib.gnn_profile_enable(engine.ctx, 0))
    engine.knn_graph(rows, 5)
    assert engine.knn_graph_pass_ms().shape == (0,)
