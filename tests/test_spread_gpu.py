"""Label spreading on the MI355X: every output array, iterations, converged and changed of NNEngine.spread equal sequence.label_spread
bit for bit - on every fixture of tests/spread_data.py, narrow and wide class counts (1, 3, 63, 64, 65, 1024), clamped and free seeds,
the smallest, the middle and the largest alpha, every number of workgroups, the dirty-row rule on and off, shuffled and relabelled
graphs, the host and the device entry points -; the 70 000-leaf star fills the 64-bit headroom exactly; graph_count_dev ->
graph_fill_dev -> spread_dev never leaves the device; bad arguments leave the outputs untouched."""
import ctypes as C
import functools

import numpy as np
import pytest

from genomad_amd import _lib, sequence
from genomad_amd._lib import GnnError
from tests import mcl_data as M, spread_data as D
from tests.clusters_data import planted

pytestmark = pytest.mark.gpu

ARRAYS = (("score", np.uint32), ("best", np.int32), ("best_score", np.uint32), ("second_score", np.uint32), ("total", np.uint64),
          ("first", np.int32))
# (clamp, alpha, max_iter): the iterations are capped so that the definition stays cheap; some of these converge, most are cut short
KNOBS = ((True, 0.5, 60), (False, 0.5, 60), (True, 63 / 64, 25), (False, 63 / 64, 25), (True, 1 / 64, 30), (False, 1 / 64, 30))
GRIDS = ((0, True), (1, True), (3, False), (0, False))          # (workgroups, the dirty-row rule)
NAMES = sorted(D.cases(1))
WIDE = ("parallel", "planted", "random_masked", "star_over")


@functools.lru_cache(maxsize=None)
def reference(name, n_classes, clamp, alpha, max_iter):
    """(graph, valid, label, the definition's answer), computed once"""
    csr, valid, label = D.cases(n_classes)[name]
    return csr, valid, label, sequence.label_spread(*csr, label, n_classes, valid, alpha, clamp, max_iter)


def assert_equal(res, want, what, scores=True):
    for k, dtype in ARRAYS[0 if scores else 1:]:
        got = getattr(res, k)
        assert got.dtype == dtype and got.shape == want[k].shape and np.array_equal(got, want[k]), (what, k)
    assert res.iterations == want["iterations"] and res.converged == want["converged"], what
    assert res.changed.dtype == np.int64 and np.array_equal(res.changed, want["changed"]), what
    assert np.array_equal(res.seed, want["seed"]), what


@pytest.fixture
def knobs(engine):
    """the engine's workgroups and its dirty-row rule are the library's own before and after the test"""
    engine.set_spread_groups(0)
    engine.set_spread_skip(True)
    yield engine
    engine.set_spread_groups(0)
    engine.set_spread_skip(True)


def sweep(engine, name, n_classes, knob_list, grids=GRIDS):
    for clamp, alpha, max_iter in knob_list:
        csr, valid, label, want = reference(name, n_classes, clamp, alpha, max_iter)
        for groups, skip in grids:
            engine.set_spread_groups(groups)
            engine.set_spread_skip(skip)
            res = engine.spread(*csr, label, n_classes, valid, alpha, clamp, max_iter)
            assert_equal(res, want, (name, n_classes, clamp, alpha, groups, skip))


@pytest.mark.parametrize("n_classes", [1, 3])
@pytest.mark.parametrize("name", NAMES)
def test_narrow_rows_equal_the_definition_for_every_knob_grid_and_rule(knobs, name, n_classes):
    sweep(knobs, name, n_classes, KNOBS)


@pytest.mark.parametrize("n_classes", [63, 64, 65])
@pytest.mark.parametrize("name", WIDE)
def test_wide_rows_equal_the_definition(knobs, name, n_classes):
    sweep(knobs, name, n_classes, (KNOBS[0], KNOBS[3]))


def test_1024_classes_on_the_random_graph(knobs):
    sweep(knobs, "random", 1024, ((True, 0.5, 12),), GRIDS[:3])


def test_a_run_to_convergence_and_one_cut_short(knobs):
    engine = knobs
    csr, valid, label = D.cases(3)["random"]
    want = sequence.label_spread(*csr, label, 3, valid, 0.5, True, 1000)
    assert want["converged"] and want["iterations"] > 5
    for skip in (True, False):
        engine.set_spread_skip(skip)
        assert_equal(engine.spread(*csr, label, 3, valid, 0.5, True, 1000), want, ("converged", skip))
        for k in (1, 2, 3, want["iterations"] - 1):
            cut = sequence.label_spread(*csr, label, 3, valid, 0.5, True, k)
            res = engine.spread(*csr, label, 3, valid, 0.5, True, k)
            assert not res.converged and res.iterations == k
            assert_equal(res, cut, ("cut", k, skip))
    print(f"\nrandom, 3 classes: {want['iterations']} iterations, changed {want['changed'].tolist()}")


@pytest.mark.parametrize("name", ["planted", "random_masked", "fan"])
def test_shuffled_rows_and_relabelled_nodes(knobs, name):
    engine = knobs
    csr, valid, label, want = reference(name, 3, False, 0.5, 60)
    assert_equal(engine.spread(*M.shuffled_rows(csr), label, 3, valid, 0.5, False, 60), want, "shuffled")
    n = D.n_of(csr)
    perm = np.random.default_rng(11).permutation(n)
    lab2, val2 = np.empty_like(label), None if valid is None else np.empty_like(valid)
    lab2[perm] = label
    if valid is not None:
        val2[perm] = valid
    res = engine.spread(*M.relabelled(csr, perm), lab2, 3, val2, 0.5, False, 60)
    for k, _ in ARRAYS:
        assert np.array_equal(getattr(res, k)[perm], want[k]), k
    assert res.iterations == want["iterations"] and np.array_equal(res.changed, want["changed"])


def test_the_70000_leaf_star_exactly(knobs):
    engine = knobs
    label = D.star_labels(D.STAR_LEAVES, 3)
    for clamp, alpha in ((True, 63 / 64), (False, 0.5)):
        want = sequence.label_spread(*D.STAR, label, 3, None, alpha, clamp, 8)
        for groups, skip in GRIDS[:3]:
            engine.set_spread_groups(groups)
            engine.set_spread_skip(skip)
            assert_equal(engine.spread(*D.STAR, label, 3, None, alpha, clamp, 8), want, ("star", clamp, groups, skip))
    p = (1 << 31) // D.STAR_LEAVES
    want = sequence.label_spread(*D.STAR, label, 3, None, 63 / 64, True, 8)
    assert D.STAR_LEAVES * p << 30 > 1 << 60 and want["score"][0, 2] == (63 * ((D.STAR_LEAVES * p << 30) >> 31)) >> 6 and want["best"][0] == 2


def dev_call(engine, csr, valid, label, n_classes, want_scores=True, **kw):
    """spread_dev on uploaded arrays: (the result, the downloaded arrays)"""
    indptr, col, sim = (np.ascontiguousarray(x, dtype=t) for x, t in zip(csr, (np.int64, np.int32, np.float32)))
    n, nnz = len(indptr) - 1, len(col)
    ins = [indptr, col if nnz else np.zeros(1, np.int32), sim if nnz else np.zeros(1, np.float32), np.ascontiguousarray(label, dtype=np.int64)]
    if valid is not None:
        ins.append(np.ascontiguousarray(valid, dtype=np.uint8))
    sizes = [4 * n * n_classes, 4 * n, 4 * n, 4 * n, 8 * n, 4 * n]
    bufs = [engine.alloc(max(a.nbytes, 8)) for a in ins] + [engine.alloc(max(s, 8)) for s in sizes]
    try:
        for b, a in zip(bufs, ins):
            b.upload(a)
        outs = bufs[len(ins):]
        res = engine.spread_dev(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, n, nnz, n_classes, *(b.ptr for b in outs[1:]),
                                score_ptr=outs[0].ptr if want_scores else None, valid_ptr=bufs[4].ptr if valid is not None else None, **kw)
        shapes = [(n, n_classes)] + [(n,)] * 5
        got = {k: b.download(s, dtype) for (k, dtype), b, s in zip(ARRAYS, outs, shapes)}
    finally:
        for b in bufs:
            b.free()
    return res, got


@pytest.mark.parametrize("name,n_classes", [("planted", 3), ("random_masked", 65), ("parallel", 1), ("star_over", 3)])
def test_the_device_entry_point_agrees(knobs, name, n_classes):
    clamp, alpha, max_iter = KNOBS[1]
    csr, valid, label, want = reference(name, n_classes, clamp, alpha, max_iter)
    res, got = dev_call(knobs, csr, valid, label, n_classes, alpha=alpha, clamp=clamp, max_iter=max_iter)
    assert res.score is None and res.best is None and res.iterations == want["iterations"] and res.converged == want["converged"]
    assert np.array_equal(res.changed, want["changed"])
    for k, _ in ARRAYS:
        assert np.array_equal(got[k], want[k]), k


def test_without_the_score_matrix_nothing_is_copied_there(knobs):
    engine = knobs
    csr, valid, label, want = reference("random_masked", 3, True, 0.5, 60)
    res = engine.spread(*csr, label, 3, valid, 0.5, True, 60, scores=False)
    assert res.score is None
    assert_equal(res, want, "no scores", scores=False)
    # the raw call with a NULL score pointer: the poisoned matrix it was not given stays as it is, the other outputs are the same
    rc, outs, _ = raw(engine, csr, label, 3, 32, valid=valid, score=False)
    assert rc == 0 and (outs[0] == 0x5A).all()
    for (k, _), o in zip(ARRAYS[1:], outs[1:]):
        assert np.array_equal(o, want[k]), k
    _, got = dev_call(engine, csr, valid, label, 3, want_scores=False, alpha=0.5, clamp=True, max_iter=60)
    for k, _ in ARRAYS[1:]:
        assert np.array_equal(got[k], want[k]), k


def raw(engine, csr, label, n_classes, a, valid=None, max_iter=60, score=True, fill=0x5A):
    """gnn_spread itself on outputs filled with a sentinel: (its status, the outputs, whether all of them still hold the sentinel)"""
    indptr, col, sim = np.asarray(csr[0], np.int64), np.asarray(csr[1], np.int32), np.asarray(csr[2], np.float32)
    n = len(indptr) - 1
    label = np.asarray(label, np.int64)
    ok = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    outs = [np.full(s, fill, dtype=d) for s, d in (((n, n_classes), np.uint32), (n, np.int32), (n, np.uint32), (n, np.uint32), (n, np.uint64),
                                                   (n, np.int32))]
    changed, iterations, converged = np.full(max(max_iter, 1), fill, np.int64), C.c_int64(fill), C.c_int(fill)
    rc = engine.lib.gnn_spread(engine.ctx, indptr.ctypes.data, col.ctypes.data, sim.ctypes.data, None if ok is None else ok.ctypes.data,
                               label.ctypes.data, n, len(col), n_classes, a, 1, max_iter, outs[0].ctypes.data if score else None,
                               *(o.ctypes.data for o in outs[1:]), changed.ctypes.data, C.addressof(iterations), C.addressof(converged))
    same = all((o == np.array(fill, o.dtype)).all() for o in outs) and (changed == fill).all() and iterations.value == fill and converged.value == fill
    return rc, outs, same


def test_bad_arguments_are_errors_and_leave_the_outputs_untouched(knobs):
    engine = knobs
    good = ([0, 2, 3, 3, 3], [1, 2, 3], [0.9, 0.8, 0.7])
    label = [0, -1, -1, 1]
    rc, outs, same = raw(engine, good, label, 2, 32)
    assert rc == 0 and not same
    bad_graphs = {"a column beyond n": ([0, 2, 3, 3, 3], [1, 4, 3], good[2]), "a column at its row": ([0, 2, 3, 3, 3], [1, 2, 1], good[2]),
                  "a NaN": (good[0], good[1], [np.nan, 0.8, 0.7]), "a similarity of 64": (good[0], good[1], [0.9, 0.8, 64.0]),
                  "indptr that falls": ([0, 2, 1, 3, 3], good[1], good[2]), "indptr that stops short": ([0, 2, 2, 2, 2], good[1], good[2])}
    for what, g in bad_graphs.items():
        rc, _, same = raw(engine, g, label, 2, 32)
        assert rc == _lib.ERR_ARG and same, what
        assert b"gnn_spread" in engine.lib.gnn_last_error() and b"CSR" in engine.lib.gnn_last_error()
    for what, lab in (("a label of n_classes", [0, 2, -1, 1]), ("a label below -1", [0, -2, -1, 1])):
        rc, _, same = raw(engine, good, lab, 2, 32)
        assert rc == _lib.ERR_ARG and same, what
        assert b"label" in engine.lib.gnn_last_error()
    for what, kw in (("alpha of 0", dict(a=0)), ("alpha of 64", dict(a=64)), ("no iteration", dict(a=32, max_iter=0)),
                     ("too many iterations", dict(a=32, max_iter=10001))):
        rc, _, same = raw(engine, good, label, 2, **kw)
        assert rc == _lib.ERR_ARG and same, what
    for nc in (0, 1025):
        rc, _, same = raw(engine, good, label, nc, 32)
        assert rc == _lib.ERR_ARG and same, nc
    assert engine.lib.gnn_spread(None, None, None, None, None, None, 4, 3, 0, 32, 1, 10, *([None] * 9)) == _lib.ERR_ARG      # before the ctx
    with pytest.raises(GnnError, match="error -1"):
        engine.spread([0, 1, 1], [2], [0.5], [0, -1], 1)
    for kw in (dict(alpha=0.3), dict(alpha=1.0), dict(max_iter=0), dict(n_classes=1025)):
        with pytest.raises(ValueError):
            engine.spread(*good, **{"label": label, "n_classes": 2, **kw})
    with pytest.raises(ValueError, match="label is outside"):
        engine.spread(*good, [0, 2, -1, 1], 2)


def test_no_rows_no_seeds_and_rows_without_entries(knobs):
    engine = knobs
    res = engine.spread([0], [], [], np.zeros(0, np.int64), 2)
    assert res.iterations == 1 and res.converged and res.changed.tolist() == [0] and res.score.shape == (0, 2) and len(res.best) == 0
    csr, valid, label = D.cases(3)["planted"]
    none = np.full(len(label), -1)
    res = engine.spread(*csr, none, 3)
    assert_equal(res, sequence.label_spread(*csr, none, 3), "no seeds")
    assert res.iterations == 1 and res.converged and not res.score.any() and (res.best == -1).all() and (res.first == -1).all()
    empty = (np.zeros(5, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))
    lab, val = np.array([1, -1, 0, 1]), np.array([True, True, False, True])
    for clamp in (True, False):
        res = engine.spread(*empty, lab, 2, val, 0.25, clamp)
        assert_equal(res, sequence.label_spread(*empty, lab, 2, val, 0.25, clamp), ("isolated", clamp))
        assert res.best.tolist() == [1, -1, -1, 1] and res.iterations == 2 and res.converged


def test_graph_to_spread_without_leaving_the_device(knobs):
    engine = knobs
    rows, t = np.ascontiguousarray(planted()[0][:300]), 0.8
    n = len(rows)
    label = D.scattered_labels(n, 4, every=6, seed=2)
    host = engine.graph(rows, t)
    via_graph = host.spread(engine, label, 4, alpha=0.75)
    want = sequence.label_spread(host.indptr, host.col, host.sim, label, 4, host.valid, 0.75)
    assert_equal(via_graph, want, "host graph")
    bufs = [engine.alloc(rows.nbytes), engine.alloc(8 * (n + 1)), engine.alloc(8 * n)]
    try:
        bufs[0].upload(rows)
        bufs[2].upload(label)
        total = engine.graph_count_dev(bufs[0].ptr, n, t, bufs[1].ptr)
        assert total == host.n_edges > 100
        bufs += [engine.alloc(4 * total), engine.alloc(4 * total)]
        outs = [engine.alloc(s) for s in (4 * n * 4, 4 * n, 4 * n, 4 * n, 8 * n, 4 * n)]
        bufs += outs
        engine.graph_fill_dev(bufs[0].ptr, n, t, bufs[3].ptr, bufs[4].ptr, total)
        res = engine.spread_dev(bufs[1].ptr, bufs[3].ptr, bufs[4].ptr, bufs[2].ptr, n, total, 4, *(b.ptr for b in outs[1:]), score_ptr=outs[0].ptr,
                                alpha=0.75)
        got = {k: b.download(s, dtype) for (k, dtype), b, s in zip(ARRAYS, outs, [(n, 4)] + [(n,)] * 5)}
    finally:
        for b in bufs:
            b.free()
    assert host.valid.all()                                      # the device call had no validity to pass on
    for k, _ in ARRAYS:
        assert np.array_equal(got[k], want[k]), k
    assert res.iterations == want["iterations"] and res.converged == want["converged"] and np.array_equal(res.changed, want["changed"])
    assert (want["best"] >= 0).sum() > (label >= 0).sum()        # labels reached rows that had none


def test_one_hop_at_a_large_alpha_names_the_votes_winner(knobs):
    """Where every row without a label touches seeds only, two iterations under ``clamp`` give it F[c] = (a * ((sum over its seed
    neighbours of class c of p_ij * 2^30) >> 31)) >> 6 with p_ij = (q_ij << 31) // d_i - a non-decreasing function of Q_c = the sum of
    the q of class c.  The vote's weight of class c is the sum of rint(s * 2^32) over the same neighbours, and for a float32 s in
    [0.5, 2) both s * 2^24 and s * 2^32 are integers: weight_c = 256 * Q_c exactly.  So the class the vote names has the largest Q, and
    with it the largest score: score[i][vote's label] == best_score[i].  (``best`` itself can be a smaller class that the floors tied.)"""
    engine = knobs
    rows, t = np.ascontiguousarray(planted()[0][:300]), 0.8
    g = engine.graph(rows, t)
    label = D.scattered_labels(len(rows), 3, every=2, seed=4)
    a, b = sequence.graph_edges(g.indptr, g.col)
    keep = (label[a] >= 0) | (label[b] >= 0)                     # an entry between two rows without a label goes
    indptr = np.concatenate([[0], np.cumsum(np.bincount(a[keep], minlength=len(rows)))]).astype(np.int64)
    res = engine.spread(indptr, g.col[keep], g.sim[keep], label, 3, g.valid, 63 / 64, True, 2)
    seeds, others = np.flatnonzero(label >= 0), np.flatnonzero(label < 0)
    vote = engine.vote(rows[others], rows[seeds], label[seeds], 3, t)
    voted = vote.predict("weight")[0]
    assert (g.sim[keep] >= 0.5).all() and (voted >= 0).sum() > 10
    for k, i in enumerate(others):
        if voted[k] >= 0:
            assert res.score[i, voted[k]] == res.best_score[i] > 0, i
        else:
            assert res.best[i] == -1, i
