"""The exact t-SNE layout on the MI355X: ``NNEngine.tsne_forces`` and ``NNEngine.tsne`` against the numpy definition
(``sequence.tsne_forces``, ``sequence.tsne_layout``) bit for bit - at sizes around the granule of 256 columns, with invalid rows,
coincident points, points 10^3 apart, parallel entries, dropped entries and a hub row that a workgroup attracts -, for every split of
the columns, for the host and the device entry points and after the workspace grew; ``GraphResult.tsne`` on the device's own
k-nearest-neighbour graph; and the errors, which leave every output as it was."""
import ctypes as C

import numpy as np
import pytest

from genomad_amd import sequence
from genomad_amd._lib import GnnError, check
from genomad_amd.engine import TSNEResult

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 255, 256, 257, 700)
SPLITS = (1, 2, 3, 7)
FORCES = ("zi", "rx", "ry", "ax", "ay")
SENTINEL = 0x5A


def graph_case(n, seed=0):
    """(indptr, col, sim, valid, y): about six entries per row in any order, some of them parallel, some with a similarity <= 0 (they
    do not exist); row 0 a hub with an entry to every other row (more than 256 from n = 258 on: a workgroup's row); invalid rows;
    two coincident points, and a few points 10^3 away from the rest"""
    rng = np.random.default_rng(1000 + n + seed)
    cols, sims = [], []
    for i in range(n):
        c = rng.integers(i + 1, n, size=min(6, 2 * (n - 1 - i))) if i < n - 1 else np.zeros(0, dtype=np.int64)
        if i == 0:
            c = np.concatenate([np.arange(1, n), c])
        s = rng.uniform(0.05, 1.0, size=len(c))
        s[rng.random(len(c)) < 0.1] = -0.25
        s[rng.random(len(c)) < 0.05] = 0.0
        cols.append(c)
        sims.append(s)
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    col = np.concatenate(cols).astype(np.int32) if n else np.zeros(0, dtype=np.int32)
    sim = np.concatenate(sims).astype(np.float32) if n else np.zeros(0, dtype=np.float32)
    valid = np.ones(n, dtype=bool)
    y = (3 * rng.standard_normal((n, 2))).astype(np.float32)
    if n >= 255:
        valid[[5, 200, n - 1]] = False
        y[7] = y[3]                                           # dx = dy = 0
        y[[11, 130, n - 2]] += np.float32(1e3)
        y[200] = np.nan                                       # an invalid row's point is never read
    return indptr, col, sim, valid, y


@pytest.fixture(scope="module")
def cases():
    """every size's graph with the definition's forces, computed once"""
    out = {}
    for n in SIZES:
        indptr, col, sim, valid, y = graph_case(n)
        _, i, j, p, _, m2, ok = sequence.tsne_affinities(indptr, col, sim, valid)
        want = dict(zip(FORCES, sequence.tsne_forces(y, i, j, p, ok)), m2=m2)
        out[n] = (indptr, col, sim, valid, y, want)
    return out


@pytest.fixture(scope="module")
def run300():
    """the 300-row graph, its init and the definition's 60 iterations, 20 of them exaggerated, computed once"""
    indptr, col, sim, valid, _ = graph_case(300, seed=5)
    init = sequence.tsne_init(300)
    kw = dict(n_iter=60, exaggeration_iter=20)
    return indptr, col, sim, valid, init, kw, sequence.tsne_layout(indptr, col, sim, init, valid, **kw)


@pytest.fixture(autouse=True)
def default_split(engine):
    yield
    engine.set_tsne_split(0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_layout(res, want):
    assert isinstance(res, TSNEResult) and res.layout.dtype == np.float32 and res.z_trace.dtype == np.uint64
    assert np.array_equal(res.z_trace, want["z_trace"])
    assert np.array_equal(res.valid, want["valid"]) and res.iterations == want["iterations"]
    assert np.isnan(res.layout[~want["valid"]]).all()
    ok = want["valid"]
    assert np.array_equal(bits(res.layout[ok]), bits(want["layout"][ok]))


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("n", SIZES)
def test_forces_equal_the_definition_bit_for_bit(engine, cases, n, split):
    indptr, col, sim, valid, y, want = cases[n]
    engine.set_tsne_split(split)
    got = engine.tsne_forces(indptr, col, sim, y, valid)
    assert got["m2"] == want["m2"]
    for k in FORCES:
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), k
    if n >= 255:
        assert (want["zi"][valid] > 0).all() and want["m2"] > 0 and np.abs(want["ax"]).max() > 0       # the case is no empty one
        assert all((got[k][~valid] == 0).all() for k in FORCES)


def test_forces_do_not_depend_on_the_order_of_a_rows_entries(engine, cases):
    indptr, col, sim, valid, y, want = cases[700]
    rng = np.random.default_rng(3)
    col2, sim2 = col.copy(), sim.copy()
    for i in range(len(indptr) - 1):
        o = rng.permutation(indptr[i + 1] - indptr[i]) + indptr[i]
        col2[indptr[i]:indptr[i + 1]], sim2[indptr[i]:indptr[i + 1]] = col[o], sim[o]
    got = engine.tsne_forces(indptr, col2, sim2, y, valid)
    assert got["m2"] == want["m2"] and all(np.array_equal(got[k], want[k]) for k in FORCES)


@pytest.mark.parametrize("split", SPLITS)
def test_layout_equals_the_definition_bit_for_bit(engine, run300, split):
    indptr, col, sim, valid, init, kw, want = run300
    engine.set_tsne_split(split)
    res = engine.tsne(indptr, col, sim, init, valid, **kw)
    assert_layout(res, want)
    assert len(np.unique(want["z_trace"])) > 50 and np.isfinite(want["layout"][want["valid"]]).all()      # the run moves
    assert res.kl_divergence == sequence.tsne_kl(indptr, col, sim, want["layout"], want["z_trace"][-1], valid)


def test_layout_after_the_workspace_grew_and_from_the_device_entry_point(engine, cases, run300):
    indptr, col, sim, valid, init, kw, want = run300
    small = cases[2]
    engine.tsne_forces(*small[:3], small[4], small[3])
    assert_layout(engine.tsne(indptr, col, sim, init, valid, **kw), want)
    big = cases[700]
    got = engine.tsne_forces(*big[:3], big[4], big[3])        # larger buffers, other contents
    assert all(np.array_equal(got[k], big[5][k]) for k in FORCES)
    assert_layout(engine.tsne(indptr, col, sim, init, valid, **kw), want)
    n, nnz, n_iter = 300, len(col), kw["n_iter"]
    ins = [indptr, col, sim, valid.astype(np.uint8), init]
    bufs = [engine.alloc(max(a.nbytes, 8)) for a in ins]
    outs = [engine.alloc(n * 8), engine.alloc((n_iter + 1) * 8), engine.alloc(max(n, 8))]
    try:
        for b, a in zip(bufs, ins):
            b.upload(a)
        res = engine.tsne_dev(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, n, nnz, bufs[4].ptr, outs[0].ptr, outs[1].ptr, outs[2].ptr,
                              valid_ptr=bufs[3].ptr, n_valid=int(valid.sum()), **kw)
        engine.sync()
        assert res.layout is None and res.iterations == n_iter
        dev = TSNEResult(layout=outs[0].download((n, 2), np.float32), z_trace=outs[1].download(n_iter + 1, np.uint64),
                         valid=outs[2].download(n, np.uint8).astype(bool), iterations=res.iterations)
        assert_layout(dev, want)
    finally:
        for b in bufs + outs:
            b.free()


def test_default_learning_rate_and_zero_iterations(engine, run300):
    indptr, col, sim, valid, init, _, _ = run300
    want = sequence.tsne_layout(indptr, col, sim, init, valid, n_iter=0)
    res = engine.tsne(indptr, col, sim, init, valid, n_iter=0)
    assert_layout(res, want)
    assert res.learning_rate == 50.0 and len(res.z_trace) == 1
    assert np.array_equal(bits(res.layout[valid]), bits(init[valid]))


def planted_rows(families=4, per=64, noise=64, seed=8):
    """512-wide rows: tight families around random centres, and noise rows; one zero row (invalid under cosine)"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((families, 512))
    rows = np.concatenate([c + 0.3 * rng.standard_normal((per, 512)) for c in centres] + [rng.standard_normal((noise, 512))])
    rows[per + 3] = 0
    return rows.astype(np.float32)


def test_graph_result_tsne_on_the_devices_knn_graph(engine):
    rows = planted_rows()
    g = engine.knn_graph(rows, 15)
    assert not g.valid[67] and g.valid.sum() == len(rows) - 1
    kw = dict(n_iter=40, exaggeration_iter=15)
    res = g.tsne(engine, **kw)
    want = sequence.tsne_layout(g.indptr, g.col, g.sim, sequence.tsne_init(g.n), g.valid, **kw)
    assert_layout(res, want)
    assert len(res.table()) == g.n and res.table()[67]["x"] is None
    chained = engine.tsne_rows(rows, k=15, **kw)
    init = engine.tsne_pca_init(rows)
    assert abs(float(init[g.valid, 0].astype(np.float64).std()) - 1e-4) < 1e-9 and (init[67] == 0).all()
    assert_layout(chained, sequence.tsne_layout(g.indptr, g.col, g.sim, init, g.valid, **kw))


def raw_tsne(engine, indptr, col, sim, valid, init, n=None, n_iter=5, exaggeration_iter=2, exaggeration=12.0, lr=50.0):
    """``gnn_tsne`` itself with sentinels in every output: (the status, whether the outputs are untouched)"""
    n = len(indptr) - 1 if n is None else n
    rows = len(indptr) - 1
    outs = [np.full(rows * 2, SENTINEL, np.uint32).view(np.float32), np.full(max(n_iter, 0) + 1, SENTINEL, np.uint64), np.full(rows, SENTINEL, np.uint8)]
    keep = [o.copy() for o in outs]
    rc = engine.lib.gnn_tsne(engine.ctx, indptr.ctypes.data, col.ctypes.data, sim.ctypes.data, None if valid is None else valid.ctypes.data,
                             n, len(col), init.ctypes.data, n_iter, exaggeration_iter, exaggeration, lr, *(o.ctypes.data for o in outs))
    return rc, all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(outs, keep))


def test_errors_leave_the_outputs_untouched(engine, cases):
    indptr, col, sim, valid, y, _ = cases[257]
    ok8 = valid.astype(np.uint8)
    init = sequence.tsne_init(257)
    rc, untouched = raw_tsne(engine, indptr, col, sim, ok8, init)
    assert rc == 0 and not untouched                          # the call as such is good
    bad_col = col.copy()
    bad_col[indptr[3]] = 3                                    # not in (row, n)
    bad_ptr = indptr.copy()
    bad_ptr[4] = bad_ptr[3] - 1
    bad_sim = sim.copy()
    bad_sim[10] = np.inf
    nan_init = init.copy()
    nan_init[9, 1] = np.nan
    inf_init = init.copy()
    inf_init[0, 0] = -np.inf
    for args, kw in (((indptr, bad_col, sim, ok8, init), {}), ((bad_ptr, col, sim, ok8, init), {}), ((indptr, col, bad_sim, ok8, init), {}),
                     ((indptr, col, sim, ok8, nan_init), {}), ((indptr, col, sim, None, inf_init), {}),
                     ((indptr, col, sim, ok8, init), dict(n=(1 << 21) + 1)), ((indptr, col, sim, ok8, init), dict(n=-1)),
                     ((indptr, col, sim, ok8, init), dict(n_iter=-1)), ((indptr, col, sim, ok8, init), dict(n_iter=100001)),
                     ((indptr, col, sim, ok8, init), dict(exaggeration_iter=100001)), ((indptr, col, sim, ok8, init), dict(exaggeration=0.5)),
                     ((indptr, col, sim, ok8, init), dict(exaggeration=float("nan"))), ((indptr, col, sim, ok8, init), dict(lr=0.0)),
                     ((indptr, col, sim, ok8, init), dict(lr=float("inf")))):
        rc, untouched = raw_tsne(engine, *args, **kw)
        assert rc < 0 and untouched, kw
        with pytest.raises(GnnError):
            check(rc)
    nan_at_invalid = init.copy()
    nan_at_invalid[5] = np.nan                                # row 5 does not take part
    rc, _ = raw_tsne(engine, indptr, col, sim, ok8, nan_at_invalid)
    assert rc == 0
    with pytest.raises(GnnError, match="not finite"):
        engine.tsne(indptr, col, sim, nan_init, valid, n_iter=3)
    with pytest.raises(GnnError, match="no upper-triangle CSR"):
        engine.tsne_forces(indptr, bad_col, sim, y, valid)
    with pytest.raises(ValueError):
        engine.tsne(indptr, col, sim, init, valid, n_iter=100001)
    # the device entry point: the outputs on the device stay as they were
    ins = [indptr, bad_col, sim, ok8, init]
    bufs = [engine.alloc(a.nbytes) for a in ins]
    outs = [engine.alloc(257 * 8), engine.alloc(6 * 8), engine.alloc(264)]
    try:
        for b, a in zip(bufs, ins):
            b.upload(a)
        for o in outs:
            o.upload(np.full(o.nbytes, SENTINEL, np.uint8))
        with pytest.raises(GnnError):
            engine.tsne_dev(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, 257, len(col), bufs[4].ptr, outs[0].ptr, outs[1].ptr, outs[2].ptr,
                            valid_ptr=bufs[3].ptr, n_iter=5, exaggeration_iter=2)
        engine.sync()
        assert all((o.download(o.nbytes, np.uint8) == SENTINEL).all() for o in outs)
    finally:
        for b in bufs + outs:
            b.free()


def test_empty_graphs(engine):
    e = (np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))
    res = engine.tsne(*e, np.zeros((0, 2), np.float32), n_iter=4)
    assert res.layout.shape == (0, 2) and np.array_equal(res.z_trace, np.zeros(5, np.uint64)) and res.kl_divergence == 0.0
    assert engine.tsne_forces(*e, np.zeros((0, 2), np.float32))["m2"] == 0
    # rows without an entry, one of them valid: Z = 0, nothing moves
    ptr = np.zeros(4, np.int64)
    init = sequence.tsne_init(3)
    valid = np.array([False, True, False])
    res = engine.tsne(ptr, e[1], e[2], init, valid, n_iter=3)
    assert np.array_equal(res.z_trace, np.zeros(4, np.uint64)) and np.array_equal(bits(res.layout[1]), bits(init[1]))
    assert np.isnan(res.layout[[0, 2]]).all()
