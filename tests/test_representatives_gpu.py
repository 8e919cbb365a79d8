"""Representatives among encoder embeddings on the MI355X: rep, size, rank and rounds against the numpy definition
(sequence.greedy_representatives) - exactly, on the planted path rows whose fp64 similarities keep 1e-4 from the threshold
(tests/representatives_data.py asserts it; the device's f32 values are within 1e-5) under three priority orders, and on integer rows
whose dots are exact with ties at the threshold -, independence of how the base is split over workgroups, the device's own values (the
pair i < j of the permuted rows is what neighbours returns for query i and base row j), many maxima at once on distinct keys and a tie
on one key, the edges of the interface, and embed_contigs -> representatives end to end.  333 rows are six 64-row tiles and two
256-column steps, off every boundary; the path needs 40 rounds."""
import numpy as np
import pytest

from genomad_amd import sequence, synthetic
from genomad_amd._lib import GnnError
from tests.neighbours_data import rows
from tests.representatives_data import PATH, THRESHOLD, conditioned, planted_path, sims64, walk, weightings

pytestmark = pytest.mark.gpu

ORDERS = ("index", "random", "reversed")
SIM_BOUND = 1e-5                     # the neighbour search's bound on |f32 similarity - fp64 cosine|


def exact(res, want, bits=False):
    """rep, size, rank and rounds exactly, NaN where the definition has NaN; sim bit for bit where `bits`"""
    rep, sim, size, rank, rounds = want
    for k, a, b in (("rep", res.rep, rep), ("size", res.size, size), ("rank", res.rank, rank)):
        assert a.dtype == np.int64 and np.array_equal(a, b), (k, np.flatnonzero(a != b)[:10])
    assert res.rounds == rounds and res.sim.dtype == np.float32 and np.array_equal(np.isnan(res.sim), np.isnan(sim))
    if bits:
        assert np.array_equal(res.sim.view(np.uint32)[~np.isnan(sim)], np.asarray(sim, np.float32).view(np.uint32)[~np.isnan(sim)])
    return True


def same_bits(a, b):
    return (all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("rep", "size", "rank")) and a.rounds == b.rounds
            and np.array_equal(a.sim.view(np.uint32), b.sim.view(np.uint32)))


@pytest.fixture(scope="module")
def data():
    """the planted path rows, the three weightings and the definition's answers, computed once"""
    r, groups = planted_path()
    w = weightings(groups, len(r))
    s64, want = sims64(r, r), {k: sequence.greedy_representatives(r, THRESHOLD, w[k]) for k in ORDERS}
    assert all(conditioned(s64, float(np.float32(THRESHOLD)), want[k][0], want[k][3]) for k in ORDERS)
    return {"rows": r, "groups": groups, "weights": w, "s64": s64, "want": want}


@pytest.fixture(scope="module")
def found(engine, data):
    """the device's answers, computed once with the library's own split"""
    engine.set_neighbour_split(0)
    return {k: engine.representatives(data["rows"], THRESHOLD, data["weights"][k]) for k in ORDERS}


@pytest.mark.parametrize("order", ORDERS)
def test_planted_path_rows_equal_the_definition(data, found, order):
    res, want = found[order], data["want"][order]
    assert exact(res, want)
    assert res.threshold == float(np.float32(THRESHOLD)) and res.metric == "cosine" and res.n_clusters == int((want[0] == np.arange(333)).sum())
    member = ~np.isnan(want[1])
    err = np.abs(res.sim[member].astype(np.float64) - data["s64"][res.rep[member], np.flatnonzero(member)]).max()
    print(f"\n{order}: {res.n_clusters} clusters in {res.rounds} rounds; max |sim - fp64 cosine| = {err:.2e}")
    assert err <= SIM_BOUND
    if order != "random":
        assert res.rounds == PATH
    if order == "index":
        path = data["groups"]["path"]
        assert list(res.rep[path]) == [p for p in path[0::2] for _ in range(2)] and (res.size[path] == 2).all()      # 20 stars of 2
        assert [c["size"] for c in res.table() if c["rep"] in set(path)] == [2] * 20


@pytest.mark.parametrize("order", ORDERS)
def test_results_do_not_depend_on_the_split_and_the_device_path_agrees(engine, data, found, order):
    r, w, first = data["rows"], data["weights"][order], found[order]
    try:
        for split in (32, 100, 333, 4096, 0):
            engine.set_neighbour_split(split)
            assert same_bits(engine.representatives(r, THRESHOLD, w), first), split
        engine.set_neighbour_split(100)
        by_rank = sequence.priority_order(w, len(r))
        p = np.ascontiguousarray(r[by_rank])                           # the C level takes the rows in priority order
        n = len(p)
        bufs = [engine.alloc(p.nbytes), engine.alloc(8 * n), engine.alloc(4 * n), engine.alloc(8 * n)]
        try:
            bufs[0].upload(p)
            rounds = engine.representatives_dev(bufs[0].ptr, n, THRESHOLD, *(b.ptr for b in bufs[1:]))
            engine.sync()
            rep_p, sim_p, size_p = bufs[1].download((n,), np.int64), bufs[2].download((n,), np.float32), bufs[3].download((n,), np.int64)
            assert rounds == first.rounds
            assert np.array_equal(np.where(rep_p >= 0, by_rank[np.maximum(rep_p, 0)], -1), first.rep[by_rank])
            assert np.array_equal(sim_p.view(np.uint32), first.sim[by_rank].view(np.uint32)) and np.array_equal(size_p, first.size[by_rank])
        finally:
            for buf in bufs:
                buf.free()
    finally:
        engine.set_neighbour_split(0)


def test_the_values_are_those_neighbours_returns_for_the_rows_in_priority_order(engine):
    """pins the orientation (query = the row of smaller rank, base row = the other), the >=, the tie rule on the f32, and that the
    searches compute the same f32: a brute-force walk on the device's own values gives rep, sim and size bit for bit"""
    r = rows(65, 9)
    w = np.random.default_rng(10).integers(0, 4, 65).astype(np.float64)
    by_rank = sequence.priority_order(w, 65)
    p = np.ascontiguousarray(r[by_rank])
    engine.set_neighbour_split(0)
    idx, sim = engine.neighbours(p, None, 64)
    assert (idx >= 0).all()
    s = np.full((65, 65), np.nan, np.float32)
    np.put_along_axis(s, idx, sim, axis=1)                             # s[i, j]: query i, base row j, both by rank
    upper = s[np.triu_indices(65, 1)]
    threshold = np.sort(upper)[int(len(upper) * 0.9)]                  # one of the returned f32 values: a tie exactly at the threshold
    assert threshold.dtype == np.float32 and (upper == threshold).any()
    rep_p, sim_p, size_p, _ = walk(s.tolist(), float(threshold))       # by rank; walk reads s[a][b] with a before b only
    assert 1 < int((rep_p == np.arange(65)).sum()) < 65 and (rep_p != np.arange(65)).sum() > 5
    res = engine.representatives(r, threshold, w)
    assert np.array_equal(res.rep[by_rank], by_rank[rep_p]) and np.array_equal(res.size[by_rank], size_p)
    assert np.array_equal(res.sim[by_rank].view(np.uint32), sim_p.view(np.uint32))
    assert np.array_equal(res.rank[by_rank], np.arange(65))


def test_integer_dots_with_ties_at_the_threshold_equal_the_definition(engine):
    rng = np.random.default_rng(11)
    base = rng.integers(0, 8, (200, 512)).astype(np.float32)          # every dot is an integer below 512 * 49 < 2^24: exact on the device
    base[40:60] = base[10]
    base[150] = base[3]
    base[199] = base[3]
    dots = base.astype(np.float64) @ base.astype(np.float64).T
    upper = dots[np.triu_indices(200, 1)]
    w = np.random.default_rng(3).integers(0, 4, 200)
    try:
        for threshold in (float(np.median(upper)), float(dots[0, 1])):
            assert (upper == threshold).sum() > 10
            for weight in (None, w):
                want = sequence.greedy_representatives(base, threshold, weight, "dot")
                for split in (0, 32):
                    engine.set_neighbour_split(split)
                    assert exact(engine.representatives(base, threshold, weight, "dot"), want, bits=True), (threshold, split)
        res = engine.representatives(base, float(dots[0, 1]), None, "dot")
        assert res.rep[1] == 0 and res.sim[1] == dots[0, 1]           # row 1 holds on to row 0 by the tie alone
    finally:
        engine.set_neighbour_split(0)


def test_one_star_of_300_many_maxima_at_once(engine):
    r = rows(333, 13)
    copies = np.sort(np.random.default_rng(14).permutation(333)[:300])
    r[copies] = r[copies[0]]
    w = np.random.default_rng(15).integers(0, 3, 333).astype(np.float64)
    try:
        for weight in (None, w):
            want = sequence.greedy_representatives(r, 0.99, weight)
            first = copies[np.argmin(want[3][copies])]                  # the copy of lowest rank
            for split in (0, 32):
                engine.set_neighbour_split(split)
                got = engine.representatives(r, 0.99, weight)
                assert exact(got, want), split
                assert (got.rep[copies] == first).all() and (got.size[copies] == 300).all() and got.n_clusters == 34 and got.rounds == 2
                members = copies[copies != first]
                assert len(set(got.sim[members].view(np.uint32))) == 1 and abs(float(got.sim[members[0]]) - 1.0) <= SIM_BOUND
    finally:
        engine.set_neighbour_split(0)


def test_two_identical_representatives_tie_on_one_key(engine):
    """Under dot two identical short rows A and B are both representatives (A.B below the threshold) of long copies of themselves
    (A.m = B.m above it): a member behind B has two candidates with the same f32 and must take the one of smaller rank."""
    r = rows(333, 13)
    u = r[7].copy()
    q = float(u.astype(np.float64) @ u.astype(np.float64))
    threshold = 2.0 * q
    a, b = 0, 150
    copies = np.sort(np.setdiff1d(np.random.default_rng(14).permutation(333)[:302], [a, b])[:300])
    r[copies] = 4.0 * u                                                # m.A = m.B = 4 q, m.m = 16 q
    r[a] = r[b] = u                                                    # A.B = q
    s64 = sims64(r, r, "dot")
    assert np.abs(s64[np.triu_indices(333, 1)] - threshold).min() >= 1e-4 * threshold      # nothing else near the threshold
    assert (copies < b).any() and (copies > b).any()
    to_b_first = np.zeros(333)
    to_b_first[b] = 1                                                  # B before A: the tie goes the other way
    try:
        for weight, winner in ((None, a), (to_b_first, b)):
            want = sequence.greedy_representatives(r, threshold, weight, "dot")
            assert want[0][a] == a and want[0][b] == b and (want[0][copies] == winner).all()
            for split in (0, 32):
                engine.set_neighbour_split(split)
                got = engine.representatives(r, threshold, weight, "dot")
                assert exact(got, want), split
                assert (got.rep[copies] == winner).all() and got.size[winner] == 301 and got.size[a + b - winner] == 1
                assert len(set(got.sim[copies].view(np.uint32))) == 1
    finally:
        engine.set_neighbour_split(0)


@pytest.mark.parametrize("n", (1, 64, 65, 257))
def test_tile_and_step_edges_with_invalid_rows(engine, n):
    engine.set_neighbour_split(0)
    r = rows(n, 4)
    r[n // 2:] = r[0]                                                  # the upper half, the last row included: copies of row 0
    if n > 3:
        r[1] = 0
        r[3, 100] = np.nan
        r[n - 2, 511] = np.inf
    for metric, threshold in (("cosine", 0.6), ("dot", 0.6 * float(r[0].astype(np.float64) @ r[0].astype(np.float64)))):
        ok = np.isfinite(r).all(axis=1) & ((r != 0).any(axis=1) | (metric == "dot"))
        s = sims64(np.where(ok[:, None], r, 1), np.where(ok[:, None], r, 1), metric)
        pairs = s[np.ix_(ok, ok)][np.triu_indices(int(ok.sum()), 1)]
        assert n == 1 or np.abs(pairs - float(np.float32(threshold))).min() >= 1e-4 * max(1.0, threshold)
        w = None if metric == "cosine" else np.arange(n) % 3
        want = sequence.greedy_representatives(r, threshold, w, metric)
        assert conditioned(s, float(np.float32(threshold)), want[0], want[3], 1e-4 * max(1.0, threshold))
        got = engine.representatives(r, threshold, w, metric)
        assert exact(got, want), metric
        assert (got.rep[~ok] == -1).all() and (got.size[~ok] == 0).all() and np.isnan(got.sim[~ok]).all()
        if n > 3:
            assert got.size[0] >= n - n // 2


def test_edges_of_the_interface(engine, data):
    engine.set_neighbour_split(0)
    p = data["rows"]
    got = engine.representatives(p[:0], 0.5)
    assert got.rep.shape == got.sim.shape == got.size.shape == got.rank.shape == (0,) and got.rounds == 0 and got.n_clusters == 0
    assert got.table() == []
    got = engine.representatives(p[:1], 0.5)
    assert (list(got.rep), list(got.size), list(got.rank), got.rounds) == ([0], [1], [0], 1) and np.isnan(got.sim[0])
    got = engine.representatives(np.zeros((70, 512), np.float32), 0.5)     # no valid row: nothing to decide
    assert (got.rep == -1).all() and (got.size == 0).all() and np.isnan(got.sim).all() and got.rounds == 0
    got = engine.representatives(p, 1.5)                               # above every similarity: everybody founds a cluster, in one round
    assert exact(got, sequence.greedy_representatives(p, 1.5)) and got.rounds == 1 and got.is_rep.all() and np.isnan(got.sim).all()
    got = engine.representatives(p, -1.0, np.arange(len(p)))          # one star around the heaviest row
    assert (got.rep == len(p) - 1).all() and (got.size == len(p)).all() and got.rounds == 2 and got.n_clusters == 1
    with pytest.raises(GnnError, match=r"gnn_representatives: threshold nan is outside .* finite"):
        engine.representatives(p, float("nan"))
    with pytest.raises(GnnError, match=r"gnn_representatives: metric 9 is outside \[0, 1\]"):
        engine.representatives(p, 0.5, None, 9)
    with pytest.raises(GnnError, match=r"gnn_representatives_dev: -1 rows is outside \[0, 2\^31\)"):
        engine.representatives_dev(0, -1, 0.5, 0, 0, 0)
    with pytest.raises(ValueError, match="weight"):
        engine.representatives(p, 0.5, np.ones(5))


def test_embed_contigs_to_representatives_end_to_end(engine):
    rng = np.random.default_rng(5)
    windows = synthetic.synth_windows(900, 30)
    contigs = [windows[a:a + n].reshape(-1)[:int(rng.integers((n - 1) * 6000 + 3000, n * 6000 + 1))]
               for a, n in zip(range(0, 24, 2), [1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 2])]
    contigs[9] = contigs[4].copy()                            # byte-identical to contig 4
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in contigs])]).astype(np.int64)
    seq = np.concatenate(contigs)
    engine.set_neighbour_split(0)
    before, _ = engine.classify_contigs(seq, offsets)
    _, emb, ids = engine.embed_contigs(seq, offsets)
    weight = np.bincount(ids, minlength=len(contigs))         # kept windows, as main() weighs the contigs
    idx0, sim0 = engine.neighbours(emb, None, 3)
    res = engine.representatives(emb, 0.999, weight)
    idx1, sim1 = engine.neighbours(emb, None, 3)              # the searches share the fragment buffers
    after, _ = engine.classify_contigs(seq, offsets)
    assert res.rep[4] == res.rep[9] and res.size[4] == res.size[9] >= 2       # identical rows see the same representatives
    s64, thr = sims64(emb, emb), float(np.float32(0.999))                     # the guarantees, in fp64 with the device's bound
    reps, members = np.flatnonzero(res.is_rep), np.flatnonzero(~res.is_rep)
    assert (s64[np.ix_(reps, reps)][np.triu_indices(len(reps), 1)] < thr + SIM_BOUND).all()
    assert (s64[res.rep[members], members] >= thr - SIM_BOUND).all() and (res.rank[res.rep[members]] < res.rank[members]).all()
    assert np.abs(res.sim[members] - s64[res.rep[members], members]).max() <= SIM_BOUND
    assert np.array_equal(res.rank, np.argsort(np.argsort(-weight, kind="stable"), kind="stable"))
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    assert np.array_equal(idx0, idx1) and np.array_equal(sim0.view(np.uint32), sim1.view(np.uint32))
