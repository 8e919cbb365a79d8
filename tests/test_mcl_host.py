"""sequence.markov_clusters without a GPU: against a dense brute force on Python integers that shares no code with it, against a float64
dense MCL's partition, the counts and iteration numbers the planted graphs are known to give, invalid rows, weights <= 0, isolated
nodes, the order within a row, a relabelling of the nodes, every ValueError and max_iter = 0."""
import math

import numpy as np
import pytest

from genomad_amd import sequence
from genomad_amd.sequence import MCL_ONE as ONE, MCL_W as W, markov_clusters
from tests import mcl_data as D


# ---- the brute force: n x n lists of Python integers, no sparse structure ---------------------------------------------------------------

def brute_prune(column, select, precision):
    """column: n integers y >= 0 -> n integers p"""
    total = sum(column)
    kept = [i for i, y in enumerate(column) if y > 0 and y * precision >= total]
    kept = sorted(kept, key=lambda i: (-column[i], i))[:select]
    total = sum(column[i] for i in kept)
    out = [0] * len(column)
    for i in kept:
        out[i] = column[i] * ONE // total
    return out


def brute_pow(u, a):
    h = math.isqrt(u * ONE)
    g = math.isqrt(h * ONE)
    y = ONE
    for _ in range(a // 4):
        y = y * u >> 30
    if a % 4 >= 2:
        y = y * h >> 30
    if a % 2:
        y = y * g >> 30
    return y


def brute_initial(n, graph, valid, select, precision):
    indptr, col, sim = graph
    q = [[0] * n for _ in range(n)]                      # q[i][j]
    for i in range(n):
        for e in range(indptr[i], indptr[i + 1]):
            j, v = int(col[e]), int(np.rint(np.float64(np.float32(sim[e])) * W))
            if v > 0 and valid[i] and valid[j]:
                q[i][j] = q[j][i] = max(q[i][j], v)
    cols = []
    for j in range(n):
        column = [q[i][j] for i in range(n)]
        column[j] = max(column) if max(column) else W
        cols.append(brute_prune(column, select, precision) if valid[j] else [0] * n)
    return cols                                          # cols[j][i] = p_ij


def brute_step(n, cols, a, select, precision):
    new = []
    for j in range(n):
        t = [sum(cols[k][i] * cols[j][k] for k in range(n)) >> 30 for i in range(n)]
        m = max(t)
        new.append(brute_prune([brute_pow(x * ONE // m, a) if x else 0 for x in t], select, precision) if m else [0] * n)
    return new


def brute_matrices(graph, valid, inflation, select, precision, iterations):
    """the matrix after 0, 1, .. iterations, each as (length, idx, val)"""
    n = len(graph[0]) - 1
    valid = [True] * n if valid is None else list(valid)
    cols, out = brute_initial(n, graph, valid, select, precision), []
    for it in range(iterations + 1):
        out.append(([sum(p > 0 for p in c) for c in cols], [i for c in cols for i, p in enumerate(c) if p], [p for c in cols for p in c if p]))
        cols = brute_step(n, cols, int(inflation * 4), select, precision)
    return out


def small_graphs():
    rng = np.random.default_rng(11)
    two = [(x, y, 0.9 + 0.09 * rng.random()) for s in (0, 9) for x in range(s, s + 9) for y in range(x + 1, s + 9)] + [(0, 9, 0.5), (3, 12, 0.5)]
    rnd = [(int(x), int(y), float(rng.random() * 1.4 - 0.2)) for x, y in rng.integers(0, 40, (150, 2)) if x != y]
    ring = [(i, (i + 1) % 25, 0.5 + 0.01 * i) for i in range(25)] + [(0, 12, 0.5), (0, 12, 0.9)]           # one pair twice
    valid = np.ones(40, bool)
    valid[[3, 17, 31]] = False
    return {"two cliques": (D.csr_of_edges(18, two), None), "random": (D.csr_of_edges(40, rnd), valid),
            "ring": (_with_parallel(25, ring), None), "path": (D.csr_of_edges(21, [(i, i + 1, 0.75) for i in range(20)]), None)}


def _with_parallel(n, edges):
    """a CSR that keeps parallel edges"""
    rows = [[] for _ in range(n)]
    for a, b, w in edges:
        rows[min(a, b)].append((max(a, b), w))
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return indptr, np.array([c for r in rows for c, _ in r], np.int32), np.array([w for r in rows for _, w in r], np.float32)


@pytest.mark.parametrize("name", sorted(small_graphs()))
@pytest.mark.parametrize("inflation,select,precision", [(2.0, 256, 10000), (1.25, 5, 10000), (2.75, 8, 50), (8.0, 3, 1 << 20)])
def test_the_matrix_equals_a_dense_brute_force_on_python_integers(name, inflation, select, precision):
    graph, valid = small_graphs()[name]
    final = markov_clusters(*graph, valid, inflation, select, precision)
    want = brute_matrices(graph, valid, inflation, select, precision, max(final["iterations"], 3))
    for it in (0, 1, 2, 3, final["iterations"]):
        got = markov_clusters(*graph, valid, inflation, select, precision, max_iter=it)
        if it <= final["iterations"]:
            assert got["iterations"] == it
        assert (got["length"].tolist(), got["idx"].tolist(), got["val"].tolist()) == want[min(it, final["iterations"])], (name, it)
    assert final["converged"] and want[final["iterations"]] == want[final["iterations"] - 1]
    assert final["length"].dtype == np.int64 and final["idx"].dtype == np.int32 and final["val"].dtype == np.uint32


# ---- float64 -----------------------------------------------------------------------------------------------------------------------------

def float_partition(graph, inflation, select=1024, precision=10000, iterations=200):
    """a dense float64 MCL with the same loops, cutoff and selection: the partition its limit gives"""
    indptr, col, sim = graph
    n = len(indptr) - 1
    m = np.zeros((n, n))
    a = np.repeat(np.arange(n), np.diff(indptr))
    keep = sim > 0
    m[a[keep], col[keep]] = m[col[keep], a[keep]] = sim[keep].astype(np.float64)
    m[np.arange(n), np.arange(n)] = np.where(m.max(axis=0) > 0, m.max(axis=0), 1.0)

    def prune(m):
        m = np.where(m * precision >= m.sum(axis=0), m, 0.0)
        if select < n:
            order = np.lexsort((np.arange(n)[:, None] + 0 * m, -m), axis=0)
            rank = np.empty_like(order)
            np.put_along_axis(rank, order, np.arange(n)[:, None] + 0 * order, axis=0)
            m = np.where(rank < select, m, 0.0)
        return m / m.sum(axis=0)

    m = prune(m)
    for _ in range(iterations):
        m = m @ m
        m = prune((m / m.max(axis=0)) ** inflation)
    label = np.arange(n)
    for _ in range(n):                                   # propagation of the smallest label over {i, j: m_ij > 1e-6}
        i, j = np.nonzero(m > 1e-6)
        low = np.minimum(label[i], label[j])
        nxt = label.copy()
        np.minimum.at(nxt, i, low)
        np.minimum.at(nxt, j, low)
        if np.array_equal(nxt, label):
            break
        label = nxt
    return D.partition(label)


PLANTED_ITERATIONS = {1.25: 45, 1.5: 26, 2.0: 16, 4.0: 9, 8.0: 6}


@pytest.fixture(scope="module")
def planted_runs():
    """the planted graph at every inflation and both selection numbers, computed once"""
    return {(infl, sel): markov_clusters(*D.PLANTED, inflation=infl, select=sel) for infl in PLANTED_ITERATIONS for sel in (1024, 64)}


@pytest.mark.parametrize("inflation", sorted(PLANTED_ITERATIONS))
def test_planted_cliques_come_out_at_every_inflation_as_in_float64(planted_runs, inflation):
    res = planted_runs[inflation, 1024]
    assert res["converged"] and res["iterations"] == PLANTED_ITERATIONS[inflation] and res["changed"][-1] == 0 and (res["changed"][:-1] > 0).all()
    assert D.partition(res["label"]) == D.partition(D.PLANTED_TRUTH) == float_partition(D.PLANTED, inflation)
    assert np.array_equal(res["size"], np.repeat(D.PLANTED_SIZES, D.PLANTED_SIZES))
    assert (res["label"][res["attractor"]] == res["label"]).all() and res["is_attractor"][res["attractor"]].all()
    # a selection number below the largest clique's size: harmless up to inflation 4, at 8 the 100-clique falls apart
    cut = planted_runs[inflation, 64]
    assert cut["converged"] and cut["iterations"] == PLANTED_ITERATIONS[inflation]
    if inflation <= 4:
        assert D.partition(cut["label"]) == D.partition(D.PLANTED_TRUTH)
    else:
        parts = D.partition(cut["label"])
        assert len(parts) > 8 and all(len({int(D.PLANTED_TRUTH[i]) for i in p}) == 1 for p in parts)
        assert D.partition(cut["label"][:117]) == D.partition(D.PLANTED_TRUTH[:117])              # the cliques of at most 64 rows stand


def test_path_clique_and_random_graph_give_the_known_counts():
    for inflation, clusters in ((1.5, 2), (2.0, 12)):
        res = markov_clusters(*D.PATH, inflation=inflation)
        assert res["converged"] and len(D.partition(res["label"])) == clusters == len(float_partition(D.PATH, inflation))
    for select in (1024, 64):
        res = markov_clusters(*D.CLIQUE, select=select)
        assert res["converged"] and res["iterations"] == 1 and res["changed"].tolist() == [0] and (res["label"] == 0).all()
        assert (res["length"] == min(select, 100)).all()
        assert np.array_equal(res["idx"][:min(select, 100)], np.arange(min(select, 100)))         # ties: the smallest indices stay
    for inflation in (2.0, 3.0):
        want = float_partition(D.RANDOM, inflation)
        for precision in (10000, 1 << 20):
            res = markov_clusters(*D.RANDOM, inflation=inflation, select=1024, precision=precision)
            assert res["converged"] and D.partition(res["label"]) == want, (inflation, precision)


@pytest.mark.parametrize("precision,clusters", [(1 << 20, 5), (10000, 6)])
def test_random_graph_at_a_low_inflation_needs_the_finer_cutoff(precision, clusters):
    res = markov_clusters(*D.RANDOM, inflation=1.5, select=1024, precision=precision)
    assert res["converged"] and len(D.partition(res["label"])) == clusters
    if precision == 1 << 20:
        assert D.partition(res["label"]) == float_partition(D.RANDOM, 1.5, precision=precision)


# ---- the rules -----------------------------------------------------------------------------------------------------------------------------

def test_invalid_rows_weights_below_zero_and_isolated_nodes():
    indptr, col, sim = D.PLANTED
    sim = sim.copy()
    start = np.cumsum((0,) + D.PLANTED_SIZES)
    a = np.repeat(np.arange(D.PLANTED_N), np.diff(indptr))
    sim[(a == 5) | (col == 5)] = -0.3                    # row 5 keeps no edge: a cluster of one
    sim[(a < 5) & (col >= 5)] = 0.0                      # the first bridge goes
    valid = np.ones(D.PLANTED_N, bool)
    valid[[20, 200]] = False
    res = markov_clusters(indptr, col, sim, valid)
    assert res["label"][[20, 200]].tolist() == [-1, -1] and res["size"][[20, 200]].tolist() == [0, 0]
    assert res["attractor"][[20, 200]].tolist() == [-1, -1] and res["flow"][[20, 200]].tolist() == [0, 0]
    assert not res["is_attractor"][[20, 200]].any() and res["length"][[20, 200]].tolist() == [0, 0]
    assert not np.isin(res["idx"], [20, 200]).any()
    assert res["label"][5] == 5 and res["size"][5] == 1 and res["attractor"][5] == 5 and res["flow"][5] == ONE and res["is_attractor"][5]
    assert (res["label"][:5] == 0).all() and (res["size"][6:17] == 11).all() and res["size"][21] == 29 and res["size"][start[4]] == 99
    # the same graph without the rows and edges that do not exist
    keep = (sim > 0) & valid[a] & valid[col]
    thin = D.csr_of_edges(D.PLANTED_N, list(zip(a[keep].tolist(), col[keep].tolist(), sim[keep].tolist())))
    other = markov_clusters(*thin, valid)
    assert all(np.array_equal(res[k], other[k]) for k in res)
    # no edges at all, no rows at all
    lone = markov_clusters([0, 0, 0], np.zeros(0, np.int32), np.zeros(0, np.float32))
    assert lone["label"].tolist() == [0, 1] and lone["val"].tolist() == [ONE, ONE] and lone["iterations"] == 1 and lone["converged"]
    none = markov_clusters([0], np.zeros(0, np.int32), np.zeros(0, np.float32))
    assert none["iterations"] == 1 and none["converged"] and len(none["label"]) == 0


def test_the_order_within_a_row_changes_no_bit():
    for graph in (D.PLANTED, D.RANDOM):
        want, got = markov_clusters(*graph, select=64), markov_clusters(*D.shuffled_rows(graph), select=64)
        assert not np.array_equal(graph[1], D.shuffled_rows(graph)[1])
        assert all(np.array_equal(want[k], got[k]) for k in want)


def test_a_relabelling_permutes_the_partition_where_select_does_not_bite():
    perm = np.random.default_rng(2).permutation(D.PLANTED_N)
    for inflation in (1.5, 2.0):
        want = markov_clusters(*D.PLANTED, inflation=inflation, select=1024)
        got = markov_clusters(*D.relabelled(D.PLANTED, perm), inflation=inflation, select=1024)
        assert {frozenset(perm[list(p)].tolist()) for p in D.partition(want["label"])} == D.partition(got["label"])
        assert got["iterations"] == want["iterations"] and np.array_equal(got["changed"], want["changed"])
        assert np.array_equal(got["flow"][perm], want["flow"]) and np.array_equal(got["size"][perm], want["size"])


def test_max_iter_zero_interprets_the_initial_matrix():
    res = markov_clusters(*D.PLANTED, max_iter=0)
    assert res["iterations"] == 0 and not res["converged"] and res["changed"].shape == (0,) and res["changed"].dtype == np.int64
    # the initial columns are the graph's neighbourhoods: the bridges join the six cliques
    assert len(D.partition(res["label"])) == 3 and res["size"][0] == 220
    assert np.array_equal(res["length"], sequence.graph_degree(D.PLANTED[0], D.PLANTED[1]) + 1)
    assert (np.add.reduceat(res["val"].astype(np.int64), np.cumsum(res["length"]) - res["length"]) <= ONE).all()
    one = markov_clusters(*D.PLANTED, max_iter=1)
    assert one["iterations"] == 1 and not one["converged"] and one["changed"].tolist() == [D.PLANTED_N - 2]      # all but the singletons


def test_every_value_error():
    indptr, col, sim = D.PATH
    for bad in (1.0, 1.3, 8.25, 0, -2, "x", None, np.nan, True):
        with pytest.raises(ValueError, match="inflation"):
            markov_clusters(indptr, col, sim, inflation=bad)
    for kw in (dict(select=0), dict(select=1025), dict(select=2.5), dict(precision=0), dict(precision=(1 << 20) + 1), dict(max_iter=-1),
               dict(max_iter=10001), dict(max_iter=True)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            markov_clusters(indptr, col, sim, **kw)
    for s in (np.inf, -np.inf, np.nan, 64.0, 1e39):
        with pytest.raises(ValueError, match="sim"):
            markov_clusters(indptr, col, np.where(np.arange(39) == 7, s, sim.astype(np.float64)))
    markov_clusters(indptr, col, np.where(np.arange(39) == 7, 63.9, sim.astype(np.float64)), max_iter=1)
    for c in (0, 7, 40, -1):                             # row 7's partner: below it, itself, beyond n, negative
        with pytest.raises(ValueError, match="col"):
            markov_clusters(indptr, np.where(np.arange(39) == 7, c, col), sim)
    for ip in (indptr[1:], np.where(np.arange(41) == 5, 3, indptr), indptr + 1, indptr[:-2], indptr.astype(np.float64)):
        with pytest.raises(ValueError, match="indptr"):
            markov_clusters(ip, col, sim)
    with pytest.raises(ValueError, match="sim"):
        markov_clusters(indptr, col, sim[:-1])
    with pytest.raises(ValueError, match="sim"):
        markov_clusters(indptr, col, np.arange(39))
    for v in (np.ones(39, bool), np.ones(40, np.int64), np.ones((40, 1), bool)):
        with pytest.raises(ValueError, match="valid"):
            markov_clusters(indptr, col, sim, v)
    with pytest.raises(ValueError, match="2\\^24"):
        markov_clusters(np.zeros((1 << 24) + 2, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))
    assert sequence.mcl_inflation(1.25) == 5 and sequence.mcl_inflation(8) == 32 and sequence.mcl_inflation(np.float32(2.75)) == 11


def test_table_and_fan():
    res = markov_clusters(*D.PLANTED)
    table = sequence.mcl_table(res["label"], res["size"], res["is_attractor"])
    assert [c["label"] for c in table] == np.cumsum((0,) + D.PLANTED_SIZES[:-1]).tolist() and [c["size"] for c in table] == list(D.PLANTED_SIZES)
    assert all(c["members"] == list(range(c["label"], c["label"] + c["size"])) and set(c["attractors"]) <= set(c["members"]) and c["attractors"]
               for c in table)
    named = sequence.mcl_table(res["label"], res["size"], res["is_attractor"], [f"c{i}" for i in range(D.PLANTED_N)])
    assert named[1]["label"] == "c5" and named[1]["members"][:2] == ["c5", "c6"]
    indptr, col, sim, support = D.fan(3, [4, 2, 5])
    assert support == 15 == len(indptr) - 1
    first = markov_clusters(indptr, col, sim, max_iter=1, precision=1 << 20)
    assert first["length"][0] == 15                      # column 0 of the first iteration is summed over every row


def test_the_dense_and_the_entry_by_entry_products_agree(monkeypatch):
    """the definition multiplies small matrices densely and large ones entry by entry: the same bits either way, on the graphs here
    and against the brute force"""
    graphs = {"planted": (D.PLANTED, None, dict(select=64)), "random": (D.RANDOM, None, dict(inflation=3.0)),
              "small": small_graphs()["random"] + (dict(inflation=1.25, select=5),)}
    want = {k: markov_clusters(*g, v, **kw) for k, (g, v, kw) in graphs.items()}
    monkeypatch.setattr(sequence, "MCL_DENSE_ROWS", 0)
    for k, (g, v, kw) in graphs.items():
        got = markov_clusters(*g, v, **kw)
        assert all(np.array_equal(got[f], want[k][f]) for f in got), k
    g, v, kw = graphs["small"]
    got = markov_clusters(*g, v, max_iter=2, **kw)
    assert (got["length"].tolist(), got["idx"].tolist(), got["val"].tolist()) == brute_matrices(g, v, 1.25, 5, 10000, 2)[2]
