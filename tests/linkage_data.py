"""For the single-linkage tests: a brute-force Kruskal over a given value matrix and a naive agglomeration, neither sharing code with
sequence.single_linkage_tree; the device's own pair values for any n; what the device tests compare a result by (bits, same,
check_shape); and the fixtures of the cluster tests that the linkage tests reuse."""
import math

import numpy as np

from tests.neighbours_data import rows


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def same(got, want):
    """two LinkageResults, or a result and an (a, b, sim) of the same f32: indices, bits, flags and rounds"""
    if isinstance(want, tuple):
        return np.array_equal(got.a, want[0]) and np.array_equal(got.b, want[1]) and np.array_equal(bits(got.sim), bits(want[2]))
    return (np.array_equal(got.a, want.a) and np.array_equal(got.b, want.b) and np.array_equal(bits(got.sim), bits(want.sim))
            and np.array_equal(got.valid, want.valid) and got.rounds == want.rounds)


def check_shape(res, n):
    assert res.a.dtype == res.b.dtype == np.int64 and res.sim.dtype == np.float32 and res.valid.dtype == np.uint8
    assert res.n == n and res.valid.shape == (n,) and res.n_valid == int(res.valid.sum())
    assert res.a.shape == res.b.shape == res.sim.shape == (res.n_edges,)
    if res.n_valid >= 2:
        assert 1 <= res.rounds <= math.ceil(math.log2(res.n_valid)), (res.rounds, res.n_valid)
    else:
        assert res.rounds == 0 and res.n_edges == 0


def kruskal(values, valid=None):
    """Brute force: (a, b, sim) of the maximum spanning forest of the complete graph over the ``valid`` rows with the weights
    ``values`` (n, n), read for i < j only.  Edges are walked by (value descending, i ascending, j ascending) - Python's own tuple
    order -, -0 counts as +0, a NaN is no edge; components are a label per row, relabelled at every join.  ``sim`` keeps the dtype
    of ``values``."""
    values = np.asarray(values)
    n = len(values)
    valid = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
    pairs = []
    for i in range(n):
        for j in range(i + 1, n):
            v = values[i, j]
            if valid[i] and valid[j] and v == v:
                pairs.append((-(float(v) + 0.0), i, j))
    pairs.sort()
    label = list(range(n))
    a, b, sim = [], [], []
    for _, i, j in pairs:
        if label[i] != label[j]:
            old, new = label[j], label[i]
            label = [new if x == old else x for x in label]
            a.append(i)
            b.append(j)
            sim.append(values[i, j] + values.dtype.type(0))
    return np.asarray(a, np.int64), np.asarray(b, np.int64), np.asarray(sim, values.dtype)


def agglomerate(values):
    """Naive agglomerative single linkage over all n rows of ``values`` (read for i < j): while two clusters are left, merge the two
    with the best pair between them, by (value descending, i ascending, j ascending).  Returns (a, b, sim, z): the best pairs in merge
    order and the linkage matrix in SciPy's convention (ids of the merged clusters, the smaller first; 1 - value; the new size)."""
    values = np.asarray(values, np.float64)
    n = len(values)
    clusters = {i: [i] for i in range(n)}                # id -> members
    a, b, sim, z = [], [], [], []
    for step in range(n - 1):
        best = None
        for p in clusters:
            for q in clusters:
                if p < q:
                    for i in clusters[p]:
                        for j in clusters[q]:
                            lo, hi = min(i, j), max(i, j)
                            key = (-values[lo, hi], lo, hi)
                            if best is None or key < best[0]:
                                best = (key, p, q)
        (neg, lo, hi), p, q = best
        a.append(lo)
        b.append(hi)
        sim.append(-neg)
        members = clusters.pop(p) + clusters.pop(q)
        clusters[n + step] = members
        z.append((p, q, 1.0 + neg, len(members)))
    return np.asarray(a, np.int64), np.asarray(b, np.int64), np.asarray(sim, np.float64), np.asarray(z, np.float64).reshape(n - 1, 4)


def device_values(engine, r, metric="cosine"):
    """The device's own f32 value of every pair: s[i, j] is what ``engine.neighbours`` returns for query i and base row j (NaN where
    it returns none), assembled per block of 64 base rows - a pair's value depends on its two rows only, so the base subset changes
    nothing."""
    n = len(r)
    s = np.full((n, n), np.nan, np.float32)
    for j0 in range(0, n, 64):
        idx, sim = engine.neighbours(r, r[j0:j0 + 64], 64, metric)
        for i in range(n):
            ok = idx[i] >= 0
            s[i, j0 + idx[i][ok]] = sim[i][ok]
    return s


def integer_rows():
    """the 200 rows of test_clusters_gpu.py::test_integer_dots_with_ties_at_the_threshold_equal_the_definition: every dot is an
    integer below 2^24, exact on the device, with many ties"""
    rng = np.random.default_rng(11)
    base = rng.integers(0, 8, (200, 512)).astype(np.float32)
    base[40:60] = base[10]
    base[150] = base[3]
    base[199] = base[3]
    return base


def integer_rows_with_two_invalid():
    base = integer_rows()
    base[5, 17] = np.nan
    base[77, 400] = np.inf
    return base


def many_copies():
    """the rows of test_clusters_gpu.py::test_many_joins_of_one_tree_at_once: 300 of 333 rows are copies of one; returns (rows, copies)"""
    r = rows(333, 13)
    copies = np.sort(np.random.default_rng(14).permutation(333)[:300])
    r[copies] = r[copies[0]]
    return r, copies


def interface_rows():
    """the 70 rows of test_clusters_gpu.py::test_edges_of_the_interface: one row 70 times, row 1 zero, rows 3 and 65 not finite"""
    r = np.tile(rows(1, 4), (70, 1))
    r[1] = 0
    r[3, 100] = np.nan
    r[65, 511] = np.inf
    return r
