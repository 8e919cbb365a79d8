"""Rows for the representative tests: the planted clusters of tests/clusters_data.py plus a planted PATH (every row within the threshold of
its two neighbours on the path and of nothing else - what single linkage chains and a greedy walk cuts into stars), and a sequential
brute-force walk that shares no code with sequence.greedy_representatives."""
import math

import numpy as np

from tests.clusters_data import planted, sims64

PATH = 40
THRESHOLD = 0.9


def planted_path(n=333, seed=21, L=PATH):
    """(rows, groups): ``clusters_data.planted(n, seed)`` with its first L background positions, ascending, overwritten by a path.
    q = the QR factor of a seeded 512 x (L + 15) Gaussian (orthonormal columns), path[t] = 3 * (q[:, t] + ... + q[:, t + 15]): path
    rows d apart share 16 - d of 16 columns, cosine (16 - d) / 16 - 0.9375 at d = 1, 0.875 at d = 2.  ``groups`` gains "path": the
    positions in path order, which is the index order.  Asserted here, in fp64 at THRESHOLD: the path's adjacency is exactly a path
    with no edge to any other row, and no pair of rows lies within 1e-4 of the threshold."""
    r, groups = planted(n, seed)
    taken = np.concatenate(list(groups.values()))
    where = np.setdiff1d(np.arange(n), taken)[:L]            # ascending
    assert len(where) == L
    q, _ = np.linalg.qr(np.random.default_rng(seed + 2).standard_normal((512, L + 15)))
    r = r.copy()
    for t in range(L):
        r[where[t]] = (3.0 * q[:, t:t + 16].sum(axis=1)).astype(np.float32)
    groups = dict(groups, path=where)
    thr = float(np.float32(THRESHOLD))
    s = sims64(r, r)
    adj = s >= thr
    adj[np.arange(n), np.arange(n)] = False
    want = np.zeros((n, n), bool)
    want[where[:-1], where[1:]] = want[where[1:], where[:-1]] = True
    assert np.array_equal(adj[where], want[where]) and np.array_equal(adj[:, where], want[:, where])
    gap = np.abs(s[np.triu_indices(n, 1)] - thr).min()
    assert gap >= 1e-4, gap
    return np.ascontiguousarray(r), groups


def order_of(weight, n):
    """the rows by (weight descending, index ascending), one comparison key per row"""
    if weight is None:
        return list(range(n))
    return sorted(range(n), key=lambda i: (-float(weight[i]), i))


def walk(s, threshold, valid=None, weight=None):
    """The sequential walk, one pair at a time in Python.  ``s[a][b]`` is read only with a of smaller rank than b (so a matrix known
    for one orientation will do); a NaN is no edge.  Returns (rep int64, sim float32, size int64, rank int64) in the caller's index
    space: -1 / NaN / 0 for a row that is not valid."""
    n = len(s)
    valid = [True] * n if valid is None else [bool(v) for v in valid]
    order = order_of(weight, n)
    rank = [0] * n
    for k, i in enumerate(order):
        rank[i] = k
    rep, sim, reps = [-1] * n, [math.nan] * n, []
    for j in order:
        if not valid[j]:
            continue
        best = None
        for i in reps:                                       # by rank: a strict > keeps the smaller rank among equals
            v = s[i][j]
            if v >= threshold and (best is None or v > s[best][j]):
                best = i
        if best is None:
            reps.append(j)
            rep[j] = j
        else:
            rep[j], sim[j] = best, s[best][j]
    size = [0 if rep[i] < 0 else sum(1 for k in range(n) if rep[k] == rep[i]) for i in range(n)]
    return np.asarray(rep, np.int64), np.asarray(sim, np.float32), np.asarray(size, np.int64), np.asarray(rank, np.int64)


def weightings(groups, n, seed=5):
    """the three orders of the tests: the index order, seeded random weights with ties, and the path walked from its other end.
    Under the random weights the path's rows share one weight, so among themselves they keep the index order while the other rows
    fall between them at random: a path row BETWEEN two representatives of smaller rank would have two candidates at cosine 15 / 16
    that differ by rounding alone, and no exact comparison with another arithmetic survives that (``conditioned`` asserts it)."""
    reverse = np.zeros(n)
    reverse[groups["path"]] = 1 + np.arange(len(groups["path"]))
    random = np.random.default_rng(seed).integers(0, 6, n).astype(np.float64)
    random[groups["path"]] = 3
    return {"index": None, "random": random, "reversed": reverse}


def conditioned(s, threshold, rep, rank, margin=1e-4):
    """True iff an answer (rep, rank) on the fp64 similarities ``s`` can be compared exactly with an arithmetic that is within
    ``margin`` of them: every member's runner-up among the representatives of smaller rank within the threshold lies at least
    ``margin`` below its representative's similarity.  (The distance of every pair from the threshold is planted_path's assertion.)"""
    n = len(rep)
    reps = [i for i in range(n) if rep[i] == i]
    for j in range(n):
        if rep[j] < 0 or rep[j] == j:
            continue
        for i in reps:
            if i != rep[j] and rank[i] < rank[j] and s[i][j] >= threshold and s[i][j] > s[rep[j]][j] - margin:
                return False
    return True
