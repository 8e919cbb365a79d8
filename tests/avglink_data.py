"""Graphs for the average-linkage tests (tests/test_avglink_host.py, tests/test_avglink_gpu.py): upper-triangle CSRs as
``sequence.threshold_graph`` returns them - (indptr int64, col int32, sim float32) - with the rows' validity, the graphs of
tests/mcl_data.py and tests/spread_data.py among them.  Built once and never written to."""
import functools

import numpy as np

from genomad_amd import sequence
from tests.clusters_data import planted
from tests.mcl_data import RANDOM, csr_of_edges
from tests.mcl_limits_data import heavy, ranged
from tests.spread_data import PARALLEL, RANDOM_VALID, n_of, star

W = 1 << 24
STAR_LEAVES = 4200                                    # the hub's row is wider than any table (4 096 slots)
COMPLETE_N = 200
PLANTED_ROWS, PLANTED_THRESHOLD = 200, 0.3


def sparse(seed, n=60, entries=300):
    """``n`` nodes, about ``entries`` entries with random 24-bit weights: sim = w / 2^24 is exact in float32, and ties are rare"""
    rng = np.random.default_rng(1000 + seed)
    a, b = rng.integers(0, n, entries), rng.integers(0, n, entries)
    w = rng.integers(1, W, entries)
    return csr_of_edges(n, [(int(x), int(y), int(q) / W) for x, y, q in zip(a, b, w) if x != y])


def tied(seed, n=24, entries=70):
    """``n`` nodes with weights in {1, 2, 3} * 2^21: heavily tied averages"""
    rng = np.random.default_rng(2000 + seed)
    a, b = rng.integers(0, n, entries), rng.integers(0, n, entries)
    w = rng.integers(1, 4, entries)
    return csr_of_edges(n, [(int(x), int(y), int(q) / 8) for x, y, q in zip(a, b, w) if x != y])


def complete_rows(n=COMPLETE_N, dim=8, seed=31):
    """``n`` unit rows with non-negative entries: every cosine lies in (0, 1]"""
    r = np.abs(np.random.default_rng(seed).standard_normal((n, dim)))
    return r / np.sqrt((r * r).sum(axis=1))[:, None]


def complete():
    """the complete graph of :func:`complete_rows`, its similarities as float32"""
    s = (complete_rows() @ complete_rows().T).astype(np.float32)
    n = len(s)
    return csr_of_edges(n, [(x, y, s[x, y]) for x in range(n) for y in range(x + 1, n)])


def planted_graph():
    """the planted families of tests/clusters_data.py through ``sequence.threshold_graph``: (csr, valid)"""
    rows = planted(PLANTED_ROWS)[0]
    indptr, col, sim = sequence.threshold_graph(rows, PLANTED_THRESHOLD)
    return (indptr, col, sim.astype(np.float32)), sequence.valid_rows(rows)


def rising_path(n=64):
    """a chain whose weights rise: every round merges the one pair at its end but for the reciprocal pairs of the first"""
    return csr_of_edges(n, [(i, i + 1, (i + 1) / (2 * n)) for i in range(n - 1)])


RANDOM_MASKED_VALID = RANDOM_VALID
STAR = star(STAR_LEAVES, 0.5)
EMPTY = (np.zeros(6, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))      # five rows, no entry
NONE = (np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))       # no row
ONE = (np.zeros(2, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))        # n = 1


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (csr, valid or None): every fixture but the star"""
    pg, pv = planted_graph()
    return {
        "sparse0": (sparse(0), None), "sparse1": (sparse(1), None), "tied0": (tied(0), None), "tied1": (tied(1), None),
        "complete": (complete(), None), "planted": (pg, pv), "path": (rising_path(), None), "parallel": (PARALLEL, None),
        "masked": (RANDOM, RANDOM_MASKED_VALID), "empty": (EMPTY, np.array([True, False, True, True, True])), "none": (NONE, None),
        "one": (ONE, None), "heavy": (heavy(), None), "ranged": (ranged(), None),
    }


NAMES = ("sparse0", "sparse1", "tied0", "tied1", "complete", "planted", "path", "parallel", "masked", "empty", "none", "one", "heavy",
         "ranged")


@functools.lru_cache(maxsize=None)
def reference(name, stop=sequence.AVGLINK_STOP_DEFAULT, max_rounds=sequence.AVGLINK_MAX_ROUNDS_MAX):
    """the definition's answer for a fixture, computed once"""
    csr, valid = (STAR, None) if name == "star" else cases()[name]
    return sequence.average_linkage(*csr, valid, stop, max_rounds)


def greedy(csr, valid=None, stop_q=1):
    """Sequential greedy UPGMA on ``Fraction``s: the globally best pair under (average descending, a, b) merges, until no pair's
    average reaches stop_q.  Returns the merges as a set of (a, b, S, size_a, size_b)."""
    from fractions import Fraction
    n, ea, eb, eq, _ = sequence.mcl_weights(*csr, valid)
    rows = {}
    for x, y, w in zip(ea.tolist(), eb.tolist(), eq.tolist()):
        rows.setdefault(x, {})[y] = rows.setdefault(x, {}).get(y, 0) + w
        rows.setdefault(y, {})[x] = rows.setdefault(y, {}).get(x, 0) + w
    size = {i: 1 for i in rows}
    out = set()
    while True:
        top = None
        for a, row in rows.items():
            for b, s in row.items():
                if a < b:
                    key = (-Fraction(s, size[a] * size[b]), a, b)
                    if top is None or key < top[0]:
                        top = (key, a, b, s)
        if top is None or -top[0][0] < stop_q:
            return out
        _, a, b, s = top
        out.add((a, b, s, size[a], size[b]))
        for c, v in rows.pop(b).items():
            del rows[c][b]
            if c != a:
                rows[a][c] = rows[a].get(c, 0) + v
                rows[c][a] = rows[c].get(a, 0) + v
        size[a] += size.pop(b)


def merge_set(res):
    return set(zip(*(np.asarray(res[k]).tolist() for k in sequence.AVGLINK_FIELDS[:5])))
