"""Inputs for the limits round of the Markov-clustering tests (tests/test_mcl_limits_host.py, tests/test_mcl_limits_gpu.py): the values
the integer power is held to Python integers on, and graphs at the ends of ``select``, ``precision``, the table's capacity, the row
index and the admitted weights, with parallel entries - upper-triangle CSRs as ``sequence.threshold_graph`` returns them.  Seeded,
built once and never written to; a fixture's definition (``sequence.markov_clusters``) is computed once and shared."""
import functools

import numpy as np

from genomad_amd import sequence
from tests.mcl_data import CLIQUE, PATH, PLANTED, RANDOM, csr_of_edges
from tests.spread_data import PARALLEL, star

ONE = 1 << 30
W = 1 << 24
A4 = tuple(range(5, 33))                              # every admitted inflation, in quarters
KNOBS = ((4096, 0), (64, 0), (0, 0), (4096, 1), (4096, 3), (64, 3))      # (table slots, workgroups) of tests/test_mcl_gpu.py
TOP = np.nextafter(np.float32(64), np.float32(0))     # the largest admitted similarity: q = 2^30 - 64
# k * 2^-25 is a rounding tie of sim * 2^24 for odd k: k -> the q that ties-to-even gives (k = 2: no tie)
TIES = {1: 0, 2: 1, 3: 2, 5: 2, 7: 4}


# ---- the power's values ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pow_values():
    """About 6000 values in [0, 2^30], ascending (uint64): the ends, the powers of two, the squares (where isqrt(u * ONE) steps: u *
    2^30 is a square exactly when u is), the k^4 >> 30 (where isqrt(h * ONE) steps), each with its neighbours, and uniform ones"""
    rng = np.random.default_rng(2024)
    v = [0, 1, 2, 3, ONE, ONE - 1, ONE - 2]
    for b in range(1, 31):
        v += [(1 << b) - 1, 1 << b, (1 << b) + 1]
    for k in list(range(1, 200)) + rng.integers(1, 1 << 15, 600).tolist() + [32767, 32768]:
        v += [k * k - 1, k * k, k * k + 1]
    for k in rng.integers(1, 1 << 15, 400).tolist():
        v += [(k ** 4 >> 30) + d for d in (-2, -1, 0, 1, 2)]
    v += rng.integers(0, ONE + 1, 1500).tolist()
    return np.array(sorted({int(x) for x in v if 0 <= x <= ONE}), dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def pow_reference(a4):
    """u ^ (a4 / 4) of every value of :func:`pow_values` on Python integers with ``math.isqrt`` (uint64)"""
    from tests.test_mcl_host import brute_pow
    return np.array([brute_pow(u, a4) for u in pow_values().tolist()], dtype=np.uint64)


# ---- graphs ---------------------------------------------------------------------------------------------------------------------------

def with_parallel(n, edges):
    from tests.test_mcl_host import _with_parallel
    return _with_parallel(n, edges)


def small_graphs():
    from tests.test_mcl_host import small_graphs as graphs
    return graphs()


def mixed():
    """14 rows: a path 0-1-2-3 of equal weights, a triangle 5-6-7 of three weights, a pair 10-11, the isolated rows 4, 8 and 13, and
    the invalid rows 9 (which has an entry to 10), 12 (isolated) and 2 (which cuts the path: 3 keeps no edge): (csr, valid)"""
    edges = [(0, 1, 0.75), (1, 2, 0.75), (2, 3, 0.75), (5, 6, 0.9), (6, 7, 0.6), (5, 7, 0.3), (9, 10, 0.8), (10, 11, 0.5)]
    valid = np.ones(14, dtype=bool)
    valid[[2, 9, 12]] = False
    return csr_of_edges(14, edges), valid


MIXED_ISOLATED = (3, 4, 8, 13)                        # valid rows without an existing edge: one-entry columns at any precision
MIXED_JOINED = (0, 1, 5, 6, 7, 10, 11)                # valid rows with one: emptied at precision 1


def lone():
    """six rows of a path, the last one isolated: the issue's probe"""
    return csr_of_edges(6, [(i, i + 1, 0.75) for i in range(4)])


def shifted_clique(first=65486, n=65600):
    """CLIQUE's 100 equal-weight nodes as the rows first .. first + 99 of ``n``: the 64 smallest of them straddle 2^16"""
    indptr, col, sim = CLIQUE
    nodes = len(indptr) - 1
    moved = np.concatenate([np.zeros(first, np.int64), indptr, np.full(n - first - nodes, indptr[-1], np.int64)])
    assert len(moved) == n + 1 and first < 65536 < first + 64
    return moved, (col + first).astype(np.int32), sim


def shifted_valid(first=65486, n=65600):
    valid = np.zeros(n, dtype=bool)
    valid[first:first + 100] = True
    return valid


def heavy():
    """PLANTED with every similarity times 60: 54 .. 59.4 (the bridges 33)"""
    return PLANTED[0], PLANTED[1], (PLANTED[2] * np.float32(60)).astype(np.float32)


def ranged():
    """PLANTED's structure with a third of the entries at 2^-24 (q = 1), a third at the largest admitted similarity (q = 2^30 - 64), and
    sprinkled over them the rounding ties 3 * 2^-25 (up to q = 2) and 5 * 2^-25 (down to q = 2), 2^-25 (to q = 0: no edge), -0.0 and
    a denormal (no edge either)"""
    rng = np.random.default_rng(77)
    sim = PLANTED[2].copy()
    kind = rng.integers(0, 3, len(sim))
    sim[kind == 0] = np.float32(2.0 ** -24)
    sim[kind == 1] = TOP
    at = rng.permutation(len(sim))[:250].reshape(5, 50)
    for rows, value in zip(at, (3 * 2.0 ** -25, 5 * 2.0 ** -25, 2.0 ** -25, -0.0, 1e-42)):
        sim[rows] = np.float32(value)
    assert sim.dtype == np.float32 and np.float32(1e-42) > 0
    return PLANTED[0], PLANTED[1], sim


def alltop():
    """PLANTED's structure with every entry at the largest admitted similarity"""
    return PLANTED[0], PLANTED[1], np.full(len(PLANTED[2]), TOP, dtype=np.float32)


def small_ranged():
    """the 18 nodes of two 9-cliques with weights over the whole admitted range - 54 .. 60 inside the cliques, the ties k * 2^-25 on
    the entries of node 4, the largest admitted similarity on the two bridges: small enough for the brute force"""
    rng = np.random.default_rng(5)
    edges = [(x, y, 54.0 + 6.0 * rng.random()) for s in (0, 9) for x in range(s, s + 9) for y in range(x + 1, s + 9)]
    ties = iter(sorted(TIES) * 2)
    edges = [(x, y, next(ties) * 2.0 ** -25 if 4 in (x, y) else w) for x, y, w in edges]
    return csr_of_edges(18, edges + [(0, 9, float(TOP)), (3, 12, float(TOP))])


DOUBLE_LEAVES = 70


def double_star():
    """a hub with 70 leaves, every leaf listed twice with two weights - the larger first for an even leaf, the smaller first for an
    odd one -, the smaller copy of every seventh at 0 or below: 71 distinct rows in the hub's column, 140 entries"""
    edges = []
    for leaf in range(1, DOUBLE_LEAVES + 1):
        large, small = 0.5 + leaf / 256, 0.3 + leaf / 512
        if leaf % 7 == 3:
            small = (0.0, -0.4)[leaf % 2]
        edges += [(0, leaf, large), (0, leaf, small)] if leaf % 2 == 0 else [(0, leaf, small), (0, leaf, large)]
    return with_parallel(DOUBLE_LEAVES + 1, edges)


def ring():
    return small_graphs()["ring"][0]


def small_random():
    return small_graphs()["random"]


STARS = (1022, 1023, 1024, 1100)                      # leaves: the hub's column has one entry more
STAR_CHANGED = {1022: [1, 1022], 1023: [1, 1023], 1024: [2, 1024], 1100: [78, 1100]}
PRECISIONS = (1, 2, 3, 1 << 20)

# name -> (graph, valid or None, markov_clusters' keywords): what runs on every knob
CASES = {f"star-{leaves}": (functools.partial(star, leaves, 0.75), None, dict(select=1024, max_iter=2)) for leaves in STARS}
CASES.update({f"select{s}-{name}": (lambda g=g: g, None, dict(select=s))
              for s in (1, 2) for name, g in (("planted", PLANTED), ("clique", CLIQUE), ("random", RANDOM))})
CASES.update({f"precision{p}-{name}": (lambda g=g: g, None, dict(precision=p))
              for p in PRECISIONS for name, g in (("path", PATH), ("planted", PLANTED))})
CASES.update({f"precision{p}-mixed": (lambda: mixed()[0], lambda: mixed()[1], dict(precision=p)) for p in PRECISIONS})
CASES.update({
    "heavy": (heavy, None, dict(select=64)), "ranged": (ranged, None, dict(select=64)), "alltop": (alltop, None, dict(select=64)),
    "small-ranged": (small_ranged, None, dict(select=6)),
    "ring": (ring, None, {}), "parallel": (lambda: PARALLEL, None, {}), "double-star": (double_star, None, {}),
    "double-star-select": (double_star, None, dict(select=40, inflation=1.75)),
})
# fixtures with knobs of their own
for _leaves in (4095, 4096, 63, 64):
    CASES[f"loop-{_leaves}"] = (functools.partial(star, _leaves, 0.75), None, dict(max_iter=1))
CASES["beyond-some"] = (shifted_clique, shifted_valid, dict(select=64))
CASES["beyond-all"] = (shifted_clique, None, dict(select=64))
for _a4 in A4:
    CASES[f"inflation{_a4}-random"] = (lambda: small_random()[0], lambda: small_random()[1], dict(inflation=_a4 / 4, select=8))
    CASES[f"inflation{_a4}-planted"] = (lambda: PLANTED, None, dict(inflation=_a4 / 4, select=64))

OWN_KNOBS = tuple(n for n in CASES if n.startswith(("loop-", "beyond-", "inflation")))
EVERY_KNOB = tuple(n for n in CASES if n not in OWN_KNOBS)


@functools.lru_cache(maxsize=None)
def case(name):
    """(graph, valid, keywords, the definition's answer), computed once"""
    graph, valid, kw = CASES[name]
    graph, valid = graph(), None if valid is None else valid()
    return graph, valid, kw, sequence.markov_clusters(*graph, valid, **kw)
