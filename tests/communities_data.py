"""Graphs for the modularity-community tests (tests/test_communities_host.py, tests/test_communities_gpu.py): upper-triangle CSRs as
``sequence.threshold_graph`` returns them - (indptr int64, col int32, sim float32) - with the rows' validity.  Deterministic, built
once and never written to.  Two inputs are *searched*: the first seeds at which the definition reports a rejected sweep and a split
community; :func:`search` is the search (on the CPU, in Python integers), its hits are fixed below and checked by the host tests."""
import functools

import numpy as np

from genomad_amd import sequence
from tests.clusters_data import planted          # noqa: F401 - the tests take it from here too
from tests.mcl_data import RANDOM, csr_of_edges
from tests.mcl_limits_data import heavy, ranged
from tests.spread_data import PARALLEL, RANDOM_VALID, n_of, star

W = 1 << 24
KINDS = ("unit", "quarter", "random")
RESOLUTIONS = (0.25, 1.0, 2.5, 4.0)                   # r = 16, 64, 160, 256
STAR_LEAVES = 4200                                    # the hub's row is longer than any table (4 096 slots)
STAR_HUB, STAR_PAIR = 0.5, 1.0
PLANTED_ROWS, PLANTED_THRESHOLD = 200, 0.3
# what search() found: the first seed of random_graph(seed, n, p, "unit") at r = 160 with a rejected sweep / a split community
REJECTED = dict(n=57, p=0.3, seed=0, resolution=2.5)
SPLIT = dict(n=42, p=0.08, seed=348, resolution=2.5)


def random_graph(seed, n, p, kind):
    """G(n, p) with weights of one of the three kinds: ``unit`` (sim 1), ``quarter`` (0.25, 0.5, 0.75, 1: heavy ties) or ``random``
    (w / 2^24 with a random 24-bit w: exact in float32, ties rare)"""
    rng = np.random.default_rng([seed, n, int(p * 1000), KINDS.index(kind)])
    edges = []
    for x in range(n):
        for y in range(x + 1, n):
            if rng.random() < p:
                w = {"unit": 1.0, "quarter": int(rng.integers(1, 5)) / 4, "random": int(rng.integers(1, W)) / W}[kind]
                edges.append((x, y, w))
    return csr_of_edges(n, edges)


def search(what, n, p, resolution, seeds=range(4000)):
    """the first seed whose unit-weight G(n, p) makes the definition report ``what`` ("rejected" or "split") at some level"""
    for seed in seeds:
        if sequence.modularity_communities(*random_graph(seed, n, p, "unit"), resolution=resolution)[what].any():
            return seed
    return None


def planted_graph():
    """the planted families of tests/clusters_data.py through ``sequence.threshold_graph``: (csr, valid, the families)"""
    rows, groups = planted(PLANTED_ROWS)[:2]
    indptr, col, sim = sequence.threshold_graph(rows, PLANTED_THRESHOLD)
    return (indptr, col, sim.astype(np.float32)), sequence.valid_rows(rows), groups


def path(n=64):
    return csr_of_edges(n, [(i, i + 1, 1.0) for i in range(n - 1)])


def ring_of_cliques(cliques=12, size=5):
    """``cliques`` cliques of ``size`` nodes, neighbouring cliques joined by one entry, all of weight 1"""
    edges = [(c * size + x, c * size + y, 1.0) for c in range(cliques) for x in range(size) for y in range(x + 1, size)]
    edges += [(c * size + size - 1, ((c + 1) % cliques) * size, 1.0) for c in range(cliques)]
    return csr_of_edges(cliques * size, edges)


def grid(side=12):
    at = lambda x, y: x * side + y
    return csr_of_edges(side * side, [(at(x, y), at(x + dx, y + dy), 1.0) for x in range(side) for y in range(side)
                                      for dx, dy in ((0, 1), (1, 0)) if x + dx < side and y + dy < side])


def of_networkx(g):
    """a networkx graph with nodes 0 .. n - 1 as a CSR; an edge's ``weight`` (1 without one) / 32 is its similarity"""
    return csr_of_edges(g.number_of_nodes(), [(int(a), int(b), float(d.get("weight", 1)) / 32) for a, b, d in g.edges(data=True) if a != b])


def to_networkx(csr, valid=None):
    """the definition's integer graph as a networkx graph over the valid rows, parallel entries added"""
    import networkx as nx
    n, a, b, q, ok = sequence.mcl_weights(*csr, valid)
    g = nx.Graph()
    g.add_nodes_from(np.flatnonzero(ok).tolist())
    for x, y, w in zip(a.tolist(), b.tolist(), q.tolist()):
        g.add_edge(x, y, weight=(g[x][y]["weight"] if g.has_edge(x, y) else 0) + w)
    return g


def paired_star(leaves=STAR_LEAVES):
    """Node 0 joined to ``leaves`` leaves by entries of 0.5, the leaves joined in pairs by entries of 1.  A bare star ends with its
    first sweep (the hub and half its leaves trade places, which is rejected); here the pairs form, the hub joins one, the hub's
    component gathers more than 4 096 entries in the contraction and the next level has a hub of leaves / 2 - 1 entries."""
    return csr_of_edges(leaves + 1, [(0, i, STAR_HUB) for i in range(1, leaves + 1)] + [(i, i + 1, STAR_PAIR) for i in range(1, leaves, 2)])


STAR = paired_star()
BARE_STAR = star(STAR_LEAVES, 0.5)
EMPTY = (np.zeros(6, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))      # five rows, no entry
NONE = (np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))       # no row
ONE = (np.zeros(2, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))        # n = 1


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (csr, valid or None): every fixture but the star"""
    pg, pv, _ = planted_graph()
    out = {f"{kind}{seed}": (random_graph(seed, n, p, kind), None)
           for kind in KINDS for seed, n, p in ((0, 40, 0.15), (1, 59, 0.3))}
    out.update({
        "rejected": (random_graph(REJECTED["seed"], REJECTED["n"], REJECTED["p"], "unit"), None),
        "split": (random_graph(SPLIT["seed"], SPLIT["n"], SPLIT["p"], "unit"), None),
        "planted": (pg, pv), "path": (path(), None), "ring": (ring_of_cliques(), None), "grid": (grid(), None), "parallel": (PARALLEL, None),
        "masked": (RANDOM, RANDOM_VALID), "empty": (EMPTY, np.array([True, False, True, True, True])), "none": (NONE, None),
        "one": (ONE, None), "heavy": (heavy(), None), "ranged": (ranged(), None),
    })
    return out


RANDOM_NAMES = tuple(f"{kind}{seed}" for kind in KINDS for seed in (0, 1))
NAMES = RANDOM_NAMES + ("rejected", "split", "planted", "path", "ring", "grid", "parallel", "masked", "empty", "none", "one",
                        "heavy", "ranged")


@functools.lru_cache(maxsize=None)
def reference(name, resolution=1.0, max_levels=sequence.COMM_LEVELS_MAX, max_sweeps=sequence.COMM_SWEEPS_MAX):
    """the definition's answer for a fixture, computed once"""
    csr, valid = {"star": (STAR, None), "bare_star": (BARE_STAR, None)}.get(name) or cases()[name]
    return sequence.modularity_communities(*csr, valid, resolution, max_levels, max_sweeps)
