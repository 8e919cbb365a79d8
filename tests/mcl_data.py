"""Graphs for the Markov-clustering tests (tests/test_mcl_host.py, tests/test_mcl_gpu.py): upper-triangle CSRs as
``sequence.threshold_graph`` returns them - (indptr int64, col int32, sim float32) - built once and never written to."""
import numpy as np

PLANTED_SIZES = (5, 12, 30, 70, 100, 3, 1, 1)         # cliques, the last two singletons: 222 nodes, 8 clusters
PLANTED_N = sum(PLANTED_SIZES)


def csr_of_edges(n, edges):
    """(indptr, col, sim) of a list of (a, b, w), a != b; of parallel edges the last one stays.  A row's columns come out in the
    order the edges were first listed in, which need not be ascending."""
    rows = [dict() for _ in range(n)]
    for a, b, w in edges:
        rows[min(a, b)][max(a, b)] = w
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.array([c for r in rows for c in r], dtype=np.int32)
    sim = np.array([w for r in rows for w in r.values()], dtype=np.float32)
    return indptr, col, sim


def _build():
    rng = np.random.default_rng(7)
    start = np.cumsum((0,) + PLANTED_SIZES)
    edges = []
    for s, z in zip(start, PLANTED_SIZES):
        for x in range(s, s + z):
            for y in range(x + 1, s + z):
                edges.append((x, y, 0.9 + 0.09 * rng.random()))
    for c in range(len(PLANTED_SIZES) - 3):
        edges.append((int(start[c]), int(start[c + 1]), 0.55))          # one bridge between neighbouring cliques
    planted = csr_of_edges(PLANTED_N, edges)
    random = []
    for i in range(400):
        for j in rng.choice(400, 6, replace=False):
            if i != j:
                random.append((min(i, int(j)), max(i, int(j)), float(0.3 + 0.7 * rng.random())))
    return planted, np.repeat(np.arange(len(PLANTED_SIZES)), PLANTED_SIZES), csr_of_edges(400, random)


PLANTED, PLANTED_TRUTH, RANDOM = _build()            # weights 0.90 - 0.99, bridges 0.55; 400 nodes with 6 random partners each
PATH = csr_of_edges(40, [(i, i + 1, 0.75) for i in range(39)])
CLIQUE = csr_of_edges(100, [(x, y, 0.75) for x in range(100) for y in range(x + 1, 100)])          # exactly equal weights


def partition(label):
    """the clusters of a labelling as a set of frozensets of indices; rows with a negative label belong to none"""
    label = np.asarray(label)
    return {frozenset(np.flatnonzero(label == v).tolist()) for v in np.unique(label[label >= 0])}


def fan(c, leaves):
    """A graph with ONE column whose expansion has a known support: node 0 is joined to the hubs 1 .. c, and hub r to ``leaves[r]``
    nodes of its own.  The initial columns of the hubs have disjoint supports but for node 0 and the hub itself, so column 0 of the
    first iteration is summed over exactly 1 + c + sum(leaves) rows; hub r's over 1 + c + leaves[r], a leaf's over 2 + leaves[r]:
    no other column over as many.  Equal weights: nothing is cut off at the default precision while a column has fewer than 10 000
    entries.  Returns (indptr, col, sim, support of column 0)."""
    leaves = list(leaves)
    assert len(leaves) == c
    edges = [(0, r, 0.75) for r in range(1, c + 1)]
    nxt = c + 1
    for r, d in enumerate(leaves, start=1):
        edges += [(r, nxt + x, 0.75) for x in range(d)]
        nxt += d
    return csr_of_edges(nxt, edges) + (1 + c + sum(leaves),)


def shuffled_rows(csr, seed=3):
    """the same graph with every row's entries in another order"""
    indptr, col, sim = csr
    rng = np.random.default_rng(seed)
    col, sim = col.copy(), sim.copy()
    for a, b in zip(indptr[:-1], indptr[1:]):
        p = a + rng.permutation(b - a)
        col[a:b], sim[a:b] = col[p], sim[p]
    return indptr, col, sim


def relabelled(csr, perm):
    """the same graph with node i called perm[i]"""
    indptr, col, sim = csr
    a = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    return csr_of_edges(len(indptr) - 1, [(int(perm[x]), int(perm[y]), w) for x, y, w in zip(a, col, sim)])
