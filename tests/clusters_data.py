"""Rows with planted clusters for the cluster tests, their fp64 similarities, and a brute-force component labelling that shares no code
with sequence.threshold_clusters."""
import numpy as np

from tests.neighbours_data import rows, sims64      # noqa: F401  (sims64 is re-exported)

FAMILIES, FAMILY, CHAIN = 5, 12, 24
THRESHOLDS = (0.8, 0.9)


def planted(n=333, seed=21):
    """(n, 512) float32, n >= 120: background rows of ``neighbours_data.rows`` (pairwise cosine about 0.3) plus five families of 12
    (centre + 0.15 * noise: cliques at 0.8 and 0.9), one chain of 24 (c <- c + 0.25 * noise: neighbouring links hold at both
    thresholds, the two ends are far below either) and one pair of identical rows, scattered by a fixed permutation.  Centres and
    noise are rows of the same draw, so they share its channel scales.  Returns (rows, groups): ``groups`` is a dict of the planted
    members' positions - "family0" .. "family4", "chain" (in chain order) and "pair"."""
    planted_rows = FAMILIES * FAMILY + CHAIN + 2
    pool = rows(n - planted_rows + FAMILIES + 2 + planted_rows, seed)
    background, pool = pool[:n - planted_rows], pool[n - planted_rows:]
    centres, start, twin, noise = pool[:FAMILIES], pool[FAMILIES], pool[FAMILIES + 1], pool[FAMILIES + 2:]
    out, o = [background], 0
    for f in range(FAMILIES):
        out.append(centres[f] + np.float32(0.15) * noise[o:o + FAMILY])
        o += FAMILY
    chain, c = [], start
    for _ in range(CHAIN):
        c = c + np.float32(0.25) * noise[o]
        o += 1
        chain.append(c)
    out += [np.stack(chain), np.stack([twin, twin])]
    r = np.concatenate(out).astype(np.float32)
    assert r.shape == (n, 512)
    perm = np.random.default_rng(seed + 1).permutation(n)
    where = np.empty(n, np.int64)
    where[perm] = np.arange(n)                   # row i of r lands at where[i]
    a = n - planted_rows
    groups = {f"family{f}": where[a + f * FAMILY:a + (f + 1) * FAMILY] for f in range(FAMILIES)}
    groups["chain"] = where[a + FAMILIES * FAMILY:a + FAMILIES * FAMILY + CHAIN]
    groups["pair"] = where[n - 2:]
    return np.ascontiguousarray(r[perm]), groups


def components(adj, valid=None):
    """Brute force: (label, degree, size, rep) int64 of the graph ``adj`` (n, n) bool, symmetric, its diagonal ignored; rows that are
    not ``valid`` have no edges and get -1, 0, 0, -1.  Labels by propagation: every row starts as its own label and takes the
    smallest label among itself and its neighbours until nothing changes."""
    adj = np.array(adj, dtype=bool)
    n = len(adj)
    valid = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
    adj &= valid[:, None] & valid[None, :]
    adj[np.arange(n), np.arange(n)] = False
    degree = [int(adj[i].sum()) for i in range(n)]
    label = list(range(n))
    changed = True
    while changed:
        changed = False
        for i in range(n):
            for j in range(n):
                if adj[i, j] and label[j] < label[i]:
                    label[i] = label[j]
                    changed = True
    size, rep = [0] * n, [-1] * n
    for i in range(n):
        if not valid[i]:
            label[i], degree[i] = -1, 0
            continue
        members = [j for j in range(n) if valid[j] and label[j] == label[i]]
        size[i] = len(members)
        rep[i] = min(members, key=lambda j: (-degree[j], j))
    return tuple(np.asarray(a, dtype=np.int64) for a in (label, degree, size, rep))


def device_edges(sim_upper, threshold):
    """adjacency from values known for i < j only: edge {i, j} iff sim_upper[i, j] >= threshold, i < j"""
    s = np.asarray(sim_upper)
    upper = np.triu(np.ones(s.shape, bool), 1)
    with np.errstate(invalid="ignore"):
        adj = (s >= threshold) & upper
    return adj | adj.T
