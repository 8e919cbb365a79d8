"""Inputs of the label-transfer tests, built from the rows the other searches' tests already have (tests/density_data.planted,
tests/kmeans_data.planted, tests/neighbours_data.rows), and two constructions of the four vote arrays that share no code with
sequence.class_votes: a plain double loop over a similarity matrix, and a fold of an edge list (what NNEngine.match returns).

Query: the 333 planted density rows - six 64-row tiles, off every boundary; families that are cliques at cosine about 0.91, bridges,
satellites and a path at 0.83 - 0.85, two identical rows, a zero row and a row with one NaN.
Base: a pool of 300 rows - copies of the 57 planted density rows, a zero row and a NaN row (both labelled), 60 planted k-means rows and
ReLU rows - cut at 7, 33 and 300: below a 32-column block, across one, across the 256-column step.  Every prefix holds the zero row,
the NaN row and rows labelled -1.  A row's raw label is its group's number; ``labels(n_base, n_classes)`` folds it onto
n_classes - 1 classes, so the last class has no member."""
import functools

import numpy as np

from tests import density_data, kmeans_data
from tests.neighbours_data import rows as relu_rows, sims64

NQ = 333
BASES = (7, 33, 300)
CLASSES = (3, 16, 17, 40)                        # both sides of the LDS limit, and across a 32-column block of classes
UNIT = float(1 << 32)
T_HIGH = 0.9                                     # inside the families' cliques
T_MID = 0.8                                      # below the bridges, satellites and the path
GAPPED = (T_HIGH, T_MID, -1.0)                   # the thresholds of the float64 comparison: tests/test_votes_host.py asserts the gap
GAP = 1e-5                                       # the project's bound on the device's f32 similarity against float64
NEAREST_GAP = 2e-5                               # top two of a class further apart than this: the float64 nearest is the device's


@functools.lru_cache(maxsize=None)
def query():
    r, groups = density_data.planted(NQ)
    r.setflags(write=False)
    return r, groups


@functools.lru_cache(maxsize=None)
def pool():
    """(rows (300, 512) float32, raw label int64 (300,)): -1 = unlabelled"""
    q, groups = query()
    order = ["familyA", "familyB", "familyC", "familyD", "bridges", "satellites", "hanger", "path", "pair"]
    head = [(groups["familyA"][0], 0), (groups["zero"][0], 1), (groups["familyA"][1], -1), (groups["familyB"][0], 1), (groups["nan"][0], 2),
            (groups["familyC"][0], 2), (groups["pair"][0], 8)]
    taken = {int(i) for i, _ in head}
    rest = [(int(i), g) for g, name in enumerate(order) for i in groups[name] if int(i) not in taken]
    rng = np.random.default_rng(77)
    rest_rows = [q[i] for i, _ in rest]
    rest_label = [g for _, g in rest]
    km, family = kmeans_data.planted()
    pick = np.flatnonzero(family >= 0)[:60]
    rest_rows += list(km[pick])
    rest_label += list(9 + family[pick])         # 9 .. 15
    n_relu = 300 - len(head) - len(rest_rows)
    rest_rows += list(relu_rows(n_relu, 78))
    rest_label += list(rng.integers(16, 61, n_relu))
    rest_label = np.asarray(rest_label, dtype=np.int64)
    rest_label[rng.random(len(rest_label)) < 0.1] = -1
    perm = rng.permutation(len(rest_rows))
    r = np.stack([q[i] for i, _ in head] + [rest_rows[j] for j in perm]).astype(np.float32)
    raw = np.concatenate([np.asarray([g for _, g in head], dtype=np.int64), rest_label[perm]])
    assert r.shape == (300, 512)
    r.setflags(write=False)
    raw.setflags(write=False)
    return r, raw


def base(n_base):
    return np.ascontiguousarray(pool()[0][:n_base])


def labels(n_base, n_classes):
    """int64 (n_base,) in [-1, n_classes - 1): the raw labels folded; class n_classes - 1 has no member"""
    raw = pool()[1][:n_base]
    return np.where(raw < 0, -1, raw % max(n_classes - 1, 1)).astype(np.int64)


def valid(r):
    r = np.asarray(r, np.float32)
    return np.isfinite(r).all(axis=1) & (r != 0).any(axis=1)


@functools.lru_cache(maxsize=None)
def cosines(n_base):
    """(float64 (333, n_base) cosines - 0 wherever a row is not valid -, the valid queries, the valid base rows); computed once"""
    q, b = query()[0], base(n_base)
    q_ok, b_ok = valid(q), valid(b)
    s = np.zeros((len(q), len(b)))
    s[np.ix_(np.flatnonzero(q_ok), np.flatnonzero(b_ok))] = sims64(q[q_ok], b[b_ok])
    s.setflags(write=False)
    return s, q_ok, b_ok


def loop_votes(s, q_ok, b_ok, label, n_classes, threshold, leave_one_out=False):
    """The four arrays by a plain double loop over the pairs of ``s`` (float64 or float32 similarities): a voter adds one, adds
    rint(s * 2^32) and replaces the nearest if it is more similar - the loop runs over ascending j, so among equals the smaller
    index stays."""
    thr = float(np.float32(threshold))
    nq, nb = s.shape
    count, weight = np.zeros((nq, n_classes), np.int64), np.zeros((nq, n_classes), np.int64)
    nearest, nearest_sim = np.full((nq, n_classes), -1, np.int64), np.full((nq, n_classes), np.nan, np.float32)
    best = np.full((nq, n_classes), -np.inf)
    for i in range(nq):
        if not q_ok[i]:
            continue
        for j in range(nb):
            c = int(label[j])
            v = float(s[i, j])
            if c < 0 or not b_ok[j] or (leave_one_out and i == j) or not v >= thr:
                continue
            count[i, c] += 1
            weight[i, c] += int(np.rint(v * UNIT))
            if v > best[i, c]:
                best[i, c], nearest[i, c], nearest_sim[i, c] = v, j, v
    return count, weight, nearest, nearest_sim


def fold_edges(a, b, sim, label, n_query, n_classes, leave_one_out=False):
    """The four arrays from an edge list (query a, base b, float32 sim): what the votes are when the edges are those within the
    threshold.  int64 sums of rint(float64(sim) * 2^32); the nearest by (sim descending, index ascending), with the sim's bits."""
    a, b, sim = np.asarray(a, np.int64), np.asarray(b, np.int64), np.asarray(sim, np.float32)
    c = np.asarray(label, np.int64)[b]
    keep = c >= 0
    if leave_one_out:
        keep &= a != b
    a, b, c, sim = a[keep], b[keep], c[keep], sim[keep]
    count, weight = np.zeros((n_query, n_classes), np.int64), np.zeros((n_query, n_classes), np.int64)
    np.add.at(count, (a, c), 1)
    np.add.at(weight, (a, c), np.rint(sim.astype(np.float64) * UNIT).astype(np.int64))
    nearest, nearest_sim = np.full((n_query, n_classes), -1, np.int64), np.full((n_query, n_classes), np.nan, np.float32)
    order = np.lexsort((-b, sim))                    # ascending in (sim, then index descending): the last write of a cell is the best
    nearest[a[order], c[order]] = b[order]
    nearest_sim[a[order], c[order]] = sim[order]
    return count, weight, nearest, nearest_sim


def tie_rows():
    """The 0 / 1 rows of the density tests (tests/density_data.integer_rows: 200 rows, 20 copies of row 10 and two of row 3) with
    every row brought to exactly 256 ones - the first surplus ones cleared, the first missing ones set -, so that a row's norm is 16
    and a pair's cosine is dot / 256: exact in every arithmetic, and tied in hundreds at any threshold that is one of them."""
    r = density_data.integer_rows().copy()
    for row in r:
        ones, zeros = np.flatnonzero(row == 1), np.flatnonzero(row == 0)
        if len(ones) > 256:
            row[ones[:len(ones) - 256]] = 0
        else:
            row[zeros[:256 - len(ones)]] = 1
    r[40:60] = r[10]
    r[150] = r[3]
    r[199] = r[3]
    assert ((r == 0) | (r == 1)).all() and (r.sum(axis=1) == 256).all()
    return r


@functools.lru_cache(maxsize=None)
def tie_case():
    """(rows (200, 512), cosines float64 (200, 200) - exact multiples of 1 / 256 -, the threshold: the 0.9 quantile of the pair
    cosines, one of them; labels int64 (200,) in [-1, 5))"""
    r = tie_rows()
    s = (r.astype(np.float64) @ r.astype(np.float64).T) / 256.0
    pairs = np.sort(s[np.triu_indices(len(r), 1)])
    threshold = float(pairs[int(0.9 * (len(pairs) - 1))])
    label = (np.arange(len(r)) % 6 - 1).astype(np.int64)        # -1, 0, 1, 2, 3, 4, -1, ...
    r.setflags(write=False)
    s.setflags(write=False)
    return r, s, threshold, label
