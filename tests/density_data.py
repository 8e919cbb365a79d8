"""Rows with planted density structure for the density tests - controlled geometry on fresh orthonormal directions, so that every
margin is known -, the 0/1 integer rows whose dots tie, and a brute-force DBSCAN that shares no code with
sequence.density_clusters."""
import numpy as np

from tests.neighbours_data import sims64      # noqa: F401  (re-exported)

FAMILY, EPS, RHO, T = 10, 0.3, 0.5, 0.8
PLANTED = 4 * FAMILY + 3 + 4 + 2 + 6 + 2         # 57 rows that are not background
MIN_POINTS = (1, 2, 3, 6, 11)                    # the host tests; the GPU tests use all but 2


def planted(n=333, seed=41):
    """(n, 512) float32, n >= 59.  All planted rows are built from orthonormal directions (the columns of one QR), so their
    similarities are the coefficients below up to rounding.
      familyA .. familyD  10 rows each, unit(centre + (0.3 + 0.004 j) * fresh direction): cliques at 0.8 (cosine about 0.91).  The
                          centres of A and B have cosine 0.5 (members about 0.46: no edge); C and D are orthogonal to everything.
      bridges             3 rows between A[k] and B[k] at cosine 0.83 to the nearer and a little less to the other: each has one
                          edge into A, one into B and one to either other bridge, and leans to B, A, B.
      satellites          4 rows at 0.85 of C[0..3]: one edge each.
      hanger              s0 at 0.85 of D[0]; s1 at 0.85 of s0: s1's only edge is to s0.
      path                6 rows, each at 0.85 of the one before: edges between neighbours only (0.85^2 < 0.8).
      pair                two identical rows.
      background          standard normal rows (pairwise cosine about 0.04), the first a zero row and the second a row with one NaN.
    Every row is scaled by a power of two of its own (cosine does not see it), then all are scattered by a fixed permutation.
    Returns (rows, groups): ``groups`` is a dict of the planted members' positions, in the order they were built."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((512, 120)))
    d = iter(q.T)
    nxt = lambda: next(d)                                    # noqa: E731  (a fresh orthonormal direction)
    unit = lambda v: v / np.sqrt((v * v).sum(-1, keepdims=True))      # noqa: E731
    cA = nxt()
    cB = RHO * cA + np.sqrt(1 - RHO * RHO) * nxt()
    cC = nxt()
    cD = nxt()
    fam = {k: np.stack([unit(c + (EPS + 0.004 * j) * nxt()) for j in range(FAMILY)]) for k, c in zip("ABCD", (cA, cB, cC, cD))}
    bridges = []
    for k, w in enumerate((1.04, 0.96, 1.02)):               # lean to B, to A, to B
        b = unit(fam["A"][k] + w * fam["B"][k])
        g = 0.83 / max(b @ fam["A"][k], b @ fam["B"][k])
        bridges.append(g * b + np.sqrt(1 - g * g) * nxt())
    c85 = np.sqrt(1 - 0.85 ** 2)
    satellites = [0.85 * fam["C"][k] + c85 * nxt() for k in range(4)]
    s0 = 0.85 * fam["D"][0] + c85 * nxt()
    s1 = 0.85 * s0 + c85 * nxt()                             # hangs on the border row s0
    path = [nxt()]
    for _ in range(5):
        path.append(0.85 * path[-1] + c85 * nxt())
    t = nxt()
    parts = [("familyA", fam["A"]), ("familyB", fam["B"]), ("familyC", fam["C"]), ("familyD", fam["D"]), ("bridges", np.stack(bridges)),
             ("satellites", np.stack(satellites)), ("hanger", np.stack([s0, s1])), ("path", np.stack(path)), ("pair", np.stack([t, t]))]
    background = rng.standard_normal((n - PLANTED, 512))
    r = np.concatenate([p for _, p in parts] + [background])
    assert r.shape == (n, 512)
    r = (r * np.exp2(rng.integers(-3, 4, (n, 1)))).astype(np.float32)
    r[PLANTED] = 0
    r[PLANTED + 1, 77] = np.nan
    perm = rng.permutation(n)
    where = np.empty(n, np.int64)
    where[perm] = np.arange(n)                               # row i of r lands at where[i]
    groups, o = {}, 0
    for name, p in parts:
        groups[name] = where[o:o + len(p)]
        o += len(p)
    groups["zero"], groups["nan"] = where[PLANTED:PLANTED + 1], where[PLANTED + 1:PLANTED + 2]
    return np.ascontiguousarray(r[perm]), groups


def valid_sims64(r, metric="cosine"):
    """(valid bool (n,), sim float64 (n, n)) of float32 rows: the similarities of the valid rows, 0 wherever a row is not valid"""
    r = np.asarray(r, np.float32)
    valid = np.isfinite(r).all(axis=1)
    if metric == "cosine":
        valid &= (r != 0).any(axis=1)
    s = np.zeros((len(r), len(r)))
    ok = np.flatnonzero(valid)
    s[np.ix_(ok, ok)] = sims64(r[ok], r[ok], metric)
    return valid, s


def integer_rows():
    """200 rows of 0 / 1 (every dot is an exact integer, in any arithmetic), 20 copies of row 10 and two of row 3: the dots tie in
    hundreds, at the threshold and between anchors."""
    r = np.random.default_rng(12).integers(0, 2, (200, 512)).astype(np.float32)
    r[40:60] = r[10]
    r[150] = r[3]
    r[199] = r[3]
    return r


def integer_case():
    """(rows, dots float64, threshold, min_points) of the integer rows: the threshold is the 0.9 quantile of the pair dots (one of
    them), min_points the median degree + 1"""
    r = integer_rows()
    dots = sims64(r, r, "dot")
    pairs = np.sort(dots[np.triu_indices(len(r), 1)])
    threshold = float(pairs[int(0.9 * (len(pairs) - 1))])
    adj = dots >= threshold
    adj[np.arange(len(r)), np.arange(len(r))] = False
    return r, dots, threshold, int(np.median(adj.sum(axis=1))) + 1


def dbscan(adj, sim, min_points, valid=None):
    """Brute force: (label, degree, size, anchor int64; sim float64; kind uint8) of the graph ``adj`` (n, n) bool, symmetric, its
    diagonal ignored, with the edge values ``sim`` (n, n), symmetric; rows that are not ``valid`` have no edges.  Labels by
    propagation over the core rows: every core row starts as its own label and takes the smallest label among itself and its core
    neighbours until nothing changes.  Anchors by an explicit walk over the core neighbours in ascending order: a later one wins only
    when it is strictly more similar."""
    adj = np.array(adj, dtype=bool)
    n = len(adj)
    valid = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
    adj &= valid[:, None] & valid[None, :]
    adj[np.arange(n), np.arange(n)] = False
    degree = [int(adj[i].sum()) for i in range(n)]
    core = [bool(valid[i]) and degree[i] + 1 >= min_points for i in range(n)]
    label = [i if core[i] else -1 for i in range(n)]
    changed = True
    while changed:
        changed = False
        for i in range(n):
            if not core[i]:
                continue
            for j in np.flatnonzero(adj[i]):
                if core[j] and label[j] < label[i]:
                    label[i] = label[j]
                    changed = True
    anchor, best, kind = [-1] * n, [float("nan")] * n, [0] * n
    for i in range(n):
        if core[i]:
            anchor[i], kind[i] = i, 3
        elif valid[i]:
            kind[i] = 1
            for j in range(n):
                if adj[i, j] and core[j] and (anchor[i] < 0 or sim[i, j] > best[i]):
                    anchor[i], best[i], kind[i] = j, float(sim[i, j]), 2
            if anchor[i] >= 0:
                label[i] = label[anchor[i]]
    size = [sum(1 for j in range(n) if label[j] == label[i]) if label[i] >= 0 else 0 for i in range(n)]
    return (*(np.asarray(a, dtype=np.int64) for a in (label, degree, size, anchor)), np.asarray(best, dtype=np.float64),
            np.asarray(kind, dtype=np.uint8))


def second_gap(adj, sim, result):
    """For every border row with more than one core neighbour: the gap between its best and its second-best core neighbour's
    similarity.  Returns a float64 array (one entry per such row)."""
    label, degree, size, anchor, best, kind = result
    gaps = []
    for i in np.flatnonzero(kind == 2):
        near = np.flatnonzero(adj[i] & (kind == 3))
        if len(near) > 1:
            s = np.sort(sim[i, near])
            gaps.append(s[-1] - s[-2])
    return np.asarray(gaps, dtype=np.float64)


def same(got, want, sim_tol=0.0):
    """the six arrays: integers and kinds equal, dtypes as documented, NaN where NaN stands, ``sim`` within ``sim_tol``"""
    if len(got) != 6 or len(want) != 6:
        return False
    for k in (0, 1, 2, 3):
        if got[k].dtype != np.int64 or not np.array_equal(got[k], want[k]):
            return False
    if got[5].dtype != np.uint8 or not np.array_equal(got[5], want[5]):
        return False
    a, b = np.asarray(got[4], np.float64), np.asarray(want[4], np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    return bool((np.abs(a - b)[~np.isnan(a)] <= sim_tol).all())
