"""Inputs and an exact oracle that take the density clusters (gnn_density.hip, NNEngine.density) to the limits tests/test_density_gpu.py
stays away from.  The rows come from the generators of tests/embedding_limits_data.py, tests/graph_limits_data.py and
tests/neighbours_data.py; what is made here is only what density needs on top of them:

  density_of_graph            DBSCAN by this project's rules from an upper-triangle CSR, with numpy in O(edges): the edges and values
                              of density are by construction those of the graph, so engine.density(r, t, m) must equal
                              density_of_graph(*engine.graph(r, t), valid, m) on ANY input, bit for bit - dense random graphs included,
                              which no fp64 reference can decide
  border_contest              integer rows under dot whose border rows' best core neighbour has a similarity <= 0: the `u >> 31`
                              branch of nn_image / nn_unimage, `s + 0.f`, ties on a negative key, 0 against negative rivals
  chain_case                  2176 rows: a path of 511 rows scattered over all 34 tiles (nn_root on a deep tree, cl_join through
                              top[]) and, at the debug split 32, 2312 (tile, range) flags - more than rows - with core-core edges in
                              workgroups whose flag lies beyond n
  signed_case, prefixes       dense signed graphs; n on and beside the 32-column block, the 64-row tile and the 256-column step
  two_range_case              65350 rows: a second base range, border rows whose core neighbours lie in the other range or in both,
                              clusters whose core rows lie in both

tests/test_density_limits_host.py shows that the oracle agrees with sequence.density_clusters and with density_data.dbscan and that
the comparison rejects a result that is wrong in one place."""
import numpy as np

from tests import embedding_limits_data as lim
from tests import graph_limits_data as gd
from tests.embedding_limits_data import GAP
from tests.neighbours_data import DIM, sims64

KIND_INVALID, KIND_NOISE, KIND_BORDER, KIND_CORE = 0, 1, 2, 3
FIELDS = ("label", "degree", "size", "anchor", "sim", "kind")


# ---- the exact oracle ------------------------------------------------------------------------------------------------------------------

def components(n, a, b):
    """int64 (n,): the smallest index of every row's component under the edges (a[e], b[e]).  Minimum-label propagation with pointer
    jumping: lab[i] is always a row of i's component with lab[i] <= i; a pass takes the minimum over the neighbours, then follows the
    labels' own labels.  Ends: a pass that changes nothing leaves every edge with equal labels at both ends, and the smallest row of a
    component can only be its own label."""
    lab = np.arange(n, dtype=np.int64)
    while len(a):
        new = lab.copy()
        np.minimum.at(new, a, lab[b])
        np.minimum.at(new, b, lab[a])
        while True:                                               # ends: labels only fall, and are bounded below by 0
            hop = new[new]
            if np.array_equal(hop, new):
                break
            new = hop
        if np.array_equal(new, lab):
            break
        lab = new
    return lab


def density_of_graph(indptr, col, sim, valid, min_points):
    """(label, degree, size, anchor int64; sim float32; kind uint8) of the graph given as an upper-triangle CSR (row i owns its
    partners j > i) with the f32 value of every edge: core = valid and degree + 1 >= min_points; clusters = the components of the
    core rows under core-core edges, named by their smallest row; a valid row that is not core takes the core neighbour of the largest
    f32 value as its anchor, among equals the smallest index (-0 equals +0, and the value goes out as +0); the others are noise."""
    indptr, col = np.asarray(indptr, np.int64), np.asarray(col, np.int64)
    sim = np.asarray(sim, np.float32)
    valid = np.asarray(valid, bool)
    n = len(indptr) - 1
    a = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    b = col
    degree = (np.bincount(a, minlength=n) + np.bincount(b, minlength=n)).astype(np.int64)
    core = valid & (degree + 1 >= int(min_points))
    both = core[a] & core[b]
    comp = components(n, a[both], b[both])
    label = np.where(core, comp, -1).astype(np.int64)
    anchor = np.where(core, np.arange(n), -1).astype(np.int64)
    best = np.full(n, np.nan, np.float32)
    kind = np.where(core, KIND_CORE, np.where(valid, KIND_NOISE, KIND_INVALID)).astype(np.uint8)
    # a row that is not core and its core neighbours, in both orientations of the CSR
    up, down = ~core[a] & core[b], core[a] & ~core[b]
    row = np.concatenate([a[up], b[down]])
    near = np.concatenate([b[up], a[down]])
    value = np.concatenate([sim[up], sim[down]]) + np.float32(0)          # -0 + 0 = +0
    order = np.lexsort((near, -value, row))                       # by row, then the f32 value descending, then the neighbour ascending
    row, near, value = row[order], near[order], value[order]
    first = np.flatnonzero(np.diff(row, prepend=-1) != 0)
    anchor[row[first]] = near[first]
    best[row[first]] = value[first]
    label[row[first]] = comp[near[first]]
    kind[row[first]] = KIND_BORDER
    size = np.zeros(n, np.int64)
    has = label >= 0
    size[has] = np.bincount(label[has], minlength=n)[label[has]]
    return label, degree, size, anchor, best, kind


def as_device(want):
    """the six arrays of sequence.density_clusters or density_data.dbscan with ``sim`` as the device returns it: float32"""
    label, degree, size, anchor, sim, kind = want
    return label, degree, size, anchor, np.asarray(sim).astype(np.float32), kind


def check_same(got, want, what=""):
    """The six arrays with no margin: the integers and kinds equal, ``sim`` float32, NaN at the same rows and the same bits elsewhere."""
    assert len(got) == len(want) == 6
    for k, x, y in zip(FIELDS, got, want):
        assert x.shape == y.shape, (what, k)
        if k == "sim":
            assert x.dtype == np.float32 and y.dtype == np.float32, (what, k)
            assert np.array_equal(np.isnan(x), np.isnan(y)), (what, k, np.flatnonzero(np.isnan(x) != np.isnan(y))[:10].tolist())
            ok = ~np.isnan(x)
            differ = x[ok].view(np.uint32) != y[ok].view(np.uint32)
            assert not differ.any(), (what, k, np.flatnonzero(ok)[differ][:10].tolist())
        else:
            assert x.dtype == (np.uint8 if k == "kind" else np.int64), (what, k)
            assert np.array_equal(x, y), (what, k, np.flatnonzero(x != y)[:10].tolist())


def counts(kind):
    """(core, border, noise, invalid)"""
    return tuple(int((kind == k).sum()) for k in (KIND_CORE, KIND_BORDER, KIND_NOISE, KIND_INVALID))


# ---- border rows whose best similarity is negative or zero ---------------------------------------------------------------------------

CONTEST_N, CONTEST_MIN_POINTS = 200, 20
CONTEST_CORES = (0, 70, 130)                                      # A, B, C
CONTEST_MEMBERS = (7, 40, 63, 64, 65, 100, 127, 128, 129, 150, 160, 170, 180, 190, 198, 199)
CONTEST_ANCHORS = (1, 2, 0, 0, 0, 1, 2, 0)                        # per pattern: B, C, A, A, A, B, C, A
CONTEST_SIMS = (-1.0, -3.0, -4.0, -8.0, 0.0, 0.0, -7.0, -4.0)


def border_contest():
    """200 integer rows for dot at lim.CONTEST_THRESHOLD = -10 and min_points 20.  A bulk of 181 rows e0 + 0/1 on the coordinates 10
    and up (pairwise dots >= 1: a clique); three rows A = e0 + 4 e1, B = e0 - 4 e1 + e2, C = e0 - 3 e1 - 23 e2 + e3 with dot 1 to
    the bulk and -15, -11, -10 to each other: core; 16 members m = -16 e0 + x e1 + y e2 + z e3 whose dots with (A, B, C) cycle
    through lim.CONTEST_PATTERNS and whose dot with every bulk row is -16: their edges are those to each other and to one to three
    of A, B, C, so they are border rows whose every core neighbour has a similarity <= 0.  Returns (rows, dots float64, want):
    ``want`` maps a member to (anchor, sim).  The conditions are asserted from the fp64 dots."""
    n, t = CONTEST_N, lim.CONTEST_THRESHOLD
    rng = np.random.default_rng(21)
    r = np.zeros((n, DIM), np.float32)
    r[:, 0] = 1
    r[:, 10:] = rng.integers(0, 2, (n, DIM - 10))
    for i, v in zip(CONTEST_CORES, ((1, 4, 0, 0), (1, -4, 1, 0), (1, -3, -23, 1))):
        r[i] = 0
        r[i, :4] = v
    want = {}
    for k, i in enumerate(CONTEST_MEMBERS):
        da, db, dc = lim.CONTEST_PATTERNS[k % len(lim.CONTEST_PATTERNS)]
        assert (da + 16) % 4 == 0
        x = (da + 16) // 4
        y = db + 16 + 4 * x
        z = dc + 16 + 3 * x + 23 * y
        r[i] = 0
        r[i, :4] = -16, x, y, z
        want[i] = (CONTEST_CORES[CONTEST_ANCHORS[k % 8]], CONTEST_SIMS[k % 8])
    dots = r.astype(np.float64) @ r.astype(np.float64).T
    assert (r == np.round(r)).all() and np.abs(r).max() <= 2048
    assert (dots == np.round(dots)).all() and np.abs(dots).max() < 2 ** 24
    a, b, c = CONTEST_CORES
    assert (dots[a, b], dots[a, c], dots[b, c]) == (-15, -11, -10)
    members = np.asarray(CONTEST_MEMBERS)
    bulk = np.setdiff1d(np.arange(n), np.concatenate([members, CONTEST_CORES]))
    assert len(bulk) == 181 and (dots[np.ix_(members, bulk)] == -16).all()
    adj = dots >= t
    adj[np.arange(n), np.arange(n)] = False
    degree = adj.sum(axis=1)
    assert (degree[bulk] == 183).all() and (degree[list(CONTEST_CORES)] >= 181).all()
    assert 16 <= degree[members].min() and degree[members].max() <= 18 < CONTEST_MIN_POINTS - 1
    ties = zero_against_negative = 0
    for k, i in enumerate(CONTEST_MEMBERS):
        pattern = lim.CONTEST_PATTERNS[k % 8]
        assert tuple(dots[i, list(CONTEST_CORES)]) == pattern
        cand = [(d, -j) for d, j in zip(pattern, CONTEST_CORES) if d >= t]
        d, j = max(cand)
        assert (-j, d) == want[i] and d <= 0
        vals = [v for v, _ in cand]
        ties += d < 0 and vals.count(d) == 2 and -j == min(-q for v, q in cand if v == d)
        zero_against_negative += d == 0 and min(vals) < 0
    assert ties >= 2 and zero_against_negative >= 2
    anchors = np.array([want[i][0] for i in CONTEST_MEMBERS])
    assert (anchors < members).any() and (anchors > members).any()        # as a column's core row and as a row's core column
    return r, dots, want


# ---- a deep tree, and more flags than rows ---------------------------------------------------------------------------------------------

CHAIN_N, CHAIN_PATH, CHAIN_MIN_POINTS, CHAIN_THRESHOLD, CHAIN_SPLIT = 2176, 511, 3, 1.0, 32


def chain_case(n=CHAIN_N, seed=81):
    """n rows for dot at the threshold 1 and min_points 3: rows 0 .. 510 are e_i + e_{i + 1} - a path whose neighbours have dot 1 and
    whose other pairs have 0 -, every further row i is -2 e_{(i - 511) mod 512}: cliques of 3 or 4 rows with dot 4, and <= 0 to the
    path.  All are scattered by one fixed permutation, so the path's tree crosses every tile.  Returns (rows, where, edges): row i of
    the construction stands at where[i]; ``edges`` are the (a, b), a < b, of the scattered rows.  Asserted: at the debug split 32 there
    are more flags than rows, and at least 5 core-core edges lie in a workgroup whose flag index is >= n."""
    assert n > CHAIN_PATH + 3 * 512
    r = np.zeros((n, DIM), np.float32)
    i = np.arange(CHAIN_PATH)
    r[i, i] = 1
    r[i, i + 1] = 1
    j = np.arange(CHAIN_PATH, n)
    r[j, (j - CHAIN_PATH) % 512] = -2
    perm = np.random.default_rng(seed).permutation(n)
    where = np.empty(n, np.int64)
    where[perm] = np.arange(n)
    r = np.ascontiguousarray(r[perm])
    dots = r.astype(np.float64) @ r.astype(np.float64).T
    a, b = np.nonzero(np.triu(dots >= CHAIN_THRESHOLD, 1))
    degree = np.bincount(a, minlength=n) + np.bincount(b, minlength=n)
    core = degree + 1 >= CHAIN_MIN_POINTS
    path = where[:CHAIN_PATH]
    assert (degree[path[1:-1]] == 2).all() and (degree[path[[0, -1]]] == 1).all() and core[where[CHAIN_PATH:]].all()
    pad_degree = degree[where[CHAIN_PATH:]]
    assert ((pad_degree == 2).sum(), (pad_degree == 3).sum()) == (1149, 516) or n != CHAIN_N
    tiles, ranges = (n + 63) // 64, (n + CHAIN_SPLIT - 1) // CHAIN_SPLIT
    if n == CHAIN_N:
        assert (tiles, ranges, tiles * ranges) == (34, 68, 2312) and tiles * ranges > n
        beyond = core[a] & core[b] & ((a // 64) * ranges + b // CHAIN_SPLIT >= n)
        assert beyond.sum() >= 5, int(beyond.sum())
    return r, where, (a, b)


# ---- dense signed graphs, prefixes -----------------------------------------------------------------------------------------------------

def signed_case():
    return gd.signed_base()


def quartile_min_points(degree):
    """three min_points from the graph's own degrees: the quartiles + 1"""
    q = np.sort(np.asarray(degree))[[len(degree) // 4, len(degree) // 2, 3 * len(degree) // 4]]
    return tuple(int(x) + 1 for x in q)


def prefix(n):
    """(rows, dots float64) of the first n of the 342 signed integer rows"""
    r = np.ascontiguousarray(lim.signed_integer_rows(gd.N_INTEGER)[:n])
    return r, r.astype(np.float64) @ r.astype(np.float64).T


def median_min_points(dots, t):
    adj = dots >= gd.threshold32(t)
    adj[np.arange(len(dots)), np.arange(len(dots))] = False
    return int(np.median(adj.sum(axis=1))) + 1


# ---- two ranges --------------------------------------------------------------------------------------------------------------------------

TWO_RANGE_MIN_POINTS = 5
FAMILY = 5
# where the plants stand: families of 5 mutually similar rows, all of range 0, all of range 1, and across both; the border rows
TWO_RANGE_ROWS = {
    "family0": (1000, 20000, 33000, 50000, 65000),
    "family1": (65310, 65311, 65312, 65313, 65314),
    "family2": (3, 45000, 65270, 65285, 65340),
    "low_to_high": 2000,          # range 0; its only core neighbour is family1[0]
    "high_to_low": 65330,         # range 1; its only core neighbour is family0[0]
    "low_both": 3000,             # range 0; best family1[1] (range 1), second best family0[1] (range 0)
    "high_both": 65320,           # range 1; best family0[2] (range 0), second best family1[2] (range 1)
}
FAMILY_SPREAD = 0.8               # members are unit(centre + 0.8 fresh): pairwise cosine 1 / 1.64 = 0.61
NEAR, BEST, SECOND = 0.75, 0.62, 0.58


def two_range_case():
    """gd.two_range_base() with planted density structure for min_points 5 at gd.TWO_RANGE_THRESHOLD = 0.55.  The plants are signed
    rows built from orthonormal directions - far from the non-negative rows of the base - so their edges are the planted ones, and
    that is asserted in fp64 against all 65350 rows with GAP to the threshold: a (plants x 65350) product.  Returns (base, plants):
    ``plants`` maps the names of TWO_RANGE_ROWS to rows, plus "expect": {border row: (anchor, second-best core neighbour or None)}."""
    base, _ = gd.two_range_base()
    n, t = len(base), gd.threshold32(gd.TWO_RANGE_THRESHOLD)
    taken = {gd.COPIES_OF, *gd.COPIES, *lim.CAPPED_PLANTS, *lim.CAPPED_TIE, *(x for i, j, _ in gd.PLANTS for x in (i, j))}
    mine = [x for v in TWO_RANGE_ROWS.values() for x in (v if isinstance(v, tuple) else (v,))]
    assert len(set(mine)) == len(mine) == 19 and not set(mine) & taken
    rng = np.random.default_rng(91)
    q, _ = np.linalg.qr(rng.standard_normal((DIM, 40)))
    d = iter(q.T)
    unit = lambda v: v / np.sqrt((v * v).sum())                   # noqa: E731
    fam = {}
    for name in ("family0", "family1", "family2"):
        c = next(d)
        fam[name] = [unit(c + FAMILY_SPREAD * next(d)) for _ in range(FAMILY)]
        for at, v in zip(TWO_RANGE_ROWS[name], fam[name]):
            base[at] = v.astype(np.float32)
    rest = lambda *c: np.sqrt(1 - sum(x * x for x in c))         # noqa: E731
    base[TWO_RANGE_ROWS["low_to_high"]] = (NEAR * fam["family1"][0] + rest(NEAR) * next(d)).astype(np.float32)
    base[TWO_RANGE_ROWS["high_to_low"]] = (NEAR * fam["family0"][0] + rest(NEAR) * next(d)).astype(np.float32)
    base[TWO_RANGE_ROWS["low_both"]] = (BEST * fam["family1"][1] + SECOND * fam["family0"][1] + rest(BEST, SECOND) * next(d)).astype(np.float32)
    base[TWO_RANGE_ROWS["high_both"]] = (BEST * fam["family0"][2] + SECOND * fam["family1"][2] + rest(BEST, SECOND) * next(d)).astype(np.float32)
    f0, f1 = TWO_RANGE_ROWS["family0"], TWO_RANGE_ROWS["family1"]
    expect = {TWO_RANGE_ROWS["low_to_high"]: (f1[0], None), TWO_RANGE_ROWS["high_to_low"]: (f0[0], None),
              TWO_RANGE_ROWS["low_both"]: (f1[1], f0[1]), TWO_RANGE_ROWS["high_both"]: (f0[2], f1[2])}
    # ---- fp64 against all rows: the planted edges and no other, each GAP away from the threshold
    mine = np.asarray(mine)
    s = lim.self64(base, mine)
    assert ((s >= t + GAP) | (s < t - GAP)).all()
    edge = s >= t
    at = {int(x): k for k, x in enumerate(mine)}
    for name in ("family0", "family1", "family2"):
        members = TWO_RANGE_ROWS[name]
        hangers = {y for pair in expect.values() for y in pair if y in members}
        for x in members:
            partners = set(np.flatnonzero(edge[at[x]]).tolist())
            assert set(members) - {x} <= partners and partners - set(members) <= set(expect), (name, x)
            assert FAMILY - 1 <= len(partners) and (x in hangers) == (len(partners) > FAMILY - 1)      # degree >= 4: core at 5
    for x, (best, second) in expect.items():
        partners = np.flatnonzero(edge[at[x]])
        assert set(partners.tolist()) == {best} | ({second} if second is not None else set()), x      # degree <= 2: not core at 5
        if second is not None:
            assert s[at[x], best] > s[at[x], second] + 10 * GAP and (best >= lim.SPLIT_MAX) != (second >= lim.SPLIT_MAX)
        assert (best >= lim.SPLIT_MAX) != (x >= lim.SPLIT_MAX) and abs(s[at[x], best] - (NEAR if second is None else BEST)) < 1e-6
    low = [x for x in TWO_RANGE_ROWS["family2"] if x < lim.SPLIT_MAX]
    assert len(low) == 3 and all(x < lim.SPLIT_MAX for x in f0) and all(x >= lim.SPLIT_MAX for x in f1)
    plants = dict(TWO_RANGE_ROWS)
    plants["expect"] = expect
    return base, plants
