"""Inputs that take the single-linkage tree (gnn_linkage.hip) to the limits its own tests never reach, each with its conditions asserted
on the CPU where it is made, and a plain Boruvka that counts rounds.  What each generator pins:

  corners        negative tree edges that a contest decides: the `u & 0x80000000 ? ~u` branch of lk_image under lk_shfl_xor, atomicMax
                 and both pick kernels, the host's sort of es[] and lk_value on a negative record
  simplex_star   every pair negative with many ties; a star, where all picks but one are not mutual, in one round
  ruler_path     a path of 2^m rows, tied throughout, that needs exactly m rounds, every component's pick mutual in every round
  dead_tiles     `if (okm == 0) return;` on a first tile without a valid row, `__all(cc < 0 ...) continue` on whole steps of invalid
                 columns, an invalid row 0 and an invalid last row
  forest_rows    valid rows all of whose pairs are NaN under dot: a forest, where the round that adds no edge ends the host's loop

The references are the numpy definition (sequence.single_linkage_tree) and the brute-force Kruskal of tests/linkage_data.py."""
import numpy as np

from genomad_amd import sequence
from tests.embedding_limits_data import signed_integer_rows
from tests.neighbours_data import DIM


# the first eight edges of extreme_base's tree under cosine: its one-hot rows (32..47) that share a position and a sign, at exactly 1
ONE_HOT_PAIRS = ((32, 40), (32, 41), (35, 42), (35, 43), (36, 44), (36, 45), (39, 46), (39, 47))


def dots64(r):
    r = np.asarray(r, np.float64)
    return r @ r.T


def boruvka(values, valid=None):
    """Plain Boruvka over the value matrix (read for i < j; NaN: no edge; -0 counts as +0) under the project's order - value
    descending, lo ascending, hi ascending: per round every component takes its best outgoing pair, then the picked pairs are joined.
    Returns (rounds that added an edge, the set of (lo, hi) taken)."""
    n = len(values)
    valid = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
    pairs = [(-(float(values[i, j]) + 0.0), i, j) for i in range(n) for j in range(i + 1, n)
             if valid[i] and valid[j] and values[i, j] == values[i, j]]
    comp, rounds, taken = list(range(n)), 0, set()
    while True:
        best = {}
        for key in pairs:
            if comp[key[1]] != comp[key[2]]:
                for c in (comp[key[1]], comp[key[2]]):
                    if c not in best or key < best[c]:
                        best[c] = key
        if not best:
            return rounds, taken
        rounds += 1
        for _, i, j in sorted(set(best.values())):
            assert comp[i] != comp[j]                    # a strict order: the picks of one round close no cycle
            taken.add((i, j))
            old, new = comp[j], comp[i]
            comp = [new if c == old else c for c in comp]


def corners(n=333, seed=71, K=16):
    """(n, 512) integer rows in four groups: columns 0..3 hold -K but 3K at the row's group, the rest integers of [-4, 4).  A dot
    within a group is 12 K^2 + noise, across groups -4 K^2 + noise: the tree's last three edges join the groups, are negative, and
    each is the best of thousands of negative cross pairs.  Asserted: exact dots, the sign gap, three negative edges at the end, each
    attained by one cross pair only.  Returns (rows, group)."""
    rng = np.random.default_rng(seed)
    r = np.zeros((n, DIM), np.float32)
    r[:, 4:] = rng.integers(-4, 4, (n, DIM - 4))
    g = rng.integers(0, 4, n)
    r[:, :4] = -K
    r[np.arange(n), g] = 3 * K
    dots = dots64(r)
    assert (dots == np.round(dots)).all() and np.abs(dots).max() < 2 ** 24
    lo, hi = np.triu_indices(n, 1)
    cross = g[lo] != g[hi]
    assert len(set(g)) == 4 and dots[lo, hi][cross].max() < 0 < dots[lo, hi][~cross].min()
    a, b, sim, valid = sequence.single_linkage_tree(r, "dot")
    assert len(a) == n - 1 and valid.all() and (sim[:-3] > 0).all() and (sim[-3:] < 0).all() and len(set(sim[-3:])) == 3
    for k in (-3, -2, -1):
        assert g[a[k]] != g[b[k]] and (dots[lo, hi][cross] == sim[k]).sum() == 1
    return r, g


def simplex_star(n=333, seed=72):
    """(n, 512) integer rows: row i is -1 in columns 0..n-1 but k[i] - 1 in column i, k of U{170..399}: the dot of i and j is
    n - k[i] - k[j], negative for every pair and tied wherever k repeats.  Every row's best partner is the row of smallest k: a star,
    which Boruvka finds in one round in which only the centre's own pick is mutual.  Returns (rows, centre)."""
    assert n <= DIM
    rng = np.random.default_rng(seed)
    k = rng.integers(170, 400, n)
    r = np.zeros((n, DIM), np.float32)
    r[:, :n] = -1
    r[np.arange(n), np.arange(n)] = k - 1
    dots = dots64(r)
    lo, hi = np.triu_indices(n, 1)
    assert np.array_equal(dots[lo, hi], (n - k[lo] - k[hi]).astype(np.float64)) and dots[lo, hi].max() <= -8
    centre = int(np.argmin(k))
    assert (k == k[centre]).sum() == 1
    a, b, sim, valid = sequence.single_linkage_tree(r, "dot")
    assert len(a) == n - 1 and valid.all() and (sim < 0).all() and len(set(sim)) <= 230 < n - 1      # k takes 230 values: ties
    assert ((a == centre) | (b == centre)).all()
    return r, centre


def ruler_path(n=256):
    """(n, 512) integer rows: row i has 1 in column i and 16 - tz(i + 1) in column i + 1 (tz: the trailing zero bits), so the dot
    of i and i + 1 is 16 - tz(i + 1) - the ruler sequence, 16 at every odd i + 1, 15 at 2 mod 4, ... - and every other pair is 0.
    The tree is the path; for n a power of two, round t joins the aligned blocks of 2^(t-1) rows in pairs, every pick mutual, and
    no round can do more: exactly log2 n rounds."""
    assert 2 <= n <= DIM
    r = np.zeros((n, DIM), np.float32)
    r[np.arange(n), np.arange(n)] = 1
    for i in range(n - 1):
        tz = ((i + 1) & -(i + 1)).bit_length() - 1
        r[i, i + 1] = 16 - tz
    dots = dots64(r)
    lo, hi = np.triu_indices(n, 1)
    near = hi - lo == 1
    assert (dots[lo, hi][~near] == 0).all() and dots[lo, hi][near].min() >= 9 and dots[lo, hi][near].max() == 16
    return r


DEAD_ROWS = np.concatenate([np.arange(64), np.arange(256, 512), [599]])


def dead_tiles():
    """signed_integer_rows(600, 11) with rows 0..63 (the whole first tile, row 0 included), 256..511 (four tiles, and whole
    256-column steps of every tile before them) and 599 (the last row) invalid: NaN at column 7, +inf at column 500 and -inf at
    column 0 in turn.  279 valid rows.  Returns (rows, invalid rows)."""
    r = signed_integer_rows(600, 11)
    for t, i in enumerate(DEAD_ROWS):
        col, v = ((7, np.nan), (500, np.inf), (0, -np.inf))[t % 3]
        r[i, col] = v
    ok = np.isfinite(r).all(axis=1)
    assert np.array_equal(np.flatnonzero(~ok), DEAD_ROWS) and int(ok.sum()) == 279 and not ok[:64].any() and not ok[599]
    return r, DEAD_ROWS.copy()


FOREST_OUT = np.concatenate([[0], np.arange(128, 192), [200, 332]])


def forest_rows():
    """The rows of ``corners`` with one element beyond the f16 range - 7e4 at column 5 and -7e4 at column 400 in turn - in rows 0,
    128..191 (a whole tile), 200 and 332: finite in f32, so the rows are valid, but each of their dots is NaN on the device, so they
    are isolated rows of a forest.  Returns (rows, out, keep)."""
    r, _ = corners()
    for t, i in enumerate(FOREST_OUT):
        if t % 2 == 0:
            r[i, 5] = 7e4
        else:
            r[i, 400] = -7e4
    keep = np.setdiff1d(np.arange(len(r)), FOREST_OUT)
    assert np.isfinite(r).all() and (np.abs(r[FOREST_OUT]).max(axis=1) > 65504).all() and np.abs(r[keep]).max() <= 48
    assert len(FOREST_OUT) == 67 and len(keep) == 266
    return r, FOREST_OUT.copy(), keep


def nan_rows_and_columns(values, out):
    """``values`` with the rows and columns ``out`` set to NaN: what the device's pair values are when those rows overflow"""
    s = np.array(values, copy=True)
    s[out, :] = np.nan
    s[:, out] = np.nan
    return s
