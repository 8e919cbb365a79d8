"""Inputs and comparison helpers that take the similarity graph (gnn_graph.hip, NNEngine.graph, gnn_graph_count* / gnn_graph_fill*) to
the limits tests/test_graph_gpu.py stays away from.  The rows come from the generators of tests/embedding_limits_data.py,
tests/neighbours_data.py and tests/clusters_data.py; what is made here is only what the graph needs on top of them:

  integer_base, PREFIXES,     342 signed integer rows (every dot exact) and the prefixes and debug splits that sit on the 32-column
  SCAN_CASES, counters        block, the 64-row tile, the 256-column step and the 1024 threads of nn_scan_kernel
  two_range_base              lim.capped_base with pairs planted across column 65280 = SPLIT_MAX: the second range of
                              gr_tile_kernel, `t.b1 > t.r0 + 1`, `max(b0, r0)`, cnt[row * splits + 1], a segment that continues
                              from part 0 into part 1
  complete_rows               333 copies of one row: the dense side of the changed-rows contract of gr_tile_kernel<true>

The helpers compare a CSR (indptr, col, sim) with fp64: exactly (check_exact, same_bits), or - where the threshold is not one of the
device's own values - by the band rule (band_rule: every pair at or above t + GAP is an edge, none below t - GAP is, the pairs between
are free) with the values within VALUE_TOL (value_rule).  tests/test_graph_limits_host.py shows that each helper rejects a wrong CSR.
VALUE_TOL and GAP are the neighbour tests'."""
import numpy as np

from tests import embedding_limits_data as lim
from tests.embedding_limits_data import GAP, VALUE_TOL
from tests.neighbours_data import rows, sims64

BAND_SHARE = 0.1          # the band may hold at most this share of the number of edges: asserted on the CPU for every band-rule input
SPLITS = (32, 100, 333, 4096, 0)          # tests/test_graph_gpu.py

SIGN_THRESHOLDS = (-0.05, 0.0, 0.05)
PREFIXES = (2, 31, 32, 33, 63, 64, 65, 255, 256, 257)
PREFIX_SPLITS = (0, 32, 64, 96)
SCAN_THREADS = 1024       # gnn_neighbours.hip
SCAN_CASES = ((341, 128, 1023), (256, 64, 1024), (342, 128, 1026))       # (rows, debug split, n * splits)
N_INTEGER = 342

TWO_RANGE_THRESHOLD = 0.55
TWO_RANGE_SPLITS = (0, 40000, lim.SPLIT_MAX)
COPIES_OF = 100
COPIES = (40000, lim.SPLIT_MAX - 1, lim.SPLIT_MAX + 1)
# (i, j, j's multiple of i): across column 65280 from tile 0, from the last row of range 0 to the last row of all, inside the second
# range in the tile whose first row is 65280
PLANTS = ((5, lim.SPLIT_MAX, 2.0), (lim.SPLIT_MAX - 1, lim.NB_CAPPED - 1, 0.5), (lim.SPLIT_MAX + 10, lim.SPLIT_MAX + 20, 1.0))


def threshold32(t):
    """the threshold as the device compares it"""
    return float(np.float32(t))


def upper64(r, metric="cosine"):
    """(n, n) fp64 similarities of the rows, -inf on and below the diagonal: only the pairs i < j can be edges"""
    s = sims64(r, r, metric)
    s[np.tril_indices(len(r))] = -np.inf
    return s


def band_counts(s64, t):
    """(pairs at or above the threshold, pairs inside [t - GAP, t + GAP)) of an fp64 matrix whose excluded pairs are -inf"""
    t = threshold32(t)
    return int((s64 >= t).sum()), int(((s64 >= t - GAP) & (s64 < t + GAP)).sum())


def band_is_narrow(s64, t):
    edges, band = band_counts(s64, t)
    return band <= BAND_SHARE * edges


# ---- the comparison helpers --------------------------------------------------------------------------------------------------------

def same_bits(got, want):
    """(indptr, col, sim) of the right dtypes, equal bit for bit (tests/test_graph_gpu.py)"""
    return (got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.float32 and len(got) == len(want) == 3
            and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            and np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)))


def check_csr(got, n):
    """a CSR over the upper triangle of n rows whose columns ascend within a row; returns (a, b)"""
    indptr, col, sim = got
    assert indptr.dtype == np.int64 and col.dtype == np.int32 and sim.dtype == np.float32
    assert indptr.shape == (n + 1,) and indptr[0] == 0 and (np.diff(indptr) >= 0).all() and len(col) == len(sim) == indptr[-1]
    a = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    b = col.astype(np.int64)
    assert (a < b).all() and (b < n).all()
    assert ((np.diff(b) > 0) | (np.diff(a) > 0)).all()
    return a, b


def dense(got, n):
    """(mask bool (n, n), values f32 (n, n), NaN where there is no edge) of a CSR that passes check_csr"""
    a, b = check_csr(got, n)
    mask, val = np.zeros((n, n), bool), np.full((n, n), np.nan, np.float32)
    mask[a, b] = True
    val[a, b] = got[2]
    return mask, val


def touching(got, mine, n):
    """the edges of a CSR over n rows that touch the rows ``mine``, as row or as column: (mask, values) of shape (len(mine), n)"""
    a, b = check_csr(got, n)
    mine = np.asarray(mine, np.int64)
    at = np.full(n, -1, np.int64)
    at[mine] = np.arange(len(mine))
    mask, val = np.zeros((len(mine), n), bool), np.full((len(mine), n), np.nan, np.float32)
    for own, other in ((a, b), (b, a)):
        hit = at[own] >= 0
        mask[at[own[hit]], other[hit]] = True
        val[at[own[hit]], other[hit]] = got[2][hit]
    return mask, val


def band_rule(mask, s64, t):
    """The edge set against fp64 where the threshold is not one of the device's values (check_sets of the neighbour tests carried
    over): every pair at or above t + GAP is an edge, none below t - GAP is (an excluded pair is -inf), the band is free."""
    t = threshold32(t)
    assert mask.shape == s64.shape
    missing, extra = ~mask & (s64 >= t + GAP), mask & (s64 < t - GAP)
    assert not missing.any(), ("left out", np.argwhere(missing)[:5].tolist())
    assert not extra.any(), ("let in", np.argwhere(extra)[:5].tolist())


def value_rule(mask, val, s64):
    """Every returned sim within VALUE_TOL of the fp64 value of its pair, and +0 where fp64 is exactly zero.  Returns the largest
    error (0 without an edge)."""
    assert not np.isnan(val[mask]).any() and np.isnan(val[~mask]).all()
    if not mask.any():
        return 0.0
    err = np.abs(val[mask].astype(np.float64) - s64[mask])
    assert err.max() <= VALUE_TOL, (float(err.max()), np.argwhere(mask)[int(np.argmax(err))].tolist())
    zero = mask & (s64 == 0)
    assert (val[zero].view(np.uint32) == 0).all(), "a zero that is not +0"
    return float(err.max())


def check_band(got, s64, t):
    """band_rule and value_rule on a whole graph; returns the largest |sim - fp64|"""
    mask, val = dense(got, len(s64))
    band_rule(mask, s64, t)
    return value_rule(mask, val, s64)


def exact_csr(exact64, t, valid=None):
    """the CSR of an fp64 matrix of EXACT similarities (integer dots): ties on the threshold are edges, sim is the value as f32"""
    n = len(exact64)
    ok = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
    keep = np.triu((exact64 >= threshold32(t)) & ok[:, None] & ok[None, :], 1)
    a, b = np.nonzero(keep)
    indptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    return indptr, b.astype(np.int32), exact64[a, b].astype(np.float32)


def check_exact(got, exact64, t, valid=None):
    """all three arrays against exact fp64 similarities, sim by its bits; returns the number of edges"""
    check_csr(got, len(exact64))
    want = exact_csr(exact64, t, valid)
    assert np.array_equal(got[0], want[0]), ("indptr", np.flatnonzero(got[0] != want[0])[:5].tolist())
    assert np.array_equal(got[1], want[1]), "col"
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), "sim"
    return len(want[1])


def renumbered(got, keep, n):
    """the CSR of the rows ``keep`` (ascending) of a CSR over n rows none of whose edges touches another row, renumbered 0 .. len(keep)"""
    a, b = check_csr(got, n)
    new = np.full(n, -1, np.int64)
    new[keep] = np.arange(len(keep))
    assert (new[a] >= 0).all() and (new[b] >= 0).all()
    indptr = np.concatenate([[0], np.cumsum(np.diff(got[0])[keep])]).astype(np.int64)
    return indptr, new[b].astype(np.int32), got[2]


# ---- the inputs --------------------------------------------------------------------------------------------------------------------

def signed_base():
    return lim.signed_rows(333, 8)


def integer_base():
    """the 342 signed integer rows of groups A and B and their exact dots"""
    r = lim.signed_integer_rows(N_INTEGER)
    return r, r.astype(np.float64) @ r.astype(np.float64).T


def counters(n, split):
    """n * splits for a debug split > 0: what nn_tile_grid makes of it - rounded up to 32 columns, at most SPLIT_MAX"""
    split_rows = min((split + 31) // 32 * 32, lim.SPLIT_MAX)
    return n * ((n + split_rows - 1) // split_rows)


def two_range_base():
    """(65350, 512): lim.capped_base(rows(70, 7)) - one full range of 65280 columns and 70 more - with row COPIES_OF copied to COPIES
    and the power-of-two multiples PLANTS.  Returns (base, pairs): every planted pair (i, j), i < j, whose cosine is 1.  Asserted: the
    multiples are exact, the planted rows are plain rows of the base, and where each pair lies."""
    base = lim.capped_base(rows(70, 7))
    assert base.shape == (lim.NB_CAPPED, 512) and lim.NB_CAPPED == 65350 and lim.SPLIT_MAX == 65280
    assert not {PLANTS[0][0], PLANTS[2][0], COPIES_OF} & (set(lim.CAPPED_PLANTS) | set(lim.CAPPED_TIE))      # plain rows are multiplied
    for at in COPIES:                                              # first: row 65279 is a copy before its own multiple is made
        base[at] = base[COPIES_OF]
    for i, j, m in PLANTS:
        base[j] = base[i] * np.float32(m)
        assert np.array_equal(base[j].astype(np.float64), base[i].astype(np.float64) * m) and np.abs(base[i]).max() > 0
    (i0, j0, _), (i1, j1, _), (i2, j2, _) = PLANTS
    assert i0 < 64 and j0 == lim.SPLIT_MAX                         # tile 0 reaches the first column of the second range
    assert i1 == lim.SPLIT_MAX - 1 and j1 == lim.NB_CAPPED - 1     # the last row of range 0, the last row of all
    assert i2 // 64 * 64 == lim.SPLIT_MAX and lim.SPLIT_MAX < i2 < j2      # both in the tile whose first row is 65280
    assert COPIES_OF < COPIES[0] < COPIES[1] == lim.SPLIT_MAX - 1 < lim.SPLIT_MAX < COPIES[2]      # part 0, part 0, part 1
    chain = (COPIES_OF,) + COPIES + (j1,)                          # row 65349 is half of a copy: the same direction
    pairs = [(i0, j0), (i2, j2)] + [(a, b) for k, a in enumerate(chain) for b in chain[k + 1:]]
    return base, pairs


def two_range_mine():
    """the 75 rows of the `capped` fixture of tests/test_embedding_limits_gpu.py: the last 70 rows and the plants"""
    mine = np.concatenate([np.arange(lim.NB_CAPPED - 70, lim.NB_CAPPED), lim.CAPPED_PLANTS[:3], lim.CAPPED_TIE])
    assert len(set(mine)) == len(mine) == 75
    return mine


def touching_counts(s64, mine, t):
    """Of the fp64 similarities (len(mine), n) of the rows ``mine`` to all rows (the own pair -inf): the entries at or above the
    threshold (a pair of two of these rows stands twice), the entries in the band, the unordered pairs at or above the threshold and
    those of them whose column - the larger row - lies in the second range."""
    t = threshold32(t)
    mine = np.asarray(mine)
    other = np.arange(s64.shape[1])[None, :]
    once = ~(np.isin(other, mine) & (other < mine[:, None]))      # a pair of two of these rows counts at its smaller row
    edge = s64 >= t
    second = once & edge & (np.maximum(other, mine[:, None]) >= lim.SPLIT_MAX)
    return int(edge.sum()), int(((s64 >= t - GAP) & (s64 < t + GAP)).sum()), int((once & edge).sum()), int(second.sum())


def complete_rows(r, n=333):
    """n copies of one valid row: its graph is complete at any threshold up to 1 - VALUE_TOL"""
    return np.ascontiguousarray(np.tile(r[:1], (n, 1)))
