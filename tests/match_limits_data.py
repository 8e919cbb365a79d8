"""Inputs and comparison helpers that take the matches against a reference (gr_tile_kernel<., true> in gnn_graph.hip, NNEngine.match,
gnn_match_count* / gnn_match_fill*) to the limits tests/test_match_gpu.py stays away from.  The rows come from the generators of
tests/embedding_limits_data.py, tests/graph_limits_data.py, tests/neighbours_data.py and tests/clusters_data.py; the helpers are the
rectangle forms of those of tests/graph_limits_data.py - its band_rule, value_rule, band_counts and same_bits take any shape and are
used as they are -; what is made here is only what the rectangle needs on top of them:

  check_csr, dense,         a CSR by query row over (nq, nb): no `a < b`, (i, i) and both orientations are there
  exact_csr, check_exact
  integer_sides             the 342 signed integer rows split into 133 query and 209 base rows, with the negated row and its ties
  SCAN_CASES                n_query * splits at 1023, 1024 and 1026 against 342 base rows: the 1024 threads of nn_scan_kernel
  slab_queries              16454 query rows: more than one QSLAB = 16384 of the neighbour search, whose buffers the match fills with
                            ALL query rows at once
  two_range_sides           75 query rows against the 65350 rows of lim.capped_base: cnt[row * splits + 1], a segment that continues
                            from part 0 into part 1
  invalid_halves            old and new rows that each hold a zero row, a NaN row and an Inf row: GraphResult.extend

tests/test_match_limits_host.py shows that each helper rejects a wrong CSR."""
import numpy as np

from tests import embedding_limits_data as lim
from tests import graph_limits_data as gd
from tests.graph_limits_data import band_counts, band_rule, same_bits, threshold32, value_rule      # noqa: F401  (re-exported)
from tests.neighbours_data import rows, sims64

SHAPES = ((133, 333), (333, 133))
SCAN_BASE = gd.N_INTEGER
SCAN_CASES = ((341, 128, 1023), (256, 96, 1024), (342, 128, 1026))       # (query rows, debug split, n_query * splits)
N_QUERY_INTEGER = 133


# ---- the comparison helpers ----------------------------------------------------------------------------------------------------------

def check_csr(got, nq, nb):
    """a CSR by query row over (nq, nb) whose columns ascend within a row; returns (a, b)"""
    indptr, col, sim = got
    assert indptr.dtype == np.int64 and col.dtype == np.int32 and sim.dtype == np.float32
    assert indptr.shape == (nq + 1,) and indptr[0] == 0 and (np.diff(indptr) >= 0).all() and len(col) == len(sim) == indptr[-1]
    a = np.repeat(np.arange(nq, dtype=np.int64), np.diff(indptr))
    b = col.astype(np.int64)
    assert (b >= 0).all() and (b < max(nb, 1)).all()
    assert ((np.diff(b) > 0) | (np.diff(a) > 0)).all()
    return a, b


def dense(got, nq, nb):
    """(mask bool (nq, nb), values f32 (nq, nb), NaN where there is no match) of a CSR that passes check_csr"""
    a, b = check_csr(got, nq, nb)
    mask, val = np.zeros((nq, nb), bool), np.full((nq, nb), np.nan, np.float32)
    mask[a, b] = True
    val[a, b] = got[2]
    return mask, val


def rows_of(got, mine, nb):
    """(mask, values) of shape (len(mine), nb): the query rows ``mine`` of a match CSR, without making the whole rectangle dense"""
    indptr, col, sim = got
    mask, val = np.zeros((len(mine), nb), bool), np.full((len(mine), nb), np.nan, np.float32)
    for k, i in enumerate(mine):
        seg = slice(indptr[i], indptr[i + 1])
        assert (np.diff(col[seg]) > 0).all() and (col[seg] >= 0).all() and (col[seg] < nb).all()
        mask[k, col[seg]] = True
        val[k, col[seg]] = sim[seg]
    return mask, val


def check_band(got, s64, t):
    """band_rule and value_rule on a whole rectangle; returns the largest |sim - fp64|"""
    mask, val = dense(got, *s64.shape)
    band_rule(mask, s64, t)
    return value_rule(mask, val, s64)


def exact_csr(exact64, t, query_valid=None, base_valid=None):
    """the match CSR of an fp64 matrix of EXACT similarities (integer dots): ties on the threshold match, sim is the value as f32"""
    nq, nb = exact64.shape
    qok = np.ones(nq, bool) if query_valid is None else np.asarray(query_valid, bool)
    bok = np.ones(nb, bool) if base_valid is None else np.asarray(base_valid, bool)
    keep = (exact64 >= threshold32(t)) & qok[:, None] & bok[None, :]
    a, b = np.nonzero(keep)
    indptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    return indptr, b.astype(np.int32), exact64[a, b].astype(np.float32)


def check_exact(got, exact64, t, query_valid=None, base_valid=None):
    """all three arrays against exact fp64 similarities, sim by its bits; returns the number of matches"""
    check_csr(got, *exact64.shape)
    want = exact_csr(exact64, t, query_valid, base_valid)
    assert np.array_equal(got[0], want[0]), ("indptr", np.flatnonzero(got[0] != want[0])[:5].tolist())
    assert np.array_equal(got[1], want[1]), "col"
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), "sim"
    return len(want[1])


def without_rows(got, keep_q, keep_b, nq, nb):
    """the CSR of the query rows ``keep_q`` and base rows ``keep_b`` (both ascending) of a match CSR over (nq, nb) none of whose
    matches touches another row, renumbered"""
    a, b = check_csr(got, nq, nb)
    new_q, new_b = np.full(nq, -1, np.int64), np.full(max(nb, 1), -1, np.int64)
    new_q[keep_q] = np.arange(len(keep_q))
    new_b[keep_b] = np.arange(len(keep_b))
    assert (new_q[a] >= 0).all() and (new_b[b] >= 0).all()
    indptr = np.concatenate([[0], np.cumsum(np.diff(got[0])[keep_q])]).astype(np.int64)
    return indptr, new_b[b].astype(np.int32), got[2]


# ---- the inputs ------------------------------------------------------------------------------------------------------------------------

def signed_sides(nq, nb):
    """the first nq and the first nb of the 333 signed rows (tests/test_match_gpu.py's shapes: the pairs (i, i) are there, at 1), and
    their fp64 cosines"""
    r = gd.signed_base()
    q, b = np.ascontiguousarray(r[:nq]), np.ascontiguousarray(r[:nb])
    return q, b, sims64(q, b)


def band_is_narrow(s64, t):
    matches, band = band_counts(s64, t)
    return band <= gd.BAND_SHARE * matches


SLAB_THRESHOLD = 0.1
SLAB_BASE = 333


def slab_sample():
    """200 query rows of the 16454 that include the rows on both sides of the slab border and the last"""
    fixed = [0, 5, 100, lim.QSLAB - 1, lim.QSLAB, lim.QSLAB - 1 + 64, lim.NQ_SLABS - 1]
    more = np.random.default_rng(32).permutation(lim.NQ_SLABS)[:200 - len(fixed)]
    mine = np.unique(np.concatenate([fixed, more]))
    assert {lim.QSLAB - 1, lim.QSLAB, lim.NQ_SLABS - 1} <= set(mine.tolist()) and 190 <= len(mine) <= 200
    return mine


def integer_sides():
    """The 342 signed integer rows split at 133: query = rows 0 .. 132 (with row 3, its negation 77 and the copies of row 10), base =
    rows 133 .. 341 (with the copies of row 3 at 150 and 341) and, in front of them, rows 3 and 77 themselves: (query (133, 512),
    base (211, 512), dots float64).  The negated query 77 has the dot -dots[3, 3] with the base rows 0 (row 3), 19 (row 150) and 210."""
    r = lim.signed_integer_rows(gd.N_INTEGER)
    q = np.ascontiguousarray(r[:N_QUERY_INTEGER])
    b = np.ascontiguousarray(np.concatenate([r[[3, 77]], r[N_QUERY_INTEGER:]]))
    dots = q.astype(np.float64) @ b.astype(np.float64).T
    same = [0, 2 + 150 - N_QUERY_INTEGER, len(b) - 1]
    assert same == [0, 19, 210] and all(np.array_equal(b[j], r[3]) for j in same)
    assert (dots[77, same] == -dots[3, 0]).all() and dots[3, 0] > 0 and dots[77, 1] == dots[3, 0]
    assert (dots == np.round(dots)).all() and np.abs(dots).max() < 2 ** 24
    return q, b, dots


def integer_prefix(nq, nb):
    """query = the first nq of the 342 signed integer rows, base = the LAST nb of them reversed - rows that differ, so a wrong column
    has a wrong value - and their exact dots"""
    r = lim.signed_integer_rows(gd.N_INTEGER)
    q, b = np.ascontiguousarray(r[:nq]), np.ascontiguousarray(r[::-1][:nb])
    return q, b, q.astype(np.float64) @ b.astype(np.float64).T


def counters(nq, nb, split):
    """n_query * splits for a debug split > 0: what nn_tile_grid makes of it over the BASE - rounded up to 32 columns, at most SPLIT_MAX"""
    split_rows = min((split + 31) // 32 * 32, lim.SPLIT_MAX)
    return nq * ((nb + split_rows - 1) // split_rows)


def slab_queries():
    """lim.slab_rows(): 16454 signed rows, (rows, pairs, triple)"""
    return lim.slab_rows()


TWO_RANGE_THRESHOLD = 0.34        # 1824 matches of the 75 x 65350 pairs in fp64, one in the band, 57 in the second range


def two_range_sides():
    """(query (75, 512), base (65350, 512)): rows(70, 7) and eight times its rows 0 .. 4 - two tiles, the second with 11 rows -
    against lim.capped_base of the 70.  Queries i and 70 + i, i < 5, match base row CAPPED_PLANTS[i] at 1; query 5 matches both rows
    of CAPPED_TIE."""
    q70 = rows(70, 7)
    q = np.ascontiguousarray(np.concatenate([q70, q70[:5] * np.float32(8.0)]))
    base = lim.capped_base(q70)
    assert q.shape == (75, 512) and base.shape == (lim.NB_CAPPED, 512)
    return q, base


def invalid_halves(seed=71):
    """(old (200, 512), new (133, 512)) integer rows in [-4, 4), each half with a zero row, a NaN row and an Inf row: under dot every
    value is exact, under cosine the zero rows are invalid too.  The invalid rows sit on both sides of a 64-row tile border."""
    r = np.random.default_rng(seed).integers(-4, 4, (333, 512)).astype(np.float32)
    r[63] = 0
    r[64, 5] = np.nan
    r[130, 500] = np.inf
    r[200 + 0] = 0
    r[200 + 64, 0] = -np.inf
    r[200 + 132, 511] = np.nan
    return np.ascontiguousarray(r[:200]), np.ascontiguousarray(r[200:])
