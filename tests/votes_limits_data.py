"""Inputs that take label transfer (gnn_votes.hip) to the limits tests/test_votes_gpu.py stays away from, each with its conditions
asserted on the CPU where it is made, and the references the device tests compare with.  What each pins:

  big_queries, tiled_self_votes   QSLAB = 262144 in vt_run: a second query slab (q0 > 0) - the period 333 does not divide 262144, so
                                  the slab's border falls inside a period -, and a last slab of one full and one partial tile
  self_labels                     the own[] mask of the self form under every split of the base and on both paths
  dead_case                       a query tile without a valid row, whole 256-column steps without a voter, invalid first and last rows
  scale_case, gapped_threshold    nn_prepare_kernel's per-row power of two under the vote: rows from all-subnormal to FLT_MAX, one-hot
                                  and heavy rows, at thresholds that no float64 cosine comes within GAP of
  one_hot_case, EDGE_THRESHOLDS   pairs at exactly 1, +0 and -1 against thresholds at exactly those values, beside and beyond them
  WIDE_LABELS                     int64 labels that an int32 would fold into the classes

The references are the fold of an edge list (tests/votes_data.fold_edges) and the float64 definition (sequence.class_votes)."""
import functools

import numpy as np

from genomad_amd import sequence
from tests import embedding_limits_data as lim
from tests import linkage_limits_data as ld
from tests import votes_data as V
from tests.neighbours_data import sims64

QSLAB = 262144                                   # gnn_votes.hip
NQ_SLABS = QSLAB + 70                            # the smallest input with a second slab of a full and a partial tile
PERIOD = V.NQ                                    # 333: 262144 = 787 * 333 + 73, so row 262144 is row 73 of the period
FLT_MAX = lim.FLT_MAX
FIELDS = sequence.VOTE_FIELDS

# label transfer's thresholds at the exact values of one-hot rows: at 1, just above, at both zeros, at -1, just below, beyond every value
EDGE_THRESHOLDS = (1.0, float(np.nextafter(np.float32(1), np.float32(2))), 0.0, -0.0, -1.0,
                   float(np.nextafter(np.float32(-1), np.float32(-2))), FLT_MAX, -FLT_MAX)
WIDE_LABELS = (2 ** 32 + 1, 2 ** 31, -(2 ** 32) - 1, -2)          # as int32: 1, -2^31, -1 and -2; the first and third would pass


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def identical(got, want):
    """every array bit for bit; ``got`` / ``want``: a VoteResult or the four arrays"""
    g = [getattr(got, f) for f in FIELDS] if hasattr(got, "nearest_sim") else got
    w = [getattr(want, f) for f in FIELDS] if hasattr(want, "nearest_sim") else want
    return all(a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b)) for a, b in zip(g, w))


def differing(got, want):
    """for a failing assert: per field, the first cells that differ"""
    g = [getattr(got, f) for f in FIELDS] if hasattr(got, "nearest_sim") else got
    w = [getattr(want, f) for f in FIELDS] if hasattr(want, "nearest_sim") else want
    return {f: np.argwhere(bits(a) != bits(b))[:5].tolist() for f, a, b in zip(FIELDS, g, w) if not np.array_equal(bits(a), bits(b))}


# ---- two query slabs ---------------------------------------------------------------------------------------------------------------

def slab_index(n=NQ_SLABS, period=PERIOD):
    """row i of the tiled array is row i % period of the period"""
    idx = np.arange(n) % period
    assert n > QSLAB and QSLAB % period not in (0, period - 1) and (n - QSLAB) // 64 == 1 and (n - QSLAB) % 64 != 0
    return idx


def big_queries():
    """(262214, 512) float32, 537 MB: the 333 planted rows over and over.  Row 262144, the first of the second slab, is row 73."""
    p = V.query()[0]
    idx = slab_index()
    ok = V.valid(p)
    assert idx[QSLAB] == 73 and not ok[idx[:QSLAB]].all() and ok[idx[QSLAB:]].all()      # invalid rows in the first slab only: dead_first_copy
    return np.take(p, idx, axis=0)


def self_labels(n_classes, n=PERIOD):
    """int64 (n,) in [-1, n_classes): the pool's folded labels over the planted rows, -1s among them; row 5 alone in the last class"""
    label = V.labels(300, n_classes)[np.arange(n) % 300].copy()
    if n > 5:
        label[5] = n_classes - 1
    assert (label == -1).sum() > 0 and label.max() < n_classes
    return label


def tiled_self_votes(a, b, sim, label, n, period, n_classes, dead=()):
    """The self form's four arrays (n, n_classes) on ``n`` rows that repeat a period of ``period`` rows, from the period's own edges
    (a, b, sim: query p, base q, float32 sim, the pair (p, p) among them where the row is valid) and its labels: row q of the
    period stands mult(q) = #{i < n: i % period == q} times in the base.  ``dead``: rows below ``period`` that are made invalid in the
    tiled array - the first copy of a row, while its later copies live: they have no votes and are no voters.
      count    the sum of mult(q) over the edges of p = i % period with label[q] = c, minus one where (p, p) is an edge of that class
      weight   the same over rint(float64(sim) * 2^32)
      nearest  the best by (sim descending, index ascending) among the candidates of each edge: the first live copy of q other than
               i itself - row q, or row q + period where that is dead or i itself, or q + 2 period where both are"""
    a, b, sim = np.asarray(a, np.int64), np.asarray(b, np.int64), np.asarray(sim, np.float32)
    label = np.asarray(label, np.int64)
    dead = np.asarray(dead, np.int64)
    assert len(label) == period and n >= period and (dead < period).all()
    idx = np.arange(n) % period
    mult = np.bincount(idx, minlength=period)
    mult[dead] -= 1
    is_dead = np.zeros(4 * period, bool)
    is_dead[dead] = True
    c = label[b]
    keep = c >= 0
    a, b, c, sim = a[keep], b[keep], c[keep], sim[keep]
    units = np.rint(sim.astype(np.float64) * V.UNIT).astype(np.int64)
    count, weight = np.zeros((period, n_classes), np.int64), np.zeros((period, n_classes), np.int64)
    np.add.at(count, (a, c), mult[b])
    np.add.at(weight, (a, c), mult[b] * units)
    own = a == b
    np.add.at(count, (a[own], c[own]), -1)
    np.add.at(weight, (a[own], c[own]), -units[own])
    tiled = label[np.arange(4 * period) % period]
    out = (count[idx], weight[idx], np.empty((n, n_classes), np.int64), np.empty((n, n_classes), np.float32))
    for block in (2, 1, 0):                              # the query is row a + block * period; from 2 period on nothing changes
        cand = np.full(len(b), -1, np.int64)
        for k in (3, 2, 1, 0):                           # the smallest live copy that is not the query itself
            copy = b + k * period
            cand = np.where(~is_dead[copy] & (copy != a + block * period) & (copy < n), copy, cand)
        fold = V.fold_edges(a[cand >= 0], cand[cand >= 0], sim[cand >= 0], tiled, period, n_classes)
        rows = slice(2 * period, None) if block == 2 else slice(block * period, (block + 1) * period)
        out[2][rows], out[3][rows] = fold[2][idx[rows]], fold[3][idx[rows]]
    for arr, empty in zip(out, (0, 0, -1, np.nan)):
        arr[dead] = empty
    return out


def dead_first_copy(label, threshold):
    """a row i < 64 of the period for the self form over two slabs: with it made invalid, the flags of row i and of row QSLAB + i -
    a copy of row (QSLAB + i) % PERIOD, which has a voter at ``threshold`` - differ, and a flag read without the slab's offset shows"""
    s, ok = period_sims32()
    voter = ok & (np.asarray(label) >= 0)
    for i in range(64):
        p = (QSLAB + i) % PERIOD
        if ok[i] and ok[p] and (s[p][voter & (np.arange(PERIOD) != p) & (np.arange(PERIOD) != i)] >= threshold + 1e-3).any():
            return i
    raise AssertionError("no such row")


@functools.lru_cache(maxsize=None)
def period_sims32():
    """(float32 (333, 333) cosines of the planted rows, rounded from float64 - 0 wherever a row is not valid -, the valid rows)"""
    p = V.query()[0]
    ok = V.valid(p)
    s = np.zeros((len(p), len(p)), np.float32)
    at = np.flatnonzero(ok)
    s[np.ix_(at, at)] = sims64(p[ok], p[ok]).astype(np.float32)
    s.setflags(write=False)
    return s, ok


def edges_of(s, q_ok, b_ok, threshold):
    """(a, b, sim): the pairs of valid rows of the matrix ``s`` within the threshold, as NNEngine.match lists them - row by row"""
    with np.errstate(invalid="ignore"):
        a, b = np.nonzero((s >= np.float32(threshold)) & q_ok[:, None] & b_ok[None, :])
    return a, b, s[a, b]


# ---- dead tiles and steps ----------------------------------------------------------------------------------------------------------

def dead_case(unlabelled_head):
    """(rows (600, 512), label int64 (600,) in [-1, 4), dead rows, voters): linkage_limits_data.dead_tiles - rows 0..63, 256..511 and
    599 invalid - with the labels arange(600) % 5 - 1; ``unlabelled_head``: rows 64..255 are labelled -1 as well, so that the 256-column
    steps 0..255 and 256..511 hold no voter for any tile."""
    r, dead = ld.dead_tiles()
    label = (np.arange(600) % 5 - 1).astype(np.int64)
    if unlabelled_head:
        label[64:256] = -1
    ok = np.ones(600, bool)
    ok[dead] = False
    voters = np.flatnonzero(ok & (label >= 0))
    assert not ok[:64].any() and not ok[256:512].any() and not ok[0] and not ok[599] and np.array_equal(ok, V.valid(r))
    assert (voters >= 512).all() if unlabelled_head else (voters < 256).any()
    assert len(set(label[voters])) == 4
    return r, label, dead, voters


# ---- row scales --------------------------------------------------------------------------------------------------------------------

def gapped_threshold(s64, target, gap=2 * V.GAP):
    """the float32 nearest above ``target``, in steps of 5e-5, that no entry of ``s64`` comes within ``gap`` of"""
    flat = np.sort(np.asarray(s64, np.float64).ravel())
    for k in range(1000):
        t = float(np.float32(target + 5e-5 * k))
        at = np.searchsorted(flat, t)
        near = [abs(flat[j] - t) for j in (at - 1, at) if 0 <= j < len(flat)]
        if min(near) > gap:
            return t
    raise AssertionError(f"no gapped threshold near {target}")


SCALE_TARGETS = (0.03, -0.03)                    # both signs; 0 itself is the exact value of the orthogonal one-hot pairs


@functools.lru_cache(maxsize=None)
def scale_case(which):
    """(query, base or None, label, n_classes, float64 cosines (nq, nb), thresholds).  "extreme": extreme_queries against extreme_base
    (rows with elements up to FLT_MAX, all-subnormal rows, one-hot rows, heavy rows); "heavy": heavy_rows(333, 8) among themselves.
    The thresholds are chosen here, from the float64 cosines alone: none of them comes within 2 GAP of a threshold."""
    if which == "extreme":
        b = lim.extreme_base()
        q = lim.extreme_queries(b)
        s = sims64(q, b)
    else:
        q, b = lim.heavy_rows(333, 8), None
        s = sims64(q, q)
    label = (np.arange(s.shape[1]) % 5 - 1).astype(np.int64)
    off = s[~np.eye(len(s), dtype=bool)] if b is None else s           # the own pair (cosine 1) does not vote
    thresholds = tuple(gapped_threshold(off, t) for t in SCALE_TARGETS)
    assert np.isfinite(s).all() and V.valid(q).all()
    for arr in (q, s):
        arr.setflags(write=False)
    return q, b, label, 5, s, thresholds


def against_float64(res, s, label, n_classes, threshold, self_form):
    """The four arrays ``res`` against the float64 definition on cosines ``s`` (all rows valid) that keep GAP clear of the threshold,
    by the rules of tests/test_votes_gpu.py::test_votes_equal_the_float64_definition_where_it_is_well_defined: count exactly, weight
    within GAP per voter, nearest wherever the definition's top two of the class are more than NEAREST_GAP apart - at least 95 % of
    the cells with a voter -, nearest_sim within GAP.  Returns (largest weight error per voter, largest nearest_sim error)."""
    got_count, got_weight, got_nearest, got_nsim = [getattr(res, f) for f in FIELDS] if hasattr(res, "nearest_sim") else res
    thr = float(np.float32(threshold))
    s = np.array(s, np.float64)
    assert np.abs(s - thr).min() > V.GAP
    if self_form:
        s[np.arange(len(s)), np.arange(len(s))] = -np.inf
    count, weight = np.zeros(got_count.shape, np.int64), np.zeros(got_count.shape)
    nearest, nearest_sim = np.full(got_count.shape, -1, np.int64), np.full(got_count.shape, np.nan)
    clear = np.zeros(got_count.shape, bool)
    for c in range(n_classes):
        cols = np.flatnonzero(label == c)
        if not len(cols):
            continue
        v = np.where(s[:, cols] >= thr, s[:, cols], -np.inf)
        count[:, c] = np.isfinite(v).sum(axis=1)
        weight[:, c] = np.where(np.isfinite(v), v, 0.0).sum(axis=1)
        best = np.argmax(v, axis=1)
        has = count[:, c] > 0
        nearest[has, c] = cols[best[has]]
        nearest_sim[has, c] = v[has, best[has]]
        top = np.sort(np.concatenate([v, np.full((len(v), 1), -np.inf)], axis=1), axis=1)[:, -2:]
        clear[:, c] = has & (top[:, 1] - np.where(np.isfinite(top[:, 0]), top[:, 0], -9.0) > V.NEAREST_GAP)
    assert np.array_equal(got_count, count), np.argwhere(got_count != count)[:5]
    err = np.abs(got_weight.astype(np.float64) / V.UNIT - weight)
    assert (err <= V.GAP * count).all()
    assert clear.sum() >= 0.95 * (count > 0).sum(), (clear.sum(), (count > 0).sum())
    assert np.array_equal(got_nearest[clear], nearest[clear])
    assert np.array_equal(got_nearest < 0, count == 0) and np.array_equal(np.isnan(got_nsim), count == 0)
    nerr = float(np.abs(got_nsim[count > 0].astype(np.float64) - nearest_sim[count > 0]).max(initial=0))
    assert nerr <= V.GAP
    return float((err / np.maximum(count, 1)).max()), nerr


# ---- threshold edges ---------------------------------------------------------------------------------------------------------------

def one_hot_case():
    """(rows (16, 512), label int64 (16,) in [-1, 3), the exact cosines float64 (16, 16)): embedding_limits_data.one_hot_rows - every
    pair's cosine is 1, 0 or -1 and exact in any arithmetic.  Asserted: all three occur off the diagonal, in every class."""
    r, pos, sign = lim.one_hot_rows()
    s = np.where(pos[:, None] == pos[None, :], (sign[:, None] * sign[None, :]).astype(np.float64), 0.0)
    assert np.array_equal(sims64(r, r), s)
    label = (np.arange(16) % 4 - 1).astype(np.int64)
    off = ~np.eye(16, dtype=bool)
    for c in range(3):
        assert {float(x) for x in s[:, label == c][off[:, label == c]]} == {1.0, 0.0, -1.0}
    return r, label, s
