"""Inputs that take the embedding searches (neighbours, cluster, representatives) to the limits their own tests never reach, each with
its conditions asserted on the CPU where it is made.  What each generator pins in the kernels:

  signed_rows, heavy_rows   negative similarities through nn_insert / nn_precedes (gnn_neighbours.hip) and the `u >> 31` branch of
                            rp_image / rp_unimage (gnn_representatives.hip); heavy rows reach f16-subnormal low limbs despite the 2^8
                            scale of nn_prepare_kernel (gnn_nn_frag.h)
  signed_integer_rows       the same orders on exact values: ties, a negated row, both signs of the threshold
  negative_contest          rp_image on negative keys whose order decides the representative, a tie on a negative key, 0 against < 0
  slab_rows                 QSLAB = 16384 in nn_search: `qfrag = w.bfrag + q0 / 32 * BLK_U4`, `self_off = q0`, the offsets `q0 * k`
  capped_base               SPLIT_MAX = 65280 and `uint16_t loff` in nn_tile_kernel: offsets 32767, 32768, 65279, the first row of a
                            second range, a tie across bit 15 of the offset
  power_of_two_scaled,      the frexpf / ldexpf scaling of nn_prepare_kernel: rows from all-subnormal to FLT_MAX, one-hot rows
  extreme_base
  dot_range_rows,           the dot metric's documented range (the unscaled split of nn_prepare_kernel): |element| up to 6e4 and
  small_dot_rows,           down to 2^-7 within the relative bound, 7e4 never returned (`s == s` in nn_tile_kernel, `s >= threshold`
  out_of_range_base         in cl_tile_kernel and rp_tile_kernel)

The references are fp64 (sims64) and the numpy definitions of genomad_amd/sequence.py; the tolerances are the neighbour tests'."""
import numpy as np

from tests.neighbours_data import DIM, rows, sims64

VALUE_TOL = 1e-5        # tests/test_neighbours_gpu.py
GAP = 2e-5
CAP = 0.9               # the exact-order check may leave rows out, but at least this share must qualify

QSLAB = 16384           # gnn_neighbours.hip
SPLIT_MAX = 65280       # gnn_nn_frag.h
NQ_SLABS = QSLAB + 70
NB_CAPPED = SPLIT_MAX + 70
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)        # the smallest normal


def qualifies(s64, k):
    """rows of the fp64 similarities whose top-(k + 1) gaps all exceed GAP: there the device's order must be the definition's"""
    top = -np.sort(-s64, axis=1)[:, :k + 1]
    return (-np.diff(top, axis=1) > GAP).all(axis=1)


def order64(s64, k):
    """the k best columns of every row of the fp64 matrix by (similarity descending, index ascending)"""
    return np.argsort(-s64, axis=1, kind="stable")[:, :k]


def self64(r, rows_of=None):
    """fp64 cosine of the rows ``rows_of`` (all of them by default) against all rows of r, the own pair at -inf"""
    rows_of = np.arange(len(r)) if rows_of is None else np.asarray(rows_of)
    s = sims64(r[rows_of], r)
    s[np.arange(len(rows_of)), rows_of] = -np.inf
    return s


def signed_rows(n, seed):
    """(n, 512) float32: N(0, 1) * 2^U{-3..2} per channel - ``neighbours_data.rows`` without the ReLU.  Asserted on the first 64
    rows: between 40 % and 60 % of their similarities are negative."""
    rng = np.random.default_rng(seed)
    scale = np.exp2(rng.integers(-3, 3, DIM)).astype(np.float32)
    r = (rng.standard_normal((n, DIM)).astype(np.float32) * scale).astype(np.float32)
    head = r[:64]
    if len(head) > 1:
        neg = (sims64(head, head)[np.triu_indices(len(head), 1)] < 0).mean()
        assert 0.4 < neg < 0.6, neg
    return r


def heavy_rows(n, seed):
    """(n, 512) float32: N(0, 1) * exp(3 N(0, 1)) per element - heavy tails.  Asserted: the median over the rows of max / median
    |element| lies in [3e3, 5e4] (about 1.3e4): a unit row's small elements, times 2^8, have low limbs below the f16 normals."""
    rng = np.random.default_rng(seed)
    r = (rng.standard_normal((n, DIM)) * np.exp(3.0 * rng.standard_normal((n, DIM)))).astype(np.float32)
    a = np.abs(r.astype(np.float64))
    ratio = float(np.median(a.max(axis=1) / np.median(a, axis=1)))
    assert np.isfinite(r).all() and 3e3 <= ratio <= 5e4, ratio
    return r


def signed_integer_rows(n=200, seed=11):
    """(n, 512) float32, n >= 200: integers of [-4, 4), every other row negated, so every dot is an integer of magnitude
    <= 512 * 16 < 2^24, exact on the device, and as often negative as positive.  Rows 40..59 equal row 10 and rows 150 and n - 1
    equal row 3 (ties across and within 32-row blocks); row 77 is minus row 3."""
    assert n >= 200
    rng = np.random.default_rng(seed)
    r = rng.integers(-4, 4, (n, DIM)).astype(np.float32)
    r[1::2] *= -1                                          # the mean element is -0.5: without this a dot is 128 +- 119
    r[40:60] = r[10]
    r[150] = r[3]
    r[n - 1] = r[3]
    r[77] = -r[3]
    dots = r.astype(np.float64) @ r.astype(np.float64).T
    assert np.abs(r).max() <= 4 and np.abs(dots).max() < 2 ** 24 and (dots == np.round(dots)).all()
    assert (dots[77, [3, 150, n - 1]] == -dots[3, 3]).all() and dots[3, 3] > 0
    upper = dots[np.triu_indices(n, 1)]
    assert 0.4 < (upper < 0).mean() < 0.6
    return r


def integer_thresholds(r):
    """(negative, positive): two dots that more than 10 pairs of the integer rows attain - the quartiles of the pairs' dots"""
    dots = r.astype(np.float64) @ r.astype(np.float64).T
    upper = np.sort(dots[np.triu_indices(len(r), 1)])
    neg, pos = float(upper[len(upper) // 4]), float(upper[3 * len(upper) // 4])
    assert neg < 0 < pos and (upper == neg).sum() > 10 and (upper == pos).sum() > 10
    return neg, pos


NEGATIVE_TAIL_BASE = 80           # base rows of the k = 64 case whose lists must end in negative values: about 40 of 80 are positive


CONTEST_THRESHOLD = -10.0
CONTEST_REPS = (0, 40, 70)                       # A, B, C: mutually below the threshold
# a member's dots with (A, B, C); d_A is a multiple of 4 and >= the threshold, so A alone already keeps the row from founding a cluster
CONTEST_PATTERNS = ((-4, -1, -20),               # B wins: not the candidate of smallest rank
                    (-8, -8, -3),                # C wins
                    (-4, -4, -20),               # a tie of A and B on -4: the smaller rank
                    (-8, -20, -8),               # a tie of A and C on -8
                    (0, -5, -20),                # 0 against a negative value: A, and sim is +0
                    (-4, 0, -9),                 # B at 0
                    (-8, -9, -7),                # three negative candidates, C wins
                    (-4, -20, -20))              # A alone


def negative_contest():
    """Integer rows for the dot metric at CONTEST_THRESHOLD = -10, after the construction A = 4 e1, B = -4 e1 + e2 (A.B = -16) with a
    third C = -3 e1 - 23 e2 + e3 (C.A = -12, C.B = -11): a row m = x e1 + y e2 + z e3 has m.A = 4 x, m.B = y - 4 x and
    m.C = z - 3 x - 23 y, so any triple of dots with m.A a multiple of 4 can be had.  100 rows: A, B, C at CONTEST_REPS, every other
    row a member that cycles through CONTEST_PATTERNS - more than one 64-row tile and every 32-row block.  Returns (rows, orders):
    ``orders`` maps a name to (weight, the ranks' expected representatives as a dict member -> rep).  "index": members between the
    representatives see only those of smaller index.  "cab": C, A, B first (weights 3, 2, 1), then the members.  The properties the
    issue lists are asserted here from the fp64 dots for both orders."""
    n = 100
    r = np.zeros((n, DIM), np.float32)
    a, b, c = CONTEST_REPS
    r[a, 1] = 4
    r[b, 1], r[b, 2] = -4, 1
    r[c, 1], r[c, 2], r[c, 3] = -3, -23, 1
    members = [i for i in range(n) if i not in CONTEST_REPS]
    for t, i in enumerate(members):
        da, db, dc = CONTEST_PATTERNS[t % len(CONTEST_PATTERNS)]
        x = da // 4
        y = db + 4 * x
        z = dc + 3 * x + 23 * y
        r[i, 1], r[i, 2], r[i, 3] = x, y, z
    dots = r.astype(np.float64) @ r.astype(np.float64).T
    assert (dots == np.round(dots)).all() and np.abs(dots).max() < 2 ** 24
    thr = CONTEST_THRESHOLD
    assert dots[a, b] < thr and dots[a, c] < thr and dots[b, c] < thr
    weight = np.zeros(n)
    weight[[c, a, b]] = 3, 2, 1
    orders = {}
    for name, w in (("index", None), ("cab", weight)):
        rank = np.arange(n) if w is None else np.argsort(np.argsort(-w, kind="stable"), kind="stable")
        want, not_first, tie, zero_and_negative, all_negative = {}, 0, 0, 0, 0
        for m in members:
            cand = sorted((i for i in CONTEST_REPS if rank[i] < rank[m] and dots[i, m] >= thr), key=lambda i: rank[i])
            assert cand and all(dots[i, m] <= 0 for i in cand)
            best = max(cand, key=lambda i: (dots[i, m], -rank[i]))
            want[m] = best
            vals = [dots[i, m] for i in cand]
            all_negative += max(vals) < 0
            not_first += max(vals) < 0 and best != cand[0]
            tie += max(vals) < 0 and vals.count(max(vals)) == 2
            zero_and_negative += max(vals) == 0 and min(vals) < 0
        assert all_negative >= 8 and not_first >= 2 and tie >= 1 and zero_and_negative >= 1, (name, all_negative, not_first, tie)
        orders[name] = (w, want)
    return r, orders


def slab_rows(seed=31):
    """(16454, 512) signed rows for the self-search over two query slabs, planted across the border at 16384: row 16384 = 2 x row 5,
    row 16383 = 0.5 x row 16390, and rows 100, 16447 and 16453 identical.  Returns (rows, pairs, triple)."""
    r = signed_rows(NQ_SLABS, seed)
    r[QSLAB] = 2 * r[5]
    r[QSLAB - 1] = np.float32(0.5) * r[QSLAB + 6]
    triple = (100, QSLAB - 1 + 64, NQ_SLABS - 1)
    r[triple[1]] = r[triple[0]]
    r[triple[2]] = r[triple[0]]
    assert np.array_equal(r[QSLAB].astype(np.float64), 2.0 * r[5]) and np.array_equal(2.0 * r[QSLAB - 1].astype(np.float64), r[QSLAB + 6])
    return r, ((5, QSLAB), (QSLAB - 1, QSLAB + 6)), triple


CAPPED_PLANTS = (32767, 32768, SPLIT_MAX - 1, SPLIT_MAX, NB_CAPPED - 1)        # query i's multiple, i = 0 .. 4
CAPPED_TIE = (32768 + 1, SPLIT_MAX - 1 - 1)                                    # both hold the same multiple of query 5


def capped_base(query, seed=41):
    """(65350, 512) rows of ``neighbours_data.rows`` - one full range of SPLIT_MAX rows and 70 more - with power-of-two multiples of
    queries 0 .. 4 at CAPPED_PLANTS and the same multiple of query 5 at both rows of CAPPED_TIE."""
    base = rows(NB_CAPPED, seed)
    for i, at in enumerate(CAPPED_PLANTS):
        base[at] = query[i] * np.float32(2.0 ** (i - 2))
    for at in CAPPED_TIE:
        base[at] = query[5] * np.float32(4.0)
    return base


def power_of_two_scaled(r, seed):
    """r * 2^e with one e of U{-100..100} per row.  Asserted: the scaling is exact and no non-zero element leaves the f32 normals."""
    e = np.random.default_rng(seed).integers(-100, 101, len(r))
    out = (r * np.exp2(e).astype(np.float32)[:, None]).astype(np.float32)
    assert np.array_equal(out.astype(np.float64), r.astype(np.float64) * np.exp2(e.astype(np.float64))[:, None])
    a = np.abs(out[out != 0])
    assert a.min() >= FLT_MIN and a.max() <= FLT_MAX and e.max() - e.min() > 150
    return out


EXTREME_KINDS = {"huge": slice(0, 16), "subnormal": slice(16, 32), "one_hot": slice(32, 48), "heavy": slice(48, 64)}


def one_hot_rows():
    """16 rows with one non-zero element each, not a power of two: positions 0, 0, 7, 7, 300, 300, 511, 511 twice over, the signs
    +, -, +, -, ... in the first eight and +, +, -, -, ... in the last.  Returns (rows, position, sign)."""
    pos = np.array([0, 0, 7, 7, 300, 300, 511, 511] * 2)
    sign = np.array([1, -1] * 4 + [1, 1, -1, -1] * 2)
    r = np.zeros((16, DIM), np.float32)
    r[np.arange(16), pos] = sign * np.float32(3.0) * np.exp2(np.arange(16) * 5 - 40).astype(np.float32)
    return r, pos, sign


def extreme_base(seed=51):
    """(333, 512) signed rows whose first 64 are, by EXTREME_KINDS: 16 rows with the largest element in [2^127, FLT_MAX], 16 rows
    times 2^-140 (every element subnormal or zero, the row not zero), 16 one-hot rows, 16 heavy rows.  Asserted here."""
    r = signed_rows(333, seed)
    huge = r[EXTREME_KINDS["huge"]].astype(np.float64)
    _, ex = np.frexp(np.abs(huge).max(axis=1))
    huge = huge * np.exp2(128 - ex)[:, None]
    assert (np.abs(huge).max(axis=1) >= 2.0 ** 127).all() and np.abs(huge).max() <= FLT_MAX
    r[EXTREME_KINDS["huge"]] = huge.astype(np.float32)
    assert np.array_equal(r[EXTREME_KINDS["huge"]].astype(np.float64), huge)
    tiny = (r[EXTREME_KINDS["subnormal"]].astype(np.float64) * 2.0 ** -140).astype(np.float32)
    assert (np.abs(tiny) < FLT_MIN).all() and ((tiny != 0).sum(axis=1) > 400).all()
    r[EXTREME_KINDS["subnormal"]] = tiny
    r[EXTREME_KINDS["one_hot"]] = one_hot_rows()[0]
    r[EXTREME_KINDS["heavy"]] = heavy_rows(16, seed + 1)
    assert np.isfinite(r).all()
    return r


def extreme_queries(base, seed=52):
    """(70, 512): base rows 0..5 (huge), 16..21 (subnormal), all 16 one-hot rows, 48..53 (heavy) - each times a power of two that
    keeps its kind, or as it is - and 36 fresh signed rows."""
    q = signed_rows(70, seed)
    q[0:6] = base[0:6] * np.float32(0.5)
    q[6:12] = base[16:22]
    q[12:28] = base[32:48] * np.float32(8.0)
    q[28:34] = base[48:54] * np.float32(0.25)
    return q


def dot_range_rows(n, seed):
    """heavy rows scaled so that the largest |element| of the whole array is 6e4: inside the f16 range the dot metric needs"""
    r = heavy_rows(n, seed).astype(np.float64)
    r = (r * (6e4 / np.abs(r).max())).astype(np.float32)
    assert 5.99e4 <= np.abs(r).max() <= 6e4 < 65504
    return r


DOT_RANGE_LOW = 2.0 ** -7         # include/genomad_nn.h: the dot metric's relative bound holds from here up (or for a zero element)


def small_dot_rows(n, seed):
    """(n, 512) float32, every element +-2^-7 (1 + |N(0, 1)|): all in [2^-7, 2^-3), the lower end of the range for which the header
    states the relative bound of the dot metric.  Below 2^-3 the low limb of an unscaled element is an f16 subnormal and carries it
    to 2^-25 absolute: 2^-18 relative at 2^-7, for both rows 7.6e-6 of sum |x_i y_i|, plus 2.4e-7 for the dropped lo.lo product."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, DIM))
    r = (np.where(g < 0, -1.0, 1.0) * DOT_RANGE_LOW * (1.0 + np.abs(g))).astype(np.float32)
    assert np.abs(r).min() >= DOT_RANGE_LOW and np.abs(r).max() < 2.0 ** -3
    return r


def dot_bound(query, base):
    """the per-pair bound on |f32 dot - fp64 dot|: VALUE_TOL * sum_i |x_i y_i| - the cosine bound's form carried to unnormalised rows"""
    return VALUE_TOL * (np.abs(np.asarray(query, np.float64)) @ np.abs(np.asarray(base, np.float64)).T)


def split_f16_dots(query, base):
    """fp64 dots of the rows as the device holds them under dot: hi = f16(x), lo = f16(x - hi), the three products hi.lo, lo.hi, hi.hi
    (lo.lo is dropped).  What the limbs alone cost, without the f32 accumulation of the matrix pipe."""
    def limbs(r):
        r = np.asarray(r, np.float32)
        hi = r.astype(np.float16)
        lo = (r - hi.astype(np.float32)).astype(np.float16)
        return hi.astype(np.float64), lo.astype(np.float64)
    qh, ql = limbs(query)
    bh, bl = limbs(base)
    return qh @ bl.T + ql @ bh.T + qh @ bh.T


OUT_OF_RANGE = (17, 250)


def out_of_range_base(seed=61):
    """(333, 512) signed integer rows in [-4, 4) - every dot among them exact - but rows 17 and 250 hold one element of 7e4 and
    -7e4: beyond the f16 range, finite in f32, so the definition counts them as valid and the device must not return them."""
    r = np.random.default_rng(seed).integers(-4, 4, (333, DIM)).astype(np.float32)
    r[OUT_OF_RANGE[0], 5] = 7e4
    r[OUT_OF_RANGE[1], 400] = -7e4
    return r
