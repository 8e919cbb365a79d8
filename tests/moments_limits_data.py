"""The exact oracle and the inputs that take the k-means update and the principal-component moments (gnn_kmeans.hip, gnn_pca.hip) to
the limits their first tests stay away from.  Pure numpy; shares no code with genomad_amd/sequence.py.

The oracle.  Both files sum integers whose bits depend on nothing but the rows: q_i = (hi + lo) * 2^24 of row i's fragments, the image
of its unit vector in units of 2^-32.  Once q is known - a one-row call returns it: with n = 1, S is q - every device sum has an exact
host value:
  S            the int64 sum of q over the rows (sum_oracle: by group)
  centroid     f32(S / sqrt(sum S^2)) in float64 (centroid_oracle)
  G            per granule of 256 rows ALIGNED TO THE ABSOLUTE ROW INDEX a chain acc = fmaf(x_i[a], x_i[b], acc) over the rows in
               ascending order from zero, x = q * 2^-24 the f32 the Gram pass stages, one f32 rounding per step (what the f32-input
               matrix instruction computes); the granule contributes rint(acc * 2^16) and integers are added from there (gram_oracle)
fmaf32 is that fused multiply-add, correctly rounded: the product of two f32 is exact in float64, TwoSum gives the exact remainder of
its float64 sum with c, and where the float64 sum stands exactly half way between two f32 the remainder's sign decides - float64
a * b + c followed by a cast would round twice there.  tests/test_pca_limits_host.py compares it with fractions.Fraction.

The inputs, each built once per process and read-only: harvest_rows (607 rows: planted h1-like rows, ten rows of each extreme kind of
tests/embedding_limits_data.py, seven invalid rows at granule and range borders), launch_rows (enough rows for more than 64 per
workgroup of the sums and more than one granule per default Gram range), range_rows (65 600 rows for k = 65 535: two forced centroid
ranges), axis_rows (+-e_7 times powers of two: a Gram chain at its stated limit)."""
import functools
import hashlib

import numpy as np

from tests.embedding_limits_data import EXTREME_KINDS, SPLIT_MAX, extreme_base
from tests.pca_data import planted_rows, with_invalid

DIM = 512
GRANULE = 256                                    # gnn_pca.hip: rows of one f32 chain
Q_REL = 4.2e-7                                   # |q / 2^32 - u| <= Q_REL |u|: tests/test_kmeans_gpu.py derives it
Q_NORM = 3 * 2.0 ** -24                          # its part that is not the low limb's: the norm's sum, its root, the division
Q_ABS = 2.0 ** -33                               # half a unit of an f16 subnormal (2^-25) of x = 2^8 u


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------

def fmaf32(a, b, c):
    """The correctly rounded f32 fused multiply-add RN32(a * b + c) on float32 arrays (broadcast).  Exact wherever the result is zero
    or in the f32 normals and nothing overflows (asserted): p = a * b is exact in float64 (48 bits), s = RN64(p + c) and TwoSum's e
    give p + c = s + e exactly, and RN32(s) = RN32(s + e) unless s is a tie of f32 (no float64 lies between s and a tie it is not) -
    there e != 0 decides: towards the larger magnitude iff e has the sign of s."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    p = np.asarray(a * b)
    s = np.asarray(p + c)
    t = s - p
    e = (p - (s - t)) + (c - t)
    mag = np.abs(s)
    assert not ((mag != 0) & (mag < 2.0 ** -126)).any() and (mag < 2.0 ** 127).all()
    bits = s.view(np.uint64)
    tie = ((bits & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)) & (e != 0)
    out = s.astype(np.float32)
    if tie.any():
        down = bits & ~np.uint64(0x1FFFFFFF)                               # towards zero: the low 29 bits cleared
        up = down + np.uint64(0x20000000)                                  # the next f32 in magnitude; a carry moves the exponent
        away = (e > 0) == (s > 0)
        fixed = np.where(away, up, down).view(np.float64).astype(np.float32)
        out = np.where(tie, fixed, out)
    return out


def staged(q):
    """x = q * 2^-24: the f32 the Gram pass stages for an image q (exact: asserted)"""
    x = np.asarray(q, np.int64).astype(np.float64) * 2.0 ** -24
    x32 = x.astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), x)
    return x32


def granule_gram(q):
    """int64 (512, 512): what one granule (<= 256 rows of images q, in order) adds to G.  A zero row changes nothing, and the first
    step fmaf(a, b, +0) is the product rounded once."""
    q = np.asarray(q, np.int64)
    assert q.ndim == 2 and q.shape[1] == DIM and len(q) <= GRANULE
    acc = None
    for x in staged(q):
        if not x.any():
            continue
        acc = fmaf32(x[:, None], x[None, :], np.float32(0) if acc is None else acc)
    if acc is None:
        return np.zeros((DIM, DIM), np.int64)
    return np.rint(acc.astype(np.float64) * 65536.0).astype(np.int64)


class Frozen:
    """a read-only array that hashes by its bytes: the key of the granules' cache"""

    def __init__(self, a):
        self.a = np.ascontiguousarray(a)
        self.a.setflags(write=False)
        self.key = (self.a.shape, self.a.dtype.str, hashlib.sha1(self.a).digest())

    def __hash__(self):
        return hash(self.key)

    def __eq__(self, other):
        return self.key == other.key


@functools.lru_cache(maxsize=16)
def _granule_cached(frozen):
    g = granule_gram(frozen.a)
    g.setflags(write=False)
    return g


def gram_oracle(q, n=None):
    """int64 (512, 512): the G of the first ``n`` rows of the images q (row 0 of q is absolute row 0)"""
    q = np.asarray(q, np.int64)
    n = len(q) if n is None else int(n)
    assert 1 <= n <= len(q)
    G = np.zeros((DIM, DIM), np.int64)
    for r0 in range(0, n, GRANULE):
        G += _granule_cached(Frozen(q[r0:min(n, r0 + GRANULE)]))
    return G


def sum_oracle(q, label, k):
    """int64 (k, 512): the sums of the images by group; a label outside [0, k) is nobody's"""
    q, label = np.asarray(q, np.int64), np.asarray(label, np.int64)
    S = np.zeros((k, DIM), np.int64)
    inside = (label >= 0) & (label < k)
    np.add.at(S, label[inside], q[inside])
    return S


def centroid_oracle(S):
    """float32 (k, 512): f32(S / sqrt(sum S^2)) in float64; a zero row where the sum is zero (an empty group's is)"""
    S = np.atleast_2d(np.asarray(S, np.int64)).astype(np.float64)
    norm = np.sqrt((S * S).sum(axis=1))
    return np.where(norm[:, None] > 0, S / np.where(norm > 0, norm, 1.0)[:, None], 0.0).astype(np.float32)


def ulp_distance(a, b):
    """int64: how many f32 lie between a and b, +0 and -0 being one value; finite inputs"""
    def ordered(x):
        i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


# ---- the condition the comparison of q rests on ----------------------------------------------------------------------------------------

def unit64(rows):
    """the float64 unit vectors of valid float32 rows, scaled first so that no square overflows or vanishes"""
    r = np.asarray(rows, np.float32).astype(np.float64)
    r = r / np.abs(r).max(axis=1)[:, None]
    return r / np.sqrt((r * r).sum(axis=1))[:, None]


def fragment_image(rows):
    """int64 (n, 512): a numpy emulation of the prologue's split on valid rows - the f32 unit row times 2^8, hi = f16(x),
    lo = f16(x - hi), q = (hi + lo) * 2^24 - and whether hi + lo is an f32.  Not the device's bits (its norm is summed in another
    order): what the device's q is compared with is float64, through q_bound."""
    r = np.asarray(rows, np.float32)
    _, ex = np.frexp(np.abs(r).max(axis=1))
    x = np.ldexp(r.astype(np.float64), -ex[:, None]).astype(np.float32)   # exact: a power of two, into [0.5, 1)
    norm = np.sqrt((x * x).sum(axis=1, dtype=np.float32))
    x = x / norm[:, None] * np.float32(256)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    total = hi.astype(np.float64) + lo.astype(np.float64)
    exact = np.array_equal(total.astype(np.float32).astype(np.float64), total)
    q = total * 2.0 ** 24
    assert np.array_equal(q, np.rint(q))
    return q.astype(np.int64), exact


def q_bound(u):
    """The bound on |q / 2^32 - u| per element, derived.  x = f32(2^8 u) is within Q_NORM of its magnitude (the norm's sum, its root
    and the division round once each).  hi = f16(x) leaves a remainder of at most 2^-11 |x|, exact in f32; lo rounds it to 11 bits,
    2^-22 |x| - together Q_REL = 4.2e-7 of the element - as long as lo is an f16 normal.  Below that (|u| < 2^-11: the remainder is
    under 2^-14) lo, or hi itself, is a subnormal on the grid 2^-24 and rounds by at most 2^-25 of x, Q_ABS = 2^-33 of u, which is
    also all that is lost where an element is below 2^-32 of its row and its image is zero.  So the relative bound holds wherever
    it is the larger of the two."""
    a = np.abs(u)
    return np.maximum(Q_REL * a, Q_NORM * a + Q_ABS)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------

HARVEST_INVALID = (0, 255, 256, 300, 511, 512, 606)      # granule borders, range borders of set_pca_split(256), the last row
HARVEST_NS = (255, 256, 257, 600)                         # prefixes: below a granule, at it, one row beyond, three granules
EXTREME_TAKEN = 10                                        # rows of each of the four kinds


@functools.lru_cache(maxsize=None)
def harvest_rows():
    """((607, 512) float32, the mask of its 600 valid rows, the index in it of every extreme row by kind).  560 planted rows and 40
    extreme rows (huge, subnormal, one-hot, heavy: ten each) shuffled together by a fixed permutation, so that every granule holds
    some of each, then seven invalid rows (zero, NaN, Inf) inserted at HARVEST_INVALID."""
    ext = extreme_base()
    parts, kinds = [planted_rows()[:560]], []
    for name, sl in EXTREME_KINDS.items():
        parts.append(ext[sl][:EXTREME_TAKEN])
        kinds += [name] * EXTREME_TAKEN
    base = np.concatenate(parts)
    perm = np.random.default_rng(17).permutation(len(base))
    r, keep = with_invalid(base[perm], HARVEST_INVALID)
    assert len(r) == 607 and keep.sum() == 600 and not keep[-1]
    at = np.flatnonzero(keep)
    where = {name: np.sort(at[np.flatnonzero(np.isin(perm, 560 + np.flatnonzero(np.asarray(kinds) == name)))]) for name in EXTREME_KINDS}
    assert all(len(v) == EXTREME_TAKEN for v in where.values())
    r.setflags(write=False)
    keep.setflags(write=False)
    return r, keep, where


def launch_n(cus):
    """rows beyond which the sums take more than 64 per workgroup and the default Gram range more than one granule"""
    return 64 * 2 * cus + 4 * GRANULE + 77


@functools.lru_cache(maxsize=2)
def launch_rows(cus):
    """((n, 512) float32, its valid mask), n = launch_n(cus): the planted rows tiled, every row times a power of two of its own in
    2^-30 .. 2^30 and a sign of its own, three invalid rows at the front and two at the end"""
    n = launch_n(cus)
    p = planted_rows()
    rng = np.random.default_rng(23)
    scale = np.exp2(rng.integers(-30, 31, n)).astype(np.float32) * rng.choice(np.float32([-1, 1]), n)
    r = p[np.arange(n) % len(p)] * scale[:, None]
    keep = np.ones(n, bool)
    r[0] = 0
    r[1, 9] = np.nan
    r[2, 500] = np.inf
    r[n - 2, 0] = -np.inf
    r[n - 1] = 0
    keep[[0, 1, 2, n - 2, n - 1]] = False
    assert np.isfinite(r[keep]).all() and (np.abs(r[keep]).max(axis=1) > 0).all()
    r.setflags(write=False)
    keep.setflags(write=False)
    return r, keep


RANGE_N = 65600
RANGE_K = 65535                                           # K_MAX; beyond SPLIT_MAX = 65280: always two centroid ranges
RANGE_SOURCES = (0, 31, 32, 32767, SPLIT_MAX - 1, SPLIT_MAX, SPLIT_MAX + 1, RANGE_K - 1)


@functools.lru_cache(maxsize=1)
def range_rows(seed=71):
    """((65600, 512) float32, the source of every row): rows 0 .. 65534 standard normal - each the centroid of itself -, rows
    65535 .. 65599 copies of RANGE_SOURCES, cycled, times powers of two in 2^-20 .. 2^20 (exact)"""
    rng = np.random.default_rng(seed)
    r = rng.standard_normal((RANGE_N, DIM), dtype=np.float32)
    source = np.arange(RANGE_N)
    for j, i in enumerate(range(RANGE_K, RANGE_N)):
        source[i] = RANGE_SOURCES[j % len(RANGE_SOURCES)]
        r[i] = r[source[i]] * np.float32(2.0 ** int(rng.integers(-20, 21)))
    assert SPLIT_MAX < RANGE_K and np.isfinite(r).all()
    r.setflags(write=False)
    source.setflags(write=False)
    return r, source


def axis_rows(plus, minus, seed=29):
    """((plus + minus, 512) float32, the sign of every row): +-e_7 times a power of two of its own in 2^-100 .. 2^100, the signs
    shuffled; row 0 is positive"""
    rng = np.random.default_rng(seed)
    sign = np.concatenate([np.ones(plus), -np.ones(minus)])
    sign[1:] = rng.permutation(sign[1:])
    r = np.zeros((plus + minus, DIM), np.float32)
    r[:, 7] = sign * np.exp2(rng.integers(-100, 101, plus + minus))
    return r, sign
