"""Inputs that take the interval fold (genomad_amd/csrc/gnn_intervals.hip) to the limits its own tests never
reach, each with its conditions asserted on the CPU where it is made.  What each generator pins in the kernel:

  cuts, with_empty_runs   the bisection of launch_fold and the 8-row batch of interval_fold_kernel: ranges of every length 0 .. 25 whose
                          starts hit every residue mod 8, masked first / last rows, runs of empty ranges on slab edges
  poisoned, poison_free   the masking is a select, not a product: NaN / inf / FLT_MAX in every masked row, in rows no interval owns,
                          in the row before a range and behind it (the clamped prefetch reads the range's last row, never beyond)
  long_ranges             the growth of the sequential f32 sum of unit rows: 65, 1000 and 2000 kept members
  scaled                  the rule for a unit row: every finite row that is not all zeros has one, from all-subnormal to FLT_MAX
  both_strands            sum_rev / unit_rev of interval_finish_kernel on rows of the test's choosing

A fixture is a dict of ``rows`` (n, 512) float32, ``scores`` (n, 3) float32, ``kept`` (n,) bool, ``w_lo`` / ``w_hi`` int64 and what
else its test needs.  The references are ``definition`` (sequence.interval_embeddings) and ``coherence_gram``, which share no code.

The coherence tolerance ``coh_tol(n, strands)`` is twice a bound derived here from the kernel's arithmetic alone, before the device
was run; eps = 2^-24 (float32 rounding to nearest), n kept members per strand.

- A unit row.  The squared norm of a row is 4 products and 3 additions in a lane, 6 butterfly levels inside a wave and one addition
  between the two waves; all terms are non-negative, so its relative error is at most (1 + 3 + 6 + 1) eps = 11 eps.  A row whose
  plain sum lies in [2^-116, FLT_MAX] is used as it is: products below 2^-126 lose at most 512 * 2^-150 = 2^-141 absolute, 0.5 eps of
  2^-116, so 11.5 eps.  Every other valid row is first scaled by the power of two that brings its largest element into [0.5, 1):
  exact, but for elements that fall below 2^-149 and change the unit row by less than 2^-148 - the scaling adds nothing to the
  11 eps, and the term does not depend on the row's scale.  rsqrt halves the error and adds its own of at most 1 ulp = 2 eps, the
  product with the element one more eps: a unit row is off by at most (5.75 + 2 + 1) eps < 9 eps of its own length 1.
- The n unit rows are added one after the other: addition i rounds a partial sum of length at most i, so the sum is off by at most
  (1 + 2 + ... + n) eps = n (n + 1) / 2 eps; with the rows' own errors |dU| <= (9 n + n (n + 1) / 2) eps.
- Under ``both`` each strand's sum has n members and that error; the finish adds the two once, rounding a vector of length at most
  2 n: |d(U_f + U_r)| <= (18 n + n (n + 1) + 2 n) eps.
- The division by the number of unit rows, n or 2 n, gives (9 + (n + 1) / 2) eps, or (10 + (n + 1) / 2) eps under ``both``.
- The final norm (11 eps as above, halved by the square root, plus the root's and the division's rounding) adds at most 8 eps of a
  value <= 1.

Together (16 + strands + (n + 1) / 2) eps, and coh_tol is twice that: (n + 33 + 2 strands) * 2^-24, 1.2e-4 at n = 2000.  The same
derivation stands in tests/test_intervals_gpu.py for one strand, and its fixed COH_TOL = 1e-5 covers n <= 64 (5.9e-6)."""
import functools
import math

import numpy as np

from genomad_amd import sequence

DIM = 512
EPS = 2.0 ** -24
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)        # the smallest normal
KEYS = ("count", "embedding", "scores", "coherence")


def coh_tol(n, strands=1):
    """the coherence tolerance for n kept members per strand: twice the bound of the module docstring"""
    return 2.0 * (16 + strands + (n + 1) / 2.0) * EPS


def definition(fx, rows_rev=None):
    return sequence.interval_embeddings(fx["rows"], fx["scores"], fx["kept"], fx["w_lo"], fx["w_hi"], rows_rev=rows_rev)


def valid_rows(rows):
    """the rows that have a unit row: every element finite and one of them not zero"""
    rows = np.asarray(rows)
    return np.isfinite(rows).all(axis=1) & (rows != 0).any(axis=1)


def coherence_gram(rows, members, rows_rev=None):
    """coherence without a sequential sum and without a loop over unit rows: |sum_i u_i|^2 = sum_ij cos(e_i, e_j) over the valid members
    (both strands' under ``rows_rev``), so the square root of the sum of the float64 cosine matrix, divided by the number of members.
    Where directions cancel, the square root would turn 1e-17 left over in the sum into 3e-9: up to 64 rows the dots are sums of
    products in one fixed order, so that opposite rows have opposite cosines to the last bit, and the matrix is summed exactly."""
    members = np.asarray(members, np.int64)
    x = rows[members] if rows_rev is None else np.concatenate([rows[members], rows_rev[members]])
    count = len(x)
    if count == 0:
        return 0.0
    x = x[valid_rows(x)].astype(np.float64)
    x = x / np.abs(x).max(axis=1, keepdims=True)                   # float64 holds the square of any float32 either way
    gram = (x[:, None, :] * x[None, :, :]).sum(axis=-1) if len(x) <= 64 else x @ x.T
    norm = np.sqrt(np.diag(gram))
    return float(np.sqrt(max(math.fsum((gram / np.outer(norm, norm)).ravel()), 0.0)) / count)


def members_of(fx, i):
    a, b = int(fx["w_lo"][i]), int(fx["w_hi"][i])
    return np.arange(a, b)[fx["kept"][a:b]]


def signed(rng, n):
    """standard_normal * 2^[-3, 3] per row"""
    return (rng.standard_normal((n, DIM)).astype(np.float32) * np.exp2(rng.integers(-3, 4, size=(n, 1))).astype(np.float32)).astype(np.float32)


# ---- cuts -----------------------------------------------------------------------------------------------------------------------
N_RANGES = 26
N_CUTS = 325
LAST_ROW_MASKED = (8, 10)         # ranges (= their lengths) whose last row is masked
FIRST_ROW_MASKED = 17
ALL_MASKED = 12
ALL_KEPT = 20
ODD_LAST_ROW = (9, 16)            # their last row is kept: the test plants a zero row, an inf and a NaN there


@functools.lru_cache(maxsize=None)
def _cuts():
    rng = np.random.default_rng(501)
    length = np.arange(N_RANGES, dtype=np.int64)
    w_lo = np.concatenate([[0], np.cumsum(length)[:-1]]).astype(np.int64)
    w_hi = w_lo + length
    assert list(w_lo[:9]) == [0, 0, 1, 3, 6, 10, 15, 21, 28] and int(w_hi[-1]) == N_CUTS
    assert set((w_lo % 8).tolist()) == set(range(8))
    assert {0, 1, 7, 8, 9, 15, 16, 17} <= set(length.tolist())
    rows = signed(rng, N_CUTS)
    scores = rng.random((N_CUTS, 3), dtype=np.float32)
    kept = rng.random(N_CUTS) < 0.8
    for i in LAST_ROW_MASKED:
        kept[w_lo[i]:w_hi[i] - 1] = True
        kept[w_hi[i] - 1] = False
    kept[w_lo[FIRST_ROW_MASKED]] = False
    kept[w_lo[FIRST_ROW_MASKED] + 1:w_hi[FIRST_ROW_MASKED]] = True
    kept[w_lo[ALL_MASKED]:w_hi[ALL_MASKED]] = False
    kept[w_lo[ALL_KEPT]:w_hi[ALL_KEPT]] = True
    for i in ODD_LAST_ROW:
        kept[w_hi[i] - 1] = True
    assert 0.7 < kept.mean() < 0.9
    assert all(not kept[w_hi[i] - 1] and kept[w_lo[i]:w_hi[i] - 1].all() for i in LAST_ROW_MASKED)
    assert not kept[w_lo[FIRST_ROW_MASKED]] and kept[w_lo[FIRST_ROW_MASKED] + 1:w_hi[FIRST_ROW_MASKED]].all()
    assert length[ALL_MASKED] >= 9 and not kept[w_lo[ALL_MASKED]:w_hi[ALL_MASKED]].any()
    assert length[ALL_KEPT] >= 17 and kept[w_lo[ALL_KEPT]:w_hi[ALL_KEPT]].all()
    assert [int(length[i]) for i in ODD_LAST_ROW] == [9, 16] and all(kept[w_hi[i] - 1] for i in ODD_LAST_ROW)
    assert np.isfinite(rows).all() and rows.dtype == np.float32 and rows.shape == (N_CUTS, DIM)
    return dict(rows=rows, scores=scores, kept=kept, w_lo=w_lo, w_hi=w_hi)


def cuts():
    """325 signed rows in 26 consecutive ranges of the lengths 0, 1, ..., 25 (range i has length i): the starts 0, 0, 1, 3, 6, 10,
    15, 21, 28, ... hit every residue mod 8.  About 80 % of the rows are kept; ranges 8 and 10 have their last row masked, range 17 its
    first, range 12 is masked and range 20 kept altogether; the last rows of ranges 9 and 16 are kept."""
    return {k: v.copy() for k, v in _cuts().items()}


EMPTY_TOTAL = 4096
EMPTY_RUN_AT = (0, 120, 136, 325)
EMPTY_RUN_MIN = 100


def with_empty_runs(fx):
    """The rows of ``cuts`` under 4096 intervals: its 26 ranges in order and empty ranges (w_lo == w_hi) before the first, behind the
    last and between every two.  Ranges must be ordered (w_lo >= the w_hi before), so an empty range can sit only where one range
    ends and the next begins: at 0, 0, 1, 3, 6, 10, ..., 300, 325.  Runs of at least 100 sit at rows 0, 120, 136 and 325, which are
    the boundaries that are also edges of 8-row slices (rows 8 and 64 lie inside the ranges [6, 10) and [55, 66): no empty range can
    sit there); with 1-row slices every boundary is an edge.  ``index`` holds the new places of the 26 ranges."""
    w_lo, w_hi = fx["w_lo"], fx["w_hi"]
    assert len(w_lo) == N_RANGES and (w_lo[1:] == w_hi[:-1]).all()
    at = [0] + [int(x) for x in w_hi]                              # the 27 slots: before range 0, behind each range
    size = [1 + s % 3 for s in range(len(at))]
    first_slot = {p: at.index(p) for p in EMPTY_RUN_AT}            # the first slot at that row
    spare = EMPTY_TOTAL - N_RANGES - sum(size)
    for n, p in enumerate(EMPTY_RUN_AT):
        size[first_slot[p]] += spare // 4 + (spare % 4 if n == 0 else 0)
    lo, hi, index = [], [], []
    for s, p in enumerate(at):
        lo += [p] * size[s]
        hi += [p] * size[s]
        if s < N_RANGES:
            index.append(len(lo))
            lo.append(int(w_lo[s]))
            hi.append(int(w_hi[s]))
    lo, hi, index = np.array(lo, np.int64), np.array(hi, np.int64), np.array(index, np.int64)
    assert len(lo) == EMPTY_TOTAL and np.array_equal(lo[index], w_lo) and np.array_equal(hi[index], w_hi)
    assert (lo[1:] >= hi[:-1]).all() and (lo <= hi).all()
    empty = np.ones(EMPTY_TOTAL, bool)
    empty[index] = False
    assert (lo[empty] == hi[empty]).all() and empty[0] and empty[-1] and (np.diff(index) > 1).all()
    for p in EMPTY_RUN_AT:
        assert int((empty & (lo == p)).sum()) >= EMPTY_RUN_MIN and (p % 8 == 0 or p == N_CUTS)
    return dict(fx, w_lo=lo, w_hi=hi, index=index)


# ---- poison ---------------------------------------------------------------------------------------------------------------------
GAP_BEHIND = (6, 7, 8, 9, 14, 15, 16, 17, 21, 23, 24, 25)          # a gap follows these ranges: 7-9, 15-17, 24 and 25 lie between two


def _with_gaps(fx):
    """cuts with 1 to 3 rows owned by no interval behind the ranges of GAP_BEHIND (the last among them); the gap rows are marked
    kept: only the ranges keep them out.  Returns the fixture and the mask of the gap rows."""
    rng = np.random.default_rng(502)
    pieces = {k: [] for k in ("rows", "scores", "kept", "gap")}
    lo, hi, at = [], [], 0
    for i in range(N_RANGES):
        a, b = int(fx["w_lo"][i]), int(fx["w_hi"][i])
        lo.append(at)
        hi.append(at + b - a)
        at += b - a
        pieces["rows"].append(fx["rows"][a:b]), pieces["scores"].append(fx["scores"][a:b]), pieces["kept"].append(fx["kept"][a:b])
        pieces["gap"].append(np.zeros(b - a, bool))
        if i in GAP_BEHIND:
            g = 1 + GAP_BEHIND.index(i) % 3
            pieces["rows"].append(signed(rng, g)), pieces["scores"].append(rng.random((g, 3), dtype=np.float32))
            pieces["kept"].append(np.ones(g, bool)), pieces["gap"].append(np.ones(g, bool))
            at += g
    out = {k: np.concatenate(v) for k, v in pieces.items()}
    gap = out.pop("gap")
    out.update(w_lo=np.array(lo, np.int64), w_hi=np.array(hi, np.int64))
    assert len(gap) == at == N_CUTS + int(gap.sum()) and gap[-1] and 1 <= int(gap.sum()) <= 3 * len(GAP_BEHIND)
    return out, gap


POISON = (np.nan, np.inf, -np.inf, FLT_MAX, -FLT_MAX)


def _poison_mask(fx, gap):
    owned = np.zeros(len(gap), bool)
    for a, b in zip(fx["w_lo"], fx["w_hi"]):
        owned[a:b] = True
    assert not (owned & gap).any() and (owned | gap).all()
    return gap | ~fx["kept"]


def poisoned(fx):
    """``cuts`` with gaps, and poison in every masked row and every gap row: the rows cycle through NaN, +inf, -inf, +FLT_MAX and
    -FLT_MAX, in turn filling the whole row or single elements of a signed row; their scores are NaN.  Asserted: no kept member of a
    range is touched, and the row before the start and the row behind the end are poison for at least four ranges, one of a length
    that is a multiple of 8 and one that is not.  Returns the fixture with ``poison`` (the mask of those rows)."""
    out, gap = _with_gaps(fx)
    bad = _poison_mask(out, gap)
    clean = out["rows"].copy()
    for n, r in enumerate(np.flatnonzero(bad)):
        value = np.float32(POISON[n % len(POISON)])
        if (n // len(POISON)) % 2 == 0:
            out["rows"][r] = value
        else:
            out["rows"][r, [(7 * n) % DIM, (7 * n + 255) % DIM, DIM - 1 - n % 3]] = value
        out["scores"][r] = np.nan
    out["poison"] = bad
    assert np.array_equal(out["rows"][~bad], clean[~bad]) and not np.isfinite(out["rows"][bad]).all(axis=1).all()
    assert np.isnan(out["scores"][bad]).all() and np.isfinite(out["scores"][~bad]).all()
    kinds = [np.isnan(out["rows"][bad]).any(), (out["rows"][bad] == np.inf).any(), (out["rows"][bad] == -np.inf).any(),
             (out["rows"][bad] == np.float32(FLT_MAX)).any(), (out["rows"][bad] == np.float32(-FLT_MAX)).any()]
    assert all(kinds)
    both_sides = [i for i in range(N_RANGES) if out["w_hi"][i] > out["w_lo"][i] > 0 and out["w_hi"][i] < len(bad)
                  and bad[out["w_lo"][i] - 1] and bad[out["w_hi"][i]]]
    lengths = [int(out["w_hi"][i] - out["w_lo"][i]) for i in both_sides]
    assert len(both_sides) >= 4 and any(n % 8 == 0 for n in lengths) and any(n % 8 for n in lengths), lengths
    out["both_sides"] = both_sides
    return out


def poison_free(fx):
    """the twin of ``poisoned``: zeros, rows and scores, in the same places"""
    out, gap = _with_gaps(fx)
    bad = _poison_mask(out, gap)
    out["rows"][bad] = 0.0
    out["scores"][bad] = 0.0
    out["poison"] = bad
    return out


# ---- long ranges ----------------------------------------------------------------------------------------------------------------
LONG = ((65, False), (1000, False), (2000, False), (2000, True))      # (members, every third row masked)
LONG_KINDS = ("clustered", "relu")


@functools.lru_cache(maxsize=None)
def _long_range(kind, n, thirds):
    rng = np.random.default_rng(600 + 7 * LONG_KINDS.index(kind) + n + thirds)
    scale = np.exp2(rng.integers(-3, 4, size=(n, 1)))
    if kind == "clustered":
        base = rng.standard_normal(DIM) + 0.05 * rng.standard_normal((n, DIM))
    else:
        base = np.maximum(rng.standard_normal((n, DIM)), 0.0)
    rows = (base * scale).astype(np.float32)
    kept = np.ones(n, bool)
    if thirds:
        kept[2::3] = False
    fx = dict(rows=rows, scores=rng.random((n, 3), dtype=np.float32), kept=kept, w_lo=np.array([0], np.int64), w_hi=np.array([n], np.int64))
    coherence = coherence_gram(rows, np.flatnonzero(kept))
    assert abs(coherence - (0.9988 if kind == "clustered" else 0.57)) < (2e-4 if kind == "clustered" else 0.02), coherence
    assert np.isfinite(rows).all() and len(set(np.frexp(np.abs(rows).max(axis=1))[1].tolist())) >= 7
    return fx


def long_ranges():
    """[(kind, members, every third masked, fixture)]: one interval of 65, 1000 and 2000 kept members, and one of 2000 members of
    which every third is masked, of clustered rows (c + 0.05 noise: coherence 0.9988, the worst case for the growth of the
    sequential sum) and of ReLU rows (max(N(0, 1), 0): coherence 0.57, the shape encoder rows have); per-row scales 2^[-3, 3]"""
    return [(kind, n, thirds, _long_range(kind, n, thirds)) for kind in LONG_KINDS for n, thirds in LONG]


# ---- scales ---------------------------------------------------------------------------------------------------------------------
N_BASE = 24
ONE_HOT_K = (-149, -126, -64, -63, 0, 63, 64, 127)
OPPOSITE = ((60, -60), (0, 100), (-100, 0))
FIVE_SCALES = (-140, -60, 0, 60, 120)


def _exact_scale(r, e):
    """r * 2^e, float32, asserted exact"""
    out = (r.astype(np.float64) * np.exp2(np.float64(e))).astype(np.float32)
    assert np.array_equal(out.astype(np.float64), r.astype(np.float64) * np.exp2(np.float64(e)))
    return out


@functools.lru_cache(maxsize=None)
def _scaled():
    rng = np.random.default_rng(503)
    base = signed(rng, N_BASE)
    groups = {}                                                    # name -> (rows, twin rows or None)
    # (a) huge: the largest |element| of every row in [2^126, FLT_MAX]
    _, ex = np.frexp(np.abs(base).max(axis=1))
    huge = np.stack([_exact_scale(base[i], 127 + (i % 2) - ex[i]) for i in range(N_BASE)])
    _, hx = np.frexp(np.abs(huge).max(axis=1))
    assert set(hx.tolist()) == {127, 128} and np.isfinite(huge).all()
    groups["huge"] = (huge, base)
    # (b) subnormal: times 2^-140 in float64, then rounded; the twin is that row times 2^140, which is exact
    tiny = (base.astype(np.float64) * 2.0 ** -140).astype(np.float32)
    assert (np.abs(tiny) < FLT_MIN).all() and ((tiny != 0).sum(axis=1) > 400).all()
    groups["subnormal"] = (tiny, np.stack([_exact_scale(t, 140) for t in tiny]))
    # (c) one direction at five scales; the subnormal member has lost mantissa bits
    d = base[0] / np.float32(2.0 ** int(ex[0] - 1))                # largest |element| in [1, 2)
    five = np.stack([(d.astype(np.float64) * 2.0 ** e).astype(np.float32) if e == FIVE_SCALES[0] else _exact_scale(d, e) for e in FIVE_SCALES])
    assert (np.abs(five[0]) < FLT_MIN).all() and five[0].any() and np.isfinite(five).all()
    groups["five_scales"] = (five, np.stack([_exact_scale(five[0], 140)] + [d] * 4))
    # (d) opposite directions at scales far apart
    for a, b in OPPOSITE:
        pair = np.stack([_exact_scale(d, a), _exact_scale(-d, b)])
        assert (np.abs(pair[pair != 0]) >= FLT_MIN).all()
        groups[f"opposite_{a}_{b}"] = (pair, np.stack([d, -d]))
    # (e) one-hot rows: the f32 squared norm is 0, subnormal, FLT_MIN, exact or inf
    for n, k in enumerate(ONE_HOT_K):
        for sign in (1.0, -1.0):
            hot, twin = np.zeros((1, DIM), np.float32), np.zeros((1, DIM), np.float32)
            j = (0, 7, 300, 511)[n % 4]
            hot[0, j], twin[0, j] = np.float32(sign * 2.0 ** k), sign
            assert hot[0, j] != 0 and np.isfinite(hot[0, j]) and float(hot[0, j]) == sign * 2.0 ** k
            groups[f"one_hot_{k}_{'+' if sign > 0 else '-'}"] = (hot, twin)
    with np.errstate(over="ignore", under="ignore"):
        n2 = {k: np.float32(2.0 ** k) * np.float32(2.0 ** k) for k in ONE_HOT_K}
        assert n2[-149] == 0 and 0 < n2[-64] < FLT_MIN and n2[-63] == np.float32(FLT_MIN) and n2[0] == 1 and np.isfinite(n2[63]) \
            and np.isinf(n2[64]) and np.isinf(n2[127])
    # (f) the twins follow their intervals
    names, twin_of, rows, lo, hi, at = [], {}, [], [], [], 0
    for name, (r, twin) in groups.items():
        for nm, block in ((name, r), (name + "/twin", twin)):
            names.append(nm)
            rows.append(block)
            lo.append(at)
            hi.append(at + len(block))
            at += len(block)
        twin_of[name] = name + "/twin"
    rows = np.concatenate(rows).astype(np.float32)
    assert valid_rows(rows).all()
    return dict(rows=rows, scores=rng.random((at, 3), dtype=np.float32), kept=np.ones(at, bool), w_lo=np.array(lo, np.int64),
                w_hi=np.array(hi, np.int64), names=names, twin_of=twin_of)


def scaled():
    """Intervals of rows at the ends of the float32 range, each followed by its unscaled twin (``names``; ``twin_of`` maps a name to
    its twin's): "huge" (24 signed rows, largest |element| in [2^126, FLT_MAX]), "subnormal" (the same rows times 2^-140: every
    element subnormal or zero), "five_scales" (one direction at 2^-140, 2^-60, 1, 2^60, 2^120), "opposite_a_b" (d 2^a and -d 2^b) and
    single-member "one_hot_k_+" / "one_hot_k_-" (+-2^k e_j).  Every row is valid; all are kept."""
    fx = _scaled()
    return dict(fx, rows=fx["rows"].copy())


def interval(fx, name):
    return fx["names"].index(name)


# ---- both strands ---------------------------------------------------------------------------------------------------------------
N_BOTH = 64
BOTH_KINDS = ("negated", "permuted", "independent")


def both_strands(kind):
    """the first 64 rows of ``cuts`` with its ranges and mask (the range across row 64 is cut there) and ``rows_rev``: the negated rows,
    the rows permuted within each range, or independent signed rows"""
    fx = cuts()
    live = fx["w_lo"] < N_BOTH
    out = dict(rows=fx["rows"][:N_BOTH], scores=fx["scores"][:N_BOTH], kept=fx["kept"][:N_BOTH], w_lo=fx["w_lo"][live],
               w_hi=np.minimum(fx["w_hi"][live], N_BOTH))
    assert int(out["w_hi"][-1]) == N_BOTH and len(out["w_lo"]) == 12
    rng = np.random.default_rng(504)
    if kind == "negated":
        rev = -out["rows"]
    elif kind == "permuted":
        rev = out["rows"].copy()
        for a, b in zip(out["w_lo"], out["w_hi"]):
            rev[a:b] = out["rows"][a + rng.permutation(b - a)]
        assert not np.array_equal(rev, out["rows"])
    else:
        rev = signed(rng, N_BOTH)
    out["rows_rev"] = np.ascontiguousarray(rev, dtype=np.float32)
    return out
