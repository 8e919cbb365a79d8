"""What tests/test_graph_limits_gpu.py leans on, without a GPU: every input of tests/graph_limits_data.py is made (the generators
assert their own conditions) and has the edge counts, ties, zeros and band counts the GPU tests are written for - from fp64 alone -,
the band of every input compared by the band rule holds at most 10 % as many pairs as there are edges, and every comparison helper
accepts the numpy definition (sequence.threshold_graph) and rejects a CSR that is wrong in one place: an edge left out, an edge let
in, two columns swapped, a value off by 2e-5, a -0 where +0 belongs.  The device is not touched: a failure here is a failure of a
test input or of a helper, not of a kernel."""
import numpy as np
import pytest

from genomad_amd import sequence
from tests import embedding_limits_data as lim
from tests import graph_limits_data as gd
from tests.clusters_data import planted
from tests.embedding_limits_data import GAP, VALUE_TOL
from tests.neighbours_data import rows, sims64


def definition(r, t, metric="cosine"):
    """the definition's CSR with sim as the device returns it: float32"""
    indptr, col, sim = sequence.threshold_graph(r, t, metric)
    return indptr, col, sim.astype(np.float32)


# ---- the inputs ----------------------------------------------------------------------------------------------------------------------

def test_signed_rows_have_the_stated_edges_and_a_narrow_band():
    r = gd.signed_base()
    s = gd.upper64(r)
    assert [gd.band_counts(s, t) for t in gd.SIGN_THRESHOLDS] == [(40110, 10), (27568, 12), (15119, 9)]
    assert all(gd.band_is_narrow(s, t) for t in gd.SIGN_THRESHOLDS)
    assert ((s >= -0.05 + GAP) & (s < -GAP)).sum() > 10000            # at -0.05 negative sims must be present, whatever the band does
    assert not (s == 0).any()
    upper = np.sort(s[np.triu_indices(333, 1)])
    tenth = upper[len(upper) // 10]                                   # where the device's own 10th percentile will lie: negative
    assert tenth < -0.05 and ((upper > tenth - 1e-3) & (upper < tenth + 1e-3)).sum() > 100
    for t in gd.SIGN_THRESHOLDS:                                      # the definition's edges are the pairs at or above f32(t)
        assert len(sequence.threshold_graph(r, t)[1]) == gd.band_counts(s, t)[0]


def test_integer_rows_have_the_stated_ties_zeros_and_prefixes():
    r, dots = gd.integer_base()
    assert r.shape == (342, 512) and lim.integer_thresholds(r) == (-131.0, 133.0)
    neg, pos = lim.integer_thresholds(r)
    upper = dots[np.triu_indices(342, 1)]
    assert (upper == neg).sum() == 132 and (upper == pos).sum() == 107 and (upper == 0).sum() == 107
    assert np.abs(dots).max() < 2 ** 24 and (dots == np.round(dots)).all() and not np.signbit(dots[dots == 0]).any()
    for t in (neg, pos):                                              # exact_csr is the definition on these rows
        want = definition(r, t, "dot")
        assert gd.same_bits(gd.exact_csr(dots, t), want)
    zeros = gd.exact_csr(dots, neg)[2] == 0
    assert zeros.sum() == 107 and (gd.exact_csr(dots, neg)[2][zeros].view(np.uint32) == 0).all()       # edges at -131, and +0
    for n in gd.PREFIXES:
        d = dots[:n, :n][np.triu_indices(n, 1)]
        assert ((d >= neg).sum() > 0) and ((d >= pos).sum() > 0) == (n >= 31), n
    assert dots[0, 1] >= neg and dots[0, 1] < pos                     # n = 2: one pair, an edge at the negative threshold only
    assert {n for n in gd.PREFIXES if n > 2} == {31, 32, 33, 63, 64, 65, 255, 256, 257} and gd.PREFIX_SPLITS == (0, 32, 64, 96)
    # the scan: below its thread count, on it, and just above, where a thread's run is two counters
    assert [gd.counters(n, split) for n, split, _ in gd.SCAN_CASES] == [total for _, _, total in gd.SCAN_CASES] == [1023, 1024, 1026]
    assert [-(-total // gd.SCAN_THREADS) for _, _, total in gd.SCAN_CASES] == [1, 1, 2]
    assert all(n <= gd.N_INTEGER for n, _, _ in gd.SCAN_CASES)
    assert gd.counters(333, 100) == 333 * 3 and gd.counters(65350, 1 << 20) == 65350 * 2      # the rounding to 32, the cap


def test_row_scale_inputs_have_the_stated_edges():
    r = gd.signed_base()
    lim.power_of_two_scaled(r, 3)                                     # asserts that no bit of a significand changes
    base = lim.extreme_base()
    assert sequence.valid_rows(base).all()
    s = gd.upper64(base)
    assert gd.band_counts(s, 0.05) == (13356, 14) and gd.band_counts(s, 0.5) == (12, 0)
    assert gd.band_is_narrow(s, 0.05) and gd.band_is_narrow(s, 0.5)
    _, pos, sign = lim.one_hot_rows()
    hot = lim.EXTREME_KINDS["one_hot"]
    same = np.triu((pos[:, None] == pos[None, :]) & (sign[:, None] == sign[None, :]), 1)
    assert np.array_equal(s[hot, hot] >= 0.5, same) and (s[hot, hot][same] == 1.0).all()
    assert same.sum() == 12 == gd.band_counts(s, 0.5)[0]              # the 12 edges at 0.5 are the one-hot pairs, and nothing else
    assert set(s[hot, hot][np.triu_indices(16, 1)]) == {-1.0, 0.0, 1.0}
    s = gd.upper64(lim.heavy_rows(333, 8))
    assert gd.band_counts(s, 0.05) == (1297, 0) and gd.band_counts(s, 0.2) == (266, 0)
    base = lim.out_of_range_base()
    out = list(lim.OUT_OF_RANGE)
    assert out == [17, 250] and sequence.valid_rows(base, "dot").all()
    rest = np.delete(base, out, axis=0)
    dots = rest.astype(np.float64) @ rest.astype(np.float64).T
    assert (dots == np.round(dots)).all() and np.abs(dots).max() < 2 ** 24
    t = float(np.sort(dots[np.triu_indices(331, 1)])[int(331 * 330 / 2 * 0.98)])
    edges = len(gd.exact_csr(dots, t)[1])
    assert 1000 < edges < 1400 and (dots[np.triu_indices(331, 1)] == t).sum() > 1      # about 2 % of the pairs, a tie on the threshold
    assert gd.same_bits(gd.exact_csr(dots, t), definition(rest, t, "dot"))


def test_two_range_base_has_its_plants_and_the_stated_counts():
    base, pairs = gd.two_range_base()
    mine = gd.two_range_mine()
    t = gd.TWO_RANGE_THRESHOLD
    assert len(pairs) == 12 and all(a < b for a, b in pairs)
    for a, b in pairs:
        assert abs(sims64(base[a:a + 1], base[b:b + 1])[0, 0] - 1) < 1e-12
    assert sequence.valid_rows(base[mine]).all()
    s = lim.self64(base, mine)
    assert gd.touching_counts(s, mine, t) == (701, 2, 696, 690)      # entries, in the band, unordered pairs, column in the second range
    assert 2 <= gd.BAND_SHARE * 701
    plain = lim.capped_base(rows(70, 7))
    assert gd.touching_counts(lim.self64(plain, mine), mine, t) == (651, 2, 650, 649)
    # row 100: its copies are its only partners near 1, in this order, and the segment crosses from part 0 into part 1
    own = sims64(base[gd.COPIES_OF:gd.COPIES_OF + 1], base)[0]
    assert list(np.flatnonzero(own > 0.999)) == [gd.COPIES_OF, *gd.COPIES, lim.NB_CAPPED - 1]
    assert gd.COPIES[1] < lim.SPLIT_MAX <= gd.COPIES[2]


def test_contract_rows_are_sparse_and_complete():
    p, _ = planted()
    n = len(p)
    assert n == 333 and len(sequence.threshold_graph(p, 0.8)[1]) == 602 < n * (n - 1) // 2
    c = gd.complete_rows(p)
    assert c.shape == p.shape and sequence.valid_rows(c).all()
    indptr, col, sim = sequence.threshold_graph(c, 0.8)
    assert len(col) == n * (n - 1) // 2 == 55278 and (np.abs(sim - 1) < 1e-12).all()


# ---- the helpers: each accepts the definition and rejects a CSR that is wrong in one place ------------------------------------------

def row_of(csr, e):
    return int(np.searchsorted(csr[0], e, side="right") - 1)


def without(csr, e):
    indptr = csr[0].copy()
    indptr[row_of(csr, e) + 1:] -= 1
    return indptr, np.delete(csr[1], e), np.delete(csr[2], e)


def with_edge(csr, i, j, v):
    indptr = csr[0].copy()
    at = int(indptr[i] + np.searchsorted(csr[1][indptr[i]:indptr[i + 1]], j))
    indptr[i + 1:] += 1
    return indptr, np.insert(csr[1], at, j).astype(np.int32), np.insert(csr[2], at, v).astype(np.float32)


def swapped(csr, e):
    assert row_of(csr, e) == row_of(csr, e + 1)
    col, sim = csr[1].copy(), csr[2].copy()
    col[[e, e + 1]], sim[[e, e + 1]] = col[[e + 1, e]], sim[[e + 1, e]]
    return csr[0], col, sim


def shifted(csr, e, by):
    sim = csr[2].copy()
    sim[e] = np.float32(np.float64(sim[e]) + by)
    return csr[0], csr[1], sim


def negative_zero(csr, e):
    assert csr[2][e] == 0 and not np.signbit(csr[2][e])
    sim = csr[2].copy()
    sim[e] = np.float32(-0.0)
    return csr[0], csr[1], sim


def wrong_csrs(right, s64, t, seen):
    """the five wrong CSRs of a right one, each wrong at a pair (i, j) with seen(i, j); None where the input has no exact zero"""
    t = gd.threshold32(t)
    a, b = gd.check_csr(right, len(s64))
    ok = np.array([seen(i, j) for i, j in zip(a, b)])
    val = s64[a, b]
    clear = np.flatnonzero(ok & (val >= t + GAP))
    out = clear[np.argmin(val[clear])]                                # the edge nearest the band: the helper must still miss it
    cand = np.argwhere(np.isfinite(s64) & (s64 < t - GAP))
    cand = cand[[seen(i, j) for i, j in cand]]
    i, j = cand[np.argmax(s64[cand[:, 0], cand[:, 1]])]               # the pair nearest below the band
    twin = next(e for e in np.flatnonzero(ok[:-1]) if a[e] == a[e + 1])
    zero = np.flatnonzero(ok & (val == 0))
    return {"an edge left out": without(right, out), "an edge let in": with_edge(right, i, j, np.float32(s64[i, j])),
            "two columns swapped": swapped(right, twin), "a value off by 2e-5": shifted(right, clear[0], 2e-5),
            "a value off by -2e-5": shifted(right, clear[-1], -2e-5),
            "-0 where +0 belongs": negative_zero(right, zero[0]) if len(zero) else None}


def check_touching(got, s64, t, mine):
    """how group D compares: the edges that touch ``mine``, as row or as column, by the band rule and the value rule"""
    mask, val = gd.touching(got, mine, len(s64))
    full = np.maximum(s64, s64.T)[mine]                               # upper64 is -inf below the diagonal; the own pair stays -inf
    gd.band_rule(mask, full, t)
    return gd.value_rule(mask, val, full)


def test_every_helper_accepts_the_definition_and_rejects_each_wrong_csr():
    r, dots = gd.integer_base()
    t = lim.integer_thresholds(r)[0]                                  # -131: the 107 zero dots are edges
    s64 = dots.copy()
    s64[np.tril_indices(len(r))] = -np.inf
    right = definition(r, t, "dot")
    mine = np.arange(1, len(r), 2)
    helpers = {"check_band": lambda got: gd.check_band(got, s64, t), "check_exact": lambda got: gd.check_exact(got, dots, t),
               "same_bits": lambda got: _assert(gd.same_bits(got, right)), "touching": lambda got: check_touching(got, s64, t, mine)}
    wrong = wrong_csrs(right, s64, t, lambda i, j: i % 2 == 1 or j % 2 == 1)
    assert all(w is not None for w in wrong.values())
    for name, helper in helpers.items():
        helper(right)
        for what, csr in wrong.items():
            with pytest.raises(AssertionError):
                helper(csr)
                print(f"{name} accepted {what}")
    # what the band leaves free and the exact comparison does not: a tie on the threshold left out
    a, b = gd.check_csr(right, len(r))
    tie = without(right, int(np.flatnonzero(dots[a, b] == t)[0]))
    gd.check_band(tie, s64, t)
    with pytest.raises(AssertionError):
        gd.check_exact(tie, dots, t)


@pytest.mark.parametrize("t", gd.SIGN_THRESHOLDS)
def test_the_band_helper_on_signed_cosine_rows(t):
    r = gd.signed_base()
    s64 = gd.upper64(r)
    right = definition(r, t)
    assert gd.check_band(right, s64, t) <= 1e-7                       # the f32 rounding of the fp64 value
    wrong = wrong_csrs(right, s64, t, lambda i, j: True)
    assert wrong.pop("-0 where +0 belongs") is None                   # no pair of these rows is exactly orthogonal
    for what, csr in wrong.items():
        with pytest.raises(AssertionError):
            gd.check_band(csr, s64, t)
            print(f"check_band accepted {what}")
    # inside the band the rule decides nothing: the pair nearest the threshold may go either way
    a, b = gd.check_csr(right, 333)
    near = int(np.argmin(np.abs(s64[a, b] - gd.threshold32(t))))
    assert abs(s64[a[near], b[near]] - gd.threshold32(t)) < GAP
    gd.check_band(without(right, near), s64, t)


def test_value_rule_bounds():
    """VALUE_TOL itself passes and 2e-5 does not; renumbered drops rows without edges and refuses an edge at a dropped row"""
    r = gd.signed_base()[:65]
    s64 = gd.upper64(r)
    right = definition(r, 0.0)
    mask, val = gd.dense(right, 65)
    assert gd.value_rule(mask, val, s64) < 1e-7
    e = int(np.argmax(right[2]))
    gd.check_band(shifted(right, e, 0.9 * VALUE_TOL), s64, 0.0)
    with pytest.raises(AssertionError):
        gd.check_band(shifted(right, e, 2e-5), s64, 0.0)
    r, dots = gd.integer_base()                                       # exact values: the definition on fewer rows gives the same bits
    r, t = r[:65], -131.0
    right = definition(r, t, "dot")
    keep = np.delete(np.arange(65), [7])
    with pytest.raises(AssertionError):
        gd.renumbered(right, keep, 65)                                # row 7 has edges
    a, b = gd.check_csr(right, 65)
    stay = (a != 7) & (b != 7)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(a[stay], minlength=65))]).astype(np.int64)
    got = gd.renumbered((indptr, right[1][stay], right[2][stay]), keep, 65)
    assert gd.same_bits(got, definition(r[keep], t, "dot"))


def _assert(ok):
    assert ok
