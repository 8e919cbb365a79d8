"""What tests/test_match_limits_gpu.py leans on, without a GPU: every input of tests/match_limits_data.py is made and has the matches,
ties, zeros and band counts the GPU tests are written for - from fp64 alone -, the band of every input compared by the band rule holds
at most 10 % as many pairs as there are matches, and every comparison helper accepts the numpy definition
(sequence.threshold_matches) and rejects a CSR that is wrong in one place: a match left out, one let in below the band, two columns
swapped, a value off by 2e-5, a -0 where +0 belongs.  The device is not touched: a failure here is a failure of a test input or of a
helper, not of a kernel."""
import numpy as np
import pytest

from genomad_amd import sequence
from tests import embedding_limits_data as lim
from tests import graph_limits_data as gd
from tests import match_limits_data as md
from tests.clusters_data import planted
from tests.embedding_limits_data import GAP, VALUE_TOL
from tests.neighbours_data import sims64
from tests.test_graph_limits_host import negative_zero, shifted, swapped, with_edge, without


def definition(q, b, t, metric="cosine"):
    """the definition's CSR with sim as the device returns it: float32"""
    indptr, col, sim = sequence.threshold_matches(q, b, t, metric)
    return indptr, col, sim.astype(np.float32)


# ---- the inputs ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nq, nb", md.SHAPES)
def test_signed_sides_have_negative_matches_and_a_narrow_band(nq, nb):
    q, b, s64 = md.signed_sides(nq, nb)
    assert s64.shape == (nq, nb) and 0.4 < (s64 < 0).mean() < 0.6 and not (s64 == 0).any()
    for t in gd.SIGN_THRESHOLDS:
        matches, band = md.band_counts(s64, t)
        assert md.band_is_narrow(s64, t) and matches > 10000, (t, matches, band)
        assert len(sequence.threshold_matches(q, b, t)[1]) == matches
    assert ((s64 >= -0.05 + GAP) & (s64 < -GAP)).sum() > 5000        # at -0.05 negative values must come out


def test_integer_sides_have_ties_zeros_and_the_negated_row():
    q, b, dots = md.integer_sides()
    neg, pos = lim.integer_thresholds(lim.signed_integer_rows(gd.N_INTEGER))
    assert (neg, pos) == (-131.0, 133.0) and q.shape == (133, 512) and b.shape == (211, 512)
    assert (dots == neg).sum() > 10 and (dots == pos).sum() > 10 and (dots == 0).sum() > 10
    for t in (neg, pos):
        assert md.same_bits(md.exact_csr(dots, t), definition(q, b, t, "dot"))
    # the negated row against row 3 and its copies: -dots[3, 3] is far below the negative threshold, so it matches none of them
    assert -dots[3, 0] < neg and not (dots[77, [0, 19, 210]] >= neg).any()
    assert dots[77, 1] >= pos and (dots[3, [0, 19, 210]] >= pos).all()         # itself, and row 3 its three copies
    zeros = md.exact_csr(dots, neg)[2] == 0
    assert zeros.sum() == (dots == 0).sum() and (md.exact_csr(dots, neg)[2][zeros].view(np.uint32) == 0).all()


def test_prefixes_and_scan_cases():
    for n in gd.PREFIXES:
        for nq, nb in ((n, gd.N_INTEGER), (70, n)):
            q, b, dots = md.integer_prefix(nq, nb)
            assert q.shape == (nq, 512) and b.shape == (nb, 512) and (dots == np.round(dots)).all()
            for t in lim.integer_thresholds(lim.signed_integer_rows(gd.N_INTEGER)):
                assert md.same_bits(md.exact_csr(dots, t), definition(q, b, t, "dot"))
                assert len(md.exact_csr(dots, t)[1]) > 0
    q, b, _ = md.integer_prefix(70, 64)
    assert not any(np.array_equal(x, y) for x, y in zip(q, b))        # rows that differ
    assert [md.counters(nq, md.SCAN_BASE, split) for nq, split, _ in md.SCAN_CASES] == [total for _, _, total in md.SCAN_CASES]
    assert [total for _, _, total in md.SCAN_CASES] == [1023, 1024, 1026]
    assert [-(-total // gd.SCAN_THREADS) for _, _, total in md.SCAN_CASES] == [1, 1, 2]
    assert all(nq <= gd.N_INTEGER for nq, _, _ in md.SCAN_CASES)
    assert md.counters(75, lim.NB_CAPPED, 1 << 20) == 150 and md.counters(133, 333, 100) == 133 * 3


def test_slab_queries_have_their_plants_and_a_narrow_band():
    q, pairs, triple = md.slab_queries()
    assert q.shape == (lim.NQ_SLABS, 512) and lim.NQ_SLABS > lim.QSLAB
    base = q[:md.SLAB_BASE]
    mine = md.slab_sample()
    s64 = sims64(q[mine], base)
    matches, band = md.band_counts(s64, md.SLAB_THRESHOLD)
    assert md.band_is_narrow(s64, md.SLAB_THRESHOLD) and matches > 1000, (matches, band)
    where = {int(i): k for k, i in enumerate(mine)}
    assert abs(s64[where[lim.QSLAB], 5] - 1) < 1e-12                                  # row 16384 = 2 x row 5
    assert abs(s64[where[triple[1]], triple[0]] - 1) < 1e-12 and abs(s64[where[triple[2]], triple[0]] - 1) < 1e-12
    assert pairs[0] == (5, lim.QSLAB) and triple[0] < md.SLAB_BASE
    mirror = sims64(base, q)                                          # (333, 16454)
    assert md.band_is_narrow(mirror, md.SLAB_THRESHOLD)


def test_two_range_sides_have_their_plants_and_a_row_with_matches_in_both_ranges():
    q, base = md.two_range_sides()
    s64 = sims64(q, base)
    t = md.TWO_RANGE_THRESHOLD
    matches, band = md.band_counts(s64, t)
    assert md.band_is_narrow(s64, t) and (matches, band) == (1824, 1)
    for i, at in enumerate(lim.CAPPED_PLANTS):
        assert abs(s64[i, at] - 1) < 1e-12 and abs(s64[70 + i, at] - 1) < 1e-12
    assert all(abs(s64[5, at] - 1) < 1e-12 for at in lim.CAPPED_TIE)
    clear = s64 >= gd.threshold32(t) + GAP
    both = clear[:, :lim.SPLIT_MAX].any(axis=1) & clear[:, lim.SPLIT_MAX:].any(axis=1)
    assert both.sum() == 47 and both[3] and both[4]                   # e.g. queries 3 and 4: their plants are at 65280 and 65349
    assert clear[:, lim.SPLIT_MAX:].sum() == 57


def test_row_scale_inputs():
    base = lim.extreme_base()
    q = lim.extreme_queries(base)
    assert sequence.valid_rows(q).all() and sequence.valid_rows(base).all()
    s64 = sims64(q, base)
    for t in (0.05, 0.5):
        matches, band = md.band_counts(s64, t)
        assert md.band_is_narrow(s64, t) and matches > 20, (t, matches, band)
    out = lim.out_of_range_base()
    assert sequence.valid_rows(out, "dot").all()
    old, new = md.invalid_halves()
    for metric, bad in (("cosine", 3), ("dot", 2)):
        assert (~sequence.valid_rows(old, metric)).sum() == bad and (~sequence.valid_rows(new, metric)).sum() == bad


def test_contract_rows():
    p, _ = planted()
    q, b = p[:133], p
    assert len(sequence.threshold_matches(q, b, 0.8)[1]) == 488
    cq, cb = gd.complete_rows(p, 133), gd.complete_rows(p, 333)
    indptr, col, sim = sequence.threshold_matches(cq, cb, 0.8)
    assert len(col) == 133 * 333 and (np.abs(sim - 1) < 1e-12).all()


# ---- the helpers: each accepts the definition and rejects a CSR that is wrong in one place ------------------------------------------

def wrong_csrs(right, s64, t):
    """the wrong CSRs of a right one; None where the input has no exact zero"""
    t = gd.threshold32(t)
    a, b = md.check_csr(right, *s64.shape)
    val = s64[a, b]
    clear = np.flatnonzero(val >= t + GAP)
    out = clear[np.argmin(val[clear])]                                # the match nearest the band: the helper must still miss it
    cand = np.argwhere(s64 < t - GAP)
    i, j = cand[np.argmax(s64[cand[:, 0], cand[:, 1]])]               # the pair nearest below the band
    twin = next(e for e in range(len(a) - 1) if a[e] == a[e + 1])
    zero = np.flatnonzero(val == 0)
    return {"a match left out": without(right, out), "a match let in": with_edge(right, i, j, np.float32(s64[i, j])),
            "two columns swapped": swapped(right, twin), "a value off by 2e-5": shifted(right, clear[0], 2e-5),
            "a value off by -2e-5": shifted(right, clear[-1], -2e-5),
            "-0 where +0 belongs": negative_zero(right, zero[0]) if len(zero) else None}


def _assert(ok):
    assert ok


def test_every_helper_accepts_the_definition_and_rejects_each_wrong_csr():
    q, b, dots = md.integer_sides()
    t = -131.0                                                        # the zero dots are matches
    right = definition(q, b, t, "dot")
    mine = np.arange(len(q))
    helpers = {"check_band": lambda got: md.check_band(got, dots, t), "check_exact": lambda got: md.check_exact(got, dots, t),
               "same_bits": lambda got: _assert(md.same_bits(got, right)),
               "rows_of": lambda got: (md.band_rule(md.rows_of(got, mine, len(b))[0], dots, t),
                                       md.value_rule(*md.rows_of(got, mine, len(b)), dots))}
    wrong = wrong_csrs(right, dots, t)
    assert all(w is not None for w in wrong.values())
    for name, helper in helpers.items():
        helper(right)
        for what, csr in wrong.items():
            with pytest.raises(AssertionError):
                helper(csr)
                print(f"{name} accepted {what}")
    a, _ = md.check_csr(right, *dots.shape)
    tie = without(right, int(np.flatnonzero(dots[a, right[1]] == t)[0]))      # what the band leaves free and the exact comparison does not
    md.check_band(tie, dots, t)
    with pytest.raises(AssertionError):
        md.check_exact(tie, dots, t)
    with pytest.raises(AssertionError):                               # a column beyond the base
        md.check_csr((right[0], np.where(np.arange(len(right[1])) == 0, len(b), right[1]).astype(np.int32), right[2]), len(q), len(b))


@pytest.mark.parametrize("t", gd.SIGN_THRESHOLDS)
def test_the_band_helper_on_signed_cosine_rows(t):
    q, b, s64 = md.signed_sides(133, 333)
    right = definition(q, b, t)
    assert md.check_band(right, s64, t) <= 1e-7
    wrong = wrong_csrs(right, s64, t)
    assert wrong.pop("-0 where +0 belongs") is None
    for what, csr in wrong.items():
        with pytest.raises(AssertionError):
            md.check_band(csr, s64, t)
            print(f"check_band accepted {what}")
    e = int(np.argmax(right[2] < 0.99))
    md.check_band(shifted(right, e, 0.9 * VALUE_TOL), s64, t)       # VALUE_TOL itself passes


def test_without_rows_renumbers_and_refuses_a_match_at_a_dropped_row():
    q, b, dots = md.integer_sides()
    right = definition(q, b, -131.0, "dot")
    keep_q, keep_b = np.delete(np.arange(len(q)), [7]), np.delete(np.arange(len(b)), [9])
    with pytest.raises(AssertionError):
        md.without_rows(right, keep_q, keep_b, len(q), len(b))       # row 7 has matches
    a, c = md.check_csr(right, len(q), len(b))
    stay = (a != 7) & (c != 9)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(a[stay], minlength=len(q)))]).astype(np.int64)
    got = md.without_rows((indptr, right[1][stay], right[2][stay]), keep_q, keep_b, len(q), len(b))
    assert md.same_bits(got, definition(q[keep_q], b[keep_b], -131.0, "dot"))
