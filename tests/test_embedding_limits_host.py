"""The inputs of tests/test_embedding_limits_gpu.py, on the CPU: every generator of tests/embedding_limits_data.py is run (their
conditions are assertions inside them), the share of rows that qualify for the exact-order check is asserted from fp64 alone for every
input that check is applied to (the 90 % cap of tests/test_neighbours_gpu.py), and the exactness the GPU tests lean on is established:
integer dots below 2^24, power-of-two scalings that change no significand, the properties of negative_contest against the brute-force
walk and the numpy definitions, and what the split into f16 limbs alone costs the dot metric (the element range that
include/genomad_nn.h states).  The device is not touched: a failure here is a failure of a test input, not of a kernel."""
import numpy as np

from genomad_amd import sequence
from tests import embedding_limits_data as lim
from tests.clusters_data import components
from tests.neighbours_data import rows, sims64
from tests.representatives_data import walk


def share(s64, k):
    return float(lim.qualifies(s64, k).mean())


def test_signed_and_heavy_rows_qualify_for_the_order_check_as_stated():
    q, b = lim.signed_rows(70, 7), lim.signed_rows(333, 8)
    pairs, own = sims64(q, b), lim.self64(b)
    assert 0.49 < (pairs < 0).mean() < 0.52 and 0.49 < (own[np.isfinite(own)] < 0).mean() < 0.52
    got = [share(pairs, 1), share(own, 1), share(pairs, 10), share(own, 10)]
    assert got[0] == got[1] == 1.0 and abs(got[2] - 0.943) < 5e-4 and abs(got[3] - 0.952) < 5e-4, got
    q, b = lim.heavy_rows(70, 7), lim.heavy_rows(333, 8)
    pairs, own = sims64(q, b), lim.self64(b)
    got = [share(pairs, 1), share(own, 1), share(pairs, 10), share(own, 10)]
    assert got[0] == got[1] == 1.0 and abs(got[2] - 0.986) < 5e-4 and abs(got[3] - 0.988) < 5e-4, got
    assert min(got) >= lim.CAP
    # Of 333 signed base rows about 166 are on a query's positive side: its 64 best are all positive.  The lists that must END in
    # negative values are those of the first 80 base rows, where the 64th best of every row is negative
    q, b = lim.signed_rows(70, 7), lim.signed_rows(333, 8)
    assert (-np.sort(-sims64(q, b), axis=1)[:, 63] > 0).all()
    b = b[:lim.NEGATIVE_TAIL_BASE]
    for s in (sims64(q, b), lim.self64(b)):
        assert (-np.sort(-s, axis=1)[:, 63] < -lim.GAP).all() and (-np.sort(-s, axis=1)[:, 0] > lim.GAP).all()


def test_query_slab_inputs():
    q, b = lim.signed_rows(lim.NQ_SLABS, 30), lim.signed_rows(333, 8)
    assert len(q) == 16454 > lim.QSLAB
    s = sims64(q, b)
    got = share(s, 1), share(s, 10)
    assert got[0] >= 0.99 and abs(got[1] - 0.943) < 5e-3 and min(got) >= lim.CAP, got
    r, pairs, triple = lim.slab_rows()
    edge = np.concatenate([np.arange(64), np.arange(lim.QSLAB - 64, lim.NQ_SLABS)])
    assert len(edge) == 198 and r.shape == (16454, 512)
    own = lim.self64(r, edge)
    at = {int(i): n for n, i in enumerate(edge)}
    for a, b_ in pairs:                                            # planted across the border, each the other's best by a wide margin
        assert a < lim.QSLAB <= b_ or a < lim.QSLAB - 1 < b_
        for x, y in ((a, b_), (b_, a)):
            if x in at:
                row = own[at[x]]
                assert int(np.argmax(row)) == y and abs(row[y] - 1) < 1e-12 and np.sort(row)[-2] < 0.5
    assert triple == (100, 16447, 16453)
    assert np.array_equal(r[triple[0]], r[triple[1]]) and np.array_equal(r[triple[0]], r[triple[2]])
    row = own[at[triple[2]]]
    assert np.sort(row)[-3] < 0.5 and set(np.argsort(row)[-2:]) == {100, 16447}


def test_capped_base_inputs():
    q = rows(70, 7)
    base = lim.capped_base(q)
    assert base.shape == (lim.SPLIT_MAX + 70, 512) and lim.CAPPED_PLANTS == (32767, 32768, 65279, 65280, 65349)
    assert lim.CAPPED_TIE == (32769, 65278)
    s = sims64(q, base)
    assert share(s, 1) >= lim.CAP                                  # k = 10 does not reach the cap at this base size: order at k = 1 only
    print(f"\ncapped base: {share(s, 1):.1%} of the rows qualify at k = 1, {share(s, 10):.1%} at k = 10")
    assert share(s, 10) < lim.CAP
    best = lim.order64(s, 2)
    assert list(best[:5, 0]) == list(lim.CAPPED_PLANTS) and list(best[5]) == list(lim.CAPPED_TIE)
    for i, at in enumerate(lim.CAPPED_PLANTS):                     # exact multiples: the device sees the query's own fragments
        assert np.array_equal(base[at].astype(np.float64), q[i].astype(np.float64) * 2.0 ** (i - 2))
    assert (np.sort(s[:6], axis=1)[:, -3] < 0.9).all()             # nothing else comes near the plants


def test_signed_integer_rows_are_exact_and_have_ties_at_both_thresholds():
    r = lim.signed_integer_rows(200)
    dots = r.astype(np.float64) @ r.astype(np.float64).T
    assert np.abs(dots).max() <= 512 * 16 < 2 ** 24
    upper = dots[np.triu_indices(200, 1)]
    for t in lim.integer_thresholds(r):
        assert (upper == t).sum() > 10
    neg, pos = lim.integer_thresholds(r)
    assert neg < 0 < pos and 0.02 < (upper >= pos).mean() < 0.98 and 0.02 < (upper < neg).mean()
    # the definitions agree with their brute-force doubles on these rows: what the GPU tests compare with is right
    w = np.random.default_rng(3).integers(0, 4, 200)
    for t in (neg, pos):
        assert all(np.array_equal(a, b) for a, b in zip(sequence.threshold_clusters(r, t, "dot"), components(dots >= t)))
        for weight in (None, w):
            rep, sim, size, rank, _ = sequence.greedy_representatives(r, t, weight, "dot")
            order = sequence.priority_order(weight, 200)
            rep_p, sim_p, size_p, _ = walk(dots[np.ix_(order, order)].tolist(), t)
            assert np.array_equal(rep[order], order[rep_p]) and np.array_equal(size[order], size_p)
            assert np.array_equal(sim[order].view(np.uint32), sim_p.view(np.uint32))
            assert 1 < int((rep == np.arange(200)).sum()) < 200
    # about 100 of 199 candidates are on a row's positive side: lists of 64 that END in negative values need the 80-row base
    _, sim = sequence.nearest_neighbours(r, r[:lim.NEGATIVE_TAIL_BASE], 64, "dot")
    assert (sim[:, -1] < 0).all() and (sim[:, 0] > 0).all()
    assert int(np.argmin(dots[3])) == 77                           # the negated row is the farthest of all


def test_negative_contest_has_the_properties_and_the_definition_decides_as_constructed():
    r, orders = lim.negative_contest()
    assert set(orders) == {"index", "cab"} and len(r) == 100
    for name, (weight, want) in orders.items():
        rep, sim, size, rank, rounds = sequence.greedy_representatives(r, lim.CONTEST_THRESHOLD, weight, "dot")
        assert [i for i in range(100) if rep[i] == i] == sorted(lim.CONTEST_REPS), name
        assert all(rep[m] == w for m, w in want.items()), name
        assert {int(rep[m]) for m in want} == set(lim.CONTEST_REPS)         # every representative wins somebody
        members = np.array(sorted(want))
        assert (sim[members] <= 0).all() and (sim[members] < 0).sum() >= 8
        zeros = members[sim[members] == 0]
        assert len(zeros) >= 1 and not np.signbit(sim[zeros]).any()          # the definition's zero is +0
        assert int(size[0]) + int(size[40]) + int(size[70]) == 100


def test_power_of_two_scalings_are_exact_and_the_extreme_rows_are_what_they_claim():
    r, q = lim.signed_rows(333, 8), lim.signed_rows(70, 7)
    lim.power_of_two_scaled(r, 3)
    lim.power_of_two_scaled(q, 4)
    base = lim.extreme_base()
    query = lim.extreme_queries(base)
    k = lim.EXTREME_KINDS
    assert (np.abs(base[k["huge"]]).max(axis=1) >= 2.0 ** 127).all() and np.isfinite(base).all() and np.isfinite(query).all()
    assert (np.abs(base[k["subnormal"]]) < lim.FLT_MIN).all() and (np.abs(query[6:12]) < lim.FLT_MIN).all()
    assert ((base[k["one_hot"]] != 0).sum(axis=1) == 1).all() and ((query[12:28] != 0).sum(axis=1) == 1).all()
    valid = np.sqrt((base.astype(np.float64) ** 2).sum(axis=1)) > 0                   # fp64 holds the square of a subnormal
    assert valid.all()
    s = sims64(query, base)
    assert np.isfinite(s).all() and np.abs(s).max() <= 1 + 1e-12
    _, pos, sign = lim.one_hot_rows()
    hot = s[12:28, k["one_hot"]]
    assert np.array_equal(hot, np.where(pos[:, None] == pos[None, :], sign[:, None] * sign[None, :], 0))
    assert {-1.0, 0.0, 1.0} == set(hot.ravel())
    # the order check on heavy rows alone
    hq, hb = lim.heavy_rows(70, 7), lim.heavy_rows(333, 8)
    assert min(share(sims64(hq, hb), kk) for kk in (1, 10)) >= lim.CAP and min(share(lim.self64(hb), kk) for kk in (1, 10)) >= lim.CAP


def test_what_the_f16_limbs_cost_the_dot_metric():
    """The split alone, in fp64 (the device adds its f32 accumulation): inside the stated element range the relative bound holds with
    room; four binades below its lower end it does not - the reason the header states a range."""
    for name, q, b in (("heavy, max 6e4", lim.dot_range_rows(70, 71), lim.dot_range_rows(333, 72)),
                       ("2^-7 .. 2^-3", lim.small_dot_rows(70, 81), lim.small_dot_rows(333, 82))):
        ratio = (np.abs(lim.split_f16_dots(q, b) - sims64(q, b, "dot")) / lim.dot_bound(q, b)).max()
        print(f"\ndot limbs, {name}: max |split-f16 dot - fp64 dot| / (1e-5 sum |x y|) = {ratio:.3f}")
        assert ratio < 1
    q, b = lim.signed_rows(70, 7) * np.float32(2.0 ** -14), lim.signed_rows(333, 8) * np.float32(2.0 ** -14)
    ratio = (np.abs(lim.split_f16_dots(q, b) - sims64(q, b, "dot")) / lim.dot_bound(q, b)).max()
    assert np.abs(q).max() < lim.DOT_RANGE_LOW and ratio > 1, ratio


def test_out_of_range_rows_are_valid_for_the_definition():
    r = lim.out_of_range_base()
    assert np.isfinite(r).all() and np.abs(r[list(lim.OUT_OF_RANGE)]).max() == 7e4 > 65504
    rest = np.delete(r, lim.OUT_OF_RANGE, axis=0)
    assert np.abs(rest).max() <= 4 and len(rest) == 331
    with np.errstate(over="ignore"):
        assert np.isinf(r.astype(np.float16)).sum() == 2           # what the device's high limb becomes
