"""What tests/test_linkage_limits_gpu.py leans on, without a GPU: every generator of tests/linkage_limits_data.py runs (each asserts its
own conditions), its tree under the numpy definition has the stated shape, the brute-force Kruskal of tests/linkage_data.py - which
shares no code with the definition - gives the same tree, so the two references do not share a mistake, and the plain Boruvka counts
the rounds the device tests expect."""
import math

import numpy as np
import pytest

from genomad_amd import sequence
from tests import embedding_limits_data as lim
from tests import linkage_limits_data as ld
from tests.linkage_data import kruskal


def same_tree(got, want):
    """(a, b, sim) of the brute force over float64 values against the definition's: indices, and the values rounded as it rounds them"""
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2].astype(np.float32), want[2])


def ordered(a, b, sim):
    order = list(zip((-sim.astype(np.float64)).tolist(), a.tolist(), b.tolist()))
    return order == sorted(order) and bool((a < b).all())


def test_corners_three_negative_edges_decided_by_contests():
    r, g = ld.corners()
    a, b, sim, valid = want = sequence.single_linkage_tree(r, "dot")
    assert len(a) == 332 and valid.all() and ordered(a, b, sim)
    assert np.flatnonzero(sim < 0).tolist() == [329, 330, 331] and len(set(sim[-3:])) == 3
    dots = ld.dots64(r)
    lo, hi = np.triu_indices(333, 1)
    cross = dots[lo, hi][g[lo] != g[hi]]
    assert cross.max() == sim[-3] and (cross < 0).all() and len(cross) > 30000           # the best of that many negative values
    assert dots[lo, hi][g[lo] == g[hi]].min() > 2000
    assert same_tree(kruskal(dots), want[:3])
    rounds, taken = ld.boruvka(dots)
    assert taken == set(zip(a.tolist(), b.tolist())) and 2 <= rounds <= math.ceil(math.log2(333))
    a, b, sim, valid = sequence.single_linkage_tree(r)                                   # and under cosine
    assert len(a) == 332 and np.flatnonzero(sim < 0).tolist() == [329, 330, 331]


def test_simplex_star_is_a_star_of_negative_edges_in_one_round():
    r, centre = ld.simplex_star()
    a, b, sim, valid = want = sequence.single_linkage_tree(r, "dot")
    assert len(a) == 332 and valid.all() and ordered(a, b, sim) and (sim <= -8).all()
    assert 100 < len(set(sim)) < 332 and ((a == centre) | (b == centre)).all()
    dots = ld.dots64(r)
    assert dots[np.triu_indices(333, 1)].max() <= -8
    assert same_tree(kruskal(dots), want[:3])
    rounds, taken = ld.boruvka(dots)
    assert rounds == 1 and taken == set(zip(a.tolist(), b.tolist()))


def test_ruler_path_is_a_tied_path_that_needs_every_round():
    r = ld.ruler_path()
    a, b, sim, valid = want = sequence.single_linkage_tree(r, "dot")
    assert len(a) == 255 and valid.all() and ordered(a, b, sim) and (b - a == 1).all()
    assert sorted(set(sim.tolist())) == [9, 10, 11, 12, 13, 14, 15, 16]
    dots = ld.dots64(r)
    assert same_tree(kruskal(dots), want[:3])
    rounds, taken = ld.boruvka(dots)
    assert rounds == 8 == math.ceil(math.log2(256)) and taken == set(zip(a.tolist(), b.tolist()))
    # the device test's second case.  Without row 255 the last block is joined by a pick that is not mutual, a round early
    rounds, taken = ld.boruvka(dots, np.arange(256) < 255)
    assert rounds == 7 and taken == set(zip(a[b < 255].tolist(), b[b < 255].tolist()))
    assert ld.boruvka(ld.dots64(ld.ruler_path(64)))[0] == 6 and ld.boruvka(ld.dots64(ld.ruler_path(128)))[0] == 7


def test_dead_tiles_leave_279_rows_and_a_tied_tree():
    r, dead = ld.dead_tiles()
    a, b, sim, valid = want = sequence.single_linkage_tree(r, "dot")
    ok = valid.astype(bool)
    assert np.array_equal(np.flatnonzero(~ok), dead) and int(ok.sum()) == 279
    assert len(a) == 278 and len(set(sim)) == 144 and ordered(a, b, sim)
    assert not np.isin(dead, np.concatenate([a, b])).any()
    dots = ld.dots64(np.where(ok[:, None], r, 0))
    assert (dots == np.round(dots)).all() and np.abs(dots).max() < 2 ** 24
    assert same_tree(kruskal(dots, ok), want[:3])
    rounds, taken = ld.boruvka(dots, ok)
    assert taken == set(zip(a.tolist(), b.tolist())) and rounds <= math.ceil(math.log2(279))
    r[64] = 0                                                                            # the cosine case of the device test
    assert np.array_equal(np.flatnonzero(sequence.single_linkage_tree(r)[3] == 0), np.sort(np.append(dead, 64)))


def test_forest_rows_map_to_the_tree_of_the_kept_rows():
    r, out, keep = ld.forest_rows()
    a, b, sim, valid = sequence.single_linkage_tree(r[keep], "dot")
    assert len(a) == 265 and valid.all() and np.flatnonzero(sim < 0).tolist() == [262, 263, 264]
    full = sequence.single_linkage_tree(r, "dot")
    assert len(full[0]) == 332 and full[3].all()             # fp64 holds 7e4: not the reference for the full array
    # the brute force on the matrix the device sees - NaN in the rows and columns of ``out`` - is the mapped tree of the kept rows
    fa, fb, fs = kruskal(ld.nan_rows_and_columns(ld.dots64(r), out))
    assert np.array_equal(fa, keep[a]) and np.array_equal(fb, keep[b]) and np.array_equal(fs.astype(np.float32), sim)
    assert not np.isin(out, np.concatenate([fa, fb])).any() and len(fa) == 333 - 1 - len(out)
    # a float16 holds none of the planted elements, and every other one exactly
    with np.errstate(over="ignore"):
        h = r.astype(np.float16)
    assert np.array_equal(np.flatnonzero(np.isinf(h).any(axis=1)), out) and np.array_equal(h[keep].astype(np.float32), r[keep])


def test_the_negative_contest_rows_have_zero_and_negative_tree_edges():
    r, _ = lim.negative_contest()
    a, b, sim, valid = want = sequence.single_linkage_tree(r, "dot")
    assert len(a) == 99 and valid.all() and (sim < 0).sum() >= 1 and (sim == 0).sum() >= 1 and len(set(sim)) < 99
    assert same_tree(kruskal(ld.dots64(r)), want[:3])


def test_the_row_scale_inputs():
    r = lim.signed_rows(333, 8)
    r2 = lim.power_of_two_scaled(r, 3)                       # asserts that the scaling is exact
    assert r2.dtype == np.float32 and not np.array_equal(r2, r)
    a, b, sim, valid = sequence.single_linkage_tree(r)
    assert len(a) == 332 and valid.all()
    a, b, sim, valid = sequence.single_linkage_tree(lim.extreme_base())
    assert len(a) == 332 and valid.all() and 0.014 < sim.min() < 0.015
    assert list(zip(a[:8].tolist(), b[:8].tolist())) == list(ld.ONE_HOT_PAIRS) and (sim[:8] == 1).all() and sim[8] < 0.5
    a, b, sim, valid = sequence.single_linkage_tree(lim.heavy_rows(333, 8))
    assert len(a) == 332 and valid.all() and sim.max() < 1


@pytest.mark.parametrize("case", ("no edge", "nan", "minus zero"))
def test_the_plain_boruvka_on_small_matrices(case):
    if case == "no edge":
        assert ld.boruvka(np.full((3, 3), np.nan)) == (0, set()) and ld.boruvka(np.zeros((1, 1))) == (0, set())
    elif case == "nan":                                      # row 2 is isolated: a forest, and the loop ends on a round without a pick
        v = np.array([[0, -1.0, np.nan, -3], [0, 0, np.nan, -2], [0, 0, 0, np.nan], [0, 0, 0, 0]])
        assert ld.boruvka(v) == (1, {(0, 1), (1, 3)})
    else:                                                    # -0 ties with +0: the smaller lo wins
        v = np.array([[0, -0.0, 0.0], [0, 0, 0.0], [0, 0, 0]])
        assert ld.boruvka(v) == (1, {(0, 1), (0, 2)})
