"""What tests/test_density_tree_limits_gpu.py leans on, without a GPU: every input of tests/density_tree_limits_data.py is made (each
generator asserts its own conditions), its tree under the numpy definition has the stated shape - negative cores and tied weights,
the forest's rows without a core, the rounds a plain Boruvka needs, the one-hot edges, the few-row trees -, and the brute-force Kruskal
over the mutual-reachability values, which shares no code with the definition, gives the same tree, so the two references of the
device tests do not share a mistake."""
import math

import numpy as np
import pytest

from genomad_amd import sequence
from genomad_amd.engine import DensityTreeResult
from tests import density_tree_limits_data as T
from tests import linkage_limits_data as ld
from tests.density_tree_data import last_finite, mutual
from tests.linkage_data import kruskal


def kruskal_is_the_definition(values64, want, valid=None):
    """the brute force over mutual(float64 values, the definition's float64 core) against the definition's tree"""
    a, b, sim, core, ok = want
    core64 = core.astype(np.float64)                     # exact inputs: the float32 core is the float64 one
    got = kruskal(mutual(values64, core64), ok.astype(bool) if valid is None else valid)
    return np.array_equal(got[0], a) and np.array_equal(got[1], b) and np.array_equal(got[2].astype(np.float32), sim)


def result_of(want, m, metric, rounds):
    return DensityTreeResult.build(want, m, metric, rounds)


@pytest.mark.parametrize("m", T.M_ALL)
@pytest.mark.parametrize("which", ("corners", "simplex_star", "negative_contest"))
def test_negative_values_and_cores_under_dot(which, m):
    r = T.fixture_rows(which)
    a, b, sim, core, valid = want = T.definition(which, m, "dot")
    assert len(a) == len(r) - 1 and valid.all() and not np.isnan(core).any()
    assert (np.diff(sim) <= 0).all() and (a < b).all()
    assert (sim <= np.minimum(core[a], core[b])).all()                       # a weight is capped by both ends' cores
    assert kruskal_is_the_definition(ld.dots64(r), want)
    res = result_of(want, m, "dot", 1)
    T.check_tree(res, len(r), m)
    assert T.exact(res, want) and T.zeros_are_plus_zero(res)
    if which == "corners":
        assert (sim < 0).sum() == 3 and (sim[-3:] < 0).all() and (core > 0).all()
    elif which == "simplex_star":                                            # every core and every weight is negative, and tied
        assert (sim < 0).all() and (core < 0).all()
        distinct, least_tied, _ = T.star_ties(m)
        assert distinct < 200 < len(sim) and least_tied >= 1, (distinct, least_tied)
    else:
        assert (sim < 0).sum() >= 1 and ((sim == 0).sum() >= 1 or m == 65) and ((core == 0).sum() >= 1 or m == 65)


def test_the_star_at_min_points_5_ties_every_rows_best_value_four_times():
    distinct, least_tied, median_tied = T.star_ties(5)
    assert (distinct, least_tied, median_tied) == (183, 4, 4)
    a, b, sim, core, valid = T.definition("simplex_star", 5, "dot")
    assert len(np.unique(core)) < 200 and np.bincount(np.concatenate([a, b])).max() == 332        # still a star: the order decides among the tied


def test_the_forest_rows_without_a_partner_have_no_core():
    r, out, keep = ld.forest_rows()
    sub, out40, keep40 = T.forest_40()
    for m in T.M_ALL:
        a, b, sim, core, valid = want = T.definition("forest_part", m, "dot")
        assert len(a) == 265 and valid.all() and not np.isnan(core).any() and (sim < 0).sum() >= 3   # at 65 a group of fewer rows has negative cores
        # the matrix the device sees - NaN in the rows and columns of ``out`` - with the core of the kept rows, NaN at the others
        full_core = np.full(333, np.nan)
        full_core[keep] = core
        fa, fb, fs = kruskal(mutual(ld.nan_rows_and_columns(ld.dots64(r), out), full_core))
        assert np.array_equal(fa, keep[a]) and np.array_equal(fb, keep[b]) and np.array_equal(fs.astype(np.float32), sim)
        assert not np.isin(out, np.concatenate([fa, fb])).any()
        # the forest-aware check takes such a result and refuses a core at a row without a partner, or none at a row with one
        res = result_of((keep[a], keep[b], sim, full_core.astype(np.float32), np.ones(333, np.uint8)), m, "dot", 4)
        T.check_tree(res, 333, m, no_partner=out)
        with pytest.raises(AssertionError):
            T.check_tree(res, 333, m)
        with pytest.raises(AssertionError):
            T.check_tree(res, 333, m, no_partner=np.append(out, keep[0]))
        assert (res.cut(float(sim[100]))[out] == -1).all()
    with pytest.raises(ValueError, match="265 edges among 333 valid rows: hdbscan needs a spanning tree, not a forest"):
        sequence.hdbscan_clusters(res.a, res.b, res.sim, res.valid, 2)
    with pytest.raises(ValueError, match="metric 'dot': 1 - sim is a distance under cosine only"):
        res.hdbscan(2)
    # 40 connected rows at min_points 65: the definition's core is the least similar of 39 partners
    a, b, sim, core, valid = T.definition("forest_40_part", 65, "dot")
    dots = ld.dots64(T.fixture_rows("forest_40_part"))
    np.fill_diagonal(dots, np.inf)
    assert len(a) == 39 and np.array_equal(core, dots.min(axis=1).astype(np.float32)) and len(sub) == 107
    padded = np.full((40, 64), np.nan, np.float32)
    np.fill_diagonal(dots, -np.inf)
    padded[:, :39] = -np.sort(-dots, axis=1)[:, :39]
    assert np.array_equal(last_finite(padded), core)


@pytest.mark.parametrize("m", T.M_ALL)
def test_dead_tiles_under_the_definition(m):
    r, dead = T.fixture_rows("dead_tiles"), ld.DEAD_ROWS
    a, b, sim, core, valid = want = T.definition("dead_tiles", m, "dot")
    ok = valid.astype(bool)
    assert len(a) == 278 and np.array_equal(np.flatnonzero(~ok), dead) and np.isnan(core[dead]).all() and not np.isnan(core[ok]).any()
    assert not np.isin(dead, np.concatenate([a, b])).any() and len(set(sim.tolist())) < 278
    assert kruskal_is_the_definition(ld.dots64(np.where(ok[:, None], r, 0)), want)
    res = result_of(want, m, "dot", 3)
    T.check_tree(res, 600, m)
    assert (res.cut(float(sim[100]))[dead] == -1).all()
    zero = sequence.mutual_reachability_tree(T.fixture_rows("dead_tiles_zero"), m)             # the cosine case of the device test
    assert np.array_equal(np.flatnonzero(zero[4] == 0), np.sort(np.append(dead, 64))) and len(zero[0]) == 277


def test_the_rounds_of_the_ruler_path_under_mutual_reachability():
    """at min_points 2 every core is 16 (15 at the last row of the cut path), the best value there is, and caps no pair that decides: the
    ruler's own 8 rounds, 7 without the last row.  At min_points 3 a row's core is its second-best value - 0 at both ends of the path -,
    the weights are other ones, far pairs tie with near ones at 0, and a plain Boruvka over them needs a round less: 7 and 6.  The
    device must take these numbers, whatever the ruler alone would need."""
    want = {("ruler_path", 2): 8, ("ruler_cut", 2): 7, ("ruler_path", 3): 7, ("ruler_cut", 3): 6}
    for (name, m), rounds in want.items():
        a, b, sim, core, valid = tree = T.definition(name, m, "dot")
        n_valid = int(valid.sum())
        assert len(a) == n_valid - 1 and ((b - a == 1).all() or m == 3)      # at 3 the cores of 0 tie far pairs with near ones
        got, taken = T.ruler_rounds(name, m)
        assert got == rounds <= math.ceil(math.log2(n_valid)) and taken == set(zip(a.tolist(), b.tolist())), (name, m, got)
        ok = valid.astype(bool)
        assert kruskal_is_the_definition(ld.dots64(np.where(ok[:, None], T.fixture_rows(name), 0)), tree)
    assert len(set(T.definition("ruler_path", 3, "dot")[2].tolist())) == 8


def test_the_row_scale_inputs_and_the_one_hot_edges():
    assert T.one_hot_first_edges() == list(ld.ONE_HOT_PAIRS)
    a, b, sim, core, valid = T.definition("extreme_base", 2, "cosine")
    assert len(a) == 332 and valid.all() and (core[[32, 35, 36, 39, 40, 41, 42, 43, 44, 45, 46, 47]] == 1).all()
    assert (core[[33, 34, 37, 38]] < 0.05).all()                             # a one-hot row without an identical partner
    for which in ("extreme_base", "heavy_rows", "signed_rows"):
        for m in (2, 17):
            a, b, sim, core, valid = T.definition(which, m, "cosine")
            assert len(a) == 332 and valid.all() and not np.isnan(core).any() and (sim <= np.minimum(core[a], core[b])).all()


@pytest.mark.parametrize("metric", ("dot", "cosine"))
@pytest.mark.parametrize("which", T.FEW)
def test_two_and_three_valid_rows(which, metric):
    r, live = T.few_rows(which)
    for m in (2, 3, 65):
        a, b, sim, core, valid = want = sequence.mutual_reachability_tree(r, m, metric)
        assert np.array_equal(np.flatnonzero(valid), live) and len(a) == len(live) - 1 and np.isin(a, live).all() and np.isin(b, live).all()
        assert np.isnan(np.delete(core, live)).all() and not np.isnan(core[live]).any()
        values = ld.dots64(np.where(valid.astype(bool)[:, None], r, 0)) / (256.0 if metric == "cosine" else 1.0)
        assert kruskal_is_the_definition(values, want)
        if len(live) == 2:
            assert sim[0] == core[a[0]] == core[b[0]] == values[live[0], live[1]]
        elif m >= 3:
            assert sim[0] == sim[1] == values[np.ix_(live, live)][np.triu_indices(3, 1)].min()     # all three pairs tie: the order decides
            assert (a[0], b[0], a[1], b[1]) == (live[0], live[1], live[0], live[2])
        T.check_tree(result_of(want, m, metric, 1), len(r), m)


def test_check_tree_and_the_references_on_small_inputs():
    """the comparison helpers of the device tests on the definition's own result, and on a wrong one"""
    r = T.fixture_rows("rows65")
    a, b, sim, core, valid = want = sequence.mutual_reachability_tree(r, 3)
    res = result_of(want, 3, "cosine", 3)
    T.check_tree(res, 65, 3)
    assert T.exact(res, want)
    s = np.array(sequence._pair_values(r, "cosine")[0], np.float32)
    assert T.exact(result_of(T.kruskal_reference(s, core) + (core, valid), 3, "cosine", 3), want)
    err, cerr = T.errors_against_fp64(res, want, "rows65")
    assert err == 0 and cerr == 0
    wrong = core.copy()
    wrong[7] = np.nan
    with pytest.raises(AssertionError):
        T.check_tree(result_of((a, b, sim, wrong, valid), 3, "cosine", 3), 65, 3)
    with pytest.raises(AssertionError):
        T.exact(result_of((a, b, sim, wrong, valid), 3, "cosine", 3), want)
