"""Inputs and references that take the density-aware linkage tree (the MR = true instantiation of lk_tile_kernel / lk_candidates and
lk_core_kernel in gnn_linkage.hip) to the limits tests/test_density_tree_gpu.py stays away from.  The inputs are those of the
single-linkage and embedding limits (tests/linkage_limits_data.py, tests/embedding_limits_data.py); what is added here:

  fixture_rows, definition   the named inputs and their trees under the numpy definition (sequence.mutual_reachability_tree), once
  check_tree                 tests/test_density_tree_gpu.py's check of a result's shape in a forest-aware form: core is NaN at every
                             invalid row, and at a valid row only where the caller says so (a row without a partner)
  forest_40                  the forest with 40 connected rows only: at min_points 65 their neighbour lists are NaN-padded
  ruler_rounds               the rounds a plain Boruvka needs over the ruler path's mutual-reachability values - not the ruler's own 8
  one_hot_first_edges        the first edges of extreme_base's tree at min_points 2, from the definition
  few_rows                   two and three valid rows, alone, among invalid ones and across a tile border; exact under both metrics
  kruskal_reference          the brute-force Kruskal over mutual(device values, device core): shares no code with the definition"""
import functools

import numpy as np

from genomad_amd import sequence
from tests import embedding_limits_data as lim
from tests import linkage_limits_data as ld
from tests import votes_data
from tests.density_tree_data import mutual
from tests.linkage_data import bits, check_shape, kruskal, same
from tests.neighbours_data import rows

M_ALL = (2, 5, 65)                               # the least, the default, the most: lists of 1, 4 and 64 partners


@functools.lru_cache(maxsize=None)
def fixture_rows(name):
    """the rows of a named input, made once and read-only"""
    r = {"corners": lambda: ld.corners()[0], "simplex_star": lambda: ld.simplex_star()[0],
         "negative_contest": lambda: lim.negative_contest()[0], "ruler_path": ld.ruler_path, "ruler_cut": ruler_cut,
         "dead_tiles": lambda: ld.dead_tiles()[0], "dead_tiles_zero": dead_tiles_zero, "forest_rows": lambda: ld.forest_rows()[0],
         "forest_part": lambda: np.ascontiguousarray(ld.forest_rows()[0][ld.forest_rows()[2]]),
         "forest_40_part": lambda: np.ascontiguousarray(ld.forest_rows()[0][forest_40()[2]]),
         "signed_rows": lambda: lim.signed_rows(333, 8), "extreme_base": lim.extreme_base, "heavy_rows": lambda: lim.heavy_rows(333, 8),
         "rows65": lambda: rows(65, 9)}[name]()
    r.flags.writeable = False
    return r


@functools.lru_cache(maxsize=None)
def definition(name, m, metric):
    """the numpy definition's (a, b, sim, core, valid) of a named input, computed once"""
    return sequence.mutual_reachability_tree(fixture_rows(name), m, metric)


def check_tree(res, n, m, no_partner=()):
    """the shape of a DensityTreeResult.  core is NaN at every invalid row; a valid row's core is NaN exactly at the rows
    ``no_partner`` - valid rows whose every pair value is NaN (include/genomad_nn.h: "NaN for a row without one")."""
    check_shape(res, n)
    assert res.core.dtype == np.float32 and res.core.shape == (n,) and res.min_points == m
    nan = np.isnan(res.core)
    assert nan[res.valid == 0].all()
    alone = np.zeros(n, bool)
    alone[np.asarray(no_partner, np.int64)] = True
    if res.n_valid >= 2:
        assert np.array_equal(nan & (res.valid == 1), alone & (res.valid == 1)), np.flatnonzero(nan & (res.valid == 1) != alone)[:10]


def exact(res, want):
    """the whole result against a definition's (a, b, sim, core, valid): every index, the bits of every sim and core, every flag"""
    a, b, sim, core, valid = want
    assert res.n_edges == len(a), (res.n_edges, len(a))
    assert same(res, (a, b, sim)), np.flatnonzero((res.a != a) | (res.b != b) | (bits(res.sim) != bits(sim)))[:10]
    assert np.array_equal(bits(res.core), bits(core)), np.flatnonzero(bits(res.core) != bits(core))[:10]
    assert np.array_equal(res.valid, valid)
    return True


def zeros_are_plus_zero(res):
    return bool((bits(res.sim[res.sim == 0]) == 0).all() and (bits(res.core[res.core == 0]) == 0).all())


def kruskal_reference(values, core, valid=None):
    """(a, b, sim) by the brute force over min(values, core_i, core_j) in float32"""
    values = np.asarray(values, np.float32)
    w = mutual(values, np.asarray(core, np.float32))
    assert w.dtype == np.float32
    return kruskal(w, valid)


def errors_against_fp64(res, want, what):
    """(largest |sorted device weight - sorted fp64 weight|, largest |device core - fp64 core|), printed"""
    a, b, sim, core, valid = want
    assert res.n_edges == len(sim) and np.array_equal(np.isnan(res.core), np.isnan(core))
    err = float(np.abs(np.sort(res.sim).astype(np.float64) - np.sort(sim).astype(np.float64)).max())
    ok = ~np.isnan(core)
    cerr = float(np.abs(res.core[ok].astype(np.float64) - core[ok].astype(np.float64)).max())
    print(f"\n{what}: largest |sorted device weight - sorted fp64 weight| = {err:.3g}, largest |device core - fp64 core| = {cerr:.3g}")
    return err, cerr


# ---- negative values ---------------------------------------------------------------------------------------------------------------

def star_ties(m=5):
    """simplex_star at min_points ``m``: (distinct weights of the tree, the least number of partners that tie for a row's best
    mutual-reachability value).  The dot of i and j is n - k_i - k_j, a row's core n - k_i - (its (m - 1)-th smallest other k): every
    pair with one of the m - 1 rows of smallest k is capped by the row's own core, so every other row's best value is tied m - 1 times."""
    r = fixture_rows("simplex_star")
    a, b, sim, core, valid = definition("simplex_star", m, "dot")
    w = mutual(ld.dots64(r), core.astype(np.float64))
    np.fill_diagonal(w, -np.inf)
    best = w.max(axis=1)
    tied = (w == best[:, None]).sum(axis=1)
    return len(set(sim.tolist())), int(tied.min()), int(np.median(tied))


# ---- a forest ----------------------------------------------------------------------------------------------------------------------

def forest_40():
    """(rows (107, 512), out, keep): the 67 forest rows beyond the f16 range and the first 40 of the others, in index order - at
    min_points 65 every connected row has 39 partners and a list padded with 25 NaN"""
    r, out, keep = ld.forest_rows()
    take = np.sort(np.concatenate([out, keep[:40]]))
    sub = np.ascontiguousarray(r[take])
    out40 = np.flatnonzero(np.isin(take, out))
    keep40 = np.flatnonzero(~np.isin(take, out))
    assert len(out40) == 67 and len(keep40) == 40 and (np.abs(sub[keep40]).max() <= 48)
    return sub, out40, keep40


# ---- dead tiles --------------------------------------------------------------------------------------------------------------------

def dead_tiles_zero():
    """dead_tiles with row 64 zeroed: valid under dot, invalid under cosine"""
    r = np.array(ld.dead_tiles()[0])
    r[64] = 0
    return r


# ---- rounds ------------------------------------------------------------------------------------------------------------------------

def ruler_cut():
    """ruler_path with its last row invalid"""
    r = np.array(ld.ruler_path())
    r[255, 0] = np.nan
    return r


def ruler_rounds(name, m):
    """(rounds, edges) of a plain Boruvka over the mutual-reachability values of ``name`` (ruler_path or ruler_cut) under dot, from
    float64 dots and sequence.core_similarity's core"""
    r = fixture_rows(name)
    core, valid = sequence.core_similarity(r, m, "dot")
    ok = valid.astype(bool)
    dots = ld.dots64(np.where(ok[:, None], r, 0))
    return ld.boruvka(mutual(dots, core), ok)


# ---- row scales --------------------------------------------------------------------------------------------------------------------

def one_hot_first_edges():
    """the edges of extreme_base's tree at min_points 2 whose value is exactly 1, from the definition: the pairs of
    linkage_limits_data.ONE_HOT_PAIRS whose both ends have core 1 - an identical partner each"""
    a, b, sim, core, valid = definition("extreme_base", 2, "cosine")
    first = [(int(x), int(y)) for x, y, s in zip(a, b, sim) if s == 1]
    assert first == [p for p in ld.ONE_HOT_PAIRS if core[p[0]] == 1 and core[p[1]] == 1]
    assert (sim[:len(first)] == 1).all() and (sim[len(first):] < 1).all()
    return first


# ---- few rows ----------------------------------------------------------------------------------------------------------------------

FEW = ("two", "three", "two_of_four", "three_of_66")


def few_rows(which):
    """(rows, the valid rows): two and three valid rows, alone, two among four and three among 66 - rows 10, 63 and 65, across the
    border of the first tile.  The rows are votes_data.tie_rows: 0 / 1 rows with 256 ones each, so a dot is an integer and a cosine
    is dot / 256, exact in every arithmetic: the definition is the reference under both metrics.  Invalid rows hold a NaN or an
    infinity (a zero row would be valid under dot)."""
    t = votes_data.tie_rows()
    n, live = {"two": (2, [0, 1]), "three": (3, [0, 1, 2]), "two_of_four": (4, [1, 3]), "three_of_66": (66, [10, 63, 65])}[which]
    r = np.array(t[:n])
    for k, i in enumerate(np.setdiff1d(np.arange(n), live)):
        r[i, (7, 500, 0)[k % 3]] = (np.nan, np.inf, -np.inf)[k % 3]
    ok = np.isfinite(r).all(axis=1)
    assert np.array_equal(np.flatnonzero(ok), live)
    dots = ld.dots64(r[live])
    upper = dots[np.triu_indices(len(live), 1)]
    assert len(set(upper.tolist())) == len(upper) and (r[live].sum(axis=1) == 256).all()       # distinct values: one tree
    return r, np.asarray(live)
