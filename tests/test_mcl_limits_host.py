"""The limits round of sequence.markov_clusters without a GPU: the integer power against Python integers (math.isqrt) on values chosen
where its roots step, every inflation against the dense brute force of tests/test_mcl_host.py, a cutoff that empties valid columns
(precision 1 raised an IndexError on a graph without an isolated node), ``select`` at 1 and around a column's size, the q of the
rounding ties, weights up to 64 and parallel entries - and what the fixtures of tests/mcl_limits_data.py are said to contain, so that
a changed fixture is noticed before the device tests lose their point."""
from fractions import Fraction

import numpy as np
import pytest

from genomad_amd import sequence
from genomad_amd.sequence import markov_clusters
from tests import mcl_data, mcl_limits_data as D
from tests.spread_data import PARALLEL, star
from tests.test_mcl_host import brute_matrices

ONE, W = D.ONE, D.W


def matrix(res):
    return res["length"].tolist(), res["idx"].tolist(), res["val"].tolist()


def assert_is_brute(graph, valid, its, **kw):
    """the definition's matrix behind 0 .. its iterations equals the brute force's; behind convergence neither moves"""
    knobs = dict(inflation=2.0, select=256, precision=10000)
    knobs.update(kw)
    want = brute_matrices(graph, valid, knobs["inflation"], knobs["select"], knobs["precision"], its)
    for it in range(its + 1):
        assert matrix(markov_clusters(*graph, valid, max_iter=it, **knobs)) == want[it], (kw, it)


# ---- 0: a cutoff that keeps nothing ----------------------------------------------------------------------------------------------------

def test_precision_one_empties_every_column_of_the_path():
    res = markov_clusters(*mcl_data.PATH, precision=1)
    n = 40
    assert res["length"].tolist() == [0] * n and res["label"].tolist() == list(range(n)) and res["size"].tolist() == [1] * n
    assert res["attractor"].tolist() == [-1] * n and res["flow"].tolist() == [0] * n and not res["is_attractor"].any()
    assert res["iterations"] == 1 and res["converged"] and res["changed"].tolist() == [0]
    assert len(res["idx"]) == len(res["val"]) == 0 and res["idx"].dtype == np.int32 and res["val"].dtype == np.uint32
    assert res["length"].dtype == np.int64 and res["changed"].dtype == np.int64 and res["flow"].dtype == np.uint32


def test_precision_one_with_an_isolated_node():
    res = markov_clusters(*D.lone(), precision=1)
    assert res["length"].tolist() == [0, 0, 0, 0, 0, 1] and res["label"].tolist() == list(range(6)) and res["size"].tolist() == [1] * 6
    assert res["attractor"].tolist() == [-1] * 5 + [5] and res["flow"].tolist() == [0] * 5 + [ONE]
    assert res["is_attractor"].tolist() == [False] * 5 + [True] and res["iterations"] == 1 and res["converged"]


@pytest.mark.parametrize("precision", D.PRECISIONS)
def test_small_cutoffs_equal_the_brute_force(precision):
    graphs = D.small_graphs()
    assert_is_brute(*graphs["path"], 3, precision=precision)
    assert_is_brute(D.lone(), None, 3, precision=precision)
    assert_is_brute(*D.mixed(), 3, precision=precision)
    assert_is_brute(*graphs["random"], 2, precision=precision, select=8)


def test_prune_with_nothing_kept_returns_three_empty_arrays():
    cj, ci, y = np.array([0, 0, 1, 1], np.int64), np.array([0, 1, 0, 1], np.int64), np.array([5, 5, 7, 7], np.uint64)
    out = sequence._mcl_prune(cj, ci, y, 4, 1)
    assert [len(a) for a in out] == [0, 0, 0] and [a.dtype for a in out] == [np.int64, np.int64, np.uint64]
    one = sequence._mcl_prune(cj, ci, np.array([5, 5, 7, 8], np.uint64), 4, 2)       # column 0 stays, of column 1 only row 1
    assert [a.tolist() for a in one] == [[0, 0, 1], [0, 1, 1], [ONE // 2, ONE // 2, ONE]]


# ---- 1: the power ------------------------------------------------------------------------------------------------------------------------

def test_the_value_set_holds_what_it_is_said_to():
    u = D.pow_values()
    have = set(u.tolist())
    assert u.dtype == np.uint64 and 5500 < len(u) < 6500 and u[0] == 0 and u[-1] == ONE and (np.diff(u.astype(np.int64)) > 0).all()
    assert {0, 1, 2, 3, ONE - 2, ONE - 1, ONE} <= have
    assert all({(1 << b) - 1, 1 << b, (1 << b) + 1} - {ONE + 1} <= have for b in range(1, 31))
    assert all({k * k - 1, k * k, k * k + 1} - {ONE + 1} <= have for k in list(range(1, 200)) + [32767, 32768])
    squares = sum(int(x) == int(np.sqrt(float(x)) + 0.5) ** 2 for x in u.tolist())
    assert squares > 750                                 # 199 + two ends + 600 random roots, a few of them met twice


@pytest.mark.parametrize("a4", D.A4)
def test_the_definitions_power_equals_python_integers(a4):
    got = sequence._mcl_pow(D.pow_values(), a4)
    assert got.dtype == np.uint64 and np.array_equal(got, D.pow_reference(a4))


def test_the_power_at_its_ends_and_exact_points():
    for a4 in D.A4:
        want = dict(zip(D.pow_values().tolist(), D.pow_reference(a4).tolist()))
        assert want[0] == 0 and want[ONE] == ONE
        assert want[1 << 26] == 1 << (30 - a4) if a4 <= 30 else want[1 << 26] == 0       # (2^-4) ^ (a4 / 4) = 2^-a4: every root is exact
        assert all(want[a] <= want[b] for a, b in zip(list(want)[:-1], list(want)[1:]))   # floors of a rising function rise


# ---- 2: every inflation ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("a4", D.A4)
def test_every_inflation_equals_the_brute_force_on_two_cliques(a4):
    graph, valid = D.small_graphs()["two cliques"]
    assert_is_brute(graph, valid, 3, inflation=a4 / 4, select=8)


def test_every_inflation_converges_on_the_device_fixtures():
    for a4 in D.A4:
        for name in (f"inflation{a4}-random", f"inflation{a4}-planted"):
            want = D.case(name)[3]
            assert want["converged"] and want["iterations"] > 1, name
    assert D.case("inflation5-planted")[3]["iterations"] == 45 and D.case("inflation32-planted")[3]["iterations"] == 6


# ---- 3: the selection's ends --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("select", (1, 8, 9, 10))
def test_select_around_a_column_of_nine_equal_entries_equals_the_brute_force(select):
    assert_is_brute(star(8, 0.75), None, 3, select=select)
    assert_is_brute(star(8, 0.75), None, 3, select=select, inflation=1.75)


def test_the_stars_cut_where_they_are_said_to():
    for leaves in D.STARS:
        graph, _, kw, want = D.case(f"star-{leaves}")
        assert kw == dict(select=1024, max_iter=2) and want["changed"].tolist() == D.STAR_CHANGED[leaves], leaves
        first = markov_clusters(*graph, select=1024, max_iter=0)
        assert first["length"][0] == min(leaves + 1, 1024) and (first["length"][1:] == 2).all()
        assert np.array_equal(first["idx"][:first["length"][0]], np.arange(first["length"][0]))        # the cut falls on the row index


def test_select_one_and_two():
    planted = D.case("select1-planted")[3]
    assert len(np.unique(planted["label"])) == 112 and planted["iterations"] == 2 and (planted["length"] == 1).all()
    clique = D.case("select1-clique")[3]
    assert (clique["label"] == 0).all() and (clique["idx"] == 0).all() and (clique["length"] == 1).all()
    for name in ("planted", "clique", "random"):
        for s in (1, 2):
            want = D.case(f"select{s}-{name}")[3]
            assert want["converged"] and want["length"].max() == s, (name, s)
    assert_is_brute(*D.small_graphs()["random"], 3, select=1)
    assert_is_brute(*D.small_graphs()["two cliques"], 3, select=2)


# ---- 4: the cutoff's fixtures -------------------------------------------------------------------------------------------------------------

def test_the_cutoff_fixtures_hold_emptied_valid_rows():
    path = D.case("precision1-path")[3]
    assert (path["length"] == 0).all() and (path["label"] == np.arange(40)).all()
    planted = D.case("precision2-planted")[3]
    assert np.bincount(planted["length"]).tolist() == [220, 2]
    _, valid, _, want = D.case("precision1-mixed")
    assert want["length"][list(D.MIXED_ISOLATED)].tolist() == [1] * 4 and want["length"][list(D.MIXED_JOINED)].tolist() == [0] * 7
    assert want["label"].tolist() == [i if valid[i] else -1 for i in range(14)] and valid.sum() == 11
    assert want["size"][list(D.MIXED_JOINED)].tolist() == [1] * 7 and want["attractor"][list(D.MIXED_JOINED)].tolist() == [-1] * 7
    two = D.case("precision2-mixed")[3]                 # two equal entries stay, the triangle's columns of three are emptied
    assert two["length"].tolist() == [2, 2, 0, 1, 1, 0, 0, 0, 1, 0, 2, 2, 0, 1]
    three = D.case("precision3-mixed")[3]               # here the triangle survives the initial pass and moves for two iterations
    assert three["length"][[5, 6, 7]].tolist() == [2, 2, 2] and three["changed"].tolist() == [1, 1, 0]
    for p in D.PRECISIONS:
        for name in ("path", "planted", "mixed"):
            assert D.case(f"precision{p}-{name}")[3]["iterations"] >= 1


# ---- 5, 6: the fixtures with knobs of their own ------------------------------------------------------------------------------------------

def test_the_loop_fixtures_are_stars_of_the_tables_size():
    for leaves in (4095, 4096, 63, 64):
        graph, _, kw, want = D.case(f"loop-{leaves}")
        assert kw == dict(max_iter=1) and len(graph[1]) == leaves and np.diff(graph[0]).tolist()[:2] == [leaves, 0]
        first = markov_clusters(*graph, max_iter=0)
        assert want["iterations"] == 1 and first["length"][0] == min(leaves + 1, 256) and (first["length"][1:] == 2).all()


def test_rows_beyond_two_to_the_sixteenth():
    for name, ones in (("beyond-some", 0), ("beyond-all", 65500)):
        graph, valid, kw, want = D.case(name)
        assert len(graph[0]) - 1 == 65600 and kw == dict(select=64)
        assert np.bincount(want["length"], minlength=65).tolist() == [65500 - ones, ones] + [0] * 62 + [100]
        kept = want["idx"][np.cumsum(want["length"])[65486] - 64:np.cumsum(want["length"])[65486]]
        assert kept.tolist() == list(range(65486, 65550)) and kept[0] < 65536 < kept[-1]      # the tie is broken across 2^16
        assert (want["label"][65486:65586] == 65486).all() and want["converged"]


# ---- 7: weights and parallel entries -----------------------------------------------------------------------------------------------------

def test_the_ties_round_to_even():
    for k, q in D.TIES.items():
        sim = np.array([k * 2.0 ** -25], dtype=np.float32)
        assert Fraction(float(sim[0])) == Fraction(k, 1 << 25)                                # exact in float32
        exact = Fraction(k, 1 << 25) * W                                                      # k / 2
        assert round(exact) == q == int(np.rint(np.float64(sim[0]) * W))                      # Python's round of a Fraction ties to even
        weights = sequence.mcl_weights([0, 1, 1], [1], sim)[3].tolist()
        assert weights == ([q] if q else [])
    assert int(np.rint(np.float64(D.TOP) * W)) == (1 << 30) - 64 and float(D.TOP) < 64.0
    assert Fraction(float(D.TOP)) * W == (1 << 30) - 64


def test_the_weight_fixtures_span_the_admitted_range():
    q = lambda g: np.rint(g[2].astype(np.float64) * W).astype(np.int64)
    heavy, ranged, alltop = q(D.heavy()), q(D.ranged()), q(D.alltop())
    assert heavy.min() > 32 * W and heavy.max() < 60 * W and (heavy >= 54 * W).sum() > 7000
    assert (alltop == (1 << 30) - 64).all()
    counts = {v: int((ranged == v).sum()) for v in (0, 1, 2, (1 << 30) - 64)}
    assert counts[1] > 2000 and counts[(1 << 30) - 64] > 2000 and counts[2] >= 90 and counts[0] >= 140
    sim = D.ranged()[2]
    assert np.signbit(sim[sim == 0]).all() and (sim == 0).sum() >= 45                          # -0.0
    assert ((sim > 0) & (sim < np.finfo(np.float32).tiny)).sum() >= 45                        # the denormal
    for s in (3, 5, 1):
        assert (sim == np.float32(s * 2.0 ** -25)).sum() >= 40
    for name in ("heavy", "ranged", "alltop"):
        graph, _, kw, want = D.case(name)
        first = markov_clusters(*graph, max_iter=0, **kw)                                     # the selection cuts: keys with y >= 2^24
        assert want["converged"] and want["iterations"] > 2 and first["length"].max() == 64, name
    # weights of 2^24 and above reach the selection key's top digit in the initial pass
    assert (q(D.heavy()) >> 24).min() >= 33


def test_small_weights_and_parallel_entries_equal_the_brute_force():
    assert_is_brute(D.small_ranged(), None, 3, select=6)
    assert_is_brute(D.small_ranged(), None, 3, select=256, inflation=1.75)
    assert_is_brute(PARALLEL, None, 3)
    assert_is_brute(D.double_star(), None, 2)
    assert_is_brute(D.double_star(), None, 2, select=40, inflation=1.75)


def test_the_double_star_lists_every_leaf_twice():
    indptr, col, sim = D.double_star()
    assert indptr.tolist() == [0] + [140] * 71 and np.bincount(col).tolist() == [0] + [2] * 70
    pairs = sim.reshape(70, 2)
    leaf = np.arange(1, 71)
    assert ((pairs[:, 0] > pairs[:, 1]) == (leaf % 2 == 0)).all() and (pairs.min(axis=1) <= 0).sum() == 10
    want = markov_clusters(indptr, col, sim, max_iter=0)
    assert want["length"][0] == 71 and (want["length"][1:] == 2).all()
    # the hub's column holds the larger copy of every leaf: p rises with the leaf's larger weight
    assert (np.diff(want["val"][1:71].astype(np.int64)) >= 0).all() and want["val"][0] == want["val"][70]
