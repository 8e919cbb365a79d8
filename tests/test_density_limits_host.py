"""What tests/test_density_limits_gpu.py leans on, without a GPU: the exact oracle of tests/density_limits_data.py (density_of_graph)
gives what the numpy definition (sequence.density_clusters) and the brute force (density_data.dbscan) give, on planted rows, on 0/1
rows with ties, on the border contest with its negative and zero similarities, on the chain of 2176 rows and on a dense signed graph;
the comparison rejects a result that is wrong in one place - a flipped tie, an anchor of second-best similarity, a border row promoted
to core, two clusters merged, a -0 where +0 belongs -; every generator's conditions hold (they are asserted where the input is made)
and the expectations the GPU tests state follow from the definition.  The device is not touched: a failure here is a failure of a test
input or of the oracle, not of a kernel."""
import time

import numpy as np
import pytest

from genomad_amd import sequence
from tests import density_data as dd
from tests import density_limits_data as dl
from tests import embedding_limits_data as lim
from tests import graph_limits_data as gd


def graph32(r, t, metric="cosine"):
    """the definition's graph with sim as the device returns it: float32"""
    indptr, col, sim = sequence.threshold_graph(r, t, metric)
    return indptr, col, sim.astype(np.float32)


def oracle(r, t, m, metric="cosine"):
    return dl.density_of_graph(*graph32(r, t, metric), sequence.valid_rows(r, metric), m)


def definition(r, t, m, metric="cosine"):
    return dl.as_device(sequence.density_clusters(r, t, m, metric))


def brute(r, t, m, metric="cosine"):
    """density_data.dbscan on the fp64 similarities of the valid rows"""
    valid, s = dd.valid_sims64(r, metric)
    s = np.maximum(s, s.T)
    return dl.as_device(dd.dbscan(s >= gd.threshold32(t), s, m, valid))


# ---- the oracle against the definition and the brute force ---------------------------------------------------------------------------

@pytest.mark.parametrize("min_points", dd.MIN_POINTS)
def test_the_oracle_on_planted_rows(min_points):
    r, _ = dd.planted()
    got = oracle(r, dd.T, min_points)
    dl.check_same(got, definition(r, dd.T, min_points), "definition")
    dl.check_same(got, brute(r, dd.T, min_points), "brute force")
    assert dl.counts(got[5])[3] == 2                                  # the zero row and the NaN row


def test_the_oracle_on_integer_rows_with_ties():
    r, dots, t, m = dd.integer_case()
    got = oracle(r, t, m, "dot")
    dl.check_same(got, definition(r, t, m, "dot"), "definition")
    dl.check_same(got, brute(r, t, m, "dot"), "brute force")
    core, border, _, _ = dl.counts(got[5])
    assert core >= 20 and border >= 20


def test_the_border_contest_has_its_anchors_signs_and_ties():
    r, dots, want = dl.border_contest()                               # asserts its own conditions
    t, m = lim.CONTEST_THRESHOLD, dl.CONTEST_MIN_POINTS
    got = oracle(r, t, m, "dot")
    dl.check_same(got, definition(r, t, m, "dot"), "definition")
    dl.check_same(got, brute(r, t, m, "dot"), "brute force")
    label, degree, size, anchor, sim, kind = got
    assert dl.counts(kind) == (184, 16, 0, 0) and (label[kind > 0] == 0).all() and (size == 200).all()
    members = list(dl.CONTEST_MEMBERS)
    assert [int(x) for x in anchor[members]] == [want[i][0] for i in members] == [dl.CONTEST_CORES[k] for k in dl.CONTEST_ANCHORS * 2]
    assert [float(x) for x in sim[members]] == [want[i][1] for i in members] == list(dl.CONTEST_SIMS * 2)
    assert (sim[members] <= 0).all() and (sim[members] < 0).sum() == 12
    zero = sim[members] == 0
    assert zero.sum() == 4 and (sim[members][zero].view(np.uint32) == 0).all()


def test_the_chain_is_one_cluster_of_511_rows_among_513():
    r, where, (a, b) = dl.chain_case()                                # asserts the flags beyond n
    n = len(r)
    got = oracle(r, dl.CHAIN_THRESHOLD, dl.CHAIN_MIN_POINTS, "dot")
    graph = graph32(r, dl.CHAIN_THRESHOLD, "dot")
    t0 = time.perf_counter()
    again = dl.density_of_graph(*graph, np.ones(n, bool), dl.CHAIN_MIN_POINTS)
    seconds = time.perf_counter() - t0
    print(f"\ndensity_of_graph on {n} rows, {len(graph[1])} edges: {seconds:.4f} s")
    assert seconds < 1.0
    dl.check_same(again, got)
    dl.check_same(got, definition(r, dl.CHAIN_THRESHOLD, dl.CHAIN_MIN_POINTS, "dot"), "definition")
    assert_chain(got, where)
    assert np.array_equal(np.stack([a, b]), np.stack(sequence.graph_edges(graph[0], graph[1])))


def assert_chain(got, where):
    """what the issue states of chain_case, from a result: shared with the GPU tests"""
    label, degree, size, anchor, sim, kind = got
    n, path = len(label), where[:dl.CHAIN_PATH]
    inner, ends = path[1:-1], path[[0, -1]]
    assert (kind[inner] == dl.KIND_CORE).all() and (kind[ends] == dl.KIND_BORDER).all() and dl.counts(kind) == (n - 2, 2, 0, 0)
    assert np.array_equal(anchor[ends], path[[1, -2]]) and (sim[ends] == 1).all()
    assert (label[path] == inner.min()).all() and (size[path] == dl.CHAIN_PATH).all()
    assert int((label == np.arange(n)).sum()) == 513
    assert sorted(np.bincount(size[where[dl.CHAIN_PATH:]]).nonzero()[0].tolist()) == [3, 4]


def test_the_oracle_on_a_dense_signed_graph_equals_the_brute_force_on_the_same_f32_values():
    """here fp64 decides nothing - two f32 values may tie where fp64 does not -, so both get the same f32 edge values"""
    r = dl.signed_case()
    t = gd.SIGN_THRESHOLDS[2]
    graph = graph32(r, t)
    a, b = sequence.graph_edges(graph[0], graph[1])
    n = len(r)
    adj, s = np.zeros((n, n), bool), np.zeros((n, n), np.float32)
    adj[a, b] = adj[b, a] = True
    s[a, b] = s[b, a] = graph[2]
    degree = adj.sum(axis=1)
    assert len(a) == 15119 and degree.min() > 30                      # thousands of one-core edges per tile at the median degree
    for m in dl.quartile_min_points(degree):
        got = dl.density_of_graph(*graph, np.ones(n, bool), m)
        want = dd.dbscan(adj, s, m)
        dl.check_same(got, dl.as_device(want), m)
    core, border, noise, _ = dl.counts(got[5])
    print(f"\nsigned rows at {t}, min_points {m}: {core} core, {border} border, {noise} noise")
    m = dl.quartile_min_points(degree)[1]
    kind = dl.density_of_graph(*graph, np.ones(n, bool), m)[5]
    assert dl.counts(kind)[0] >= n // 4 and dl.counts(kind)[1] >= n // 4


def test_prefixes_have_core_and_border_rows():
    full = lim.signed_integer_rows(gd.N_INTEGER)
    for n in gd.PREFIXES:
        r, dots = dl.prefix(n)
        assert r.shape == (n, 512) and np.array_equal(r, full[:n])
        for t in lim.integer_thresholds(full):
            m = dl.median_min_points(dots, t)
            got = oracle(r, t, m, "dot")
            dl.check_same(got, definition(r, t, m, "dot"), (n, t))
            core, border, noise, invalid = dl.counts(got[5])
            assert core + border + noise == n and invalid == 0 and core >= n // 2      # the median degree: at least half are core
            if n >= 63 and t < 0:
                assert border > 0, (n, t)


def test_the_two_range_case_has_its_plants():
    base, plants = dl.two_range_case()                                # asserts the planted edges against all 65350 rows
    assert base.shape == (lim.NB_CAPPED, 512) and sequence.valid_rows(base[:64]).all()
    expect = plants["expect"]
    assert len(expect) == 4 and sum(x < lim.SPLIT_MAX for x in expect) == 2
    assert sum(second is not None for _, second in expect.values()) == 2
    chain = [gd.COPIES_OF, *gd.COPIES, lim.NB_CAPPED - 1]             # the five copies of row 100: a clique across the border
    assert sum(x >= lim.SPLIT_MAX for x in chain) == 2 and len(chain) == dl.TWO_RANGE_MIN_POINTS


# ---- the comparison rejects a result that is wrong in one place ------------------------------------------------------------------------

def changed(got, **at):
    out = [x.copy() for x in got]
    for k, (i, v) in at.items():
        out[dl.FIELDS.index(k)][i] = v
    return tuple(out)


def test_the_comparison_rejects_each_wrong_result():
    r, dots, want = dl.border_contest()
    right = oracle(r, lim.CONTEST_THRESHOLD, dl.CONTEST_MIN_POINTS, "dot")
    dl.check_same(right, tuple(x.copy() for x in right))
    a, b, c = dl.CONTEST_CORES
    tie, second, zero = dl.CONTEST_MEMBERS[2], dl.CONTEST_MEMBERS[0], dl.CONTEST_MEMBERS[4]
    assert want[tie] == (a, -4.0) and dots[tie, b] == -4 and want[second] == (b, -1.0) and dots[second, a] == -4 and want[zero] == (a, 0.0)
    wrong = {"a flipped tie": changed(right, anchor=(tie, b)),
             "an anchor of second-best similarity": changed(right, anchor=(second, a), sim=(second, np.float32(-4))),
             "a border row promoted to core": changed(right, kind=(tie, dl.KIND_CORE), anchor=(tie, tie), sim=(tie, np.float32(np.nan))),
             "-0 where +0 belongs": changed(right, sim=(zero, np.float32(-0.0)))}
    # two clusters merged: on the chain, where there are 513
    r, where, _ = dl.chain_case()
    chain = oracle(r, dl.CHAIN_THRESHOLD, dl.CHAIN_MIN_POINTS, "dot")
    roots = np.flatnonzero(chain[0] == np.arange(len(r)))
    lo, hi = roots[0], roots[1]
    label, size = chain[0].copy(), chain[2].copy()
    label[chain[0] == hi] = lo
    size[label == lo] = (label == lo).sum()
    merged = (label, chain[1], size) + chain[3:]
    with pytest.raises(AssertionError):
        dl.check_same(merged, chain)
        print("check_same accepted two clusters merged")
    for what, got in wrong.items():
        with pytest.raises(AssertionError):
            dl.check_same(got, right)
            print(f"check_same accepted {what}")
    # and the oracle itself takes each of them for wrong: it is not the changed result that it computes
    flipped = dl.density_of_graph(*graph32(r, dl.CHAIN_THRESHOLD, "dot"), np.ones(len(r), bool), dl.CHAIN_MIN_POINTS + 1)
    with pytest.raises(AssertionError):
        dl.check_same(flipped, chain)                                 # another min_points is another result
