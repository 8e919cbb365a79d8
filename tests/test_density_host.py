"""Density clusters among encoder embeddings without a GPU: the numpy definition (sequence.density_clusters) against a brute-force
DBSCAN on planted rows and on 0/1 integer rows, the margins the GPU tests rest on, the planted structure by group, the two identities
with threshold_clusters, ties at the threshold and between anchors, border-border edges, invalid rows, the edges of n and of the
arguments, density_table and DensityResult, the ABI's argument checks (before the ctx is looked at: no GPU needed), and main()'s
GENOMAD_AMD_DENSITY switches over a fake engine served from the definition."""
import os

import numpy as np
import pytest

from genomad_amd import _lib, nn_classification as nnc, sequence
from genomad_amd.engine import DensityResult, NNEngine
from tests.density_data import MIN_POINTS, T, dbscan, integer_case, planted, same, second_gap, valid_sims64
from tests.neighbours_data import rows
from tests.test_neighbours_host import SWITCHES, FakeNeighbourEngine
from tests.test_strand_host import FakeStrandEngine, _npz, _same_npz, _tree, _write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T32 = float(np.float32(T))
# min_points -> (clusters, core, border, noise) on the planted rows at T
COUNTS = {1: (279, 331, 0, 0), 2: (5, 57, 0, 274), 3: (4, 48, 7, 276), 6: (4, 40, 8, 283), 11: (4, 11, 37, 283)}


@pytest.fixture(scope="module")
def plant():
    r, groups = planted()
    valid, s64 = valid_sims64(r)
    adj = (s64 >= T32) & valid[:, None] & valid[None, :]
    adj[np.arange(len(r)), np.arange(len(r))] = False
    return r, groups, valid, s64, adj


@pytest.fixture(scope="module")
def defined(plant):
    """the definition at every min_points of the tests, computed once"""
    return {m: sequence.density_clusters(plant[0], T, m) for m in MIN_POINTS}


def counts(result):
    label, kind = result[0], result[5]
    return int((label == np.arange(len(label))).sum()), int((kind == 3).sum()), int((kind == 2).sum()), int((kind == 1).sum())


def test_the_planted_threshold_keeps_its_distance_from_every_similarity(plant):
    """the GPU tests compare with the definition exactly: the device's f32 similarity is within 1e-5 of the fp64 one, so no pair may
    lie closer to the threshold than that - asserted with a factor of ten"""
    r, _, valid, s64, adj = plant
    iu = np.triu_indices(len(r), 1)
    both = (valid[:, None] & valid[None, :])[iu]
    gap = np.abs(s64[iu] - T32)[both].min()
    print(f"\nplanted: min |sim64 - {T}| = {gap:.3e}, {int(adj[iu].sum())} edges")
    assert gap >= 1e-4


@pytest.mark.parametrize("min_points", MIN_POINTS)
def test_the_planted_anchors_keep_their_distance_from_the_runner_up(plant, defined, min_points):
    """a border row's anchor is an argmax over f32 values on the device and over f64 values here: the best and the second-best core
    neighbour must lie further apart than both errors - asserted with the same factor"""
    r, _, valid, s64, adj = plant
    gaps = second_gap(adj, s64, defined[min_points])
    print(f"\nplanted, min_points {min_points}: {len(gaps)} borders with several core neighbours, smallest gap "
          f"{gaps.min() if len(gaps) else float('nan'):.3e}")
    assert (gaps >= 1e-4).all()
    if min_points in (6, 11):
        assert len(gaps) >= 3                                 # the case exists: the bridges at 6, the families' members at 11


@pytest.mark.parametrize("min_points", MIN_POINTS)
def test_definition_equals_the_brute_force_on_planted_rows(plant, defined, min_points):
    r, _, valid, s64, adj = plant
    got = defined[min_points]
    assert same(got, dbscan(adj, s64, min_points, valid), 1e-12)
    assert got[4].dtype == np.float64 and counts(got) == COUNTS[min_points]


@pytest.mark.parametrize("min_points", (1, 3, 6))
def test_definition_equals_the_brute_force_on_planted_rows_under_dot(min_points):
    """dot sees the row scales: unit rows times sqrt(2)^k, a threshold between the similarities"""
    r, _ = planted(150, 5)
    valid = np.isfinite(r).all(axis=1)
    unit = np.where(valid[:, None], r, 0).astype(np.float64)
    norm = np.sqrt((unit * unit).sum(axis=1))
    r = (unit / np.where(norm > 0, norm, 1)[:, None] * np.exp2(np.arange(150) % 3 / 2)[:, None]).astype(np.float32)
    r[~valid] = np.nan
    valid, dots = valid_sims64(r, "dot")                      # the zero row is valid under dot: it has no edge at 1.1
    adj = (dots >= float(np.float32(1.1))) & valid[:, None] & valid[None, :]
    got = sequence.density_clusters(r, 1.1, min_points, "dot")
    assert same(got, dbscan(adj, dots, min_points, valid), 1e-12)
    assert (got[5] == 3).sum() > 0 and (got[5][~valid] == 0).all()


def test_definition_equals_the_brute_force_on_integer_rows_under_dot():
    r, dots, threshold, min_points = integer_case()
    iu = np.triu_indices(len(r), 1)
    assert (dots[iu] == threshold).sum() >= 10                # ties exactly at the threshold: edges
    want = dbscan(dots >= threshold, dots, min_points)
    got = sequence.density_clusters(r, threshold, min_points, "dot")
    assert same(got, want, 0.0)
    adj = dots >= threshold
    adj[np.arange(len(r)), np.arange(len(r))] = False
    tied = int((second_gap(adj, dots, want) == 0).sum())
    print(f"\ninteger rows: threshold {threshold:g}, min_points {min_points}, kinds {counts(got)[1:]}, {tied} borders with tied anchors")
    assert tied >= 10 and min(counts(got)[1:]) >= 10          # core, border and noise rows all exist


def test_the_planted_structure(plant, defined):
    r, g, valid, s64, adj = plant
    ab = np.concatenate([g["familyA"], g["familyB"], g["bridges"]])
    # min_points 3: the bridges are core and chain A and B into one cluster, as single linkage does
    label, degree, size, anchor, sim, kind = defined[3]
    assert (kind[ab] == 3).all() and len(set(label[ab])) == 1 and label[ab[0]] == ab.min() and size[ab[0]] == 23
    single = sequence.threshold_clusters(r, T)
    assert sorted(s for s in single[2][single[0] == np.arange(len(r))] if s > 1) == [2, 6, 12, 14, 23]
    assert sorted(size[label == np.arange(len(r))]) == [6, 12, 14, 23]
    # min_points 6: the bridges are border rows and A and B are apart
    label, degree, size, anchor, sim, kind = defined[6]
    for f in "ABCD":
        m = g["family" + f]
        assert (kind[m] == 3).all() and (label[m] == m.min()).all(), f
    assert label[g["familyA"][0]] != label[g["familyB"][0]]
    assert (kind[g["bridges"]] == 2).all() and (degree[g["bridges"]] == 4).all()       # one edge into A, one into B, two bridges
    assert adj[np.ix_(g["bridges"], g["bridges"])].sum() == 6                          # border-border edges: they join nothing
    assert [("A" if a in g["familyA"] else "B" if a in g["familyB"] else "?") for a in anchor[g["bridges"]]] == ["B", "A", "B"]
    assert np.array_equal(anchor[g["bridges"]], [g["familyB"][0], g["familyA"][1], g["familyB"][2]])
    assert np.allclose(sim[g["bridges"]], 0.83, atol=1e-6)
    assert (kind[g["satellites"]] == 2).all() and np.array_equal(anchor[g["satellites"]], g["familyC"][:4])
    assert size[g["familyA"][0]] == 11 and size[g["familyB"][0]] == 12 and size[g["familyC"][0]] == 14 and size[g["familyD"][0]] == 11
    s0, s1 = g["hanger"]
    assert kind[s0] == 2 and anchor[s0] == g["familyD"][0] and adj[s0, s1]
    assert kind[s1] == 1 and label[s1] == -1 and anchor[s1] == -1 and size[s1] == 0 and np.isnan(sim[s1])     # an edge to a border row
    assert (kind[g["path"]] == 1).all() and (kind[g["pair"]] == 1).all() and (degree[g["pair"]] == 1).all()
    assert kind[g["zero"][0]] == 0 and kind[g["nan"][0]] == 0
    # min_points 11: only the rows that see their whole family and a hanger-on are core
    label, degree, size, anchor, sim, kind = defined[11]
    assert (kind[np.concatenate([g["family" + f] for f in "ABCD"])] >= 2).all() and (kind[g["satellites"]] == 1).sum() == 0


def test_the_two_identities_with_threshold_clusters(plant, defined):
    r = plant[0]
    c_label, c_degree, c_size, _ = sequence.threshold_clusters(r, T)
    for m in MIN_POINTS:
        assert np.array_equal(defined[m][1], c_degree)        # degree IS threshold_clusters' degree
    label, degree, size, anchor, sim, kind = defined[1]
    assert np.array_equal(label, c_label) and np.array_equal(size, c_size) and (kind[c_label >= 0] == 3).all()
    assert np.array_equal(anchor, np.where(c_label >= 0, np.arange(len(r)), -1)) and np.isnan(sim).all()
    label, degree, size, anchor, sim, kind = defined[2]
    assert np.array_equal(kind == 3, c_degree > 0) and np.array_equal(label[kind == 3], c_label[kind == 3])
    assert np.array_equal(kind == 1, c_size == 1) and (kind == 2).sum() == 0 and (label[kind == 1] == -1).all()


def star_rows():
    """rows whose dots draw a graph: element e of a row is 1 iff the row is at edge e.  0 is the centre of a star with 1, 2, 3; 4 has
    edges to 1 and to 5; 5 - 6; 7 alone"""
    r = np.zeros((8, 512), np.float32)
    for e, (a, b) in enumerate([(0, 1), (0, 2), (0, 3), (1, 4), (4, 5), (5, 6)]):
        r[a, e] = r[b, e] = 1
    r[7, 9] = 1
    return r


def test_a_border_border_edge_joins_nothing():
    # degrees 3 2 1 1 2 2 1 0; at min_points 4 only row 0 is core: 1, 2, 3 are its border rows; 4 has an edge to the border row 1 only
    label, degree, size, anchor, sim, kind = sequence.density_clusters(star_rows(), 1.0, 4, "dot")
    assert list(degree) == [3, 2, 1, 1, 2, 2, 1, 0]
    assert list(kind) == [3, 2, 2, 2, 1, 1, 1, 1] and list(label) == [0, 0, 0, 0, -1, -1, -1, -1]
    assert list(anchor) == [0, 0, 0, 0, -1, -1, -1, -1] and list(size) == [4, 4, 4, 4, 0, 0, 0, 0]
    assert np.isnan(sim[0]) and list(sim[1:4]) == [1.0, 1.0, 1.0] and np.isnan(sim[4:]).all()
    # at 3 the core rows are 0, 1, 4, 5: one cluster over 0 - 1 - 4 - 5, with 2, 3, 6 on its border
    label, degree, size, anchor, sim, kind = sequence.density_clusters(star_rows(), 1.0, 3, "dot")
    assert list(kind) == [3, 3, 2, 2, 3, 3, 2, 1] and list(label) == [0, 0, 0, 0, 0, 0, 0, -1] and list(anchor) == [0, 1, 0, 0, 4, 5, 5, -1]
    assert list(size) == [7] * 7 + [0]


def test_a_tie_at_the_threshold_is_an_edge():
    r = np.zeros((4, 512), np.float32)
    r[0, :2], r[1, :2], r[2, 2], r[3, 3] = (3, 0), (2, 1), 5, 1
    label, degree, size, anchor, sim, kind = sequence.density_clusters(r, 6.0, 2, "dot")           # r0.r1 = 6 exactly
    assert list(label) == [0, 0, -1, -1] and list(degree) == [1, 1, 0, 0] and list(kind) == [3, 3, 1, 1] and list(size) == [2, 2, 0, 0]
    assert list(sequence.density_clusters(r, np.nextafter(np.float32(6), np.float32(7)), 2, "dot")[0]) == [-1] * 4
    # the threshold is compared as the float32 it rounds to: 6 + 1e-9 is 6
    assert list(sequence.density_clusters(r, 6.0 + 1e-9, 2, "dot")[0]) == [0, 0, -1, -1]


def test_a_tie_between_two_anchors_goes_to_the_smaller_index():
    # rows 1, 2, 3 and 5, 6, 7 are two triangles of weight 2; row 4 has dot 2 with rows 6 and 2 alike and dot 1 with row 1
    r = np.zeros((8, 512), np.float32)
    for e, (a, b) in enumerate([(1, 2), (1, 3), (2, 3), (5, 6), (5, 7), (6, 7), (4, 6), (4, 2)]):
        r[a, 2 * e:2 * e + 2] = r[b, 2 * e:2 * e + 2] = 1
    r[4, 40] = r[1, 40] = 1
    label, degree, size, anchor, sim, kind = sequence.density_clusters(r, 1.0, 4, "dot")
    assert list(degree) == [0, 3, 3, 2, 3, 2, 3, 2] and list(kind) == [1, 3, 3, 2, 3, 2, 3, 2]
    label, degree, size, anchor, sim, kind = sequence.density_clusters(r, 1.0, 5, "dot")           # nobody is core
    assert (kind == 1).all()
    # make 4 a border row: cut its edge to 1, so that its degree is 2; cores at min_points 3: 1 2 3 5 6 7
    r[4, 40] = 0
    label, degree, size, anchor, sim, kind = sequence.density_clusters(r, 1.0, 4, "dot")
    assert list(degree) == [0, 2, 3, 2, 2, 2, 3, 2] and list(kind) == [1, 2, 3, 2, 2, 2, 3, 2]
    assert anchor[4] == 2 and label[4] == 2 and sim[4] == 2.0                # rows 2 and 6 tie at 2: the smaller index
    assert list(label) == [-1, 2, 2, 2, 2, 6, 6, 6] and list(size) == [0, 4, 4, 4, 4, 3, 3, 3]
    r[4, 12:14] = 3                                                         # the dot with row 6 is now 6: the larger similarity wins
    out = sequence.density_clusters(r, 1.0, 4, "dot")
    assert out[3][4] == 6 and out[0][4] == 6 and out[4][4] == 6.0


def test_invalid_rows():
    r = np.tile(rows(1, 4), (7, 1))
    r[1] = 0
    r[3, 100] = np.nan
    r[5, 511] = np.inf
    label, degree, size, anchor, sim, kind = sequence.density_clusters(r, 0.5, 4)
    assert list(label) == [0, -1, 0, -1, 0, -1, 0] and list(degree) == [3, 0, 3, 0, 3, 0, 3] and list(size) == [4, 0, 4, 0, 4, 0, 4]
    assert list(anchor) == [0, -1, 2, -1, 4, -1, 6] and list(kind) == [3, 0, 3, 0, 3, 0, 3] and np.isnan(sim).all()
    assert (sequence.density_clusters(r, 0.5, 5)[5] == [1, 0, 1, 0, 1, 0, 1]).all()
    label, degree, size, anchor, sim, kind = sequence.density_clusters(r, 0.0, 5, "dot")           # a zero row is valid under dot
    assert list(kind) == [3, 3, 3, 0, 3, 0, 3] and list(label) == [0, 0, 0, -1, 0, -1, 0] and degree[1] == 4


def test_edges_of_n_and_of_the_arguments():
    r = rows(9, 2)
    for n in (0, 1):
        out = sequence.density_clusters(r[:n], 0.5)
        assert [a.dtype for a in out] == [np.int64] * 4 + [np.float64, np.uint8] and all(a.shape == (n,) for a in out)
    one = sequence.density_clusters(r[:1], 0.5, 1)              # one valid row: core at 1 ...
    assert [int(a[0]) for a in one[:4]] == [0, 0, 1, 0] and one[5][0] == 3 and np.isnan(one[4][0])
    one = sequence.density_clusters(r[:1], 0.5, 2)              # ... noise at 2
    assert [int(a[0]) for a in one[:4]] == [-1, 0, 0, -1] and one[5][0] == 1 and np.isnan(one[4][0])
    label, degree, size, anchor, sim, kind = sequence.density_clusters(r, 1.0, 2)                  # above every similarity: all noise
    assert (label == -1).all() and (degree == 0).all() and (kind == 1).all()
    label, degree, size, anchor, sim, kind = sequence.density_clusters(r, -1.0, 9)                 # one cluster of all rows
    assert (label == 0).all() and (degree == 8).all() and (size == 9).all() and (kind == 3).all()
    assert (sequence.density_clusters(r, -1.0, 10)[5] == 1).all()
    assert sequence.density_clusters(r, 0.5, (1 << 31) - 1)[5].max() == 1
    for bad in (np.nan, np.inf, -np.inf, 1e39, "x"):
        with pytest.raises(ValueError, match="threshold"):
            sequence.density_clusters(r, bad)
    for bad in (0, -3, 1 << 31, 2.5, "x", None, True, np.nan):
        with pytest.raises(ValueError, match=r"min_points.*\[1, 2\^31\)"):
            sequence.density_clusters(r, 0.5, bad)
    assert sequence.density_min_points(np.int64(7)) == 7 and sequence.density_min_points(3.0) == 3
    with pytest.raises(ValueError, match="metric"):
        sequence.density_clusters(r, 0.5, 5, "euclid")
    with pytest.raises(ValueError, match="512"):
        sequence.density_clusters(r[:, :100], 0.5)


def test_density_table_and_result():
    out = sequence.density_clusters(star_rows(), 1.0, 3, "dot")
    want = [{"label": 0, "size": 7, "cores": 4, "borders": 3, "members": [0, 1, 2, 3, 4, 5, 6]}]
    assert sequence.DENSITY_FIELDS == ("label", "degree", "size", "anchor", "sim", "kind")
    assert sequence.density_table(out) == want and sequence.density_table(dict(zip(sequence.DENSITY_FIELDS, out))) == want
    res = DensityResult.build(out, 1.0, 3, "dot")
    assert res.table() == want and (res.n_clusters, res.n_core, res.n_border, res.n_noise) == (1, 4, 3, 1)
    assert res.threshold == 1.0 and res.min_points == 3 and res.metric == "dot"
    assert list(res.asdict()) == ["label", "degree", "size", "anchor", "sim", "kind", "threshold", "min_points", "metric"]
    assert res.table(list("abcdefgh"))[0] == {"label": "a", "size": 7, "cores": 4, "borders": 3, "members": list("abcdefg")}
    r = np.zeros((8, 512), np.float32)
    for e, (a, b) in enumerate([(1, 2), (1, 3), (2, 3), (5, 6), (5, 7), (6, 7), (4, 6), (4, 2)]):
        r[a, e] = r[b, e] = 1
    tab = sequence.density_table(sequence.density_clusters(r, 1.0, 4, "dot"))      # two clusters; row 0 is noise and in no record
    assert tab == [{"label": 2, "size": 4, "cores": 1, "borders": 3, "members": [1, 2, 3, 4]},
                   {"label": 6, "size": 3, "cores": 1, "borders": 2, "members": [5, 6, 7]}]
    assert sequence.density_table(sequence.density_clusters(r[:0], 1.0)) == []
    assert DensityResult.build(sequence.density_clusters(r[:0], 1.0), 1.0, 5, "cosine").n_clusters == 0


def test_abi_declares_the_entry_points_and_checks_arguments_before_the_ctx():
    text = open(os.path.join(ROOT, "include", "genomad_nn.h")).read()
    lib = _lib.load()
    for name in ("gnn_density", "gnn_density_dev"):
        assert f"int {name}(" in text and name in _lib.SIGNATURES and hasattr(lib, name)
    assert "#define GNN_K_COUNT 8" in text
    for m in ("density", "density_dev"):
        assert hasattr(NNEngine, m)
    q = rows(2, 1)
    out = [np.full(2, 7, np.int64) for _ in range(4)] + [np.full(2, 7, np.float32), np.full(2, 7, np.uint8)]
    ptrs = [a.ctypes.data for a in out]
    for fn in (lib.gnn_density, lib.gnn_density_dev):
        name = b"gnn_density_dev" if fn is lib.gnn_density_dev else b"gnn_density:"
        for n in (-1, 1 << 31):
            assert fn(None, q.ctypes.data, n, float("nan"), 0, 9, *ptrs) == _lib.ERR_ARG       # the first of four bad arguments
            assert f"{n} rows is outside [0, 2^31)".encode() in lib.gnn_last_error() and name in lib.gnn_last_error()
        for t, word in ((float("nan"), b"nan"), (float("inf"), b"inf"), (float("-inf"), b"-inf"), (1e39, b"inf")):
            assert fn(None, q.ctypes.data, 2, t, 0, 9, *ptrs) == _lib.ERR_ARG                  # before min_points and the metric
            assert b"threshold " + word in lib.gnn_last_error() and b"finite" in lib.gnn_last_error() and name in lib.gnn_last_error()
        for m in (0, -1, 1 << 31, -(1 << 40)):
            assert fn(None, q.ctypes.data, 2, 0.5, m, 9, *ptrs) == _lib.ERR_ARG                # before the metric
            assert f"min_points {m} is outside [1, 2^31)".encode() in lib.gnn_last_error() and name in lib.gnn_last_error()
        for metric in (2, -1, 9):
            assert fn(None, None, 2, 0.5, 5, metric, *ptrs) == _lib.ERR_ARG                    # before the pointers
            assert f"metric {metric} is outside [0, 1]".encode() in lib.gnn_last_error()
        for hole in range(7):
            args = [q.ctypes.data] + ptrs
            args[hole] = None
            assert fn(None, args[0], 2, 0.5, 5, 0, *args[1:]) == _lib.ERR_ARG
            assert b"bad argument to " + name.rstrip(b":") in lib.gnn_last_error()
            assert b"the rows and the six outputs are required" in lib.gnn_last_error()
        assert fn(None, q.ctypes.data, 2, 0.5, (1 << 31) - 1, 1, *ptrs) == _lib.ERR_ARG        # valid, but no ctx
        assert b"ctx is NULL" in lib.gnn_last_error()
        assert fn(None, None, 0, 0.5, 1, 0, None, None, None, None, None, None) == _lib.ERR_ARG    # n = 0 needs no pointer, but a ctx
        assert b"ctx is NULL" in lib.gnn_last_error()
    assert all((a == 7).all() for a in out)                       # nothing was written


# ---- main() over a fake engine ---------------------------------------------------------------------------------------------------
class FakeDensityEngine(FakeNeighbourEngine):
    """the stand-in of tests/test_neighbours_host.py plus density, served from sequence.density_clusters (sim as the device's f32)"""
    calls = []

    def density(self, rows, threshold, min_points=5, metric="cosine"):
        type(self).calls.append(("density", len(rows), float(threshold), int(min_points), metric))
        label, degree, size, anchor, sim, kind = sequence.density_clusters(rows, threshold, min_points, metric)
        return DensityResult.build((label, degree, size, anchor, sim.astype(np.float32), kind), threshold, min_points, metric)


ENV = ("GENOMAD_AMD_DENSITY", "GENOMAD_AMD_DENSITY_MIN_POINTS")


@pytest.fixture
def fake_main(monkeypatch):
    monkeypatch.setattr(nnc, "_engine", lambda: FakeDensityEngine())
    for k in SWITCHES + ("GENOMAD_AMD_CLUSTERS",) + ENV:
        monkeypatch.delenv(k, raising=False)
    del FakeDensityEngine.calls[:]
    return lambda fa, out, **kw: nnc.main(fa, out, False, 128, False, 1, False, False, **kw)


def test_density_switch_values(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    assert nnc.density_requested() is None
    for v, want in (("", None), (" 0.9 ", float(np.float32(0.9))), ("1", 1.0), ("-1", -1.0), ("0", 0.0), ("5e-1", 0.5)):
        monkeypatch.setenv("GENOMAD_AMD_DENSITY", v)
        assert nnc.density_requested() == (None if want is None else (want, 5))
    for v in ("1.01", "-1.5", "nan", "inf", "high", "0,9"):
        monkeypatch.setenv("GENOMAD_AMD_DENSITY", v)
        with pytest.raises(ValueError, match=r"GENOMAD_AMD_DENSITY=.*\[-1, 1\]"):
            nnc.density_requested()
    monkeypatch.setenv("GENOMAD_AMD_DENSITY", "0.5")
    for v, want in (("", 5), ("1", 1), (" 12 ", 12), ("2147483647", (1 << 31) - 1)):
        monkeypatch.setenv("GENOMAD_AMD_DENSITY_MIN_POINTS", v)
        assert nnc.density_requested() == (0.5, want)
    for v in ("0", "-2", "2.5", "many", "2147483648", "1e2"):
        monkeypatch.setenv("GENOMAD_AMD_DENSITY_MIN_POINTS", v)
        with pytest.raises(ValueError, match=r"GENOMAD_AMD_DENSITY_MIN_POINTS=.*integer >= 1"):
            nnc.density_requested()
    monkeypatch.delenv("GENOMAD_AMD_DENSITY")                   # min_points alone is refused
    monkeypatch.setenv("GENOMAD_AMD_DENSITY_MIN_POINTS", "3")
    with pytest.raises(ValueError, match="GENOMAD_AMD_DENSITY_MIN_POINTS='3' needs GENOMAD_AMD_DENSITY"):
        nnc.density_requested()


def test_main_refuses_the_switches_before_anything_is_written(tmp_path, monkeypatch, fake_main, capsys):
    fa = tmp_path / "s.fna"
    _write_fasta(fa, n=3)
    monkeypatch.setenv("GENOMAD_AMD_DENSITY", "1.5")
    with pytest.raises(ValueError, match="GENOMAD_AMD_DENSITY"):
        fake_main(fa, tmp_path / "bad")
    assert not (tmp_path / "bad").exists()                  # before anything is written
    monkeypatch.delenv("GENOMAD_AMD_DENSITY")
    monkeypatch.setenv("GENOMAD_AMD_DENSITY_MIN_POINTS", "4")
    monkeypatch.setenv("GENOMAD_AMD_EMBEDDINGS", "1")
    with pytest.raises(ValueError, match="GENOMAD_AMD_DENSITY_MIN_POINTS='4' needs GENOMAD_AMD_DENSITY"):
        fake_main(fa, tmp_path / "alone")
    assert not (tmp_path / "alone").exists()
    monkeypatch.delenv("GENOMAD_AMD_EMBEDDINGS")
    monkeypatch.setenv("GENOMAD_AMD_DENSITY", "0.9")
    with pytest.raises(SystemExit) as exc:
        fake_main(fa, tmp_path / "refused")
    assert exc.value.code == 1
    err = capsys.readouterr().err
    assert "GENOMAD_AMD_DENSITY needs GENOMAD_AMD_EMBEDDINGS=1" in err and len(err.strip().splitlines()) == 1
    assert not list((tmp_path / "refused").rglob("*.npz")) and not list((tmp_path / "refused").rglob("*.tsv"))
    assert FakeDensityEngine.calls == []


def test_main_writes_both_files_follows_the_request_and_removes_stale_ones(tmp_path, monkeypatch, fake_main):
    fa = tmp_path / "m.fna"
    recs = _write_fasta(fa, n=6)
    with open(fa, "a") as f:
        for k in range(2):
            f.write(f">twin{k} of c2\n{dict(recs)['c2']}\n")  # the same bytes as c2: the same embedding
    monkeypatch.setenv("GENOMAD_AMD_EMBEDDINGS", "1")
    fake_main(fa, tmp_path / "unset")
    assert not any(c[0] == "density" for c in FakeDensityEngine.calls)
    monkeypatch.setenv("GENOMAD_AMD_DENSITY", "0.999")
    monkeypatch.setenv("GENOMAD_AMD_DENSITY_MIN_POINTS", "3")
    out = tmp_path / "on"
    fake_main(fa, out)
    d0, d1 = tmp_path / "unset" / "m_nn_classification", out / "m_nn_classification"
    assert _tree(d1) == sorted(_tree(d0) + ["m_nn_density.npz", "m_nn_density.tsv"])
    for rel in _tree(d0):                                   # every other output: the same arrays, the same bytes
        if rel.endswith(".npz"):
            assert _same_npz(d0 / rel, d1 / rel), rel
        elif rel.endswith(".tsv"):
            assert (d0 / rel).read_bytes() == (d1 / rel).read_bytes(), rel
    z, emb = _npz(d1 / "m_nn_density.npz"), _npz(d1 / "m_nn_embeddings.npz")
    n = len(emb["contig_names"])
    t32 = float(np.float32(0.999))
    assert sorted(z) == ["anchor", "contig_names", "degree", "kind", "label", "metric", "min_points", "sim", "size", "threshold"]
    assert list(z["contig_names"]) == list(emb["contig_names"])
    assert float(z["threshold"]) == t32 and z["threshold"].dtype == np.float64 and str(z["metric"]) == "cosine"
    assert int(z["min_points"]) == 3 and z["min_points"].dtype == np.int64
    assert z["sim"].dtype == np.float32 and z["kind"].dtype == np.uint8
    assert FakeDensityEngine.calls.count(("density", n, t32, 3, "cosine")) == 1
    want = sequence.density_clusters(emb["embeddings"], 0.999, 3)
    assert same([z[k] for k in sequence.DENSITY_FIELDS], want, 1e-6)
    names = list(z["contig_names"])
    trio = sorted(names.index(k) for k in ("c2", "twin0", "twin1"))
    assert (z["kind"][trio] == 3).all() and (z["label"][trio] == trio[0]).all() and (z["size"][trio] == 3).all()
    assert (z["degree"][trio] == 2).all() and np.array_equal(z["anchor"][trio], trio)
    lines = (d1 / "m_nn_density.tsv").read_text().splitlines()
    assert lines[0] == "seq_name\tcluster\tcluster_size\tkind\tanchor\tsimilarity\tdegree" and len(lines) == n + 1
    assert lines[1 + trio[1]] == f"{names[trio[1]]}\t{names[trio[0]]}\t3\tcore\t{names[trio[1]]}\tNA\t2"
    others = [i for i in range(n) if i not in trio]
    assert others and all(lines[1 + i] == f"{names[i]}\tNA\t0\tnoise\tNA\tNA\t0" for i in others if z["kind"][i] == 1)
    runs = lambda: sum(1 for c in FakeDensityEngine.calls if c == "plain")       # noqa: E731
    before = runs()
    fake_main(fa, out)
    assert runs() == before                                  # same request, everything there: nothing runs
    monkeypatch.setenv("GENOMAD_AMD_DENSITY_MIN_POINTS", "4")
    fake_main(fa, out)                                       # another min_points: recomputed - nobody is core any more
    z = _npz(d1 / "m_nn_density.npz")
    assert runs() == before + 1 and int(z["min_points"]) == 4 and (z["label"] == -1).all() and (z["kind"] == 1).all()
    monkeypatch.setenv("GENOMAD_AMD_DENSITY", "-1")
    fake_main(fa, out)                                       # another threshold: recomputed
    z = _npz(d1 / "m_nn_density.npz")
    assert runs() == before + 2 and float(z["threshold"]) == -1.0 and (z["label"] == 0).all() and (z["size"] == n).all()
    monkeypatch.delenv("GENOMAD_AMD_DENSITY_MIN_POINTS")
    fake_main(fa, out)                                       # the default is 5, not the 4 of the file: recomputed
    assert runs() == before + 3 and int(_npz(d1 / "m_nn_density.npz")["min_points"]) == 5
    (d1 / "m_nn_density.tsv").unlink()
    fake_main(fa, out)                                       # one of the pair is gone: recomputed
    assert runs() == before + 4 and (d1 / "m_nn_density.tsv").exists()
    monkeypatch.delenv("GENOMAD_AMD_DENSITY")
    fake_main(fa, out)                                       # no request: both files go
    assert runs() == before + 5 and not (d1 / "m_nn_density.npz").exists() and not (d1 / "m_nn_density.tsv").exists()
    assert _tree(d1) == _tree(d0)
    monkeypatch.setenv("GENOMAD_AMD_DENSITY", "0.5")
    monkeypatch.setenv("GENOMAD_AMD_NEIGHBOURS", "2")        # both searches in one run
    monkeypatch.setenv("GENOMAD_AMD_STRAND", "both")
    FakeDensityEngine.classify_contigs_strand = lambda self, seq, offsets, strand="both", single_window=False, precision=None, embed=False: (
        lambda r: (r[0], r[1], FakeDensityEngine.embed_contigs(self, seq, offsets)[1], r[3], r[4]))(
            FakeStrandEngine.classify_contigs_strand(self, seq, offsets, strand, single_window, precision, embed))
    try:
        fake_main(fa, out)
    finally:
        del FakeDensityEngine.classify_contigs_strand
    assert str(_npz(d1 / "m_nn_density.npz")["strand"]) == "both" and str(_npz(d1 / "m_nn_neighbours.npz")["strand"]) == "both"


def test_the_table_names_kinds_and_writes_na_where_there_is_none(tmp_path):
    r = np.zeros((6, 512), np.float32)
    for e, (a, b) in enumerate([(0, 1), (0, 2), (1, 2), (2, 3)]):
        r[a, e] = r[b, e] = 1
    r[3, 3] = 0.5                                             # dot(2, 3) = 0.5
    r[4, 9] = 1
    res = DensityResult.build(sequence.density_clusters(r, 0.5, 3, "dot"), 0.5, 3, "dot")
    nnc.write_density_tsv(tmp_path / "t.tsv", list("abcdef"), res)
    assert (tmp_path / "t.tsv").read_text() == ("seq_name\tcluster\tcluster_size\tkind\tanchor\tsimilarity\tdegree\n"
                                                "a\ta\t4\tcore\ta\tNA\t2\nb\ta\t4\tcore\tb\tNA\t2\nc\ta\t4\tcore\tc\tNA\t3\n"
                                                "d\ta\t4\tborder\tc\t0.500000\t1\ne\tNA\t0\tnoise\tNA\tNA\t0\nf\tNA\t0\tnoise\tNA\tNA\t0\n")
    res = DensityResult.build(sequence.density_clusters(r, 0.5, 3, "cosine"), 0.5, 3, "cosine")      # f is a zero row: invalid
    nnc.write_density_tsv(tmp_path / "t.tsv", list("abcdef"), res)
    assert (tmp_path / "t.tsv").read_text().splitlines()[-1] == "f\tNA\t0\tinvalid\tNA\tNA\t0"
