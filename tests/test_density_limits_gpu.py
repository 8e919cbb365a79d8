"""Density clusters on the MI355X at the limits tests/test_density_gpu.py stays away from (inputs, the exact oracle and their CPU-side
conditions: tests/density_limits_data.py, tests/test_density_limits_host.py).  Which line of which kernel each group pins:

  A  signs           dn_link_kernel / dn_flatten_kernel (gnn_density.hip): `nn_key(nn_image(s), core row)` and `nn_unimage(best >> 32)`
                     with s <= 0 - the `u >> 31` branch, `s + 0.f`, a tie on a negative key, 0 against negative rivals -; on dense
                     signed graphs the row-side shuffle tree (`__shfl_xor(key, s)`, lkey) and the column-side `atomicMax(a.key +
                     cg[nb], key)` compete for one row thousands of times per tile.
  B  borders         `core[]` padded to the tile (`lcore[tid] = a.core[r0 + tid]`), `a.core[col]` behind `cg[nb] >= 0`, `last_blk`,
                     `t.b1 > t.r0 + 1` with n on and beside the 32-column block, the 64-row tile and the 256-column step.
  C  flags, trees    dn_init_kernel over max(n, flags) with 2312 flags for 2176 rows; `a.flag[blockIdx.x * a.splits + blockIdx.y]` of
                     workgroups whose index is >= n and that hold core-core edges; cl_join through top[] and nn_root(parent, anchor)
                     on a path of 511 rows that crosses all 34 tiles; the workspace after other searches.
  D  row scales      nn_prepare_kernel as density reaches it, and the key's image of the value and back.
  E  two ranges      SPLIT_MAX = 65280: `flag[tile * splits + 1]`, `max(b0, r0)`, a border row whose key comes from workgroups of two
                     ranges - through the LDS flush and through the per-column global maximum -, cl_join across the range border.

The reference is exact everywhere: density's edges and values are those of the graph, so engine.density(r, t, m) must equal
density_of_graph(engine.graph(r, t), m) on any input, all six arrays bit for bit (the graph has its own limits tests against fp64);
on integer rows under dot, where every value is exact, it is the numpy definition (sequence.density_clusters) itself.

Measured on an MI355X (core / border / noise rows): the border contest 184 / 16 / 0; the 333 signed rows at -0.05, 0.0 and 0.05 at
the quartiles of their degrees 267 / 66, 173 / 160 and 97 / 236, 254 / 79, 168 / 165 and 96 / 237, 261 / 72, 169 / 164 and 99 / 234,
no noise, one cluster each; the chain 2174 / 2 / 0 in 513 clusters; the 65350 rows at 0.55 (325011 edges) 63021 / 0 / 2329 in 23
clusters at min_points 2 and 51002 / 11794 / 2554 in 4 clusters at 5, 0.026 s per call with the upload of 134 MB; group E as a whole
0.8 s, no other test more than 0.03 s, the file 2.0 s.  No test found a fault in the kernels.  Two one-line changes to gnn_density.hip
change no output and so no test can see them: dn_init_kernel launched over n only (a flag byte that is not cleared is either set by
the count pass or makes a link workgroup run that finds no edge) and the padding of lcore[] read as 1 (a padded row has lok = 0 and so
no edge)."""
import time

import numpy as np
import pytest

from genomad_amd import sequence
from genomad_amd.engine import NNEngine
from tests import density_limits_data as dl
from tests import embedding_limits_data as lim
from tests import graph_limits_data as gd
from tests.embedding_limits_data import VALUE_TOL
from tests.neighbours_data import rows
from tests.test_density_limits_host import assert_chain

pytestmark = pytest.mark.gpu

FIELDS = sequence.DENSITY_FIELDS


def arrays(res):
    return tuple(getattr(res, k) for k in FIELDS)


def definition(r, t, m, metric="dot"):
    return dl.as_device(sequence.density_clusters(r, t, m, metric))


def report(what, got):
    core, border, noise, invalid = dl.counts(got[5])
    print(f"\n{what}: {core} core, {border} border, {noise} noise, {invalid} invalid, {int((got[0] == np.arange(len(got[0]))).sum())} clusters")
    return core, border, noise


# ---- A: signs ------------------------------------------------------------------------------------------------------------------------

def test_a_border_rows_whose_best_core_neighbour_is_negative_or_zero(engine):
    r, _, want = dl.border_contest()
    t, m = lim.CONTEST_THRESHOLD, dl.CONTEST_MIN_POINTS
    right = definition(r, t, m)
    members = list(dl.CONTEST_MEMBERS)
    try:
        for split in (0, 32):
            engine.set_neighbour_split(split)
            res = engine.density(r, t, m, "dot")
            got = arrays(res)
            dl.check_same(got, right, split)
            assert [int(x) for x in res.anchor[members]] == [want[i][0] for i in members], split
            assert [float(x) for x in res.sim[members]] == [want[i][1] for i in members], split
            zero = res.sim[members] == 0
            assert zero.sum() == 4 and (res.sim[members][zero].view(np.uint32) == 0).all(), split      # +0, not -0
            assert (res.n_core, res.n_border, res.n_noise, res.n_clusters) == (184, 16, 0, 1)
        report("border contest at -10, min_points 20", got)
    finally:
        engine.set_neighbour_split(0)


@pytest.mark.parametrize("t", gd.SIGN_THRESHOLDS)
def test_a_dense_signed_graphs_equal_the_oracle_of_the_devices_graph(engine, t):
    r = dl.signed_case()
    n = len(r)
    try:
        engine.set_neighbour_split(0)
        g = engine.graph(r, t)
        degree = g.degree()
        assert np.array_equal(degree, engine.cluster(r, t).degree)
        for k, m in enumerate(dl.quartile_min_points(degree)):
            engine.set_neighbour_split(0)
            want = dl.density_of_graph(g.indptr, g.col, g.sim, g.valid, m)
            first = arrays(engine.density(r, t, m))
            dl.check_same(first, want, (t, m))
            assert np.array_equal(first[1], degree)
            core, border, _ = report(f"signed rows at {t}, min_points {m}", first)
            if k == 1:
                assert core >= n // 4 and border >= n // 4
            for split in gd.SPLITS:
                engine.set_neighbour_split(split)
                dl.check_same(arrays(engine.density(r, t, m)), first, (t, m, split))
    finally:
        engine.set_neighbour_split(0)


# ---- B: block, tile and step borders -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", gd.PREFIXES)
def test_b_block_tile_and_step_borders(engine, n):
    r, dots = dl.prefix(n)
    try:
        for t in lim.integer_thresholds(lim.signed_integer_rows(gd.N_INTEGER)):
            m = dl.median_min_points(dots, t)
            right = definition(r, t, m)
            for split in gd.PREFIX_SPLITS:
                engine.set_neighbour_split(split)
                got = arrays(engine.density(r, t, m, "dot"))
                assert all(len(x) == n for x in got)
                dl.check_same(got, right, (n, t, split))
    finally:
        engine.set_neighbour_split(0)


# ---- C: flags and trees --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def chain():
    r, where, _ = dl.chain_case()
    return r, where, definition(r, dl.CHAIN_THRESHOLD, dl.CHAIN_MIN_POINTS)


def chain_density(eng, r):
    return arrays(eng.density(r, dl.CHAIN_THRESHOLD, dl.CHAIN_MIN_POINTS, "dot"))


def test_c_more_flags_than_rows_and_a_path_across_all_tiles(engine, chain):
    r, where, right = chain
    try:
        with NNEngine(0) as fresh:                                     # its flag buffer is newly allocated
            fresh.set_neighbour_split(dl.CHAIN_SPLIT)
            got = chain_density(fresh, r)
            dl.check_same(got, right, "fresh engine, split 32")
            assert_chain(got, where)
        report("chain of 511 among 2176 rows", got)
        for split in (0, 4096):
            engine.set_neighbour_split(split)
            got = chain_density(engine, r)
            dl.check_same(got, right, split)
            assert_chain(got, where)
    finally:
        engine.set_neighbour_split(0)


def test_c_the_workspace_after_other_searches(engine, chain):
    r, where, right = chain
    small, dots65 = dl.prefix(65)
    t65 = lim.integer_thresholds(lim.signed_integer_rows(gd.N_INTEGER))[1]
    m65 = dl.median_min_points(dots65, t65)                            # 33 core, 28 border, 4 noise rows
    other = rows(333, 13)
    try:
        engine.set_neighbour_split(dl.CHAIN_SPLIT)
        first = chain_density(engine, r)
        dl.check_same(first, right)
        first65 = arrays(engine.density(small, t65, m65, "dot"))
        dl.check_same(first65, definition(small, t65, m65))
        assert engine.cluster(other, 0.3).n_clusters >= 1
        assert engine.match(other[:70], other, 0.3).n_edges > 0
        dl.check_same(chain_density(engine, r), first, "the chain again")
        dl.check_same(arrays(engine.density(small, t65, m65, "dot")), first65, "65 rows again")
    finally:
        engine.set_neighbour_split(0)


# ---- D: row scales -------------------------------------------------------------------------------------------------------------------

def test_d_a_power_of_two_per_row_changes_no_bit(engine):
    r = dl.signed_case()
    r2 = lim.power_of_two_scaled(r, 3)
    try:
        engine.set_neighbour_split(0)
        own = engine.neighbours(r, None, 10)
        threshold = np.sort(own[1][:, 0])[333 // 2]                   # one of the device's values, as test_c_a_power_of_two_per_row_changes_no_bit picks it
        assert threshold.dtype == np.float32 and 0 < threshold < 1
        g = engine.graph(r, threshold)
        for need in (2, 3):                                           # 3: about 60 core and 60 border rows (fp64, on the CPU)
            want = dl.density_of_graph(g.indptr, g.col, g.sim, g.valid, need)
            first = arrays(engine.density(r, threshold, need))
            dl.check_same(first, want, need)
            report(f"signed rows at the device's own {float(threshold):.6f}, min_points {need}", first)
            for split in (0, 32):
                engine.set_neighbour_split(split)
                dl.check_same(arrays(engine.density(r2, threshold, need)), first, (need, split))
            engine.set_neighbour_split(0)
        assert dl.counts(first[5])[0] >= 20 and dl.counts(first[5])[1] >= 20
    finally:
        engine.set_neighbour_split(0)


@pytest.mark.parametrize("which, t", (("extreme", 0.05), ("extreme", 0.5), ("heavy", 0.05), ("heavy", 0.2)))
def test_d_rows_from_all_subnormal_to_flt_max_and_heavy_rows(engine, which, t):
    r = lim.extreme_base() if which == "extreme" else lim.heavy_rows(333, 8)
    try:
        for split in (0, 32):
            engine.set_neighbour_split(split)
            g = engine.graph(r, t)
            degree = g.degree()
            assert g.valid.all() and np.array_equal(degree, engine.cluster(r, t).degree)
            for m in sorted({1, 2, 3, int(np.median(degree)) + 1}):
                got = arrays(engine.density(r, t, m))
                dl.check_same(got, dl.density_of_graph(g.indptr, g.col, g.sim, g.valid, m), (which, t, m, split))
                assert np.array_equal(got[1], degree)
                if split == 0:
                    report(f"{which} rows at {t}, min_points {m}", got)
    finally:
        engine.set_neighbour_split(0)


def test_d_rows_beyond_the_f16_range_are_valid_noise_and_nobodys_anchor_under_dot(engine):
    base = lim.out_of_range_base()
    out = list(lim.OUT_OF_RANGE)
    keep = np.delete(np.arange(333), out)
    rest = np.ascontiguousarray(base[keep])
    dots = rest.astype(np.float64) @ rest.astype(np.float64).T
    threshold = float(np.sort(dots[np.triu_indices(331, 1)])[int(331 * 330 / 2 * 0.98)])      # as the graph's test thresholds it
    m = dl.median_min_points(dots, threshold)
    right = definition(rest, threshold, m)
    core, border, noise, _ = dl.counts(right[5])
    assert m >= 2 and core > 50 and border > 50
    new = np.full(333, -1, np.int64)
    new[keep] = np.arange(331)
    try:
        for split in (0, 32):
            engine.set_neighbour_split(split)
            res = engine.density(base, threshold, m, "dot")
            assert (res.kind[out] == dl.KIND_NOISE).all() and (res.degree[out] == 0).all() and (res.label[out] == -1).all()
            assert (res.anchor[out] == -1).all() and (res.size[out] == 0).all() and np.isnan(res.sim[out]).all()
            assert not np.isin(res.anchor, out).any() and not np.isin(res.label, out).any()
            label, degree, size, anchor, sim, kind = (x[keep] for x in arrays(res))
            renumbered = (np.where(label >= 0, new[label], -1), degree, size, np.where(anchor >= 0, new[anchor], -1), sim, kind)
            assert (new[label[label >= 0]] >= 0).all() and (new[anchor[anchor >= 0]] >= 0).all()
            dl.check_same(renumbered, right, split)
            one = engine.density(base, threshold, 1, "dot")          # at min_points 1 every valid row is core, alone if it has no edge
            assert (one.kind[out] == dl.KIND_CORE).all() and np.array_equal(one.label[out], out) and (one.size[out] == 1).all()
            assert np.array_equal(one.anchor[out], out) and (one.degree[out] == 0).all()
        report(f"rows beyond the f16 range, the other 331 at {threshold}, min_points {m}", arrays(res))
    finally:
        engine.set_neighbour_split(0)


# ---- E: two ranges -------------------------------------------------------------------------------------------------------------------

def test_e_a_full_range_of_65280_columns_and_a_second_one(engine):
    """65350 rows under the split 1 << 20, which clamps to 65280: two ranges, two flags per tile"""
    base, plants = dl.two_range_case()
    n, t = lim.NB_CAPPED, gd.TWO_RANGE_THRESHOLD
    try:
        engine.set_neighbour_split(1 << 20)
        g = engine.graph(base, t)
        found = {}
        for m in (2, dl.TWO_RANGE_MIN_POINTS):
            t0 = time.perf_counter()
            found[m] = arrays(engine.density(base, t, m))
            seconds = time.perf_counter() - t0
            dl.check_same(found[m], dl.density_of_graph(g.indptr, g.col, g.sim, g.valid, m), m)
            report(f"65350 rows at {t}, ranges of 65280, min_points {m}: {g.n_edges} edges, {seconds:.3f} s", found[m])
        copies = [gd.COPIES_OF, *gd.COPIES, n - 1]
        for m, (label, degree, size, anchor, sim, kind) in found.items():
            # clusters whose core rows lie in both ranges: the five copies of row 100, and family2
            for members in (copies, list(plants["family2"])):
                assert (kind[members] == dl.KIND_CORE).all() and len(set(label[members].tolist())) == 1, (m, members)
                assert min(members) < lim.SPLIT_MAX <= max(members)
            assert label[list(plants["family2"])[0]] == min(plants["family2"]) and size[min(plants["family2"])] == dl.FAMILY
        label, degree, size, anchor, sim, kind = found[dl.TWO_RANGE_MIN_POINTS]
        for x, (best, second) in plants["expect"].items():           # border rows and their anchors in the other range
            assert kind[x] == dl.KIND_BORDER and anchor[x] == best and label[x] == label[best], (x, int(kind[x]), int(anchor[x]))
            assert abs(float(sim[x]) - (dl.NEAR if second is None else dl.BEST)) <= VALUE_TOL
            assert degree[x] == (1 if second is None else 2) and kind[best] == dl.KIND_CORE
            assert second is None or kind[second] == dl.KIND_CORE
        for name in ("family0", "family1"):
            members = list(plants[name])
            assert (kind[members] == dl.KIND_CORE).all() and (label[members] == min(members)).all()
        c = engine.cluster(base, t)
        one = engine.density(base, t, 1)
        assert np.array_equal(one.label, c.label) and np.array_equal(one.degree, c.degree) and np.array_equal(one.size, c.size)
        assert np.array_equal(found[2][1], c.degree)
        for split in gd.TWO_RANGE_SPLITS:
            engine.set_neighbour_split(split)
            got = arrays(engine.density(base, t, dl.TWO_RANGE_MIN_POINTS))
            dl.check_same(got, found[dl.TWO_RANGE_MIN_POINTS], split)
    finally:
        engine.set_neighbour_split(0)
