"""Spherical k-means among encoder embeddings on the MI355X: planted rows against the numpy definition (sequence.spherical_kmeans) -
labels, sizes, iterations, the converged flag and the farthest-first picks exactly, on inputs whose best and second-best centroid
keep 1e-4 apart at every assignment (tests/test_kmeans_host.py asserts it; the device's f32 similarities are within 1e-5), the
centroids within 1e-6 -, consistency on the device's own values (label / sim ARE neighbours(rows, centroids, 1), bit for bit, tied
centroids included), bit-identity under the split of the centroids, both paths of the update, the host and the device entry points and
a permutation of the rows, signed rows against padded columns, the farthest-first traversal replayed from neighbours' values, the
edges of the interface, centroids() for the labels of cluster(), and embed_contigs -> kmeans end to end.  333 rows are six 64-row
tiles, off every boundary; k = 7, 33 and 300 lie below a 32-column block, across one and across the 256-column step."""
import numpy as np
import pytest

from genomad_amd import sequence, synthetic
from genomad_amd._lib import GnnError
from tests.kmeans_data import INITS, KS, defined, init_rows, planted, resultant, signed_init, signed_rows, unit64
from tests.neighbours_data import rows

pytestmark = pytest.mark.gpu

CASES = [(k, kind) for k in KS for kind in INITS]
SPLITS = (32, 100, 333, 0)
ARRAYS = ("label", "sim", "centroids", "size", "init_rows")


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def identical(got, first):
    """every output bit for bit, the two scalars included"""
    return (all(getattr(got, f).dtype == getattr(first, f).dtype and np.array_equal(bits(getattr(got, f)), bits(getattr(first, f)))
                for f in ARRAYS) and got.iterations == first.iterations and got.converged == first.converged)


def is_neighbours(engine, r, res):
    """label / sim are what neighbours returns for (rows, the centroids returned, k = 1), bit for bit"""
    idx, sim = engine.neighbours(r, res.centroids, 1)
    return np.array_equal(res.label, idx[:, 0]) and np.array_equal(bits(res.sim), bits(sim[:, 0]))


@pytest.fixture(scope="module")
def found(engine):
    """the device's answer on the planted rows for every case, computed once with the library's own split"""
    engine.set_neighbour_split(0)
    r, _ = planted()
    return {(k, kind): engine.kmeans(r, k, init_rows(kind, k)) for k, kind in CASES}


@pytest.mark.parametrize("k,kind", CASES)
def test_planted_rows_equal_the_definition(found, k, kind):
    """The bound on the centroids, derived.  A centroid is unit(S), S the sum of its m members' unit rows.  The device sums q_i, the
    hi + lo image of the unit row that nn_prepare made in f32: the norm's sum, its square root and the division round once each
    (3 x 2^-24 of the element) and the lo limb is an f16 rounding of a remainder below 2^-11 of the element (2^-22 of it): every
    element of q_i is within 4.2e-7 of its own magnitude of the true unit row's, so |q_i - u_i|_2 <= 4.2e-7 and |dS|_2 <= 4.2e-7 m.
    The sums themselves are exact integers.  |unit(S + dS) - unit(S)|_2 <= |dS| / |S| to first order, and |S| >= 0.5 m on these rows
    (tests/test_kmeans_host.py asserts the resultant; it is 0.78 at the least): 8.4e-7, plus the one f32 rounding of a component <= 1
    at the end (6e-8): 9e-7 <= 1e-6 for every component.  The norm itself is float64.  Errors do not pile up over the updates: a
    centroid is a function of the last labels alone, and those are equal."""
    res = found[(k, kind)]
    label, sim, cent, size, iterations, converged, picks = defined(k, kind)[0]
    err = float(np.abs(res.centroids.astype(np.float64) - cent.astype(np.float64)).max())
    print(f"\nk {k}, init {kind}: {res.iterations} updates, max |centroid - definition| = {err:.3e}, "
          f"max |sim - definition| = {np.nanmax(np.abs(res.sim.astype(np.float64) - sim)):.3e}")
    assert np.array_equal(res.label, label) and np.array_equal(res.size, size) and np.array_equal(res.init_rows, picks)
    assert res.iterations == iterations and res.converged == converged
    assert res.centroids.dtype == np.float32 and res.centroids.shape == (k, 512) and err <= 1e-6
    assert np.array_equal(np.isnan(res.sim), np.isnan(sim)) and np.nanmax(np.abs(res.sim.astype(np.float64) - sim)) <= 1e-5
    assert abs(res.objective - float(sim[label >= 0].astype(np.float64).sum())) <= 1e-5 * len(label)
    assert [t["size"] for t in res.table()] == list(size) and res.k == k


@pytest.mark.parametrize("k,kind", CASES)
def test_labels_and_similarities_are_those_neighbours_returns(engine, found, k, kind):
    engine.set_neighbour_split(0)
    assert is_neighbours(engine, planted()[0], found[(k, kind)])


def test_tied_centroids_go_to_the_smaller_index_and_an_empty_one_keeps_its_bytes(engine):
    r, family = planted()
    valid = np.flatnonzero(family >= 0)
    engine.set_neighbour_split(0)
    away = -unit64(r[valid]).sum(axis=0)                                   # negative to every row: nobody ever chooses it
    assert (unit64(r[valid]) @ (away / np.sqrt((away * away).sum()))).max() < -0.05
    init = np.concatenate([r[valid[:5]], r[valid[2:3]], away[None].astype(np.float32), r[valid[5:8]]])      # row 5 is a copy of row 2
    pure = engine.kmeans(r, 10, init, 0)                                   # max_iter = 0: the copy with the larger index is never chosen
    assert pure.iterations == 0 and not pure.converged and (pure.init_rows == -1).all()
    assert pure.size[5] == 0 and pure.size[6] == 0 and pure.size[2] >= 1 and not (pure.label == 5).any()
    assert np.array_equal(bits(pure.centroids[5]), bits(pure.centroids[2]))
    assert np.abs(pure.centroids.astype(np.float64) - unit64(init)).max() <= 1e-6
    assert is_neighbours(engine, r, pure)
    full = engine.kmeans(r, 10, init)
    assert full.iterations >= 1 and full.converged and is_neighbours(engine, r, full)
    assert full.size[6] == 0 and np.array_equal(bits(full.centroids[6]), bits(pure.centroids[6]))      # empty throughout: bit for bit
    assert full.size.sum() == len(valid)
    twins = r.copy()
    twins[valid[40:60]] = twins[valid[40]]                                 # twenty identical rows, and twin centroids after an update
    init = np.concatenate([twins[valid[40:42]], twins[valid[:6]]])
    res = engine.kmeans(twins, 8, init, 3)
    assert is_neighbours(engine, twins, res) and len(set(res.label[valid[40:60]])) == 1


@pytest.mark.parametrize("k", KS)
def test_results_do_not_depend_on_the_split_the_update_path_or_the_entry_point(engine, found, k):
    r, _ = planted()
    n = len(r)
    first = found[(k, "first")]
    init = init_rows("first", k)
    try:
        for split in SPLITS:
            engine.set_neighbour_split(split)
            assert identical(engine.kmeans(r, k, init), first), split
        engine.set_neighbour_split(100)
        assert identical(engine.kmeans(r, k), found[(k, "farthest")])
        engine.set_kmeans_lds(0)                                           # every sum straight to memory
        assert identical(engine.kmeans(r, k, init), first) and identical(engine.kmeans(r, k), found[(k, "farthest")])
        engine.set_kmeans_lds(128)
        bufs = [engine.alloc(r.nbytes), engine.alloc(init.nbytes), engine.alloc(8 * n), engine.alloc(4 * n), engine.alloc(2048 * k),
                engine.alloc(8 * k), engine.alloc(8 * k)]
        try:
            bufs[0].upload(r)
            bufs[1].upload(init)
            for ptr, want in ((bufs[1].ptr, first), (None, found[(k, "farthest")])):
                iterations, converged = engine.kmeans_dev(bufs[0].ptr, n, k, *(b.ptr for b in bufs[2:]), init_ptr=ptr)
                engine.sync()
                got = [b.download(s, t) for b, s, t in zip(bufs[2:], [(n,), (n,), (k, 512), (k,), (k,)],
                                                           [np.int64, np.float32, np.float32, np.int64, np.int64])]
                assert all(np.array_equal(bits(a), bits(getattr(want, f))) for a, f in zip(got, ARRAYS))
                assert (iterations, converged) == (want.iterations, want.converged)
        finally:
            for buf in bufs:
                buf.free()
    finally:
        engine.set_neighbour_split(0)
        engine.set_kmeans_lds(128)


@pytest.mark.parametrize("k", KS)
def test_centroids_are_bit_identical_under_a_permutation_of_the_rows(engine, found, k):
    """the test a float accumulation fails: the sums are integers, so no order of the rows - none of the adds - changes a bit"""
    r, _ = planted()
    first = found[(k, "first")]
    init = init_rows("first", k)
    engine.set_neighbour_split(0)
    for seed in (1, 2):
        perm = np.random.default_rng(seed).permutation(len(r))
        got = engine.kmeans(np.ascontiguousarray(r[perm]), k, init)
        assert np.array_equal(bits(got.centroids), bits(first.centroids)), seed
        assert np.array_equal(got.label, first.label[perm]) and np.array_equal(bits(got.sim), bits(first.sim[perm]))
        assert np.array_equal(got.size, first.size) and (got.iterations, got.converged) == (first.iterations, first.converged)


@pytest.mark.parametrize("k", (7, 33))
def test_signed_rows_never_land_on_a_padded_column_and_scales_change_no_label(engine, k):
    """every similarity to every centroid is negative: a padded column's zero fragment (similarity 0) would win wherever the kernel
    did not mask it"""
    r, plain, init = signed_rows(), signed_rows(scaled=False), signed_init(k)
    s = unit64(plain) @ unit64(init).T
    assert s.max() < -0.5
    try:
        for split in (0, 32):
            engine.set_neighbour_split(split)
            res = engine.kmeans(r, k, init, 0)
            assert res.label.min() >= 0 and res.label.max() < k and (res.sim < -0.5).all() and res.size.sum() == len(r)
            assert is_neighbours(engine, r, res)
            top = np.sort(s, axis=1)[:, -2:]
            sure = top[:, 1] - top[:, 0] >= 1e-4                           # where float64 can tell: the same centroid
            assert sure.sum() >= len(r) // 2 and np.array_equal(res.label[sure], s.argmax(axis=1)[sure])
            same = engine.kmeans(plain, k, init, 0)                        # row scales from 2^-100 to 2^100 change no label and no bit
            assert np.array_equal(same.label, res.label) and np.array_equal(bits(same.sim), bits(res.sim))
            moved = engine.kmeans(r, k, init, 2)                           # through two updates: still no padded column
            assert moved.label.min() >= 0 and moved.label.max() < k and is_neighbours(engine, r, moved)
    finally:
        engine.set_neighbour_split(0)


def test_farthest_first_replayed_from_the_values_neighbours_returns(engine):
    """the traversal's similarities are neighbours' for (row, the new centre alone as the base): replayed pick by pick in numpy, ties
    to the smaller row (planted duplicates tie exactly)"""
    r = rows(333, 31)
    r[200] = r[17]                                                         # duplicates: equal similarities to every centre
    r[150] = r[17] * 4
    r[90] = r[260]
    r[5] = 0
    r[0, 3] = np.inf                                                       # the first valid row is row 1
    valid = sequence.valid_rows(r)
    k = 12
    try:
        for split in (0, 32):
            engine.set_neighbour_split(split)
            picks, best = [int(np.flatnonzero(valid)[0])], None
            while len(picks) < k:
                sim = engine.neighbours(r, r[[picks[-1]]], 1)[1][:, 0]
                best = sim if best is None else np.maximum(best, sim)
                free = valid.copy()
                free[picks] = False
                cand = np.flatnonzero(free)
                picks.append(int(cand[np.argmin(best[cand])]))             # argmin: the first = the smaller row among equals
            res = engine.kmeans(r, k, None, 0)
            assert list(res.init_rows) == picks, split
            assert picks[0] == 1 and len(set(picks)) == k
            want = engine.centroids(r[picks], np.arange(k), k)[0]          # the centroids are the picks' unit rows
            assert np.array_equal(bits(res.centroids), bits(want)) and is_neighbours(engine, r, res)
        dup = np.repeat(rows(3, 2), 5, axis=0)                             # three directions, five copies each: every pick is a tie
        got = engine.kmeans(dup, 4, None, 0)
        assert got.init_rows[0] == 0 and sorted(got.init_rows[:3]) == [0, 5, 10]       # the first copy of each direction
        assert got.init_rows[3] in (1, 6, 11)                              # every row left is a copy of a centre: the first copy of one
    finally:
        engine.set_neighbour_split(0)


def test_edges_of_the_interface(engine):
    engine.set_neighbour_split(0)
    p, family = planted()
    valid = np.flatnonzero(family >= 0)
    one = engine.kmeans(p, 1)                                              # k = 1: one cluster of every valid row
    want = sequence.spherical_kmeans(p, 1)
    assert (one.label[valid] == 0).all() and list(one.size) == [331] and list(one.init_rows) == [valid[0]] and one.converged
    assert one.iterations == want[4] and np.abs(one.centroids.astype(np.float64) - want[2]).max() <= 1e-6 and is_neighbours(engine, p, one)
    every = engine.kmeans(p, 331, None, 2)                                 # k = the valid rows: every row is a centre
    assert sorted(every.init_rows) == list(valid) and (every.size == 1).all() and every.converged and every.iterations == 1
    assert (every.sim[valid] > 1 - 1e-5).all() and is_neighbours(engine, p, every)
    with pytest.raises(GnnError, match="gnn_kmeans: k 332 is more than the 331 valid rows of 333"):
        engine.kmeans(p, 332)
    with pytest.raises(GnnError, match="gnn_kmeans: k 1 is more than the 0 valid rows of 0"):
        engine.kmeans(p[:0], 1)                                            # n = 0: no k fits
    r = np.tile(rows(1, 4), (70, 1)) * np.exp2(np.arange(70) % 5)[:, None].astype(np.float32)
    r[1] = 0
    r[3, 100] = np.nan
    r[65, 511] = np.inf
    bad = np.isin(np.arange(70), [1, 3, 65])
    got = engine.kmeans(r, 2)
    assert (got.label[bad] == -1).all() and np.isnan(got.sim[bad]).all() and (got.label[~bad] == 0).all() and list(got.size) == [67, 0]
    assert list(got.init_rows) == [0, 2] and np.array_equal(bits(got.centroids[0]), bits(got.centroids[1]))
    with pytest.raises(GnnError, match="k 68 is more than the 67 valid rows of 70"):
        engine.kmeans(r, 68)
    with pytest.raises(ValueError, match="1 of the 2 init rows are not valid"):
        engine.kmeans(r, 2, r[[0, 1]])
    bufs = [engine.alloc(r.nbytes), engine.alloc(8 * 70), engine.alloc(4 * 70), engine.alloc(2048 * 2), engine.alloc(16), engine.alloc(16)]
    try:
        bufs[0].upload(r)
        with pytest.raises(GnnError, match="gnn_kmeans_dev: 1 of the 2 init rows are not valid"):      # rows 0 and 1 of r as the init
            engine.kmeans_dev(bufs[0].ptr, 70, 2, *(b.ptr for b in bufs[1:]), init_ptr=bufs[0].ptr)
    finally:
        for buf in bufs:
            buf.free()
    zero = np.zeros((2, 512), np.float32)
    zero[0, :3], zero[1, :3] = (1, 2, 2), (-1, -2, -2)
    init1 = np.zeros((1, 512), np.float32)
    init1[0, :5] = (1, 2, 3, 4, 5)
    res = engine.kmeans(zero, 1, init1)                                    # one cluster of x and -x: the sum is exactly zero
    kept = engine.kmeans(zero, 1, init1, 0)
    assert list(res.label) == [0, 0] and list(res.size) == [2] and res.converged and res.iterations == 1
    assert np.array_equal(bits(res.centroids), bits(kept.centroids)) and np.abs(kept.centroids[0, :5] * np.sqrt(55) - (1, 2, 3, 4, 5)).max() < 1e-5
    big = rows(16454, 6)                                                   # one row tile beyond the neighbour search's slab of 16384
    res = engine.kmeans(big, 300, big[:300], 1)
    assert res.iterations == 1 and res.size.sum() == 16454 and is_neighbours(engine, big, res)
    small = engine.kmeans(p, 7)                                            # a small call after a large one: the buffers are reused
    assert identical(small, engine.kmeans(p, 7)) and np.array_equal(small.label, defined(7)[0][0])
    for bad_k, bad_it in ((0, 5), (65536, 5)):
        with pytest.raises(ValueError, match=r"k .*\[1, 65535\]"):
            engine.kmeans(p, bad_k, None, bad_it)
    with pytest.raises(ValueError, match=r"max_iter .*\[0, 1000\]"):
        engine.kmeans(p, 2, None, 1001)
    with pytest.raises(GnnError, match=r"gnn_kmeans_dev: k 0 is outside \[1, 65535\]"):
        engine.kmeans_dev(0, 4, 0, 0, 0, 0, 0, 0)
    with pytest.raises(GnnError, match="bad argument to gnn_kmeans_dev"):
        engine.kmeans_dev(0, 4, 2, 0, 0, 0, 0, 0)


def test_centroids_of_the_clusters_of_cluster(engine):
    r, family = planted()
    engine.set_neighbour_split(0)
    c = engine.cluster(r, 0.45)
    roots = np.unique(c.label[c.label >= 0])
    k = len(roots)
    label = np.where(c.label >= 0, np.searchsorted(roots, c.label), -1)    # relabelled to 0 .. k - 1
    assert 5 <= k <= 200
    cent, size = engine.centroids(r, label, k + 2)                         # two groups without members
    want, want_size = sequence.group_centroids(r, label, k + 2)
    err = float(np.abs(cent.astype(np.float64) - want).max())
    print(f"\ncentroids of {k} clusters: max |device - definition| = {err:.3e}")
    assert np.array_equal(size, want_size) and err <= 1e-6 and (cent[k:] == 0).all() and list(size[k:]) == [0, 0]
    assert np.array_equal(size[:k], np.bincount(label[label >= 0], minlength=k))
    try:
        for seed, lds in ((1, 16), (2, 0)):
            engine.set_kmeans_lds(lds)
            perm = np.random.default_rng(seed).permutation(len(r))
            c2, s2 = engine.centroids(np.ascontiguousarray(r[perm]), label[perm], k + 2)
            assert np.array_equal(bits(c2), bits(cent)) and np.array_equal(s2, size), seed
        few = np.where(label >= 0, label % 3, -1)                          # three groups: the LDS path, and straight to memory
        a = engine.centroids(r, few, 3)
        engine.set_kmeans_lds(128)
        b = engine.centroids(r, few, 3)
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])
        # groups that mix families have a shorter resultant: the bound of test_planted_rows_equal_the_definition with it in place of 0.5
        assert np.abs(a[0].astype(np.float64) - sequence.group_centroids(r, few, 3)[0]).max() <= 4.2e-7 / resultant(r, few, 3).min() + 6e-8
    finally:
        engine.set_kmeans_lds(128)
    for bad in (k + 2, -2):
        wrong = label.copy()
        wrong[100] = bad
        bufs = [engine.alloc(r.nbytes), engine.alloc(8 * len(r)), engine.alloc(2048 * (k + 2)), engine.alloc(8 * (k + 2))]
        try:
            bufs[0].upload(r)
            bufs[1].upload(wrong)
            marker = np.full((k + 2, 512), 7, np.float32)
            bufs[2].upload(marker)
            bufs[3].upload(np.full(k + 2, 7, np.int64))
            with pytest.raises(GnnError, match=rf"gnn_centroids_dev: a label is outside \[-1, {k + 2}\)"):
                engine.centroids_dev(bufs[0].ptr, len(r), bufs[1].ptr, k + 2, bufs[2].ptr, bufs[3].ptr)
            engine.sync()
            assert (bufs[2].download((k + 2, 512), np.float32) == 7).all() and (bufs[3].download((k + 2,), np.int64) == 7).all()
        finally:
            for buf in bufs:
                buf.free()
        with pytest.raises(GnnError, match="gnn_centroids: a label is outside"):
            engine.centroids(r, wrong, k + 2)
    cent, size = engine.centroids(r[:0], np.zeros(0, np.int64), 3)
    assert (cent == 0).all() and list(size) == [0, 0, 0]


def test_embed_contigs_to_kmeans_end_to_end(engine):
    rng = np.random.default_rng(5)
    windows = synthetic.synth_windows(900, 30)
    contigs = [windows[a:a + n].reshape(-1)[:int(rng.integers((n - 1) * 6000 + 3000, n * 6000 + 1))]
               for a, n in zip(range(0, 24, 2), [1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 2])]
    contigs[9] = contigs[4].copy()                            # byte-identical to contig 4
    contigs[11] = contigs[4].copy()
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in contigs])]).astype(np.int64)
    seq = np.concatenate(contigs)
    engine.set_neighbour_split(0)
    before, _ = engine.classify_contigs(seq, offsets)
    _, emb, _ = engine.embed_contigs(seq, offsets)
    idx0, sim0 = engine.neighbours(emb, None, 3)
    res = engine.kmeans(emb, 4)
    idx1, sim1 = engine.neighbours(emb, None, 3)              # the searches share the fragment buffers
    after, _ = engine.classify_contigs(seq, offsets)
    assert len(set(res.label[[4, 9, 11]])) == 1 and res.size.sum() == 12 and (res.label >= 0).all() and is_neighbours(engine, emb, res)
    assert np.abs((res.centroids.astype(np.float64) ** 2).sum(axis=1) - 1).max() <= 1e-6
    assert [t["cluster"] for t in res.table()] == [0, 1, 2, 3] and res.table(list("abcdefghijkl"))[0]["nearest"] in "abcdefghijkl"
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    assert np.array_equal(idx0, idx1) and np.array_equal(sim0.view(np.uint32), sim1.view(np.uint32))
