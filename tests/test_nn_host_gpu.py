"""The host side the analyses over encoder embeddings share (genomad_amd/csrc/gnn_nn_host.h) on the MI355X: every ``*_ms`` accessor
reports exactly the passes its documented sequence names, a pass log never reads an event that went back to the pool, a landing
buffer that grows and shrinks copies out the call's own slices only.  200 rows are four 64-row tiles, the last ragged; ranges of 64
base rows make four ranges; k = 3, two classes."""
import contextlib

import numpy as np
import pytest

from genomad_amd import _lib, sequence

pytestmark = pytest.mark.gpu

N, K, CLASSES, T = 200, 3, 2, 0.5
FIELDS = ("label", "degree", "size", "anchor", "sim", "kind")


def family_rows(n=N, seed=5):
    """n valid rows in five loose families: a pair inside a family has a cosine near 0.8, a pair across families near 0 - none
    within 0.1 of T, so the float64 definition and the device decide every pair alike"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((5, 512))
    return np.ascontiguousarray(centres[np.arange(n) % 5] + 0.5 * rng.standard_normal((n, 512)), dtype=np.float32)


def blurred_rows():
    """the families under four times their noise, for k-means from three rows of ONE family: the float64 definition
    (sequence.spherical_kmeans) needs five updates to settle, so two updates leave it unconverged with room to spare"""
    noise = np.random.default_rng(6).standard_normal((N, 512))
    return np.ascontiguousarray(family_rows() + 2.0 * noise, dtype=np.float32)


@contextlib.contextmanager
def on_device(engine, *arrays):
    """device buffers: an array is uploaded, an int is that many bytes"""
    bufs = []
    try:
        for a in arrays:
            bufs.append(engine.alloc(a if isinstance(a, int) else a.nbytes))
            if not isinstance(a, int):
                bufs[-1].upload(a)
        yield bufs
    finally:
        for b in bufs:
            b.free()


@contextlib.contextmanager
def profiling(engine, on=True):
    engine.set_neighbour_split(64)
    engine.profile_enable(on)
    try:
        yield
    finally:
        engine.profile_enable(False)
        engine.set_neighbour_split(0)


def run_all(engine):
    """every analysis with a pass log once, on the host entry points -> {accessor name: (entries its sequence implies, the entries)}"""
    r, blurred = family_rows(), blurred_rows()
    label = (np.arange(N) % CLASSES).astype(np.int64)
    out = {}
    km = engine.kmeans(blurred, K, init=blurred[[0, 5, 10]], max_iter=2)
    assert km.iterations == 2 and not km.converged                              # 1 + 3 assignments, 2 x 3 other passes
    out["kmeans_pass_ms"] = (1 + (km.iterations + 1) + 3 * km.iterations, engine.kmeans_pass_ms())
    engine.vote(r, None, label, CLASSES, T)
    out["vote_pass_ms"] = (3, engine.vote_pass_ms())                            # labels; one slab: votes, finish
    g = engine.graph(r, T)
    out["graph_pass_ms"] = (2, engine.graph_pass_ms())
    engine.match(r[:70], r, T)
    out["match_pass_ms"] = (2, engine.match_pass_ms())
    engine.pca_moments(r)
    out["pca_pass_ms moments"] = (4, engine.pca_pass_ms())
    engine.project(r, r[:K])
    out["pca_pass_ms project"] = (3, engine.pca_pass_ms())
    out["representative_round_ms"] = (engine.representatives(r, T).rounds, engine.representative_round_ms())
    # every row is valid and every pair has a value: the tree is spanning, and the loop leaves behind the round that completes it
    out["linkage_round_ms"] = (engine.linkage(r).rounds, engine.linkage_round_ms())
    out["density_tree_round_ms"] = (engine.density_tree(r, 3).rounds, engine.density_tree_round_ms())
    m = engine.mcl(g.indptr, g.col, g.sim, max_iter=5)
    out["mcl_pass_ms"] = (2 + m.iterations, engine.mcl_pass_ms())
    return out


def test_every_accessor_reports_its_documented_passes(engine):
    """profiling on: the number of entries is what the sequence in the accessor's docstring implies for the call just made - k-means
    [init, then per assignment: assign, and behind every assignment but the last: update, finish, prepare], votes [labels, then per
    slab: votes, finish], graph and match [count pass, scan], PCA moments [prepare, sums, gram, mirror], PCA project [prepare rows,
    prepare components, project], MCL [validate + symmetrise, initial matrix, then every iteration], the others one per round -
    and every entry is a finite time >= 0.  Profiling off: every accessor is empty."""
    with profiling(engine):
        got = run_all(engine)
    assert got["representative_round_ms"][0] >= 1 and got["linkage_round_ms"][0] >= 1 and got["mcl_pass_ms"][0] >= 3
    for name, (want, ms) in got.items():
        assert ms.dtype == np.float64 and len(ms) == want, (name, want, ms)
        assert np.isfinite(ms).all() and (ms >= 0).all(), (name, ms)
    with profiling(engine, False):
        for name, (_, ms) in run_all(engine).items():
            assert len(ms) == 0, (name, ms)


def test_a_pass_log_reads_no_event_that_went_back_to_the_pool(engine):
    """vote_dev leaves its last slab's passes pending; profile_get then drains the profile, which returns every event to the pool,
    and the next profiled call records them again.  The log must have read its times before that: vote_pass_ms still has its 3
    entries, none negative (a re-recorded pair comes out of the LIFO pool in swapped order, so its elapsed time is negative, or the
    read fails and the entry is gone).  The same with pca project as the first call and the votes as the intruder.  The sign and the
    count are what this can see: it does not prove that a value is the pass's own time."""
    r = family_rows()
    label = (np.arange(N) % CLASSES).astype(np.int64)
    cells = N * CLASSES
    with on_device(engine, r, label, cells * 8, cells * 8, cells * 8, cells * 4, 512 * 512 * 8, 512 * 8, 8, N * K * 4) as b:
        rows, lab, cnt, wgt, near, nsim, G, S, nv, proj = (x.ptr for x in b)

        def vote():
            engine.vote_dev(rows, N, None, 0, lab, CLASSES, T, cnt, wgt, near, nsim)

        def moments():
            engine.pca_moments_dev(rows, N, G, S, nv)

        def project():
            engine.project_dev(rows, N, rows, K, proj)

        for first, intruder, read, entries in ((vote, moments, engine.vote_pass_ms, 3), (project, vote, engine.pca_pass_ms, 3)):
            with profiling(engine):
                first()
                engine.profile_get(_lib.K_NEIGHBOURS)
                intruder()
                engine.profile_get(_lib.K_NEIGHBOURS)
                ms = read()
            assert len(ms) == entries and np.isfinite(ms).all() and (ms >= 0).all(), (first.__name__, ms)
        engine.sync()


def test_density_lands_right_after_growing_and_shrinking(engine):
    """n = 70, 200, 70 on one engine: the landing buffer grows for the second call (freed first) and is larger than the third
    needs, whose slices lie elsewhere in it - every call returns the definition's arrays, nothing of an earlier call"""
    rows = family_rows()
    for n in (70, 200, 70):
        r = np.ascontiguousarray(rows[:n])
        got = engine.density(r, T, 3)
        want = dict(zip(FIELDS, sequence.density_clusters(r, T, 3)))
        for f in FIELDS:
            a, b = getattr(got, f), want[f]
            assert a.shape == b.shape, (n, f)
            if f == "sim":                                    # f32 against float64: NaN where the definition has it, 1e-5 elsewhere
                assert np.array_equal(np.isnan(a), np.isnan(b)) and (np.abs(a.astype(np.float64) - b)[~np.isnan(b)] <= 1e-5).all(), n
            else:
                assert np.array_equal(a, b), (n, f)


def test_centroids_host_and_device_entry_points_agree(engine):
    """gnn_centroids uploads the labels into a slice of its landing buffer and copies two slices out: the same arrays, bit for bit,
    as gnn_centroids_dev on the same rows and labels"""
    r = family_rows()
    label = (np.arange(N) % K).astype(np.int64)
    label[::17] = -1
    cent, size = engine.centroids(r, label, K)
    with on_device(engine, r, label, K * 512 * 4, K * 8) as b:
        engine.centroids_dev(b[0].ptr, N, b[1].ptr, K, b[2].ptr, b[3].ptr)
        engine.sync()
        assert np.array_equal(b[2].download((K, 512), np.float32).view(np.uint32), np.asarray(cent).view(np.uint32))
        assert np.array_equal(b[3].download(K, np.int64), size)
