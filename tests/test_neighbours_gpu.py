"""Nearest neighbours among encoder embeddings on the MI355X: the values against the fp64 cosine of the returned pairs, the sets and
the order against the numpy definition (sequence.nearest_neighbours), bit-exact integer dots, independence of how the base is split
over workgroups, the edges, and embed_contigs -> neighbours end to end.  Sizes are off every tile boundary: 70 queries (one 64-row tile
and 6 rows), 333 base rows (ten 32-row blocks and 13 rows; one 256-column step and 77 columns).

Measured on an MI355X (profiles/neighbours/README.md): max |sim - fp64 sim of the returned pair| 1.2e-7 .. 3.4e-7 against the bound of
1e-5; 100 % of the rows qualify for the exact-order check at k = 1, 97.1 % / 96.4 % at k = 10."""
import numpy as np
import pytest

from genomad_amd import sequence, synthetic
from genomad_amd._lib import GnnError
from tests.neighbours_data import rows, sims64

pytestmark = pytest.mark.gpu

VALUE_TOL = 1e-5        # ten times the emulated 9.3e-7 of the three-product form: the margin is for the matrix pipe's summation order
GAP = 2e-5              # fp64 similarities closer than this may legitimately swap
KS = (1, 10, 64)


@pytest.fixture(scope="module")
def data():
    """the inputs of every test here and their fp64 similarities, computed once: (70 x 333) and the self-search on the 333 rows"""
    query, base = rows(70, 7), rows(333, 8)
    s_self = sims64(base, base)
    np.fill_diagonal(s_self, -np.inf)                        # the pair (i, i) is no candidate
    return {"query": query, "base": base, "cases": {"pairs": (query, base, sims64(query, base)), "self": (base, None, s_self)}}


@pytest.fixture(scope="module")
def found(engine, data):
    """the device's answer for every case and k, computed once with the library's own split"""
    engine.set_neighbour_split(0)
    return {(name, k): engine.neighbours(q, b, k) for name, (q, b, _) in data["cases"].items() for k in KS}


@pytest.mark.parametrize("case", ["pairs", "self"])
@pytest.mark.parametrize("k", KS)
def test_similarities_are_the_fp64_cosine_of_the_returned_pairs(data, found, case, k):
    q, b, s64 = data["cases"][case]
    idx, sim = found[case, k]
    assert idx.dtype == np.int64 and sim.dtype == np.float32 and idx.shape == sim.shape == (len(q), k)
    assert (idx >= 0).all() and (idx < s64.shape[1]).all()
    assert all(len(set(r)) == k for r in idx)                # no base row twice
    if case == "self":
        assert (idx != np.arange(len(q))[:, None]).all()
    err = np.abs(sim.astype(np.float64) - np.take_along_axis(s64, idx, axis=1)).max()
    print(f"\nneighbours {case} k={k}: max |sim - fp64 sim of the returned pair| = {err:.3e}")
    assert err <= VALUE_TOL
    assert (np.diff(sim, axis=1) <= 0).all()                 # ordered on the device's own values


@pytest.mark.parametrize("case", ["pairs", "self"])
@pytest.mark.parametrize("k", KS)
def test_no_row_is_left_out_and_none_is_let_in(data, found, case, k):
    _, _, s64 = data["cases"][case]
    idx, _ = found[case, k]
    kth = -np.sort(-s64, axis=1)[:, k - 1]
    assert (np.take_along_axis(s64, idx, axis=1) >= kth[:, None] - GAP).all()
    returned = np.zeros(s64.shape, bool)
    np.put_along_axis(returned, idx, True, axis=1)
    assert returned[s64 > kth[:, None] + GAP].all()


@pytest.mark.parametrize("case", ["pairs", "self"])
@pytest.mark.parametrize("k", [1, 10])
def test_order_is_the_definitions_where_the_gaps_allow(data, found, case, k):
    q, b, s64 = data["cases"][case]
    idx, _ = found[case, k]
    ref_idx, _ = sequence.nearest_neighbours(q, b, k)
    top = -np.sort(-s64, axis=1)[:, :k + 1]
    qualifies = (-np.diff(top, axis=1) > GAP).all(axis=1)
    print(f"\nneighbours {case} k={k}: {qualifies.mean():.1%} of the rows have every top-{k + 1} gap above {GAP:g}")
    assert qualifies.mean() >= 0.9
    assert np.array_equal(idx[qualifies], ref_idx[qualifies])


@pytest.mark.parametrize("k", [1, 7, 64])
def test_integer_dots_are_bit_exact_and_ties_go_to_the_lower_index(engine, k):
    rng = np.random.default_rng(11)
    base = rng.integers(0, 8, (200, 512)).astype(np.float32)          # every dot is an integer below 512 * 49 < 2^24
    base[40:60] = base[10]                                             # duplicates: ties across and within 32-row blocks
    base[150] = base[3]
    base[199] = base[3]
    query = np.concatenate([base[[10, 3, 199]], rng.integers(0, 8, (67, 512)).astype(np.float32)])
    engine.set_neighbour_split(0)
    for q, b in ((query, base), (base, None)):
        for split in (0, 32):
            engine.set_neighbour_split(split)
            idx, sim = engine.neighbours(q, b, k, "dot")
            want_idx, want_sim = sequence.nearest_neighbours(q, b, k, "dot")
            assert np.array_equal(idx, want_idx), split
            assert np.array_equal(sim.view(np.uint32), want_sim.view(np.uint32)), split
    engine.set_neighbour_split(0)


@pytest.mark.parametrize("k", KS)
def test_results_do_not_depend_on_the_split_and_the_device_path_agrees(engine, data, found, k):
    try:
        for case, (q, b, _) in data["cases"].items():
            idx0, sim0 = found[case, k]
            for split in (32, 100, 333, 4096):
                engine.set_neighbour_split(split)
                idx, sim = engine.neighbours(q, b, k)
                assert np.array_equal(idx, idx0) and np.array_equal(sim.view(np.uint32), sim0.view(np.uint32)), (case, split)
            engine.set_neighbour_split(100)
            bufs = [engine.alloc(q.nbytes), engine.alloc(b.nbytes) if b is not None else None, engine.alloc(idx0.nbytes),
                    engine.alloc(sim0.nbytes)]
            try:
                bufs[0].upload(q)
                if b is not None:
                    bufs[1].upload(b)
                engine.neighbours_dev(bufs[0].ptr, len(q), bufs[1].ptr if b is not None else None, 0 if b is None else len(b),
                                      bufs[2].ptr, bufs[3].ptr, k)
                engine.sync()
                assert np.array_equal(bufs[2].download(idx0.shape, np.int64), idx0), case
                assert np.array_equal(bufs[3].download(sim0.shape, np.float32).view(np.uint32), sim0.view(np.uint32)), case
            finally:
                for buf in bufs:
                    if buf is not None:
                        buf.free()
    finally:
        engine.set_neighbour_split(0)


def test_edges(engine, data):
    engine.set_neighbour_split(0)
    q, b = data["query"][:9].copy(), data["base"][:40].copy()
    q[1] = 0
    q[2, 17] = np.nan
    q[3, 500] = np.inf
    b[0] = 0
    b[5, 0] = np.nan
    b[33, 511] = -np.inf
    for metric in ("cosine", "dot"):
        for k in (3, 64):                                     # 64 > the 37 valid base rows: padded
            idx, sim = engine.neighbours(q, b, k, metric)
            want_idx, want_sim = sequence.nearest_neighbours(q, b, k, metric)
            assert np.array_equal(idx < 0, want_idx < 0) and np.array_equal(np.isnan(sim), idx < 0), (metric, k)
            assert not np.isin(idx, [5, 33]).any() and ((idx != 0).all() or metric == "dot")
            assert (idx[2] == -1).all() and (idx[3] == -1).all() and ((idx[1] == -1).all() or metric == "dot")
            if k == 64:                                       # every candidate is returned: the sets and the values are the definition's
                assert np.array_equal(np.sort(idx, axis=1), np.sort(want_idx, axis=1)), metric
                assert np.allclose(np.sort(sim, axis=1), np.sort(want_sim, axis=1), rtol=VALUE_TOL, atol=VALUE_TOL, equal_nan=True), metric
        idx, sim = engine.neighbours(b, None, 64, metric)     # the same rows among themselves
        want_idx, _ = sequence.nearest_neighbours(b, None, 64, metric)
        assert np.array_equal(np.sort(idx, axis=1), np.sort(want_idx, axis=1)) and (idx != np.arange(40)[:, None]).all()
    idx, sim = engine.neighbours(data["base"][:1], None, 5)
    assert idx.shape == (1, 5) and (idx == -1).all() and np.isnan(sim).all()          # one row: nobody is left
    idx, sim = engine.neighbours(q, b[:0], 5)
    assert idx.shape == (9, 5) and (idx == -1).all() and np.isnan(sim).all()          # no base row
    idx, sim = engine.neighbours(data["query"], data["base"][:7], 10)                   # fewer base rows than k
    assert (idx[:, :7] >= 0).all() and (idx[:, 7:] == -1).all() and np.isnan(sim[:, 7:]).all()
    assert np.array_equal(np.sort(idx[:, :7], axis=1), np.tile(np.arange(7), (70, 1)))
    idx, sim = engine.neighbours(q[:0], b, 5)
    assert idx.shape == sim.shape == (0, 5)
    with pytest.raises(GnnError, match=r"k 65 is outside \[1, 64\]"):
        engine.neighbours(q, b, 65)
    with pytest.raises(GnnError, match=r"k 0 is outside \[1, 64\]"):
        engine.neighbours(q, b, 0)
    with pytest.raises(GnnError, match=r"metric 9 is outside \[0, 1\]"):
        engine.neighbours(q, b, 5, 9)


def test_embed_contigs_to_neighbours_end_to_end(engine):
    rng = np.random.default_rng(5)
    windows = synthetic.synth_windows(900, 30)
    contigs = [windows[a:a + n].reshape(-1)[:int(rng.integers((n - 1) * 6000 + 3000, n * 6000 + 1))]
               for a, n in zip(range(0, 24, 2), [1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 2])]
    contigs[9] = contigs[4].copy()                            # byte-identical to contig 4
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in contigs])]).astype(np.int64)
    seq = np.concatenate(contigs)
    before, _ = engine.classify_contigs(seq, offsets)
    _, emb, _ = engine.embed_contigs(seq, offsets)
    idx, sim = engine.neighbours(emb, None, 3)
    after, _ = engine.classify_contigs(seq, offsets)
    assert idx[4, 0] == 9 and idx[9, 0] == 4
    assert abs(float(sim[4, 0]) - 1) <= 1e-5 and abs(float(sim[9, 0]) - 1) <= 1e-5
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    s64 = sims64(emb, emb)
    np.fill_diagonal(s64, -np.inf)
    assert np.abs(sim - np.take_along_axis(s64, idx, axis=1)).max() <= VALUE_TOL
