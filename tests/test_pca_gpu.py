"""Principal components among encoder embeddings on the MI355X.  Moments: rows whose products and partial sums are exact in f32 against
the integer definition QT Q >> 32 and sum q, exactly, at sizes around the 256-row granule; bit-identity under the row split; planted
h1-like rows against float64 within a derived bound; invalid rows at granule and range borders; row scales; the host and the device
entry points.  Projection: project(rows, components) IS neighbours(rows, components, k = ncomp) scattered by index, bit for bit;
with a mean one f32 subtraction of that; NaN rows; a canary column.  End to end: pca() on a planted spectrum within Weyl's and
Davis-Kahan's bounds computed from the device's own moments."""
import numpy as np
import pytest

from genomad_amd import sequence
from genomad_amd._lib import GnnError
from tests.pca_data import (EXACT_NS, SPECTRUM_RANK, exact_moments, exact_rows, planted_rows, spectrum_rows, subspace_residual,
                            with_invalid)

pytestmark = pytest.mark.gpu

NCOMPS = (1, 2, 32, 33, 64)                      # below a 32-column block, at it, across it, both blocks full
NS = (1, 63, 64, 65, 300)                        # below a 64-row tile, at it, one beyond, five tiles off the boundary


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("n", EXACT_NS)
def test_exact_rows_equal_the_integer_definition(engine, n):
    engine.set_pca_split(0)
    r = exact_rows(n)
    G, S, n_valid = engine.pca_moments_fixed(r)
    wG, wS = exact_moments(r)
    assert G.dtype == np.int64 and S.dtype == np.int64 and n_valid == n
    assert np.array_equal(S, wS) and np.array_equal(G, wG)
    Gf, Sf, _ = engine.pca_moments(r)
    assert np.array_equal(Gf, wG / 2.0 ** 32) and np.array_equal(Sf, wS / 2.0 ** 32)


def test_no_bit_depends_on_the_row_split(engine):
    r = planted_rows()
    r = np.concatenate([r, r[:300] * np.float32(3)])[:1000]
    try:
        engine.set_pca_split(0)
        first = engine.pca_moments_fixed(r)
        assert np.array_equal(first[0], first[0].T) and first[2] == 1000
        for split in (256, 512, 768):                      # 4, 2 and 2 ranges (768 + 232 rows)
            engine.set_pca_split(split)
            assert same(engine.pca_moments_fixed(r), first), split
        for bad in (1, 255, 300, -256):
            with pytest.raises(GnnError, match="not a multiple of 256"):
                engine.set_pca_split(bad)
    finally:
        engine.set_pca_split(0)


def test_planted_rows_against_float64(engine):
    """The bound, derived.  The device's entry is sum_i x_ia x_ib with x the fragments' image of 2^8 u: |x - 2^8 u| <= 4.2e-7 |2^8 u|
    per element (the norm's sum, its square root and the division round once each, 3 x 2^-24; the low limb rounds a remainder below
    2^-11 of the element to f16, 2^-22: tests/test_kmeans_gpu.py), so a product is within 8.4e-7 <= 2^-20 of |u_a u_b|.  A chain of
    256 fused multiply-adds rounds 256 times, each by at most 2^-24 of a partial sum that is at most the sum of the |products|: 256 x
    2^-24 of it.  The conversion to an integer rounds by half a unit of 2^-32 per granule, 2^-33 n / 256 in all, below 2^-32 n.  Over
    n: |G / 2^32 / n - C64| <= (256 x 2^-24 + 2^-20) A_ab + 2^-32 with A = mean_i |u_ia| |u_ib|."""
    engine.set_pca_split(0)
    r = planted_rows()
    n = len(r)
    G, S, n_valid = engine.pca_moments(r)
    G64, S64, _ = sequence.pca_moments(r)
    u = r.astype(np.float64)
    u /= np.sqrt((u * u).sum(axis=1))[:, None]
    A = np.abs(u).T @ np.abs(u) / n
    bound = (256 * 2.0 ** -24 + 2.0 ** -20) * A + 2.0 ** -32
    err = np.abs(G / n - G64 / n)
    print(f"\nplanted rows, n {n}: max |G / n - float64| = {err.max():.3e} at max |C| = {np.abs(G64 / n).max():.3e}, "
          f"max err / bound = {(err / bound).max():.3f}, max |S / n - float64| = {np.abs(S - S64).max() / n:.3e}")
    assert n_valid == n and (err <= bound).all()
    assert np.abs(S - S64).max() / n <= 4.2e-7 * np.abs(u).max()


def test_invalid_rows_change_no_bit(engine):
    engine.set_pca_split(256)                              # ranges end where granules do: 255, 256 and 511, 512 are borders of both
    try:
        base = planted_rows()[:600]
        clean = engine.pca_moments_fixed(base)
        where = (0, 255, 256, 300, 511, 512, 606)          # the last row of the result is invalid
        r, keep = with_invalid(base, where)
        assert len(r) == 607 and not keep[-1]
        # the valid rows keep their order but not their granules: compare with the same rows in the same places, zeros between them
        zeroed = np.where(keep[:, None], r, np.float32(0))
        got, want = engine.pca_moments_fixed(r), engine.pca_moments_fixed(zeroed)
        assert same(got, want) and got[2] == 600 == clean[2]
        assert np.array_equal(got[1], clean[1])            # S is exact: where the rows stand changes nothing
        tail, _ = with_invalid(base, (600,))               # the same rows in the same places, one invalid row behind them
        assert same(engine.pca_moments_fixed(tail), clean)
        # a whole granule of invalid rows between the first granule and the rest: every valid row keeps its place in its granule
        hole, _ = with_invalid(base[:0], range(256))
        assert same(engine.pca_moments_fixed(np.concatenate([base[:256], hole, base[256:]])), clean)
        engine.set_pca_split(0)
        assert same(engine.pca_moments_fixed(r), got)
    finally:
        engine.set_pca_split(0)


def test_row_scales_change_no_bit_and_the_mean_is_the_centroid(engine):
    engine.set_pca_split(0)
    r = planted_rows()[:300]
    first = engine.pca_moments_fixed(r)
    scale = np.exp2(np.random.default_rng(8).integers(-100, 101, (300, 1))).astype(np.float32)
    assert same(engine.pca_moments_fixed(r * scale), first)
    cent, size = engine.centroids(r, np.zeros(300, np.int64), 1)
    s = first[1].astype(np.float64)
    assert size[0] == 300 and np.abs(s / np.sqrt((s * s).sum()) - cent[0]).max() <= 1e-6


def test_host_and_device_entry_points_agree(engine):
    engine.set_pca_split(0)
    r = planted_rows()[:513]
    n = len(r)
    host = engine.pca_moments_fixed(r)
    comp = np.ascontiguousarray(planted_rows()[600:633])
    off = np.linspace(-0.5, 0.5, 33).astype(np.float32)
    bufs = [engine.alloc(r.nbytes), engine.alloc(8 * 512 * 512), engine.alloc(8 * 512), engine.alloc(8), engine.alloc(comp.nbytes),
            engine.alloc(off.nbytes), engine.alloc(4 * n * 33)]
    try:
        bufs[0].upload(r)
        engine.pca_moments_dev(bufs[0].ptr, n, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr)
        engine.sync()
        got = (bufs[1].download((512, 512), np.int64), bufs[2].download((512,), np.int64), int(bufs[3].download((1,), np.int64)[0]))
        assert same(got, host)
        bufs[4].upload(comp)
        bufs[5].upload(off)
        for mean_ptr in (None, bufs[5].ptr):
            engine.project_dev(bufs[0].ptr, n, bufs[4].ptr, 33, bufs[6].ptr, mean_ptr)
            engine.sync()
            p = bufs[6].download((n, 33), np.float32)
            raw = engine.project(r, comp)
            assert np.array_equal(bits(p), bits(raw if mean_ptr is None else raw - off[None, :]))
    finally:
        for b in bufs:
            b.free()


@pytest.fixture(scope="module")
def searched(engine):
    """neighbours(rows, components, k) on 300 rows (two of them invalid) and 64 components, scattered by index: computed once"""
    engine.set_neighbour_split(0)
    r, keep = with_invalid(planted_rows()[:298], (64, 299))
    comp = np.ascontiguousarray(planted_rows()[300:364] * np.exp2(np.arange(64) - 32).astype(np.float32)[:, None])
    out = {}
    for c in NCOMPS:
        idx, sim = engine.neighbours(r, comp[:c], c)
        s = np.full((300, c), np.nan, np.float32)
        for i in np.flatnonzero(keep):
            assert sorted(idx[i]) == list(range(c))
            s[i, idx[i]] = sim[i]
        s.setflags(write=False)
        out[c] = s
    return r, keep, comp, out


@pytest.mark.parametrize("ncomp", NCOMPS)
def test_raw_projection_is_the_neighbour_search_bit_for_bit(engine, searched, ncomp):
    r, keep, comp, want = searched
    for n in NS:
        got = engine.project(r[:n], comp[:ncomp])
        assert got.shape == (n, ncomp) and got.dtype == np.float32
        assert np.array_equal(bits(got), bits(want[ncomp][:n])), n


@pytest.mark.parametrize("ncomp", NCOMPS)
def test_projection_with_a_mean_is_one_subtraction_and_writes_no_other_column(engine, searched, ncomp):
    r, keep, comp, want = searched
    n = 300
    mean = sequence.pca_moments(r)[1] / keep.sum()
    off64 = sequence.pca_offsets(comp[:ncomp], mean)
    off = off64.astype(np.float32)
    got = engine.project(r, comp[:ncomp], mean)
    assert np.array_equal(bits(got), bits(want[ncomp] - off[None, :]))
    assert np.isnan(got[~keep]).all() and not np.isnan(got[keep]).any()
    ref = sequence.pca_project(r, comp[:ncomp], mean)
    err = np.nanmax(np.abs(got - ref))
    print(f"\nncomp {ncomp}: max |project - float64| = {err:.3e}")
    assert err <= 1e-5
    # the device entry point into a buffer one column wider than the output: [n * ncomp values | a canary of n values]
    bufs = [engine.alloc(r.nbytes), engine.alloc(4 * 512 * ncomp), engine.alloc(4 * ncomp), engine.alloc(4 * n * (ncomp + 1))]
    try:
        canary = np.full(n * (ncomp + 1), -7.5, np.float32)
        bufs[0].upload(r)
        bufs[1].upload(np.ascontiguousarray(comp[:ncomp]))
        bufs[2].upload(off)
        bufs[3].upload(canary)
        engine.project_dev(bufs[0].ptr, n, bufs[1].ptr, ncomp, bufs[3].ptr, bufs[2].ptr)
        engine.sync()
        back = bufs[3].download((n * (ncomp + 1),), np.float32)
        assert np.array_equal(bits(back[:n * ncomp].reshape(n, ncomp)), bits(got)) and (back[n * ncomp:] == -7.5).all()
    finally:
        for b in bufs:
            b.free()


def test_the_edges_of_the_interface(engine):
    r = planted_rows()[:10]
    with pytest.raises(ValueError, match="components"):
        engine.project(r, np.zeros((2, 512), np.float32))
    with pytest.raises(ValueError, match="rows"):
        engine.project(r[:0], r[:2])
    with pytest.raises(ValueError, match="rows"):
        engine.pca_moments(r[:0])
    with pytest.raises(GnnError, match="outside"):
        engine.project_dev(0, 4, 0, 65, 0)
    with pytest.raises(ValueError, match="valid rows"):
        engine.pca(np.concatenate([r[:1], np.zeros((3, 512), np.float32)]), 2)
    G, S, n_valid = engine.pca_moments_fixed(np.zeros((5, 512), np.float32))
    assert not G.any() and not S.any() and n_valid == 0
    p = engine.project(np.zeros((5, 512), np.float32), r[:3])
    assert p.shape == (5, 3) and np.isnan(p).all()


def test_pca_on_the_planted_spectrum(engine):
    """Weyl: |eigenvalue_k(C + dC) - eigenvalue_k(C)| <= |dC|_2 <= 512 max |dC|.  Davis-Kahan: the sine of the largest angle between
    the top-c eigenspaces of C and C + dC is at most |dC|_2 / gap, gap the distance from the c-th eigenvalue of one to the (c + 1)-th
    of the other.  dC is the device's covariance minus float64's, computed here from the device's own moments; the components come
    back as f32 rows (2^-24 of a unit row each, c of them)."""
    engine.set_pca_split(0)
    r, basis = spectrum_rows()
    c = SPECTRUM_RANK
    res = engine.pca(r, c)
    G, S, n_valid = engine.pca_moments(r)
    G64, S64, nv = sequence.pca_moments(r)
    ref = sequence.pca_from_moments(G64, S64, nv, c + 1)
    assert n_valid == nv == len(r) == res.n_valid and res.valid.all()
    mu, mu64 = S / n_valid, S64 / nv
    dC = (G / n_valid - np.outer(mu, mu)) - (G64 / nv - np.outer(mu64, mu64))
    weyl = 512 * np.abs(dC).max()
    d2 = np.linalg.norm(dC, 2)
    ev_err = np.abs(res.explained_variance - ref["explained_variance"][:c]).max()
    gap = ref["explained_variance"][c - 1] - ref["explained_variance"][c] - d2
    angle = subspace_residual(np.linalg.qr(res.components.astype(np.float64).T)[0].T, ref["components"][:c])
    print(f"\nplanted spectrum: max |dC| = {np.abs(dC).max():.3e}, |dC|_2 = {d2:.3e}, eigenvalue error {ev_err:.3e} (Weyl bound {weyl:.3e}), "
          f"subspace angle {angle:.3e} (Davis-Kahan bound {d2 / gap:.3e}, gap {gap:.3e})")
    assert ev_err <= weyl + 1e-15
    assert angle <= d2 / gap + c * 2.0 ** -24
    assert subspace_residual(np.linalg.qr(res.components.astype(np.float64).T)[0].T, basis) <= 0.05
    assert res.components.dtype == np.float32 and res.components.shape == (c, 512) and res.projection.shape == (len(r), c)
    for k in range(c):
        assert res.components[k, np.argmax(np.abs(res.components[k]))] > 0
    assert (np.diff(res.explained_variance) < 0).all() and res.explained_variance_ratio.sum() <= 1 + 1e-12
    # the scores: a value is within e = 1e-5 (the family's bound on a similarity) + 2 x 2^-24 (the offset's rounding, the subtraction's)
    # + 4.2e-7 (the device's mean against float64's) of u . v - mu . v, whose mean over the rows is 0 and whose variance is vT C v
    e = 1e-5 + 2 * 2.0 ** -24 + 4.2e-7
    p = res.projection.astype(np.float64)
    assert np.abs(p.mean(axis=0)).max() <= e
    margin = weyl + 2 * e * np.abs(p).max() + e * e
    assert np.abs(p.var(axis=0) - res.explained_variance).max() <= margin
    again = res.transform(r)
    assert np.array_equal(bits(again), bits(res.projection))
    assert np.array_equal(bits(engine.project(r[:70], res.components, res.mean)), bits(res.projection[:70]))
