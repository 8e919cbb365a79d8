"""Principal-component moments and projections on the MI355X at the limits tests/test_pca_gpu.py stays away from (the oracle, the
inputs and their CPU-side conditions: tests/moments_limits_data.py, tests/test_pca_limits_host.py).  Which line of gnn_pca.hip each
group pins:

  A  harvest        q_i = S of a one-row call: `(long long)((float)hi[e] * 16777216.f) + ...` of pca_sum_kernel on planted, huge,
                    subnormal, one-hot and heavy rows and on invalid ones, against float64 within the bound the host test derives; the
                    one-row G is one rounded product per entry: `x[e] = (float)hi[e] + (float)lo[e]` and the staging into xs.
  B  sums           S and G of 255, 256, 257, 600 and 607 general rows against the exact oracle, to the bit, under three row splits:
                    the fetch of hi AND lo per k-step and lane (`st.v[j][0]`, `st.v[j][1]`), the ascending row order of the chain, the
                    flush `(c & 7) == 7 || c + 1 == c1` at absolute granules, `c + 1 < c1` of the prefetch, the mirror.
  C  launch shapes  more rows than 64 per workgroup of pca_sum_kernel (`per_block`, `i0 + wave ... i += 4`) and more than one granule per
                    default range of pca_gram_kernel (`per = ceil(granules / want)`), against the device's own answers on
                    granule-aligned chunks of 4096 rows, which B pins to the oracle: integer adds make both sums exact.
  G  saturation     512 rows +-e_7: a Gram chain of 256 products of 2^16, |p * 2^16| = 2^40 per granule, the limit the header states;
                    extreme rows through pca_project_kernel against the neighbour search, bit for bit.
  H  projection     `lok[row] && cok` with an invalid component, which project() refuses on the host; 16 454 rows, beyond one slab of
                    the search it is compared with; small calls after a large one has left longer fragments in the shared buffers.

Measured on an MI355X (256 CUs).  The device's G equals the oracle at every entry, size and split: the f32-input matrix instruction
is, on this kernel, the k-ordered fmaf chain with one rounding per product.  max |q / 2^32 - u| / bound: huge rows 0.91, subnormal 0.85,
one-hot 0 (x = +-256 exactly), heavy 1.00 (elements on the absolute part of the bound: their low limbs are f16 subnormals); q mod 2^13
is non-zero at 98.0 % of the valid rows' elements (99.6 % of the planted rows').  Times: the harvest (607 one-row calls) 0.5 s, the 607
one-row G 0.8 s, B 0.07 .. 0.23 s per size (the oracle's chains), C 0.06 s, H beyond a slab 0.12 s, nothing else above 0.01 s.

Mutations of gnn_pca.hip, each applied to a scratch copy and run once (tests of this file that fail):
  lo fetched from k-step `(wave + 4 * (j & 1)) ^ 1` for lanes >= 48     B at all five sizes
  the flush at the range's end only (`(c & 7) == 7` dropped)              B at 600 and 607 rows, C.  (At 257 rows the row behind the
                                                                          border is an invalid one, and the default range is one granule.)
  `c` counted from the range's start in `(c & 7) == 7`                    not run: c0 is a multiple of 8, so it is the same program
No test found a fault in the kernels."""
import time

import numpy as np
import pytest

from tests import moments_limits_data as md
from tests.kmeans_data import planted
from tests.neighbours_data import rows
from tests.pca_data import planted_rows

pytestmark = pytest.mark.gpu

D = 512
_HARVEST = {}


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def restore(engine):
    engine.set_neighbour_split(0)
    engine.set_kmeans_lds(128)
    engine.set_pca_split(0)


def harvest_q(engine):
    """(q int64 (607, 512), n_valid int64 (607,)): S and n_valid of one one-row call per harvest row, computed once per process"""
    if "q" not in _HARVEST:
        r = md.harvest_rows()[0]
        n = len(r)
        engine.set_pca_split(0)
        bufs = [engine.alloc(r.nbytes), engine.alloc(8 * D * D), engine.alloc(8 * D * n), engine.alloc(8 * n)]
        try:
            bufs[0].upload(r)
            for i in range(n):
                engine.pca_moments_dev(bufs[0].ptr + 4 * D * i, 1, bufs[1].ptr, bufs[2].ptr + 8 * D * i, bufs[3].ptr + 8 * i)
            engine.sync()
            q, nv = bufs[2].download((n, D), np.int64), bufs[3].download((n,), np.int64)
        finally:
            for b in bufs:
                b.free()
        q.setflags(write=False)
        nv.setflags(write=False)
        _HARVEST["q"] = (q, nv)
    return _HARVEST["q"]


@pytest.fixture(scope="module")
def harvested(engine):
    return harvest_q(engine)


@pytest.fixture(autouse=True)
def settings_restored(engine):
    """every test of this file, however it ends, leaves the three test aids at the library's choice"""
    try:
        yield
    finally:
        restore(engine)


def scattered(engine, r, comp):
    """neighbours(rows, components, k = ncomp) scattered by index: NaN at an invalid row"""
    c = len(comp)
    idx, sim = engine.neighbours(r, comp, c)
    out = np.full((len(r), c), np.nan, np.float32)
    ok = idx[:, 0] >= 0
    assert (np.sort(idx[ok], axis=1) == np.arange(c)).all() and (idx[~ok] == -1).all()
    out[np.flatnonzero(ok)[:, None], idx[ok]] = sim[ok]
    return out


# ---- A: harvest and validate q ---------------------------------------------------------------------------------------------------------

def test_a_the_image_of_every_kind_of_row_is_within_the_bound_of_float64(harvested):
    """pca_sum_kernel's `(long long)((float)hi[e] * 16777216.f) + (long long)((float)lo[e] * 16777216.f)` on one row at a time"""
    q, nv = harvested
    r, keep, where = md.harvest_rows()
    assert not q[~keep].any() and not nv[~keep].any() and (nv[keep] == 1).all()
    u = md.unit64(r[keep])
    err = np.abs(q[keep] / 2.0 ** 32 - u)
    bound = md.q_bound(u)
    at = np.cumsum(keep) - 1
    for name, idx in dict(where, all=np.flatnonzero(keep)).items():
        e, b = err[at[idx]], bound[at[idx]]
        print(f"\n{name}: max |q / 2^32 - u| / bound = {(e / np.where(b > 0, b, 1)).max():.3f}, max relative error "
              f"{(e / np.where(u[at[idx]] != 0, np.abs(u[at[idx]]), np.inf)).max():.3e}")
    assert (err <= bound).all()
    x = q * 2.0 ** -24
    assert np.array_equal(x.astype(np.float32).astype(np.float64), x)     # hi + lo is an f32: what the Gram pass stages
    planted_idx = np.setdiff1d(np.flatnonzero(keep), np.concatenate(list(where.values())))
    low = (q[keep] % 2 ** 13 != 0).mean()
    print(f"\nnon-zero residues q mod 2^13: {low:.3%} of all valid rows' elements, {(q[planted_idx] % 2 ** 13 != 0).mean():.3%} of the planted rows'")
    assert low >= 0.25                                                     # the low limbs are really exercised


def test_a_the_gram_of_one_row_is_one_rounded_product_per_entry(engine, harvested):
    """pca_gram_kernel's staging `x[e] = (float)hi[e] + (float)lo[e]` -> xs and one product per accumulator entry, 607 times"""
    q, _ = harvested
    r = md.harvest_rows()[0]
    n, batch = len(r), 64
    engine.set_pca_split(0)
    bufs = [engine.alloc(r.nbytes), engine.alloc(8 * D * D * batch), engine.alloc(8 * D), engine.alloc(8)]
    try:
        bufs[0].upload(r)
        for i0 in range(0, n, batch):
            m = min(batch, n - i0)
            for j in range(m):
                engine.pca_moments_dev(bufs[0].ptr + 4 * D * (i0 + j), 1, bufs[1].ptr + 8 * D * D * j, bufs[2].ptr, bufs[3].ptr)
            engine.sync()
            G = bufs[1].download((m, D, D), np.int64)
            for j in range(m):
                assert np.array_equal(G[j], md.granule_gram(q[i0 + j:i0 + j + 1])), i0 + j
    finally:
        for b in bufs:
            b.free()


# ---- B: sums to the bit on general rows ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", md.HARVEST_NS + (607,))
def test_b_sums_of_general_rows_equal_the_oracle_bit_for_bit(engine, harvested, n):
    """pca_gram_kernel: hi and lo of every k-step and lane, the ascending chain, the flush at absolute granules; pca_sum_kernel"""
    q, nv = harvested
    r = md.harvest_rows()[0][:n]
    wG, wS = md.gram_oracle(q, n), q[:n].sum(axis=0)
    try:
        for split in (0, 256, 512):
            engine.set_pca_split(split)
            G, S, n_valid = engine.pca_moments_fixed(r)
            assert n_valid == nv[:n].sum() and np.array_equal(S, wS), split
            bad = G != wG
            if bad.any():
                rel = np.abs(G - wG)[bad] / np.maximum(np.abs(wG[bad]), 1)
                print(f"\nn {n}, split {split}: {bad.sum()} of 262144 entries differ from the oracle, by at most {np.abs(G - wG).max()} "
                      f"units of 2^-32, {rel.max():.3e} of the entry")
            assert not bad.any() and np.array_equal(G, G.T), split
    finally:
        restore(engine)


# ---- C: the library's own launch shapes ------------------------------------------------------------------------------------------------

def test_c_more_rows_than_one_unit_of_work_per_workgroup(engine):
    """pca_sum_kernel with per_block > 64 and pca_gram_kernel with a default range of more than one granule"""
    cus = engine.device_info()["cus"]
    r, keep = md.launch_rows(cus)
    n = len(r)
    assert n > 64 * 2 * cus and -(-n // 256) > -(-2 * cus // 10)           # per_block > 64; granules > want: a default range of >= 2
    t0 = time.perf_counter()
    try:
        engine.set_pca_split(0)
        G, S, n_valid = np.zeros((D, D), np.int64), np.zeros(D, np.int64), 0
        for c0 in range(0, n, 4096):                                       # 4096 rows: 16 granules and at most 64 rows per workgroup
            g, s, v = engine.pca_moments_fixed(r[c0:c0 + 4096])
            G += g
            S += s
            n_valid += v
        assert n_valid == keep.sum() == n - 5
        for split in (0, 256):
            engine.set_pca_split(split)
            got = engine.pca_moments_fixed(r)
            assert got[2] == n_valid and np.array_equal(got[1], S) and np.array_equal(got[0], G) and np.array_equal(got[0], got[0].T), split
    finally:
        restore(engine)
    print(f"\n{n} rows at {cus} CUs: {time.perf_counter() - t0:.2f} s")


# ---- G: saturation and extremes --------------------------------------------------------------------------------------------------------

def test_g_a_chain_at_the_limit_the_header_states(engine):
    """pca_gram_kernel's `llrint((double)acc * 65536.0)` at |p * 2^16| = 2^40: 256 products of 2^16 in one entry, twice"""
    try:
        for plus, minus in ((300, 212), (256, 256)):
            r, sign = md.axis_rows(plus, minus)
            for split in (0, 256):
                engine.set_pca_split(split)
                G, S, n_valid = engine.pca_moments_fixed(r)
                want = np.zeros((D, D), np.int64)
                want[7, 7] = 512 * 2 ** 32
                assert n_valid == 512 and np.array_equal(G, want)
                assert S[7] == (plus - minus) * 2 ** 32 and not np.delete(S, 7).any()
    finally:
        restore(engine)


def test_g_extreme_rows_project_as_the_neighbour_search_finds_them(engine):
    """pca_project_kernel on huge, subnormal, one-hot and heavy rows: the f32 of gnn_neighbours, bit for bit"""
    r, _, where = md.harvest_rows()
    ext = np.ascontiguousarray(r[np.sort(np.concatenate(list(where.values())))])
    comp = np.ascontiguousarray(planted_rows()[600:603])
    restore(engine)
    got = engine.project(ext, comp)
    assert got.shape == (40, 3) and not np.isnan(got).any()
    assert np.array_equal(bits(got), bits(scattered(engine, ext, comp)))


# ---- H: projection and workspace -------------------------------------------------------------------------------------------------------

def test_h_an_invalid_component_is_a_column_of_nan(engine):
    """pca_project_kernel's `lok[row] && cok` with cok false: project() refuses such a component on the host, project_dev takes it"""
    r = np.ascontiguousarray(md.harvest_rows()[0][:130])                   # rows 0 is invalid; two tiles and two rows
    n = len(r)
    comp = np.ascontiguousarray(planted_rows()[600:603])
    two = engine.project(r, comp[[0, 2]])
    bufs = [engine.alloc(r.nbytes), engine.alloc(comp.nbytes), engine.alloc(4 * n * 3)]
    try:
        bufs[0].upload(r)
        for poison in ("zero", "nan"):
            bad = comp.copy()
            bad[1] = 0
            if poison == "nan":
                bad[1] = comp[1]
                bad[1, 200] = np.nan
            bufs[1].upload(bad)
            engine.project_dev(bufs[0].ptr, n, bufs[1].ptr, 3, bufs[2].ptr)
            engine.sync()
            got = bufs[2].download((n, 3), np.float32)
            assert np.isnan(got[:, 1]).all(), poison
            assert np.array_equal(bits(np.ascontiguousarray(got[:, [0, 2]])), bits(two)), poison
        assert np.isnan(two[0]).all() and not np.isnan(two[1:]).any()
    finally:
        for b in bufs:
            b.free()


def test_h_beyond_one_slab_and_small_calls_after_a_large_one(engine):
    """pca_project_kernel over 258 row tiles against a reference that crosses its query slab of 16384; nn_reserve'd buffers that a
    larger call has left longer than the next call's rows"""
    restore(engine)
    p = planted_rows()
    comp = np.ascontiguousarray(p[600:633])
    small = (np.ascontiguousarray(p[:5]), np.ascontiguousarray(p[100:170]), planted()[0])

    def small_calls():
        k = engine.kmeans(small[2], 7)
        return (*engine.pca_moments_fixed(small[0])[:2], engine.project(small[1], comp[:3]), k.label, k.sim, k.centroids, k.size)

    before = small_calls()
    big = rows(16454, 6)
    big[[5, 16383, 16384, 16453]] = 0
    t0 = time.perf_counter()
    got = engine.project(big, comp)
    want = scattered(engine, big, comp)
    assert np.isnan(got[[5, 16383, 16384, 16453]]).all() and np.isnan(got).sum() == 4 * 33
    assert np.array_equal(bits(got), bits(want))
    engine.centroids(big, np.arange(16454) % 5, 5)                         # the k-means buffers too
    print(f"\n16454 rows on 33 components and their search: {time.perf_counter() - t0:.2f} s")
    after = small_calls()
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(before, after))
