"""The exact t-SNE layout, host side (no GPU): ``sequence.tsne_forces`` against a dense float64 evaluation with bounds derived from
the rounding units, ``sequence.tsne_kl`` against a dense float64 divergence, the quality of the layout of planted families against a
float64 twin of the same schedule, the invariances the definition promises, and ``main()`` over a fake engine."""
import shutil

import numpy as np
import pytest

from genomad_amd import nn_classification as nnc, sequence
from genomad_amd.engine import NNEngine, TSNEResult
from tests.test_analyses_host import ENV as OTHER_ENV, fake_main, same_file
from tests.test_knn_graph_host import KNN_ENV, FakeKnnEngine
from tests.test_strand_host import _npz, _same_npz, _tree, _write_fasta

U = 2.0 ** -24                     # the rounding unit of float32
G = sequence.TSNE_GRANULE


# ---- the inputs ------------------------------------------------------------------------------------------------------------------

def random_graph(n, per_row=5, seed=0, parallel=True):
    """an upper-triangle CSR of about ``per_row`` entries per row in any order, some parallel (unless told not to), some with a
    similarity <= 0; two invalid rows; a layout with two coincident points and one point 10^3 away"""
    rng = np.random.default_rng(seed)
    cols, sims = [], []
    for i in range(n - 1):
        c = rng.integers(i + 1, n, size=per_row) if parallel else rng.permutation(np.arange(i + 1, n))[:per_row]
        s = rng.uniform(0.05, 1.0, size=len(c))
        s[rng.random(len(c)) < 0.1] = -0.5
        cols.append(c)
        sims.append(s)
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in cols]), [sum(len(c) for c in cols)]]).astype(np.int64)
    valid = np.ones(n, dtype=bool)
    valid[[4, n - 3]] = False
    y = (2 * rng.standard_normal((n, 2))).astype(np.float32)
    y[9] = y[2]
    y[20] += np.float32(1e3)
    return indptr, np.concatenate(cols).astype(np.int32), np.concatenate(sims).astype(np.float32), valid, y


def planted(seed=0, families=4, per=60, noise=60, dim=16):
    """the planted input: ``families`` tight families of ``per`` rows and ``noise`` rows in ``dim`` dimensions, as 512-wide rows, and
    each row's family (-1: noise)"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((families, dim))
    rows = np.zeros((families * per + noise, 512), dtype=np.float32)
    rows[:, :dim] = np.concatenate([c + 0.25 * rng.standard_normal((per, dim)) for c in centres] + [rng.standard_normal((noise, dim))])
    return rows, np.concatenate([np.full(per, f) for f in range(families)] + [np.full(noise, -1)])


# ---- float64 references, written here ----------------------------------------------------------------------------------------------

def dense_q(y, ok):
    """float64 1 / (1 + d^2) between valid rows, 0 on the diagonal and at an invalid row or column; dx, dy"""
    y = y.astype(np.float64)
    dx, dy = y[:, None, 0] - y[None, :, 0], y[:, None, 1] - y[None, :, 1]
    with np.errstate(invalid="ignore"):
        q = 1.0 / (1.0 + dx * dx + dy * dy)
    q[~ok] = 0
    q[:, ~ok] = 0
    np.fill_diagonal(q, 0)
    return q, np.where(q > 0, dx, 0), np.where(q > 0, dy, 0)


def dense_p(n, i, j, qw, m2):
    p = np.zeros((n, n))
    np.add.at(p, (i, j), qw.astype(np.float64) / float(m2))
    return p


def granule_sums(a):
    """(n, granules): the sum of every row's entries over each granule of 256 columns"""
    n = a.shape[0]
    pad = -(-a.shape[1] // G) * G
    b = np.zeros((n, pad))
    b[:, :a.shape[1]] = a
    return b.reshape(n, pad // G, G).sum(axis=2)


def twin_layout(n, p, init, n_iter, exaggeration_iter, exaggeration, lr):
    """the float64 twin: the definition's own formulas - differences, not a Gram matrix - with the same affinities, init and schedule
    on all-valid rows, every operation and every sum in plain float64"""
    y = init.astype(np.float64)
    gain, upd = np.ones_like(y), np.zeros_like(y)
    for it in range(n_iter):
        dx, dy = y[:, None, 0] - y[None, :, 0], y[:, None, 1] - y[None, :, 1]
        q = 1.0 / (1.0 + (dx * dx + dy * dy))
        np.fill_diagonal(q, 0)
        early = it < exaggeration_iter
        w, q2 = p * q, q * q
        att = np.stack([(w * dx).sum(axis=1), (w * dy).sum(axis=1)], axis=1)
        rep = np.stack([(q2 * dx).sum(axis=1), (q2 * dy).sum(axis=1)], axis=1) / q.sum()
        g = 4.0 * ((exaggeration if early else 1.0) * att - rep)
        gain = np.maximum(np.where(((g > 0) & (upd < 0)) | ((g < 0) & (upd > 0)), gain + 0.2, gain * 0.8), 0.01)
        upd = (0.5 if early else 0.8) * upd - lr * (gain * g)
        y = y + upd
    return y


def dense_kl(p, y):
    q, _, _ = dense_q(y, np.ones(len(y), dtype=bool))
    keep = p > 0
    return float((p[keep] * np.log(p[keep] / (q[keep] / q.sum()))).sum())


# ---- the definition against a brute force ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [300, 700])
def test_one_steps_forces_lie_within_the_rounding_bounds_of_a_dense_float64_evaluation(n):
    """Bounds, per row, in the integers' own units.  Repulsion: a chain of 256 float32 operations has a relative error of at most
    256 * 2^-24 of the sum of its terms' magnitudes, and every (row, granule) adds half a unit for its rint: bound = sum over
    granules of (256 * 2^-24 * sum |term| * unit + 1/2).  Attraction: an entry's value (p q) d carries the roundings of p (1), q (6:
    dx, dx dx, the sum, 1 + s, the division, and dy's share), the two products (2) and d (1), at most 12 * 2^-24 relative, and half a
    unit for its rint: bound = sum over the row's entries of (12 * 2^-24 * |term| * 2^32 + 1/2).
    Measured, as the largest error / bound over all rows: n = 300: zi 0.19, rx 0.45, ry 0.06, ax 0.43, ay 0.57; n = 700: zi 0.75,
    rx 0.58, ry 0.17, ax 0.72, ay 0.74 - the largest ratios stand at the point 10^3 away and at rows of one or two entries, where
    the rint's half units are all of the bound; the chains' own error is far below theirs."""
    indptr, col, sim, valid, y = random_graph(n, seed=n)
    _, i, j, p, qw, m2, ok = sequence.tsne_affinities(indptr, col, sim, valid)
    zi, rx, ry, ax, ay = sequence.tsne_forces(y, i, j, p, ok)
    q, dx, dy = dense_q(y, ok)
    for name, got, term, unit in (("zi", zi, q, sequence.TSNE_Z_UNIT), ("rx", rx, q * q * dx, sequence.TSNE_F_UNIT),
                                  ("ry", ry, q * q * dy, sequence.TSNE_F_UNIT)):
        want = term.sum(axis=1) * unit
        bound = (256 * U * granule_sums(np.abs(term)) * unit + 0.5).sum(axis=1)
        ratio = np.abs(got - want)[ok] / bound[ok]
        print(f"n={n} {name}: largest error / bound = {ratio.max():.3f}")
        assert (ratio <= 1).all() and (got[~ok] == 0).all(), name
    pd = dense_p(n, i, j, qw, m2)
    count = np.bincount(i, minlength=n)
    for name, got, d in (("ax", ax, dx), ("ay", ay, dy)):
        term = pd * q * d
        want = term.sum(axis=1) * sequence.TSNE_F_UNIT
        bound = 12 * U * np.abs(term).sum(axis=1) * sequence.TSNE_F_UNIT + 0.5 * count
        live = count > 0
        ratio = np.abs(got - want)[live] / bound[live]
        print(f"n={n} {name}: largest error / bound = {ratio.max():.3f}")
        assert (ratio <= 1).all() and (got[~live] == 0).all(), name
    assert m2 == 2 * int(qw[:len(qw) // 2].sum()) and abs(float(p.astype(np.float64).sum()) - 1) < len(p) * U


def test_a_chain_is_one_float32_operation_at_a_time_in_ascending_column_order():
    """the vectorised chains of the definition against a loop that spells them out, for three rows"""
    indptr, col, sim, valid, y = random_graph(300, seed=1)
    _, i, j, p, _, _, ok = sequence.tsne_affinities(indptr, col, sim, valid)
    zi, rx, ry, _, _ = sequence.tsne_forces(y, i, j, p, ok)
    one = np.float32(1)
    for r in (0, 9, 299):
        tz = tx = ty = 0
        for g0 in range(0, 512, G):
            cz = cx = cy = np.float32(0)
            for c in range(g0, g0 + G):
                if c >= 300 or c == r or not ok[c]:
                    q, dx, dy = np.float32(0), np.float32(0), np.float32(0)
                else:
                    dx, dy = y[r, 0] - y[c, 0], y[r, 1] - y[c, 1]
                    q = one / (one + (dx * dx + dy * dy))
                cz, cx, cy = cz + q, cx + (q * q) * dx, cy + (q * q) * dy
            tz += int(np.rint(np.float64(cz) * 2.0 ** 20))
            tx += int(np.rint(np.float64(cx) * 2.0 ** 32))
            ty += int(np.rint(np.float64(cy) * 2.0 ** 32))
        assert (tz, tx, ty) == (zi[r], rx[r], ry[r])


def test_kl_lies_within_the_bound_of_a_dense_float64_divergence():
    """Without parallel entries sum p (log p - log q) + log Z is the divergence of the dense P from Q / Z.  Bound: Z's image is off
    by at most half a unit of 2^-20 per (row, granule) and 256 * 2^-24 relative for the chains; p carries one rounding and q six, each
    inside a logarithm or as a factor: 2^-24 * (sum p |log p| + 8).  Measured: error 1.7e-08, bound 1.6e-05."""
    n = 300
    indptr, col, sim, _, y = random_graph(n, seed=7, parallel=False)
    _, i, j, p, qw, m2, ok = sequence.tsne_affinities(indptr, col, sim)
    zi = sequence.tsne_forces(y, i, j, p, ok, attract=False)[0]
    got = sequence.tsne_kl(indptr, col, sim, y, int(zi.sum()))
    pd = dense_p(n, i, j, qw, m2)
    want = dense_kl(pd, y)
    zd = dense_q(y, ok)[0].sum()
    p64 = pd[pd > 0]
    bound = 0.5 * 2.0 ** -20 * n * -(-n // G) / zd + 256 * U + U * (float((p64 * np.abs(np.log(p64))).sum()) + 8)
    print(f"kl: error {abs(got - want):.2e}, bound {bound:.2e}")
    assert abs(got - want) <= bound
    assert sequence.tsne_kl(np.zeros(4, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros((3, 2), np.float32), 0) == 0.0


# ---- quality -----------------------------------------------------------------------------------------------------------------------

def test_planted_families_are_laid_out_apart_and_the_divergence_is_the_float64_twins():
    """4 families of 60 rows and 60 noise rows (16-D, cosine k-nearest-neighbour graph with k = 10, hash init, 300 iterations, 100
    of them exaggerated): the divergence falls, every family row's 5 nearest layout neighbours share its family for at least 0.98
    of the family rows, and the divergence is the float64 twin's within the twin's own spread over five shifted hash inits.
    Measured: KL 3.0413 -> 1.1928, purity 0.9917 (238 of 240); the twin from the same init 1.1979, from the five shifted inits
    1.1976, 1.2077, 1.2001, 1.2029, 1.2014 - a spread of 0.0101 against a difference of 0.0051.  The margin is coarse on purpose and
    cannot be finer: 300 iterations from an init of 1e-4 amplify the last bit, so the twin's own divergence moves by about 0.005 with
    the order of its float64 sums (two other spellings of the same twin gave 1.1955 and 1.1996 from the same init).  A gradient
    that is wrong shows in the tenths."""
    rows, family = planted()
    n = len(rows)
    g = sequence.knn_graph(rows, 10)
    kw = dict(n_iter=300, exaggeration_iter=100)
    init = sequence.tsne_init(n)
    start = sequence.tsne_layout(g["indptr"], g["col"], g["sim"], init, n_iter=0)
    kl0 = sequence.tsne_kl(g["indptr"], g["col"], g["sim"], start["layout"], start["z_trace"][-1])
    res = sequence.tsne_layout(g["indptr"], g["col"], g["sim"], init, **kw)
    kl = sequence.tsne_kl(g["indptr"], g["col"], g["sim"], res["layout"], res["z_trace"][-1])
    y = res["layout"].astype(np.float64)
    d = ((y[:, None] - y[None]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    near = np.argsort(d, axis=1)[:, :5]
    purity = float(np.mean([(family[near[r]] == family[r]).all() for r in range(n) if family[r] >= 0]))
    _, i, j, _, qw, m2, _ = sequence.tsne_affinities(g["indptr"], g["col"], g["sim"])
    pd = dense_p(n, i, j, qw, m2)
    lr = float(sequence.tsne_params(n_valid=n)[3])
    twin = [dense_kl(pd, twin_layout(n, pd, sequence.tsne_init(n, offset=2 * n * s), 300, 100, 12.0, lr)) for s in range(6)]
    spread = max(twin[1:]) - min(twin[1:])
    print(f"KL {kl0:.4f} -> {kl:.4f}, purity {purity:.4f}, twin {twin[0]:.4f}, shifted " + ", ".join(f"{t:.4f}" for t in twin[1:])
          + f", spread {spread:.4f}")
    assert np.isfinite(y).all() and res["iterations"] == 300 and len(res["z_trace"]) == 301
    assert kl < kl0 and purity >= 0.98
    assert abs(kl - twin[0]) <= spread


# ---- invariances -------------------------------------------------------------------------------------------------------------------

def test_the_order_of_a_rows_entries_changes_nothing():
    indptr, col, sim, valid, y = random_graph(300, seed=3)
    rng = np.random.default_rng(0)
    col2, sim2 = col.copy(), sim.copy()
    for r in range(len(indptr) - 1):
        o = rng.permutation(indptr[r + 1] - indptr[r]) + indptr[r]
        col2[indptr[r]:indptr[r + 1]], sim2[indptr[r]:indptr[r + 1]] = col[o], sim[o]
    assert not np.array_equal(col, col2)
    kw = dict(n_iter=12, exaggeration_iter=4)
    init = sequence.tsne_init(300)
    a, b = (sequence.tsne_layout(indptr, c, s, init, valid, **kw) for c, s in ((col, sim), (col2, sim2)))
    assert np.array_equal(a["z_trace"], b["z_trace"]) and np.array_equal(a["layout"].view(np.uint32), b["layout"].view(np.uint32))


def test_an_entry_as_two_parallel_halves_changes_the_attraction_by_its_rint_alone():
    """q even: the halves' weights add up to q, so M2 stays; p halves exactly, (p q) d halves exactly, and two rints of a half may
    differ from one rint of the whole by one unit - at the entry's two rows, nowhere else; the repulsion does not read the graph"""
    indptr, col, sim, valid, y = random_graph(300, seed=5)
    _, i, j, p, qw, m2, ok = sequence.tsne_affinities(indptr, col, sim, valid)
    base = sequence.tsne_forces(y, i, j, p, ok)
    changed = 0
    for x in np.flatnonzero(np.rint(sim.astype(np.float64) * 2.0 ** 24) % 2 == 0)[:40]:
        r = int(np.searchsorted(indptr, x, side="right") - 1)
        q = int(np.rint(float(sim[x]) * 2.0 ** 24))
        if q <= 0 or not (valid[r] and valid[col[x]]):
            continue
        half = np.float32((q // 2) / 2.0 ** 24)
        sim2 = np.concatenate([sim[:x], [half, half], sim[x + 1:]]).astype(np.float32)
        col2 = np.concatenate([col[:x], [col[x], col[x]], col[x + 1:]]).astype(np.int32)
        ptr2 = indptr.copy()
        ptr2[r + 1:] += 1
        _, i2, j2, p2, _, m22, _ = sequence.tsne_affinities(ptr2, col2, sim2, valid)
        got = sequence.tsne_forces(y, i2, j2, p2, ok)
        assert m22 == m2 and all(np.array_equal(got[k], base[k]) for k in range(3))
        for k in (3, 4):
            diff = got[k] - base[k]
            assert np.abs(diff).max() <= 1 and not diff[np.setdiff1d(np.arange(300), [r, col[x]])].any()
            changed += int(np.abs(diff).sum())
    assert changed > 0                                        # the one unit does occur


def test_invalid_rows_end_as_nan_and_move_nobody():
    indptr, col, sim, valid, y = random_graph(300, seed=9)
    init = sequence.tsne_init(300)
    kw = dict(n_iter=8, exaggeration_iter=3)
    res = sequence.tsne_layout(indptr, col, sim, init, valid, **kw)
    assert np.isnan(res["layout"][~valid]).all() and np.isfinite(res["layout"][valid]).all() and np.array_equal(res["valid"], valid)
    other = init.copy()
    other[~valid] = np.nan                                    # what stands at an invalid row is never read
    again = sequence.tsne_layout(indptr, col, sim, other, valid, **kw)
    assert np.array_equal(res["z_trace"], again["z_trace"])
    assert np.array_equal(res["layout"][valid].view(np.uint32), again["layout"][valid].view(np.uint32))
    bad = init.copy()
    bad[0, 1] = np.inf
    with pytest.raises(ValueError, match="finite"):
        sequence.tsne_layout(indptr, col, sim, bad, valid, **kw)


def test_at_most_one_valid_row_has_z_zero_and_stays_finite():
    ptr, col, sim = np.zeros(4, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32)
    init = sequence.tsne_init(3)
    for valid in (np.array([False, True, False]), np.zeros(3, dtype=bool)):
        res = sequence.tsne_layout(ptr, col, sim, init, valid, n_iter=5)
        assert not res["z_trace"].any() and len(res["z_trace"]) == 6
        assert np.array_equal(res["layout"][valid].view(np.uint32), init[valid].view(np.uint32)) and np.isnan(res["layout"][~valid]).all()
        assert sequence.tsne_kl(ptr, col, sim, res["layout"], 0, valid) == 0.0
    empty = sequence.tsne_layout(np.zeros(1, np.int64), col, sim, np.zeros((0, 2), np.float32), n_iter=2)
    assert empty["layout"].shape == (0, 2) and not empty["z_trace"].any()
    # two valid rows without an entry: they repel each other, Z > 0
    two = sequence.tsne_layout(ptr, col, sim, init, np.array([True, False, True]), n_iter=3)
    assert two["z_trace"].all() and np.isfinite(two["layout"][[0, 2]]).all()


def test_the_init_and_the_knobs():
    a = sequence.tsne_init(1000)
    assert a.dtype == np.float32 and a.shape == (1000, 2) and (a >= -1e-4).all() and (a < 1e-4).all()
    assert np.array_equal(a, sequence.tsne_init(1000)) and np.array_equal(sequence.tsne_init(1000, offset=6)[:-3], a[3:])
    assert abs(float(a.mean())) < 1e-5 and 5e-5 < float(a.std()) < 6.5e-5          # uniform: 1e-4 / sqrt(3)
    # the first output of splitmix64 from seed 0 is 0xE220A8397B1DCDAF: its top 24 bits
    assert a[0, 0] == np.float32(((0xE220A8397B1DCDAF >> 40) / 2.0 ** 23 - 1) * 1e-4)
    assert sequence.tsne_params(n_valid=262144)[3] == np.float32(262144 / 12 / 4) and sequence.tsne_params(n_valid=10)[3] == 50
    for kw in (dict(n_iter=-1), dict(n_iter=100001), dict(n_iter=1.5), dict(exaggeration_iter=100001), dict(exaggeration=0.5),
               dict(exaggeration=2000), dict(learning_rate=0), dict(learning_rate=float("nan")), dict(learning_rate=2.0 ** 21)):
        with pytest.raises(ValueError):
            sequence.tsne_params(**kw)
    with pytest.raises(ValueError, match="2\\^21"):
        sequence.tsne_affinities(np.zeros((1 << 21) + 2, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))
    t = sequence.tsne_table(np.array([[1, 2], [np.nan, np.nan]], np.float32), [True, False], ["a", "b"])
    assert t == [{"name": "a", "x": 1.0, "y": 2.0}, {"name": "b", "x": None, "y": None}]


# ---- main() through the fake engine ------------------------------------------------------------------------------------------------

BASE = {"GENOMAD_AMD_EMBEDDINGS": "1"}
FILES = ["m_nn_tsne.npz", "m_nn_tsne.tsv"]
KNN_FILES = ["m_nn_knn_graph.npz", "m_nn_knn_graph.tsv"]


class FakeTsneEngine(FakeKnnEngine):
    """the stand-in of tests/test_knn_graph_host.py plus the layout from sequence.tsne_layout; the chain and the PCA init are the
    engine's own host code over the stand-in's knn_graph and pca"""
    tsne_rows = NNEngine.tsne_rows
    tsne_pca_init = NNEngine.tsne_pca_init

    def tsne(self, indptr, col, sim, init, valid=None, n_iter=750, exaggeration_iter=250, exaggeration=12.0, learning_rate=None):
        type(self).calls.append(("tsne", len(indptr) - 1, int(n_iter)))
        r = sequence.tsne_layout(indptr, col, sim, init, valid, n_iter, exaggeration_iter, exaggeration, learning_rate)
        n_iter, ex_iter, e, lr = sequence.tsne_params(n_iter, exaggeration_iter, exaggeration, learning_rate, int(r["valid"].sum()))
        return TSNEResult(layout=r["layout"], z_trace=r["z_trace"], iterations=n_iter, valid=r["valid"], n=len(r["valid"]),
                          kl_divergence=sequence.tsne_kl(indptr, col, sim, r["layout"], r["z_trace"][-1], r["valid"]),
                          exaggeration_iter=ex_iter, exaggeration=e, learning_rate=float(lr))


def set_env(mp, env):
    """exactly the switches of ``env``, none of the others"""
    mp.setattr(nnc, "_engine", lambda: FakeTsneEngine())
    for k in OTHER_ENV + KNN_ENV + ("GENOMAD_AMD_COMMUNITIES", "GENOMAD_AMD_COMMUNITIES_MAX_LEVELS", "GENOMAD_AMD_TSNE"):
        mp.delenv(k, raising=False)
    for k, v in env.items():
        mp.setenv(k, v)


def names_of_calls():
    return [c[0] if isinstance(c, tuple) else c for c in FakeTsneEngine.calls]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """one run with the embeddings and the graph but without GENOMAD_AMD_TSNE and one with it, shared and left unchanged.  The
    contigs: c0 .. c7, one of them a run of N (no embedding)"""
    root = tmp_path_factory.mktemp("tsne")
    fa = root / "m.fna"
    _write_fasta(fa, n=8)
    off = dict(BASE, GENOMAD_AMD_KNN_GRAPH="3")
    on = dict(off, GENOMAD_AMD_TSNE="6")
    with pytest.MonkeyPatch.context() as mp:
        set_env(mp, off)
        fake_main(fa, root / "unset")
        set_env(mp, on)
        del FakeTsneEngine.calls[:]
        fake_main(fa, root / "on")
        found = list(FakeTsneEngine.calls)
    return {"fa": fa, "env": on, "off": off, "unset": root / "unset" / "m_nn_classification", "on": root / "on", "calls": found}


def test_the_switch_adds_its_two_files_and_changes_nothing_else(world):
    d0, d1 = world["unset"], world["on"] / "m_nn_classification"
    assert _tree(d1) == sorted(_tree(d0) + FILES)
    for rel in _tree(d0):                                       # every other output: the same arrays, the same bytes
        if rel.endswith(".npz"):
            assert _same_npz(d0 / rel, d1 / rel) or same_file(d0 / rel, d1 / rel), rel
        elif rel.endswith(".tsv"):
            assert (d0 / rel).read_bytes() == (d1 / rel).read_bytes(), rel
    calls = [c[0] for c in world["calls"] if isinstance(c, tuple)]
    assert calls == ["knn_graph", "knn_graph", "pca", "tsne"]      # the graph's own analysis, then the layout's chain
    log = [line for line in (world["on"] / "m_nn_classification.log").read_text().splitlines() if " written to " in line]
    assert log[-1].endswith("written to m_nn_tsne.npz and m_nn_tsne.tsv.")
    assert "t-SNE layout of the sequences (6 iterations over the 3-nearest-neighbour graph, union, weighted by similarity, from the " \
           "first two principal components: " in log[-1] and "Kullback-Leibler divergence " in log[-1]


def test_the_files_hold_the_definition_from_the_pca_init(world):
    d = world["on"] / "m_nn_classification"
    z, emb = _npz(d / FILES[0]), _npz(d / "m_nn_embeddings.npz")["embeddings"]
    g = sequence.knn_graph(emb, 3)
    eng = FakeTsneEngine()
    init = eng.tsne_pca_init(emb)
    ok = g["valid"]
    assert ok.all() and abs(float(init[:, 0].astype(np.float64).std()) - 1e-4) < 1e-9
    want = sequence.tsne_layout(g["indptr"], g["col"], g["sim"], init, ok, n_iter=6)
    assert np.array_equal(z["layout"], want["layout"], equal_nan=True) and np.array_equal(z["z_trace"], want["z_trace"])
    assert np.array_equal(z["valid"], ok) and z["layout"].dtype == np.float32 and z["z_trace"].dtype == np.uint64
    assert (z["n_iter"], z["k"], str(z["mode"]), str(z["weight"]), str(z["metric"]), str(z["init"])) == (6, 3, "union", "similarity", "cosine", "pca")
    assert (z["exaggeration_iter"], z["exaggeration"], z["learning_rate"]) == (250, 12.0, 50.0) and "strand" not in z
    assert z["kl_divergence"] == sequence.tsne_kl(g["indptr"], g["col"], g["sim"], want["layout"], want["z_trace"][-1], ok)
    names = [str(x) for x in z["contig_names"]]
    lines = (d / FILES[1]).read_bytes().decode().split("\n")
    assert lines[0] == "seq_name\tx\ty" and lines[-1] == "" and len(lines) == len(names) + 2
    assert lines[1:-1] == [f"{nm}\t{xy[0]:.6f}\t{xy[1]:.6f}" if v else f"{nm}\tNA\tNA" for nm, xy, v in zip(names, want["layout"], ok)]


def test_a_contig_without_an_embedding_has_na_in_the_tsv_and_nan_in_the_npz(tmp_path):
    rows, _ = planted(families=2, per=6, noise=3)
    rows[4] = 0                                               # no direction: invalid under cosine
    names = np.array([f"c{i}" for i in range(len(rows))])
    res = FakeTsneEngine().tsne_rows(rows, 3, n_iter=4)
    assert not res.valid[4] and res.valid.sum() == len(rows) - 1
    nnc.write_tsne(tmp_path / "t.npz", tmp_path / "t.tsv", "contig_names", names, res, (4, 3, "union", "similarity"), "both")
    z = _npz(tmp_path / "t.npz")
    assert np.isnan(z["layout"][4]).all() and np.isfinite(np.delete(z["layout"], 4, axis=0)).all() and str(z["strand"]) == "both"
    lines = (tmp_path / "t.tsv").read_text().split("\n")
    assert lines[5] == "c4\tNA\tNA" and sum(line.endswith("NA") for line in lines) == 1
    assert lines[1] == f"c0\t{res.layout[0, 0]:.6f}\t{res.layout[0, 1]:.6f}"


def test_the_same_command_again_calls_nothing_and_another_request_runs_again(world, tmp_path, monkeypatch):
    out = tmp_path / "on"
    shutil.copytree(world["on"], out)
    d = out / "m_nn_classification"
    everything = _tree(d)
    on = world["env"]
    set_env(monkeypatch, on)
    del FakeTsneEngine.calls[:]
    fake_main(world["fa"], out)
    assert FakeTsneEngine.calls == []
    runs = 0
    for env, entry in ((dict(on, GENOMAD_AMD_TSNE="7"), ("n_iter", 7)), (dict(on, GENOMAD_AMD_KNN_GRAPH="2"), ("k", 2)),
                       (dict(on, GENOMAD_AMD_KNN_GRAPH_MODE="mutual"), ("mode", "mutual")), (on, ("n_iter", 6))):
        set_env(monkeypatch, env)
        fake_main(world["fa"], out)                             # another n_iter or another graph: the stage runs again
        runs += 1
        assert names_of_calls().count("tsne") == runs and _npz(d / FILES[0])[entry[0]] == entry[1] and _tree(d) == everything
        fake_main(world["fa"], out)                             # and is resumed from
        assert names_of_calls().count("tsne") == runs
    assert same_file(d / FILES[0], world["on"] / "m_nn_classification" / FILES[0])
    assert (d / FILES[1]).read_bytes() == (world["on"] / "m_nn_classification" / FILES[1]).read_bytes()
    (d / FILES[1]).unlink()
    fake_main(world["fa"], out)                                 # one of the pair is gone: again
    assert names_of_calls().count("tsne") == runs + 1 and _tree(d) == everything
    set_env(monkeypatch, world["off"])                          # unset again: its files go, every other output is what it was
    fake_main(world["fa"], out)
    assert _tree(d) == _tree(world["unset"])
    for rel in _tree(d):
        if rel.endswith(".tsv"):
            assert (world["unset"] / rel).read_bytes() == (d / rel).read_bytes(), rel


def test_the_switch_is_refused_without_the_graph_or_the_embeddings(world, tmp_path, monkeypatch, capsys):
    for env, words in ((dict(BASE, GENOMAD_AMD_TSNE="6"),
                        "GENOMAD_AMD_TSNE needs GENOMAD_AMD_KNN_GRAPH: the layout is that of the k-nearest-neighbour graph of the per-contig "
                        "encoder embeddings. Set GENOMAD_AMD_KNN_GRAPH or unset GENOMAD_AMD_TSNE."),
                       ({"GENOMAD_AMD_TSNE": "6", "GENOMAD_AMD_KNN_GRAPH": "3"}, "GENOMAD_AMD_KNN_GRAPH needs GENOMAD_AMD_EMBEDDINGS=1: "),
                       ({"GENOMAD_AMD_TSNE": "6"}, "GENOMAD_AMD_TSNE needs GENOMAD_AMD_EMBEDDINGS=1: the layout is that of the ")):
        set_env(monkeypatch, env)
        del FakeTsneEngine.calls[:]
        capsys.readouterr()
        with pytest.raises(SystemExit) as exc:
            fake_main(world["fa"], tmp_path / "refused")
        err = capsys.readouterr().err.strip().splitlines()
        assert exc.value.code == 1 and len(err) == 1 and words in err[0], err
        assert not list((tmp_path / "refused").rglob("*.npz")) and FakeTsneEngine.calls == []


def test_the_env_parsing_and_the_tables(world, tmp_path, monkeypatch):
    on = world["env"]
    for v in ("0", "100001", "x", "1.5", "-2"):
        set_env(monkeypatch, dict(on, GENOMAD_AMD_TSNE=v))
        with pytest.raises(ValueError, match=f"GENOMAD_AMD_TSNE='{v}': expected an integer in \\[1, 100000\\]"):
            fake_main(world["fa"], tmp_path / "bad")
    set_env(monkeypatch, dict(on, GENOMAD_AMD_TSNE=" 750 ", GENOMAD_AMD_KNN_GRAPH="15", GENOMAD_AMD_KNN_GRAPH_WEIGHT="jaccard"))
    assert nnc.tsne_requested() == (750, 15, "union", "jaccard")
    set_env(monkeypatch, dict(BASE, GENOMAD_AMD_TSNE="5"))
    assert nnc.tsne_requested() == (5, None, None, None)
    set_env(monkeypatch, world["off"])
    assert nnc.tsne_requested() is None
    # the seventeenth record, in a fourth table: the three tables that the earlier analyses' tests count are untouched
    assert len(nnc.ANALYSES) == 14 and len(nnc.ALL_ANALYSES) == 15 and len(nnc.EVERY_ANALYSIS) == 16
    assert nnc.EVERY_ANALYSIS == nnc.ANALYSES + nnc.MORE_ANALYSES + nnc.KNN_ANALYSES
    assert nnc.ANALYSES_RUN == nnc.EVERY_ANALYSIS + nnc.TSNE_ANALYSES and [a.name for a in nnc.TSNE_ANALYSES] == ["tsne"]
    assert len({a.name for a in nnc.ANALYSES_RUN}) == 17 and nnc.TSNE_ANALYSES[0].after == "knn_graph" and nnc.TSNE_ANALYSES[0].tsv
    outs = nnc.Outputs("m", tmp_path)
    assert outs.files("sequence", "tsne")[1].name == "m_nn_tsne.tsv" and outs.files("provirus", "tsne")[0].name == "m_provirus_nn_tsne.npz"
    assert not (tmp_path / "bad").exists() or not list((tmp_path / "bad").rglob("*.npz"))
