"""Rows for the principal-component tests, built once per process and read-only: rows whose moments are exact in f32 with the integer
definition of the moments on them, planted h1-like rows (non-negative families plus noise, half of them sign-flipped), a planted
spectrum (a rank-5 signal with well-separated eigenvalues plus small noise), and plain loops that share no code with
sequence.pca_moments / pca_project."""
import functools

import numpy as np

EXACT_NS = (1, 31, 255, 256, 257, 513, 1000)     # below a granule of 256 rows, at it, one beyond, two granules and one row, four
EXACT_COUNTS = (1, 4, 16, 64, 256)               # non-zero entries of a row: its unit entries are 2^0 ... 2^-4
SPECTRUM_N = 1000
SPECTRUM_RANK = 5
SPECTRUM_SIGMA = (1.0, 0.7, 0.5, 0.35, 0.25)     # the signal's standard deviations: eigenvalue ratios of about 2
SPECTRUM_NOISE = 0.02                            # the noise's norm per row, against a signal of norm about 1.4


@functools.lru_cache(maxsize=None)
def exact_rows(n, seed=5):
    """(n, 512) float32: row i has EXACT_COUNTS[i % 5] non-zero entries of one magnitude and random signs, times a power of two of
    its own in 2^-20 ... 2^20.  The 256-entry rows have 64 entries in each of the four 128-feature blocks, so all 10 block pairs of
    the Gram matrix carry non-zeros.  The unit entries are 2^0 ... 2^-4: the fragments' low limbs are zero, and every product
    (2^16 ... 2^8 in the kernel's units) and every partial sum of up to 256 of them (a multiple of 2^8 below 2^25) is exact in f32."""
    rng = np.random.default_rng(seed + n)
    r = np.zeros((n, 512), np.float32)
    for i in range(n):
        m = EXACT_COUNTS[i % len(EXACT_COUNTS)]
        if m == 256:
            where = np.concatenate([b * 128 + rng.choice(128, 64, replace=False) for b in range(4)])
        else:
            where = rng.choice(512, m, replace=False)
        r[i, where] = rng.choice([-1.0, 1.0], m) * np.exp2(rng.integers(-20, 21))
    r.setflags(write=False)
    return r


def exact_moments(r):
    """the integer definition on exact rows: q = unit * 2^32 (every q is a multiple of 2^28 here), G = QT Q >> 32 and S = sum q, int64"""
    u = r.astype(np.float64)
    u /= np.sqrt((u * u).sum(axis=1))[:, None]
    q = np.rint(u * 2.0 ** 32)
    assert np.array_equal(q, u * 2.0 ** 32) and not (q % 2 ** 28).any()          # the unit entries are powers of two down to 2^-4
    q = q.astype(np.int64)
    h = q >> 16                                                                  # exact: QT Q >> 32 = (Q >> 16)T (Q >> 16)
    return h.T @ h, q.sum(axis=0)


@functools.lru_cache(maxsize=None)
def planted_rows(n=700, seed=11):
    """(n, 512) float32, h1-like: six non-negative family directions, a row = its family's direction + 0.6 * non-negative noise,
    every second row sign-flipped.  No row is invalid and no unit entry is a power of two: the products are not exact."""
    rng = np.random.default_rng(seed)
    centre = np.abs(rng.standard_normal((6, 512)))
    r = centre[rng.integers(0, 6, n)] + 0.6 * np.abs(rng.standard_normal((n, 512)))
    r[1::2] *= -1
    r = r.astype(np.float32)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def spectrum_rows(seed=13):
    """((1000, 512) float32, the planted orthonormal basis (5, 512) float64): z_i . diag(sigma) . basis + noise, z Gaussian.  The
    rows' unit vectors keep their variance in the planted subspace - normalising a row scales it, it does not turn it - with
    eigenvalues in the order of the sigmas, and the noise leaves each of the other 507 directions 4e-4 / 512 of a row's energy."""
    rng = np.random.default_rng(seed)
    basis, _ = np.linalg.qr(rng.standard_normal((512, SPECTRUM_RANK)))
    basis = basis.T.copy()
    z = rng.standard_normal((SPECTRUM_N, SPECTRUM_RANK)) * np.asarray(SPECTRUM_SIGMA)
    r = (z @ basis + SPECTRUM_NOISE * rng.standard_normal((SPECTRUM_N, 512)) / np.sqrt(512)).astype(np.float32)
    r.setflags(write=False)
    basis.setflags(write=False)
    return r, basis


def with_invalid(r, where, seed=3):
    """(a copy of ``r`` with zero, NaN and Inf rows inserted so that they stand at the indices ``where`` of the result, the mask of
    the original rows in it)"""
    rng = np.random.default_rng(seed)
    n = len(r) + len(where)
    keep = np.ones(n, bool)
    keep[list(where)] = False
    out = np.empty((n, 512), np.float32)
    out[keep] = r
    for j, i in enumerate(where):
        out[i] = 0 if j % 3 == 0 else rng.standard_normal(512)
        if j % 3 == 1:
            out[i, rng.integers(512)] = np.nan
        if j % 3 == 2:
            out[i, rng.integers(512)] = np.inf if j % 2 else -np.inf
    return out, keep


def valid_loop(r):
    return np.asarray([bool(np.isfinite(x).all() and (x != 0).any()) for x in np.asarray(r, np.float32)])


def loop_moments(r):
    """(G, S, n_valid) in float64 by a plain loop over the rows"""
    G, S, n_valid = np.zeros((512, 512)), np.zeros(512), 0
    for x, ok in zip(np.asarray(r, np.float32), valid_loop(r)):
        if not ok:
            continue
        u = x.astype(np.float64)
        u /= np.sqrt((u * u).sum())
        G += np.outer(u, u)
        S += u
        n_valid += 1
    return G, S, n_valid


def loop_project(r, comp, mean=None):
    """float64 (n, c) by a plain loop over rows and components; NaN for an invalid row"""
    comp = np.asarray(comp, np.float32).astype(np.float64)
    out = np.full((len(r), len(comp)), np.nan)
    for i, (x, ok) in enumerate(zip(np.asarray(r, np.float32), valid_loop(r))):
        if not ok:
            continue
        u = x.astype(np.float64)
        u /= np.sqrt((u * u).sum())
        for c, v in enumerate(comp):
            v = v / np.sqrt((v * v).sum())
            out[i, c] = (u * v).sum() - (0.0 if mean is None else (np.asarray(mean, np.float64) * v).sum())
    return out


def subspace_residual(found, basis):
    """the sine of the largest principal angle between the row spaces of ``found`` and ``basis`` (both with orthonormal rows, of one
    rank): the 2-norm of the part of ``found`` outside ``basis``"""
    found, basis = np.asarray(found, np.float64), np.asarray(basis, np.float64)
    return float(np.linalg.norm(found - (found @ basis.T) @ basis, 2))
