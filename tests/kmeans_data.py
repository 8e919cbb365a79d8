"""Rows with planted families for the k-means tests, the definition's answers on them (computed once per process and shared by the host
and the GPU tests), and a plain-loop group sum that shares no code with sequence.group_centroids."""
import functools

import numpy as np

N = 333                                          # six 64-row tiles, off every boundary
SIZES = (60, 55, 50, 47, 43, 40, 36)             # 331 rows in seven families, then a zero row and a row with one NaN
KS = (7, 33, 300)                                # below a 32-column block, across one, across the 256-column step
SPREAD = 0.8
SEED = 7


@functools.lru_cache(maxsize=None)
def _planted(seed):
    """(333, 512) float32 and the family of every row (int64, -1 for the two invalid rows).  A family is centre + 0.8 * noise around
    a unit centre of its own, the noise Gaussian of norm about 1: a member has cosine about 0.78 to its centre, about 0.61 to its
    siblings and about 0 +- 0.04 to the members of an orthogonal family.  The centres of families 0 and 1 have cosine 0.5, those of 2
    and 3 cosine 0.7; the others are orthogonal to everything.
    Every row is scaled by a power of two of its own (cosine does not see it), then all are scattered by a fixed permutation."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((512, len(SIZES))))
    q = q.T.copy()
    q[1] = 0.5 * q[0] + np.sqrt(1 - 0.5 ** 2) * q[1]          # families 0 and 1, 2 and 3 lean towards each other
    q[3] = 0.7 * q[2] + np.sqrt(1 - 0.7 ** 2) * q[3]
    parts, family = [], []
    for f, m in enumerate(SIZES):
        noise = rng.standard_normal((m, 512)) / np.sqrt(512)
        parts.append(q[f] + SPREAD * noise)
        family += [f] * m
    r = np.concatenate(parts + [np.zeros((2, 512))])
    family = np.asarray(family + [-1, -1], dtype=np.int64)
    r = (r * np.exp2(rng.integers(-3, 4, (N, 1)))).astype(np.float32)
    r[N - 1] = rng.standard_normal(512).astype(np.float32)
    r[N - 1, 77] = np.nan
    perm = rng.permutation(N)
    r, family = np.ascontiguousarray(r[perm]), family[perm]
    r.setflags(write=False)
    family.setflags(write=False)
    return r, family


def planted(seed=SEED):
    """the planted rows and their families, built once and read-only"""
    return _planted(seed)


INITS = ("farthest", "first")                    # the farthest-first traversal; the first k valid rows (a poor init: several updates)


def init_rows(kind, k):
    """the ``init`` argument of a case: None, or the first k valid planted rows"""
    r, family = planted()
    return None if kind == "farthest" else np.ascontiguousarray(r[np.flatnonzero(family >= 0)[:k]])


@functools.lru_cache(maxsize=None)
def defined(k, kind="farthest", max_iter=50):
    """(the definition's seven values on the planted rows, its trace): computed once, never changed by a test"""
    from genomad_amd import sequence
    trace = []
    out = sequence.spherical_kmeans(planted()[0], k, init_rows(kind, k), max_iter, trace=trace)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out, trace


def unit64(rows):
    """the float64 unit vectors of valid float32 rows"""
    r = np.asarray(rows, np.float64)
    return r / np.sqrt((r * r).sum(axis=1))[:, None]


def loop_centroids(rows, label, k):
    """(centroids float64 (k, 512), size) by a plain loop over the rows: row by row into its group's sum, then one division"""
    rows = np.asarray(rows, np.float32)
    total = np.zeros((k, 512))
    size = np.zeros(k, np.int64)
    for i in range(len(rows)):
        x = rows[i].astype(np.float64)
        if label[i] < 0 or not np.isfinite(x).all() or not (x != 0).any():
            continue
        total[label[i]] += x / np.sqrt((x * x).sum())
        size[label[i]] += 1
    for c in range(k):
        norm = np.sqrt((total[c] * total[c]).sum())
        total[c] = total[c] / norm if size[c] and norm > 0 else 0
    return total, size


def resultant(rows, label, k):
    """per group: |sum of the members' unit rows| / members (1 for a group of one direction, 0 for one that cancels); NaN for an
    empty group"""
    out = np.full(k, np.nan)
    ok = np.isfinite(rows).all(axis=1) & (rows != 0).any(axis=1)
    for c in range(k):
        m = np.flatnonzero(ok & (label == c))
        if len(m):
            out[c] = np.sqrt((unit64(rows[m]).sum(axis=0) ** 2).sum()) / len(m)
    return out


def signed_rows(n=333, seed=21, scaled=True):
    """rows whose similarity to every row of :func:`signed_init` is negative: -(a common direction) plus a little noise; ``scaled``:
    every row times a power of two of its own from 2^-100 to 2^100 (1e-30 to 1e30; exact, so cosine cannot see it)"""
    rng = np.random.default_rng(seed)
    d = np.abs(rng.standard_normal(512)) + 0.5
    r = -(d + 0.3 * rng.standard_normal((n, 512))).astype(np.float32)
    scale = np.exp2(rng.integers(-100, 101, (n, 1))).astype(np.float32)
    return r * scale if scaled else r


def signed_init(k, seed=22):
    rng = np.random.default_rng(seed)
    d = np.abs(np.random.default_rng(21).standard_normal(512)) + 0.5          # the direction of signed_rows
    return (d + 0.3 * rng.standard_normal((k, 512))).astype(np.float32)
