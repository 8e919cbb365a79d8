"""Embedding-like rows for the neighbour tests: ReLU of a Gaussian with one power-of-two scale per channel."""
import numpy as np

DIM = 512


def rows(n, seed):
    """(n, 512) float32: max(N(0, 1), 0) * 2^U{-3..2} per channel."""
    rng = np.random.default_rng(seed)
    scale = np.exp2(rng.integers(-3, 3, DIM)).astype(np.float32)
    return (np.maximum(rng.standard_normal((n, DIM)), 0).astype(np.float32) * scale).astype(np.float32)


def sims64(query, base, metric="cosine"):
    """(nq, nb) float64 similarities of finite, non-zero rows."""
    q, b = np.asarray(query, np.float64), np.asarray(base, np.float64)
    if metric == "cosine":
        q = q / np.sqrt((q * q).sum(axis=1))[:, None]
        b = b / np.sqrt((b * b).sum(axis=1))[:, None]
    return q @ b.T
