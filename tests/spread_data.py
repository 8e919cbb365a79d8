"""Graphs, seeds and labels for the label-spreading tests (tests/test_spread_host.py, tests/test_spread_gpu.py): the graphs of
tests/mcl_data.py and a few of their own, each with the rows' validity and a rule that labels some rows for any number of classes.
Built once and never written to."""
import numpy as np

from tests.mcl_data import CLIQUE, PATH, PLANTED, PLANTED_SIZES, RANDOM, csr_of_edges, fan

PLANTED_START = np.cumsum((0,) + PLANTED_SIZES)
PLANTED_SEEDED = (0, 1, 3, 4, 5)                      # the groups that hold seeds: five of the eight; 2 is a clique between two seeded ones
STAR_LEAVES = 70000
LONG_ROW = 1024                                       # gnn_spread.hip: a row of more entries is a workgroup's work


def n_of(csr):
    return len(csr[0]) - 1


def planted_labels(n_classes=5):
    """two seeds in each group of PLANTED_SEEDED (its first and its last row; a group of one row: that row), of class (the group's
    place in PLANTED_SEEDED) % n_classes"""
    label = np.full(n_of(PLANTED), -1, dtype=np.int64)
    for k, g in enumerate(PLANTED_SEEDED):
        label[[PLANTED_START[g], PLANTED_START[g + 1] - 1]] = k % n_classes
    return label


def scattered_labels(n, n_classes, every=7, seed=5):
    """about one row in ``every`` labelled, with a class drawn from all of them"""
    rng = np.random.default_rng(seed)
    label = np.full(n, -1, dtype=np.int64)
    rows = np.flatnonzero(rng.integers(0, every, n) == 0)
    label[rows] = rng.integers(0, n_classes, len(rows))
    return label


def star(leaves, sim=1.0):
    """node 0 joined to ``leaves`` leaves by entries of one similarity"""
    return (np.concatenate([[0], np.full(leaves + 1, leaves)]).astype(np.int64), np.arange(1, leaves + 1, dtype=np.int32),
            np.full(leaves, sim, dtype=np.float32))


def star_labels(leaves, n_classes=1):
    """every leaf a seed of the last class, the hub unlabelled"""
    return np.concatenate([[-1], np.full(leaves, n_classes - 1)]).astype(np.int64)


STAR = star(STAR_LEAVES)                              # the hub's sum reaches 70000 * floor(2^31 / 70000) * 2^30, just under 2^61
STAR_AT = star(LONG_ROW)                              # the longest row a wave takes
STAR_OVER = star(LONG_ROW + 1)                        # the shortest a workgroup takes
FAN = fan(3, (5, 70, 200))[:3]

# parallel entries (rows 0 and 1 list a partner twice, with different weights), similarities that round to q = 0 (1e-9, and a
# negative one) and a row (5) whose only entry does not exist: 7 rows
PARALLEL = (np.array([0, 4, 7, 8, 9, 9, 10, 10], dtype=np.int64), np.array([1, 1, 2, 3, 2, 3, 3, 4, 4, 6], dtype=np.int32),
            np.array([0.5, 0.25, 1e-9, 0.75, 0.6, 0.6, -0.3, 0.9, 0.33, 2e-8], dtype=np.float32))
PARALLEL_LABELS = np.array([0, -1, -1, -1, 1, 1, 0], dtype=np.int64)

RANDOM_VALID = np.arange(n_of(RANDOM)) % 9 != 4       # every ninth row takes no part - some of them carry a label


def cases(n_classes):
    """name -> (csr, valid or None, label) for ``n_classes`` classes: every fixture but the large star"""
    from tests.mcl_limits_data import heavy, ranged      # that module takes star() and PARALLEL from this one
    c = n_classes
    return {
        "planted": (PLANTED, None, planted_labels(c)),
        "random": (RANDOM, None, scattered_labels(n_of(RANDOM), c)),
        "random_masked": (RANDOM, RANDOM_VALID, scattered_labels(n_of(RANDOM), c, every=5, seed=6)),
        "path": (PATH, None, np.concatenate([[c - 1], np.full(n_of(PATH) - 1, -1)]).astype(np.int64)),
        "clique": (CLIQUE, None, scattered_labels(n_of(CLIQUE), c, every=10, seed=8)),
        "fan": (FAN, None, scattered_labels(n_of(FAN), c, every=6, seed=9)),
        "parallel": (PARALLEL, None, np.minimum(PARALLEL_LABELS, c - 1)),
        "star_at": (STAR_AT, None, star_labels(LONG_ROW, c)),
        "star_over": (STAR_OVER, None, star_labels(LONG_ROW + 1, c)),
        "heavy": (heavy(), None, planted_labels(c)),
        "ranged": (ranged(), None, planted_labels(c)),
    }
