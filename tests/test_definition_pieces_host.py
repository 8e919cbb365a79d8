"""The pieces the numpy definitions of the embedding analyses share (sequence._row_rule, the union-find _find / _join /
_root_labels, _namer): the rule each one states, asserted on its own.  The public definitions are tested through them by the
files of every analysis.  No GPU."""
import numpy as np
import pytest

from genomad_amd import sequence


def corner_rows():
    """(rows float32 (9, 512), what each row is): the corners of the row rule"""
    rng = np.random.default_rng(5)
    r = np.zeros((9, 512), dtype=np.float32)
    r[0] = rng.standard_normal(512)
    r[1] = r[0]                                          # identical to row 0
    r[2] = -r[0]                                         # equal to row 0 up to sign
    r[3] = r[0]
    r[3, 300] = np.nan
    r[4] = r[0]
    r[4, 511] = -np.inf
    r[5] = 0.0
    r[6] = -0.0
    r[7] = np.float32(1e-40)                             # denormals only
    r[7, ::2] = -np.float32(1.4e-45)
    r[8] = r[0] * np.float32(1e20)
    return r, ("plain", "same", "negated", "nan", "inf", "zero", "minus zero", "denormal", "large")


@pytest.mark.parametrize("metric", sequence.NEIGHBOUR_METRICS)
def test_row_rule_validity_and_exact_zeros(metric):
    r32, what = corner_rows()
    r, ok = sequence._row_rule(r32, metric)
    assert r.dtype == np.float64 and r.shape == r32.shape and ok.dtype == np.bool_
    zero_is_valid = metric == "dot"
    want = {"plain": True, "same": True, "negated": True, "nan": False, "inf": False, "zero": zero_is_valid,
            "minus zero": zero_is_valid, "denormal": True, "large": True}
    assert ok.tolist() == [want[w] for w in what]
    assert np.array_equal(ok, sequence.valid_rows(r32, metric))
    assert not r[~ok].any() and np.isfinite(r).all()             # an invalid row comes back as exact zeros
    assert not np.signbit(r[3]).any() and not np.signbit(r[4]).any()
    assert np.array_equal(r[0], r[1]) and np.array_equal(r[2], -r[0])
    if metric == "cosine":
        # float64 unit vectors: 512 squares, their pairwise sum, a root and a division are each within a few 2^-53
        assert np.abs(np.sqrt((r[ok] * r[ok]).sum(axis=1)) - 1.0).max() <= 2.0 ** -48
        assert np.abs(r[8] - r[0]).max() <= 2.0 ** -22            # the scale is gone, up to the float32 rounding of the scaled row
    else:
        assert np.array_equal(r[ok], r32[ok].astype(np.float64))  # dot: the rows themselves
        assert np.signbit(r[6]).all()


def test_row_rule_of_no_rows():
    for metric in sequence.NEIGHBOUR_METRICS:
        r, ok = sequence._row_rule(np.zeros((0, 512), np.float32), metric)
        assert r.shape == (0, 512) and ok.shape == (0,)


def test_metric_validator():
    assert [sequence.neighbour_metric(m) for m in ("cosine", "dot")] == ["cosine", "dot"]
    with pytest.raises(ValueError, match=r"metric 'l2': expected one of \('cosine', 'dot'\)"):
        sequence.neighbour_metric("l2")


def test_union_find_labels_a_chain_given_deepest_first():
    # 0 - 1 - 2 - 3 - 4 - 5, the edges from the far end: every join hangs the root so far under a new, smaller one, so before any
    # halving the path from 5 runs through every node
    root = list(range(6))
    for x, y in ((4, 5), (3, 4), (2, 3), (1, 2), (0, 1)):
        assert sequence._join(root, x, y)
    assert root == [0, 0, 1, 2, 3, 4]
    assert not sequence._join(root, 5, 0)                         # one component: nothing to join
    valid = np.array([1, 1, 1, 0, 1, 1], dtype=bool)
    label = sequence._root_labels(root, valid)
    assert label.dtype == np.int64 and label.tolist() == [0, 0, 0, -1, 0, 0]
    assert all(sequence._find(root, i) == 0 for i in range(6))


def test_union_find_keeps_components_apart_and_takes_any_keys():
    root = list(range(6))
    for x, y in ((5, 3), (1, 4), (3, 2)):
        sequence._join(root, x, y)
    assert sequence._root_labels(root, np.ones(6, bool)).tolist() == [0, 1, 2, 2, 1, 2]
    keyed = {k: k for k in (7, 30, 11)}
    assert sequence._join(keyed, 30, 11) and sequence._find(keyed, 30) == 11 and sequence._find(keyed, 7) == 7
    assert sequence._root_labels([], np.zeros(0, bool)).shape == (0,)


@pytest.mark.parametrize("names", [None, ["a", "b", "c"], np.array(["a", "b", "c"])], ids=["none", "list", "array"])
def test_namer(names):
    name = sequence._namer(names)
    for i in (0, np.int64(2), np.int32(1)):
        got = name(i)
        if names is None:
            assert type(got) is int and got == int(i)
        else:
            assert type(got) is str and got == "abc"[int(i)]
