"""The CPU-side conditions tests/test_kmeans_limits_gpu.py rests on: the group sums and the centroid of tests/moments_limits_data.py
against a plain float64 loop, the distance in f32 units it counts with, the planted labels of the two-range input (every copy is
recoverable: nothing else comes near its source), the margins of the definition where the iteration is stopped one update early and
exactly at its end, and the sizes the launch-shape input promises."""
import numpy as np
import pytest

from tests import moments_limits_data as md
from tests.embedding_limits_data import SPLIT_MAX
from tests.kmeans_data import defined, loop_centroids, resultant
from tests.pca_data import planted_rows


def test_the_sums_and_the_centroid_against_a_plain_loop():
    r, keep, _ = md.harvest_rows()
    q = np.zeros((len(r), 512), np.int64)
    q[keep] = md.fragment_image(r[keep])[0]
    for k in (7, 33):
        label = np.where(np.arange(len(r)) % 10 == 3, -1, np.arange(len(r)) % k)
        S = md.sum_oracle(q, label, k + 1)                                 # the last group is empty
        assert S.dtype == np.int64 and not S[k].any() and np.array_equal(S.sum(axis=0), q[label >= 0].sum(axis=0))
        cent = md.centroid_oracle(S)
        want, size = loop_centroids(r, label, k + 1)
        assert cent.dtype == np.float32 and not cent[k].any() and size[k] == 0
        # the bound of tests/test_kmeans_gpu.py with the groups' own resultant: 4.2e-7 m / |S| and one f32 rounding
        assert np.abs(cent.astype(np.float64) - want).max() <= 4.2e-7 / np.nanmin(resultant(r, label, k + 1)) + 6e-8


def test_the_distance_counts_f32_values():
    one = np.float32(1)
    up, down = np.nextafter(one, np.float32(2)), np.nextafter(one, np.float32(0))
    tiny = np.float32(1e-45)
    a = np.array([one, one, one, 0.0, -0.0, tiny, -one], np.float32)
    b = np.array([one, up, down, -0.0, tiny, -tiny, np.nextafter(-one, np.float32(-2))], np.float32)
    assert list(md.ulp_distance(a, b)) == [0, 1, 1, 0, 1, 2, 1]


def test_every_planted_label_of_the_two_range_input_is_recoverable():
    r, source = md.range_rows()
    assert r.shape == (md.RANGE_N, 512) and md.RANGE_K == 65535 > SPLIT_MAX and np.array_equal(source[:md.RANGE_K], np.arange(md.RANGE_K))
    copies = np.arange(md.RANGE_K, md.RANGE_N)
    assert set(source[copies]) == set(md.RANGE_SOURCES) and min(np.bincount(source[copies])[list(md.RANGE_SOURCES)]) >= 8
    sample = np.unique(np.concatenate([np.random.default_rng(3).choice(md.RANGE_K, 2100, replace=False), md.RANGE_SOURCES]))
    u = md.unit64(r[sample])
    c = u @ u.T
    np.fill_diagonal(c, 0)
    print(f"\n{len(sample)} sampled rows: the largest cosine between two of them is {np.abs(c).max():.3f}")
    assert len(sample) >= 2000 and np.abs(c).max() < 0.5
    own = (md.unit64(r[copies]) * md.unit64(r[source[copies]])).sum(axis=1)
    assert np.abs(own - 1).max() <= 1e-6
    ratio = np.abs(r[copies]).max(axis=1) / np.abs(r[source[copies]]).max(axis=1)
    assert np.array_equal(np.exp2(np.round(np.log2(ratio))), ratio) and ratio.min() >= 2.0 ** -20 and ratio.max() <= 2.0 ** 20


@pytest.mark.parametrize("k", (7, 33))
def test_the_margins_where_the_iteration_is_stopped_early_and_at_its_end(k):
    """best and second-best centroid keep 1e-4 apart at every assignment of the runs the GPU test compares exactly; stopped one update
    early the definition has not converged, stopped at ``it`` it has, after the same number of updates"""
    it = defined(k, "first")[0][4]
    assert it >= 1 and defined(k, "first")[0][5]                           # k = 33: one update, so the early stop is max_iter = 0
    for max_iter, converged in ((it - 1, False), (it, True)):
        out, trace = defined(k, "first", max_iter)
        assert out[4] == max_iter and out[5] == converged and len(trace) == max_iter + 1
        assert min(t["gap"] for t in trace) >= 1e-4
    assert np.array_equal(defined(k, "first", it)[0][0], defined(k, "first")[0][0])


def test_the_launch_shape_input_at_256_compute_units():
    cus = 256
    r, keep = md.launch_rows(cus)
    n = len(r)
    assert n == 33869 == md.launch_n(cus) and n > 64 * 2 * cus and -(-n // 256) > -(-2 * cus // 10)
    assert not keep[[0, 1, 2, n - 2, n - 1]].any() and keep.sum() == n - 5
    p = planted_rows()
    idx = np.flatnonzero(keep)[:2000]
    c = (md.unit64(r[idx]) * md.unit64(p[idx % len(p)])).sum(axis=1)
    assert np.abs(np.abs(c) - 1).max() <= 1e-12 and 0.4 < (c < 0).mean() < 0.6      # the same directions, half of them negated


def test_the_axis_rows():
    r, sign = md.axis_rows(300, 212)
    assert r.shape == (512, 512) and (sign == 1).sum() == 300 and sign[0] == 1 and ((r != 0).sum(axis=1) == 1).all()
    assert np.array_equal(np.sign(r[:, 7]), sign) and np.isfinite(r).all()
    assert np.abs(r[:, 7].astype(np.float64)).max() / np.abs(r[:, 7].astype(np.float64)).min() > 2.0 ** 100
