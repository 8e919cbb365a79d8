"""The exact oracle of tests/moments_limits_data.py against exact rational arithmetic, and the CPU-side conditions the comparisons of
tests/test_pca_limits_gpu.py and tests/test_kmeans_limits_gpu.py rest on: fmaf32 is the correctly rounded fused multiply-add (random
triples, constructed ties that a float64 a * b + c followed by a cast rounds the wrong way, whole 256-step chains), gram_oracle contains
the integer definition of tests/pca_data.py on exact rows, and the fragments' image of a unit row - emulated in numpy - is an f32 and
within q_bound of float64 on every kind of row the GPU tests harvest."""
from fractions import Fraction

import numpy as np
import pytest

from tests import moments_limits_data as md
from tests.embedding_limits_data import EXTREME_KINDS
from tests.pca_data import exact_moments, exact_rows


def round_f32(v):
    """RN32 of a Fraction in the f32 normals, ties to even, as a Fraction: integer arithmetic only"""
    if v == 0:
        return Fraction(0)
    sign, m = (-1 if v < 0 else 1), abs(v)
    e = m.numerator.bit_length() - m.denominator.bit_length()
    if Fraction(2) ** e > m:
        e -= 1
    assert Fraction(2) ** e <= m < Fraction(2) ** (e + 1) and -126 <= e < 127
    ulp = Fraction(2) ** (e - 23)
    n, rest = divmod(m, ulp)
    if rest * 2 > ulp or (rest * 2 == ulp and n % 2):
        n += 1
    return sign * n * ulp


def fma_exact(a, b, c):
    return round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def test_fmaf32_equals_rational_arithmetic_on_random_triples():
    rng = np.random.default_rng(1)
    n = 12000
    a = (rng.standard_normal(n) * np.exp2(rng.integers(-8, 9, n))).astype(np.float32)
    b = (rng.standard_normal(n) * np.exp2(rng.integers(-8, 9, n))).astype(np.float32)
    c = (rng.standard_normal(n) * np.exp2(rng.integers(-12, 20, n))).astype(np.float32)
    c[::7] = -(a[::7].astype(np.float64) * b[::7]).astype(np.float32)      # cancellation: the result is the product's own rounding error
    c[::11] = 0
    got = md.fmaf32(a, b, c)
    assert got.dtype == np.float32 and got.shape == (n,)
    want = [fma_exact(x, y, z) for x, y, z in zip(a, b, c)]
    assert all(Fraction(float(g)) == w for g, w in zip(got, want))
    assert md.fmaf32(np.float32(3), np.float32(5), np.float32(-15)) == 0 and md.fmaf32(a[:4, None], b[None, :3], c[:3]).shape == (4, 3)


def test_fmaf32_breaks_ties_by_the_remainder_where_two_roundings_go_wrong():
    """p = (8 + 2^-20)(8 - 2^-20) = 64 - 2^-40 and c = +-(2^30 + 128) or +-2^30: p + c is 2^-40 off the middle of two f32 that are 128
    apart, float64 (whose unit there is 2^-22) rounds it onto the middle, and ties-to-even then picks the f32 on the wrong side"""
    x, y = np.float32(8 + 2.0 ** -20), np.float32(8 - 2.0 ** -20)
    assert float(x) * float(y) == 64 - 2.0 ** -40
    cases, wrong, signs = [], 0, set()
    for scale in (1.0, 2.0 ** -20, 2.0 ** 40):
        for c in (2.0 ** 30 + 128, -(2.0 ** 30 + 128), 2.0 ** 30, -(2.0 ** 30), 2.0 ** 30 + 384, -(2.0 ** 30 + 384)):
            for sa in (1, -1):
                cases.append((np.float32(sa * x * np.float32(scale)), y, np.float32(c * scale)))
    for a, b, c in cases:
        exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
        s = float(a) * float(b) + float(c)
        rest = exact - Fraction(s)
        want = round_f32(exact)
        got = md.fmaf32(a, b, c)
        assert Fraction(float(got)) == want, (a, b, c)
        if rest != 0 and Fraction(float(np.float32(s))) != want:
            wrong += 1
            signs.add((rest > 0, s > 0))
    print(f"\n{len(cases)} constructed sums, {wrong} of them rounded the wrong way by float64 and a cast; (remainder > 0, sum > 0) seen: {sorted(signs)}")
    assert wrong >= 8 and len(signs) == 4                                  # a non-zero remainder of either sign, at sums of either sign


@pytest.fixture(scope="module")
def emulated():
    """the numpy emulation of the fragments on the valid harvest rows: (q, whether every hi + lo is an f32, the float64 unit rows)"""
    r, keep, where = md.harvest_rows()
    q, exact = md.fragment_image(r[keep])
    at = np.cumsum(keep) - 1                                               # a row's index among the valid ones
    return q, exact, md.unit64(r[keep]), {name: at[idx] for name, idx in where.items()}


def test_whole_chains_equal_rational_arithmetic(emulated):
    q = emulated[0][:md.GRANULE]
    G = md.gram_oracle(q)
    x = [[Fraction(float(v)) for v in row] for row in md.staged(q)[:, [0, 5, 127, 128, 300, 511]]]
    entries = ((0, 0), (0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 5), (5, 0))
    for ia, ib in entries:
        acc = Fraction(0)
        for row in x:
            acc = round_f32(row[ia] * row[ib] + acc)
        want = acc * 65536
        n, rest = divmod(want, 1)
        n += rest * 2 > 1 or (rest * 2 == 1 and n % 2 == 1)
        a, b = (0, 5, 127, 128, 300, 511)[ia], (0, 5, 127, 128, 300, 511)[ib]
        assert G[a, b] == n == G[b, a], (a, b)
    assert np.array_equal(G, G.T)


@pytest.mark.parametrize("n", (1, 31, 257))
def test_the_oracle_contains_the_integer_definition_on_exact_rows(n):
    r = exact_rows(n)
    u = md.unit64(r)
    q = np.rint(u * 2.0 ** 32)
    assert np.array_equal(q, u * 2.0 ** 32)
    wG, wS = exact_moments(r)
    assert np.array_equal(md.gram_oracle(q.astype(np.int64)), wG)
    assert np.array_equal(md.sum_oracle(q.astype(np.int64), np.zeros(n, np.int64), 1)[0], wS)


def test_a_zero_row_changes_nothing_and_granules_follow_the_absolute_index(emulated):
    q = emulated[0][:40]
    holes = np.zeros((60, 512), np.int64)
    holes[[3, 4, 10, 59]] = q[:4]
    assert np.array_equal(md.gram_oracle(holes), md.gram_oracle(q[:4]))
    moved = np.zeros((md.GRANULE + 2, 512), np.int64)                      # the same four rows, two on each side of a granule border
    moved[[254, 255, 256, 257]] = q[:4]
    assert np.array_equal(md.gram_oracle(moved), md.gram_oracle(q[:2]) + md.gram_oracle(q[2:4]))
    assert np.array_equal(md.gram_oracle(moved, 256), md.gram_oracle(q[:2]))


def test_the_fragments_image_is_an_f32_and_within_the_bound_of_float64(emulated):
    """the condition the GPU comparison of q rests on, on every kind of row that is harvested"""
    q, exact, u, where = emulated
    assert exact and q.shape == (600, 512) and np.abs(q).max() <= 2 ** 32
    err = np.abs(q / 2.0 ** 32 - u)
    bound = md.q_bound(u)
    relative = md.Q_REL * np.abs(u) >= md.Q_NORM * np.abs(u) + md.Q_ABS      # where the relative bound is the one asserted
    kinds = dict(where, planted=np.setdiff1d(np.arange(600), np.concatenate(list(where.values()))))
    assert set(where) == set(EXTREME_KINDS)
    for name, idx in kinds.items():
        ratio = (err[idx] / np.where(bound[idx] > 0, bound[idx], 1)).max()
        rel = err[idx][relative[idx]] / np.abs(u[idx][relative[idx]])
        print(f"\n{name}: max err / bound = {ratio:.3f}, max relative error where the relative bound holds = {rel.max() if len(rel) else 0:.3e}, "
              f"{(~relative[idx] & (u[idx] != 0)).mean():.3%} of the elements on the absolute bound 1.8e-7 |u| + 2^-33")
        assert (err[idx] <= bound[idx]).all(), name
    assert relative[kinds["planted"]].mean() > 0.99                        # the planted rows: the relative bound nearly everywhere
    assert (~relative[where["heavy"]] & (u[where["heavy"]] != 0)).mean() > 0.1      # heavy rows: low limbs and whole elements below the f16 normals
    one_hot = q[where["one_hot"]]
    assert ((one_hot != 0).sum(axis=1) == 1).all() and (np.abs(one_hot).max(axis=1) == 2 ** 32).all()      # x = +-256 exactly
    low = (q[kinds["planted"]] % 2 ** 13 != 0).mean()
    print(f"\nnon-zero residues q mod 2^13 on the planted rows: {low:.3%}")
    assert low >= 0.25
