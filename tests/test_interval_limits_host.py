"""The inputs of tests/test_interval_limits_gpu.py, on the CPU: every generator of tests/interval_limits_data.py is run (their
conditions are assertions inside them, the rest is asserted here), the two references - the sequential definition and the cosine
matrix - are held against each other, poison in rows that no sum may see changes nothing in the definition, the coherence tolerance
is shown to be small beside what one wrong member costs, and a float32 emulation of the kernel's arithmetic is shown to lie inside
the tolerance on every fixture.  The device is not touched: a failure here is a failure of a test input, not of a kernel."""
import numpy as np
import pytest

from tests import interval_limits_data as lim

AGREE = 1e-12


def _all_fixtures():
    """(name, fixture, rows_rev) of everything the GPU tests fold"""
    out = [("cuts", lim.cuts(), None), ("poisoned", lim.poisoned(lim.cuts()), None), ("poison_free", lim.poison_free(lim.cuts()), None),
           ("scaled", lim.scaled(), None)]
    out += [(f"long_{kind}_{n}_{int(thirds)}", fx, None) for kind, n, thirds, fx in lim.long_ranges()]
    for kind in lim.BOTH_KINDS:
        fx = lim.both_strands(kind)
        out.append((f"both_{kind}", fx, fx["rows_rev"]))
    return out


@pytest.fixture(scope="module")
def fixtures():
    return [(name, fx, rev, lim.definition(fx, rev)) for name, fx, rev in _all_fixtures()]


def test_the_tolerance_is_the_derived_one():
    assert lim.coh_tol(64) == (64 + 35) * 2.0 ** -24 < 1e-5                       # inside the fixed bound of tests/test_intervals_gpu.py
    assert lim.coh_tol(2000) == 2035 * 2.0 ** -24 and abs(lim.coh_tol(2000) - 1.2e-4) < 2e-6
    assert lim.coh_tol(10, 2) - lim.coh_tol(10) == 2 * 2.0 ** -24                 # one more rounding of a vector of length <= 2 n
    assert lim.coh_tol(1) == 36 * 2.0 ** -24


def test_cuts_and_empty_runs():
    fx = lim.cuts()
    length = fx["w_hi"] - fx["w_lo"]
    assert list(length) == list(range(26)) and fx["rows"].shape == (325, 512) and fx["scores"].shape == (325, 3)
    assert sorted(set((fx["w_lo"] % 8).tolist())) == list(range(8))
    # at 8-row slices a range ends at a slab's first row and the next begins there (120, 136); at 1-row slices every one does
    assert {120, 136} <= set(fx["w_hi"].tolist()) & set(fx["w_lo"].tolist()) and 120 % 8 == 136 % 8 == 0
    _, ex = np.frexp(np.abs(fx["rows"]).max(axis=1))
    assert ex.min() >= -2 and ex.max() <= 6 and (fx["rows"] < 0).mean() > 0.45
    want = lim.definition(fx)
    assert want["count"][lim.ALL_MASKED] == 0 and want["count"][lim.ALL_KEPT] == 20 and want["count"][0] == 0
    assert (want["count"] <= length).all() and int(want["count"].sum()) == int(fx["kept"].sum())
    wide = lim.with_empty_runs(fx)
    assert len(wide["w_lo"]) == 4096 and wide["rows"] is fx["rows"]
    got = lim.definition(wide)
    for k in lim.KEYS:                                               # the scattered definition of cuts, exact zeros everywhere else
        assert np.array_equal(got[k][wide["index"]], want[k]), k
        rest = np.delete(got[k], wide["index"], axis=0)
        assert len(rest) == 4096 - 26 and not rest.any(), k
    edges = set(range(0, 326, 8)) | {325}
    assert set(lim.EMPTY_RUN_AT) <= edges & (set(fx["w_hi"].tolist()) | {0})


def test_poison_changes_nothing_in_the_definition():
    fx = lim.cuts()
    bad, clean = lim.poisoned(fx), lim.poison_free(fx)
    assert np.array_equal(bad["poison"], clean["poison"]) and np.array_equal(bad["w_lo"], clean["w_lo"])
    assert len(bad["rows"]) > 325 and bad["poison"][-1] and len(bad["both_sides"]) >= 4
    assert not clean["rows"][clean["poison"]].any() and not clean["scores"][clean["poison"]].any()
    assert np.array_equal(bad["rows"][~bad["poison"]], clean["rows"][~clean["poison"]])
    for i in range(lim.N_RANGES):                                    # every masked row of a range holds poison, no kept one does
        a, b = int(bad["w_lo"][i]), int(bad["w_hi"][i])
        assert np.array_equal(bad["poison"][a:b], ~bad["kept"][a:b])
        assert np.isfinite(bad["rows"][a:b][bad["kept"][a:b]]).all()
    got, want = lim.definition(bad), lim.definition(clean)
    for k in ("count", "embedding", "scores"):
        assert np.array_equal(got[k], want[k]), k
    assert np.abs(got["coherence"] - want["coherence"]).max() <= AGREE
    assert all(np.isfinite(got[k]).all() for k in lim.KEYS)
    assert np.array_equal(got["count"], lim.definition(fx)["count"])


def test_long_ranges_and_scales_are_what_they_say():
    cases = lim.long_ranges()
    assert [(kind, n, thirds) for kind, n, thirds, _ in cases] == [(k, n, t) for k in lim.LONG_KINDS for n, t in lim.LONG]
    for kind, n, thirds, fx in cases:
        assert fx["rows"].shape == (n, 512) and int(fx["kept"].sum()) == (n - n // 3 if thirds else n)
        assert (fx["rows"] >= 0).all() == (kind == "relu")
    fx = lim.scaled()
    band = lambda name: np.frexp(np.abs(fx["rows"][fx["w_lo"][lim.interval(fx, name)]:fx["w_hi"][lim.interval(fx, name)]]).max(axis=1))[1]  # noqa: E731
    assert set(band("huge").tolist()) == {127, 128} and (band("subnormal") <= -126 - 1).all()
    assert list(band("five_scales")) == [e + 1 for e in lim.FIVE_SCALES]
    assert np.isfinite(fx["rows"]).all() and len(fx["names"]) == 2 * (2 + 1 + 3 + 16)
    want = lim.definition(fx)
    coh = lambda name: want["coherence"][lim.interval(fx, name)]    # noqa: E731
    assert abs(coh("five_scales") - 1) < 1e-3 and abs(coh("five_scales/twin") - coh("five_scales")) <= AGREE
    for a, b in lim.OPPOSITE:
        assert coh(f"opposite_{a}_{b}") <= AGREE and coh(f"opposite_{a}_{b}/twin") <= AGREE
    for k in lim.ONE_HOT_K:
        assert abs(coh(f"one_hot_{k}_+") - 1) <= AGREE and abs(coh(f"one_hot_{k}_-") - 1) <= AGREE
    for name, twin in fx["twin_of"].items():                         # a power of two changes no direction
        assert abs(coh(name) - coh(twin)) <= AGREE, name
    assert not np.isfinite(want["embedding"][lim.interval(fx, "huge")]).all()        # S overflows there, as the sequential sum has it
    assert want["embedding"][lim.interval(fx, "subnormal")].any()


def test_the_two_references_agree(fixtures):
    worst = 0.0
    for name, fx, rev, want in fixtures:
        for i in np.flatnonzero(want["count"] > 0):
            d = abs(lim.coherence_gram(fx["rows"], lim.members_of(fx, i), rev) - want["coherence"][i])
            worst = max(worst, d)
            assert d <= AGREE, (name, i, d)
    print(f"\nmax |definition - cosine matrix| = {worst:.2e}")


def _without(rows, members, drop):
    """the definition's coherence with member ``drop`` zeroed in U only, in float64"""
    x = rows[members].astype(np.float64)
    x = x / np.abs(x).max(axis=1, keepdims=True)
    u = x / np.sqrt(np.square(x).sum(axis=1, keepdims=True))
    u[drop] = 0.0
    return float(np.sqrt(np.square(u.sum(axis=0)).sum()) / len(members))


def test_one_wrong_member_moves_the_coherence_by_three_tolerances():
    """so that the tolerance cannot hide a member whose unit row was lost: the move is about coherence / n on the clustered rows"""
    print()
    for kind, n, thirds, fx in lim.long_ranges():
        if kind != "clustered" or n < 1000 or thirds:
            continue
        members = lim.members_of(fx, 0)
        full = lim.coherence_gram(fx["rows"], members)
        for drop in (0, n // 2, n - 1):
            move = abs(_without(fx["rows"], members, drop) - full)
            print(f"clustered n = {n}, member {drop}: move {move:.3e} = {move / lim.coh_tol(n):.1f} x coh_tol({n}) = {lim.coh_tol(n):.3e}")
            assert move >= 3 * lim.coh_tol(n) and abs(move - 0.9986 / n) < 0.01 / n
    fx = lim.scaled()
    for name in ["five_scales"] + [f"opposite_{a}_{b}" for a, b in lim.OPPOSITE]:
        members = lim.members_of(fx, lim.interval(fx, name))
        full = lim.coherence_gram(fx["rows"], members)
        for drop in range(len(members)):
            move = abs(_without(fx["rows"], members, drop) - full)
            print(f"{name}, member {drop}: move {move:.3f} = {move / lim.coh_tol(len(members)):.0f} x coh_tol")
            assert move >= 3 * lim.coh_tol(len(members))


# ---- the kernel's arithmetic in float32 -----------------------------------------------------------------------------------------
F32 = np.float32
PLAIN_MIN = F32(2.0 ** -116)          # IV_PLAIN_MIN of gnn_intervals.hip


def _norm2(v):
    """(m, 512) float32 -> (m,) float32, the reduction of the kernel: lane t holds elements 4 t .. 4 t + 3 and sums its squares as
    ((x^2 + y^2) + z^2) + w^2, a xor butterfly over the 64 lanes of each wave (offsets 1 .. 32), wave 0's part + wave 1's"""
    q = v.reshape(len(v), 128, 4)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        p = q * q
        ss = (((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3]).reshape(len(v), 2, 64)
        lanes = np.arange(64)
        for off in (1, 2, 4, 8, 16, 32):
            ss = ss + ss[..., lanes ^ off]
        assert (ss == ss[..., :1]).all() or not np.isfinite(ss).all()       # every lane holds the same bits
        return (ss[:, 0, 0] + ss[:, 1, 0]).astype(F32)


def _rsqrt(n2):
    with np.errstate(divide="ignore", invalid="ignore"):
        return (1.0 / np.sqrt(n2.astype(np.float64))).astype(F32)


def _unit_rows(rows):
    """(m, 512) float32 unit rows as interval_fold_kernel forms them, zero rows for the invalid"""
    rows = np.ascontiguousarray(rows, dtype=F32)
    n2 = _norm2(rows)
    with np.errstate(invalid="ignore"):
        plain = (n2 >= PLAIN_MIN) & (n2 <= F32(lim.FLT_MAX))
    w, r = rows.copy(), _rsqrt(n2)
    slow = ~plain & lim.valid_rows(rows)
    if slow.any():
        _, ex = np.frexp(np.abs(rows[slow]).max(axis=1))
        w[slow] = np.ldexp(rows[slow], -ex[:, None]).astype(F32)
        assert (np.abs(w[slow]).max(axis=1) >= 0.5).all() and (np.abs(w[slow]) < 1).all()
        r[slow] = _rsqrt(_norm2(w[slow]))
    ok = plain | slow
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        u = (w * r[:, None]).astype(F32)
    u[~ok] = 0
    return u


def emulate(fx, rows_rev=None):
    """float32 coherence of every interval by the kernel's arithmetic: u += f32(v * r) member after member, then the finish"""
    strands = [fx["rows"]] if rows_rev is None else [fx["rows"], rows_rev]
    units = [_unit_rows(r) for r in strands]
    out = np.zeros(len(fx["w_lo"]), F32)
    for i in range(len(out)):
        members = lim.members_of(fx, i)
        if not len(members):
            continue
        total = np.zeros(lim.DIM, F32)
        for unit in units:
            u = np.zeros(lim.DIM, F32)
            for k in members:
                u = u + unit[k]
            total = u if unit is units[0] else total + u
        d = F32(len(strands) * len(members))
        out[i] = np.sqrt(_norm2(total[None])[0]) / d
    return out


def test_a_float32_emulation_of_the_kernel_lies_inside_the_tolerance(fixtures):
    print()
    for name, fx, rev, want in fixtures:
        got = emulate(fx, rev)
        assert got.dtype == F32 and np.isfinite(got).all()
        live = want["count"] > 0
        tol = np.array([lim.coh_tol(int(n), 1 if rev is None else 2) for n in want["count"]])
        d = np.abs(got.astype(np.float64) - want["coherence"])
        share = (d[live] / tol[live]).max()
        print(f"{name}: max |emulation - float64| = {d.max():.2e}, at most {share:.3f} of coh_tol")
        assert (d <= tol).all() and not got[~live].any(), (name, d.max())
