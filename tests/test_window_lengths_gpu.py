"""Every valid length of a window through the padding skip and the time split of the streaming front ends.

A window is always 6000 bytes, so the number of valid bytes L is the only shape these kernels have: nsteps = max(1, min(STEPS,
(last + 1 + 15 + FT - 1) / FT)) steps are computed, the pooled y @ w_v rows and pair products behind them are copied from an
all-N window (tests/window_lengths.py restates this, tests/test_window_lengths_host.py checks the premise on the fp64 oracle and
the partition exhaustively).  Here: all 6001 lengths with the skip on against the skip off (bit identity), windows with the
same tokens and a different `last` (bit identity), the boundary windows against the fp64 oracle (the tolerances of
test_gpu_parity.py), and windows of 1..8 steps under every split (bit identity with the one-workgroup launch)."""
import ctypes
import functools

import numpy as np
import pytest

from genomad_amd import _lib, synthetic
from oracle import igloo_oracle, sequence_oracle
from tests import window_lengths as WL
from tests.conftest import need_tables
from tests.test_gpu_parity import F32_CHECKS, F32_SCORE_TOL, FUSED_CHECKS, FUSED_LOOSE, SCORE_TOL

pytestmark = pytest.mark.gpu

BATCH = 512                    # at least the CU count: one workgroup per window, no time split


def _geometry(engine, prec):
    """(FT, STEPS, reach) of the kernel behind `prec`: FT from the library, the reach constant from its source."""
    ft = engine.lib.gnn_fused_rows_per_step(_lib.PRECISIONS[prec])
    c = WL.kernel_constants(prec)
    assert ft == c["ft"], (prec, ft, c)
    return ft, c["steps"], c["reach"]


def _last_split(engine):
    split = ctypes.c_int()
    _lib.check(engine.lib.gnn_debug_last_split(engine.ctx, ctypes.byref(split)))
    return split.value


def _set(engine, pad_skip=None, time_split=None):
    if pad_skip is not None:
        _lib.check(engine.lib.gnn_debug_set_pad_skip(engine.ctx, int(pad_skip)))
    if time_split is not None:
        _lib.check(engine.lib.gnn_debug_set_time_split(engine.ctx, int(time_split)))


def _rows_that_differ(x, y):
    return np.nonzero((x != y).reshape(len(x), -1).any(axis=1))[0]


@functools.lru_cache(maxsize=None)
def _sweep_windows():
    w = WL.length_windows(np.arange(WL.WINDOW + 1), seed=101)           # window L: L random ACGT bytes, then N
    w.setflags(write=False)
    return w


# ------------------------------------------------------------------ 2. every length, skip on against skip off
@pytest.mark.parametrize("prec", WL.FUSED)
def test_every_length_padding_skip_on_equals_off(engine, prec, request):
    """All 6001 valid lengths, in launches of 512 windows (no time split): scores, both heads' pair-product sums and the pooled
    features with the padding skip on are the bits the skip-off launch computes.  On the 24 boundary lengths (nsteps changes
    between L = k FT - 15 and L + 1, for both step sizes) the pooled y @ w_v rows as well - and, since 24 windows are fewer than the
    CUs, once more with the time split such a launch gets by default (all against the launch with both switches off)."""
    need_tables(request, prec)
    ft, steps, reach = _geometry(engine, prec)
    bases = _sweep_windows()
    n = len(bases)
    assert n == 6001 and engine.device_info()["cus"] <= BATCH
    taps = ("m_a", "m_b", "feat")
    starts = list(range(0, n - BATCH, BATCH)) + [n - BATCH]             # the last launch overlaps the one before: none is short

    def sweep(skip):
        _set(engine, pad_skip=skip)
        out = {k: None for k in ("scores",) + taps}
        for a in starts:
            s, t = engine.debug_forward(bases[a:a + BATCH], prec, taps=taps)
            if prec != "f16c6":                                         # f16c6 has no time split
                assert _last_split(engine) == 1
            t["scores"] = s
            for k, v in t.items():
                if out[k] is None:
                    out[k] = np.empty((n,) + v.shape[1:], v.dtype)
                out[k][a:a + BATCH] = v
        return out

    lens = np.array(WL.boundary_lengths(reach))
    try:
        _set(engine, time_split=1)
        off = sweep(0)
        on = sweep(1)
        edge = {}
        for split in (0, 1):
            for skip in (0, 1):
                _set(engine, pad_skip=skip, time_split=split)
                edge[split, skip] = engine.debug_forward(bases[lens], prec, taps=taps + ("yp_a", "yp_b"))
    finally:
        _set(engine, pad_skip=1, time_split=1)
    assert np.isfinite(off["scores"]).all() and off["scores"].std(axis=0).min() > 0.01       # the sweep is not vacuous
    report = []
    for k in off:
        bad = _rows_that_differ(off[k], on[k])
        if len(bad):
            report.append(f"{k}: {len(bad)} lengths differ, first {[(int(L), int(L) % ft) for L in bad[:20]]} as (L, L mod {ft}), "
                          f"max |d| {np.abs(off[k][bad].astype(np.float64) - on[k][bad]).max():.3e}")
    for (split, skip), (s, t) in edge.items():
        want_s, want_t = edge[0, 0]
        for k, got, want in [("scores", s, want_s)] + [(k, t[k], want_t[k]) for k in t]:
            bad = _rows_that_differ(got, want)
            if len(bad):
                report.append(f"boundary lengths, time split {split}, padding skip {skip}, {k}: "
                              f"{[(int(L), int(L) % ft) for L in lens[bad][:20]]} as (L, L mod {ft})")
    assert not report, f"{prec}: " + "; ".join(report)


# ------------------------------------------------------------------ 3. same tokens, different `last`
@pytest.mark.parametrize("prec", WL.FUSED)
def test_bytes_that_make_no_token_move_last_but_not_the_results(engine, prec, request):
    """One to three ACGT bytes alone in the N tail make no token (a token needs four), so the window is the same input to the
    network - but `last` moves to the plant, nsteps grows, and the kernel computes rows the plain window copies.  Plants on, before
    and after every change of nsteps: scores and every intermediate are the unplanted window's bits (default switches)."""
    need_tables(request, prec)
    ft, steps, reach = _geometry(engine, prec)
    cases = WL.planted_cases(ft, steps, reach)
    bodies = sorted({L for L, _, _ in cases})
    assert bodies == [0, 50, 2000] and {pl for _, _, pl in cases} == {1, 3} and len(cases) > 100
    plain = np.stack([WL.planted_window(L, 0, 0) for L in bodies])
    planted = np.stack([WL.planted_window(*c) for c in cases])
    ref_of = np.array([bodies.index(L) for L, _, _ in cases])
    # the test's own premise: the token arrays are equal, `last` (hence the step count) is not
    assert np.array_equal(sequence_oracle.tokenize_closed_form(planted), sequence_oracle.tokenize_closed_form(plain)[ref_of])
    grows = 0
    for (L, p, pl), w in zip(cases, planted):
        last = int(np.nonzero(np.isin(w, list(b"ACGT")))[0].max())
        assert last == p + pl - 1
        grows += WL.nsteps_of(last, ft, steps, reach) > WL.nsteps_of(L - 1, ft, steps, reach)
    assert grows >= len(cases) * 3 // 4                                  # (a plant that ends before k FT - 15 of the body's own last step computes no more)
    taps = ("m_a", "m_b", "yp_a", "yp_b", "feat")
    s, t = engine.debug_forward(np.concatenate([plain, planted]), prec, taps=taps)
    t["scores"] = s
    report = []
    for k, v in t.items():
        bad = _rows_that_differ(v[len(plain):], v[:len(plain)][ref_of])
        if len(bad):
            report.append(f"{k}: {[cases[i] + ((cases[i][1] + cases[i][2] + reach) % ft,) for i in bad[:20]]} "
                          f"as (L, p, plant, (last + 1 + {reach}) mod {ft})")
    assert np.isfinite(s).all()
    assert not report, f"{prec}: " + "; ".join(report)


# ------------------------------------------------------------------ 4. boundary windows against the fp64 oracle
def _oracle_planted_cases():
    """A subset of section 3's cases (WL.planted_cases), chosen for BOTH step sizes so that one oracle serves every arithmetic (for
    a given kernel half of them sit on the other step size's boundaries): behind the 50-byte body the three-byte plants whose last
    byte is the first `last` that computes k + 1 steps, for every k, and the two plants that end on the window's last byte."""
    out = []
    for ft in (96, 128):
        steps = (WL.TOKENS + ft - 1) // ft
        edges = {k * ft - 15 for k in (1, 2, 3, 31, steps - 1)}
        cases = WL.planted_cases(ft, steps)
        out += [c for c in cases if c[0] == 50 and c[2] == 3 and c[1] + 2 in edges]
        out += [c for c in cases if c in ((50, WL.WINDOW - 1, 1), (2000, WL.WINDOW - 3, 3)) and c not in out]
    assert len(out) == 12, out
    return out


@pytest.fixture(scope="module")
def boundary_oracle(synth_weights):
    """fp64 oracle of the 24 boundary windows and 12 planted windows, computed once for all arithmetics."""
    lens = WL.boundary_lengths(15)
    cases = _oracle_planted_cases()
    bases = np.concatenate([_sweep_windows()[lens], np.stack([WL.planted_window(*c) for c in cases])])
    tok = sequence_oracle.tokenize_closed_form(bases)
    scores, taps = [], {}
    for a in range(0, len(bases), 6):
        s, t = igloo_oracle.forward(tok[a:a + 6], synth_weights, dtype=np.float64, return_taps=True)
        scores.append(s)
        for k, v in t.items():
            taps.setdefault(k, []).append(v)
    bases.setflags(write=False)
    return bases, np.concatenate(scores), {k: np.concatenate(v) for k, v in taps.items()}


@pytest.mark.parametrize("prec", WL.FUSED + ["f32"])
def test_boundary_windows_against_the_fp64_oracle(engine, boundary_oracle, prec, request):
    """The bit-identity tests compare the kernel with itself; this one compares the boundary and planted windows with the
    independent reference, per stage, at the tolerances the suite already holds 16 synthetic windows to."""
    need_tables(request, prec)
    bases, scores64, t64 = boundary_oracle
    if prec == "f32":
        checks, loose, score_tol = F32_CHECKS, 1.0, F32_SCORE_TOL
    else:
        checks, loose, score_tol = FUSED_CHECKS, FUSED_LOOSE.get(prec, 1.0), SCORE_TOL
    scores, taps = engine.debug_forward(bases, prec, taps=tuple(mine for mine, _, _ in checks))
    err = {mine: float(np.abs(taps[mine] - t64[ref]).max()) for mine, ref, _ in checks}
    err["scores"] = float(np.abs(scores - scores64).max())
    print(f"{prec}, {len(bases)} boundary / planted windows, max abs err vs fp64 (tolerance): "
          + ", ".join(f"{mine} {err[mine]:.2e} ({tol * loose:.1e})" for mine, _, tol in checks)
          + f", scores {err['scores']:.2e} ({score_tol:.0e})")
    for mine, _, tol in checks:
        assert err[mine] <= tol * loose, f"{prec} {mine}: max abs err {err[mine]:.3e} > {tol * loose}"
    assert err["scores"] <= score_tol <= SCORE_TOL
    assert scores64.std(axis=0).min() > 0.01                             # the windows do not all score alike


# ------------------------------------------------------------------ 5. short windows under every split
@pytest.mark.parametrize("prec", ["f16x3tc", "f16x3tk", "f16x3", "bf16x3"])
def test_short_windows_under_every_split(engine, prec, request):
    """One window per step count 1..8 (where ceil(nsteps / split), the empty runs and the warm-up step interact), STEPS - 1 and STEPS,
    first and last in launches small enough for 4, 3 and 2 workgroups per window: scores, pair-product sums and pooled rows under the
    time split are the one-workgroup launch's bits, padding skip on and off."""
    need_tables(request, prec)
    ft, steps, reach = _geometry(engine, prec)
    ks = list(range(1, 9)) + [steps - 1, steps]
    lens = [0] + [min(k * ft - reach, WL.WINDOW) for k in ks]
    assert [WL.nsteps_of(L - 1, ft, steps, reach) for L in lens] == [1] + ks
    special = WL.length_windows(lens, seed=77)
    cus = engine.device_info()["cus"]
    taps = ("m_a", "m_b", "yp_a", "yp_b")
    done, skipped = [], []
    try:
        for want in (4, 3, 2):
            n = cus // want
            if n < 2 * len(special) or max(1, min(4, cus // n)) != want:
                skipped.append(want)
                continue
            wins = np.concatenate([special, synthetic.synth_windows(7000, n - 2 * len(special)), special[::-1]])
            assert len(wins) == n
            for skip in (0, 1):
                _set(engine, pad_skip=skip, time_split=0)
                ws, wt = engine.debug_forward(wins, prec, taps=taps)
                assert _last_split(engine) == 1
                _set(engine, time_split=1)
                gs, gt = engine.debug_forward(wins, prec, taps=taps)
                assert _last_split(engine) == want, (prec, n, _last_split(engine))
                wt["scores"], gt["scores"] = ws, gs
                for k in wt:
                    bad = _rows_that_differ(gt[k], wt[k])
                    assert not len(bad), f"{prec} split {want} padding skip {skip} {k}: windows {bad[:20].tolist()} of {n} differ " \
                                         f"(the first and last {len(special)} have {[1] + ks} steps)"
                assert np.array_equal(gs[:len(special)], gs[::-1][:len(special)])          # first and last in the batch: the same window, the same bits
            done.append(want)
    finally:
        _set(engine, pad_skip=1, time_split=1)
    if skipped:
        assert done, f"a device of {cus} CUs cannot run {len(special)} special windows twice under any split"
        pytest.skip(f"a device of {cus} CUs cannot launch {2 * len(special)}+ windows with {skipped} workgroups per window "
                    f"(exercised: {done})")
    assert done == [4, 3, 2]
