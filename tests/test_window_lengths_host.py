"""The padding skip's premise and the time split's partition, without a GPU (tests/test_window_lengths_gpu.py sweeps the kernels).

Premise: a window whose last ACGT byte is byte L - 1 has its last token at L - 4, and x3[t] reads tokens t - 15 .. t, so rows
t >= L + 12 of x1, x2 and x3 are the rows of an all-N window (12 is the smallest such reach: row L + 11 differs); the kernels copy
from row nsteps * FT >= L + 15 on.  Partition: the parts of a split launch store every computed step exactly once."""
import numpy as np
import pytest

from genomad_amd import _lib
from oracle import igloo_oracle, sequence_oracle
from tests import window_lengths as WL


def test_rows_behind_the_reach_of_the_last_token_are_an_all_n_windows_rows(synth_weights):
    """fp64 oracle, every boundary length of both step sizes, random ACGT body + N tail: x1 / x2 / x3 rows >= L + 12 and pooled
    y @ w_v rows >= ceil((L + 12) / 8) of both heads equal the all-N window's rows at the same positions (rows are compared at
    the same position: the causal zero padding makes the first 15 rows of any window special), and row L + 11 of x3 does not:
    a reach of 12 is necessary, the kernels' 15 is sufficient."""
    assert WL.MIN_REACH == 12
    lens = WL.boundary_lengths(15)
    assert {81, 82, 177, 178, 5937, 5938, 113, 114, 5873, 5874} <= set(lens) and len(lens) == 24
    bases = np.concatenate([WL.length_windows(lens, seed=5), WL.length_windows([0], seed=5)])
    tok = sequence_oracle.tokenize_closed_form(bases)
    for i, L in enumerate(lens):                 # the windows are what they claim to be: tokens 0 .. L - 4 valid, the rest 0
        assert tok[i, :L - 3].all() and not tok[i, max(L - 3, 0):].any()
    keys = ("x1", "x2", "x3", "ypA", "ypB")
    allN = None
    tight = []
    for a in [len(lens)] + list(range(0, len(lens), 6)):           # the all-N window first, then six windows at a time
        b = a + 1 if a == len(lens) else min(a + 6, len(lens))
        _, taps = igloo_oracle.forward(tok[a:b], synth_weights, dtype=np.float64, return_taps=True)
        if allN is None:
            allN = {k: taps[k][0] for k in keys}
            continue
        for i, L in enumerate(lens[a:b]):
            # what each layer adds to the reach: x1 rows >= L + 2, x2 rows >= L + 7, x3 rows >= L + 12
            for k, r0 in (("x1", L + 2), ("x2", L + 7), ("x3", L + 12), ("x1", L + 12), ("x2", L + 12)):
                assert np.allclose(taps[k][i, r0:], allN[k][r0:], rtol=0, atol=1e-12), (k, L)
            q0 = -(-(L + 12) // WL.POOL)
            for k in ("ypA", "ypB"):
                assert np.allclose(taps[k][i, q0:], allN[k][q0:], rtol=0, atol=1e-12), (k, L)
            tight.append(float(np.abs(taps["x3"][i, L + 11] - allN["x3"][L + 11]).max()))
    print(f"max |x3[L + 11] - all-N| per window: {min(tight):.2e} .. {max(tight):.2e}")
    assert max(tight) > 1e-6, "row L + 11 of x3 never differs: the bound of 12 is not tight, or the windows are vacuous"


def test_kernel_constants_are_what_the_model_and_the_library_use():
    """FT from the library's geometry query and from the source agree; the reach constant is 15 in all four kernels (a change
    must come with new boundary lengths in the tests and DESIGN.md section 4.1)."""
    lib = _lib.load()
    for prec in WL.FUSED:
        c = WL.kernel_constants(prec)
        assert c["ft"] == lib.gnn_fused_rows_per_step(_lib.PRECISIONS[prec]), prec
        assert c["reach"] == 15 and c["ft"] % WL.POOL == 0, (prec, c)
        assert c["split"] == (prec != "f16c6") and c["warmup"] == (prec in ("f16x3tc", "f16x3", "bf16x3")), (prec, c)
        assert c["steps"] == {96: 63, 128: 47}[c["ft"]]
    assert _lib.TOKENS == WL.TOKENS and _lib.WINDOW == WL.WINDOW


@pytest.mark.parametrize("prec", WL.FUSED)
def test_partition_tiles_the_computed_steps_for_every_last_and_split(prec):
    """Exhaustive over last in [-1, 5999] and split in 1..4, with the constants of the kernel's own source."""
    c = WL.kernel_constants(prec)
    ft, steps, reach = c["ft"], c["steps"], c["reach"]
    seen = set()
    for last in range(-1, WL.WINDOW):
        n = WL.nsteps_of(last, ft, steps, reach)
        assert 1 <= n <= steps
        if n < steps:
            # the first copied row is past the reach of the last valid token (at last - 3, felt up to row last - 3 + 15)
            assert n * ft >= last + 1 - 3 + 12, (last, n)
            assert n * ft >= last + 1 + WL.MIN_REACH, (last, n)
            assert n * (ft // WL.POOL) * WL.POOL >= last + 1 + WL.MIN_REACH             # pooled rows are copied from row n FT / 8
        else:
            assert steps * ft >= WL.TOKENS                                             # nothing is copied, every row is computed
        if n in seen:
            continue
        seen.add(n)
        for split in ((1, 2, 3, 4) if c["split"] else (1,)):
            runs = WL.runs_of(n, split, c["warmup"])
            assert len(runs) == split
            stored = [s for lo, hi, _ in runs for s in range(lo, hi)]
            assert stored == list(range(n)), (n, split, runs)                          # every computed step stored exactly once, in order
            for part, (lo, hi, begin) in enumerate(runs):
                executed = list(range(begin, hi))
                if hi > lo:
                    want = lo - 1 if (c["warmup"] and lo > 0) else lo                  # one warm-up step for every run but the first
                    assert begin == want >= 0 and (part == 0) == (lo == 0), (n, split, part, runs)
                    assert executed == ([lo - 1] if begin < lo else []) + list(range(lo, hi))
                else:
                    assert executed == [], (n, split, part, runs)                      # an empty run executes nothing
            # the copy is the last part's, whether its run is empty or not: exactly one part has index split - 1
    assert seen == set(range(1, steps + 1))                                            # every step count occurs


def test_partition_examples_of_short_windows():
    """nsteps 3..8 are where ceil, the empty runs and the warm-up step interact."""
    assert WL.runs_of(5, 4, True) == [(0, 2, 0), (2, 4, 1), (4, 5, 3), (5, 5, 5)]
    assert WL.runs_of(1, 4, True) == [(0, 1, 0), (1, 1, 1), (1, 1, 1), (1, 1, 1)]
    assert WL.runs_of(3, 2, True) == [(0, 2, 0), (2, 3, 1)]
    assert WL.runs_of(6, 4, True) == [(0, 2, 0), (2, 4, 1), (4, 6, 3), (6, 6, 6)]
    assert WL.runs_of(7, 3, False) == [(0, 3, 0), (3, 6, 3), (6, 7, 6)]
    assert WL.runs_of(63, 4, True) == [(0, 16, 0), (16, 32, 15), (32, 48, 31), (48, 63, 47)]


def lengths_copied_too_early(reach, ft, steps):
    """Valid lengths L (L ACGT bytes, then N) at which a kernel with this reach constant copies a row the last token still
    reaches: the row L + 11 lies at or behind the first copied row nsteps FT."""
    return [L for L in range(WL.TOKEN_BYTES, WL.WINDOW + 1)
            if (n := WL.nsteps_of(L - 1, ft, steps, reach)) < steps and n * ft <= L + WL.MIN_REACH - 1]


@pytest.mark.parametrize("ft,steps", [(96, 63), (128, 47)])
def test_a_reach_constant_below_12_copies_a_row_too_early(ft, steps):
    """What the sweep of tests/test_window_lengths_gpu.py must report for a kernel built with a smaller constant
    (profiles/window_lengths.md has the run): 11 fails at L = k FT - 11 exactly, 12 and 15 nowhere."""
    assert lengths_copied_too_early(15, ft, steps) == [] and lengths_copied_too_early(12, ft, steps) == []
    assert lengths_copied_too_early(11, ft, steps) == [k * ft - 11 for k in range(1, steps)]
    assert {L % ft for L in lengths_copied_too_early(8, ft, steps)} == {ft - 11, ft - 10, ft - 9, ft - 8}
