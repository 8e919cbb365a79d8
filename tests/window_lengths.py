"""Shared by tests/test_window_lengths_host.py and tests/test_window_lengths_gpu.py: the padding skip's step count and the time
split's partition restated in Python, the constants behind them read from the kernels' source, and the windows both files use.

A window is 6000 bytes; the streaming front ends (gnn_fused_tc / _tk / _x3 / _c6.hip) compute only

    nsteps = max(1, min(STEPS, (last + 1 + REACH + FT - 1) / FT))          last = index of the last ACGT byte, -1 if none

steps of FT rows and copy the rest from an all-N window.  Under the time split part p of `split` owns the steps
[s_lo, s_hi) = [min(p per, nsteps), min(s_lo + per, nsteps)), per = ceil(nsteps / split), and starts executing at s_begin."""
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genomad_amd", "csrc")
WINDOW, TOKENS, POOL = 6000, 5997, 8
TOKEN_BYTES = 4            # a token needs four consecutive ACGT bytes (sequence.py:170-193)
KS = 6                     # taps of each of the three causal convolutions: x3[t] reads tokens t - 15 .. t
MIN_REACH = 3 * (KS - 1) - (TOKEN_BYTES - 1)   # 12: rows >= L + 12 of a window with L valid bytes are an all-N window's rows
FUSED = ["f16c6", "f16x3", "f16x3tc", "f16x3tk", "bf16x3"]
# arithmetic -> (kernel source, header that holds its geometry, names of its FT and STEPS constants)
KERNELS = {"f16x3tc": ("gnn_fused_tc.hip", "gnn_tc_dev.h", "FTT", "STEPST"), "f16x3tk": ("gnn_fused_tk.hip", "gnn_tc_dev.h", "FTT", "STEPST"),
           "f16x3": ("gnn_fused_x3.hip", "gnn_fused_x3.hip", "FTX", "STEPSX"), "bf16x3": ("gnn_fused_x3.hip", "gnn_fused_x3.hip", "FTX", "STEPSX"),
           "f16c6": ("gnn_fused_c6.hip", "gnn_fused_c6.hip", "FT6", "STEPS6")}


def _code(name):
    """a source file without its // comments"""
    return re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())


@functools.lru_cache(maxsize=None)
def kernel_constants(prec):
    """What the kernel of `prec` is compiled with, parsed from its source: dict(ft, steps, reach, split, warmup).  Raises
    AssertionError when a statement the Python model restates is no longer in the source in the form it was transcribed from."""
    src_name, hdr_name, FT, STEPS = KERNELS[prec]
    src, hdr = _code(src_name), _code(hdr_name)
    m = re.search(r"constexpr int NMB = (\w+);", hdr)
    assert m, f"{hdr_name}: NMB"
    nmb = m.group(1)
    if not nmb.isdigit():
        d = re.search(rf"#ifndef {nmb}\s*#define {nmb} (\d+)", hdr)
        assert d, f"{hdr_name}: default of {nmb}"
        nmb = d.group(1)
    assert re.search(rf"constexpr int {FT} = 32 \* NMB;", hdr), f"{hdr_name}: {FT}"
    assert re.search(rf"constexpr int {STEPS} = \(T \+ {FT} - 1\) / {FT};", hdr), f"{hdr_name}: {STEPS}"
    ft = 32 * int(nmb)
    m = re.search(rf"const int nsteps = a\.yp_c \? max\(1, min\({STEPS}, \(\*s_last \+ 1 \+ (\d+) \+ {FT} - 1\) / {FT}\)\) : {STEPS};", src)
    assert m, f"{src_name}: the nsteps statement changed - nsteps_of() restates it"
    reach = int(m.group(1))
    # the copy starts at pooled row nsteps * FT / 8 (the host test's bound on nsteps * FT) and is the last part's
    assert re.search(rf"const int q0 = nsteps \* \({FT} / GNN_POOL\);", src), \
        f"{src_name}: the first copied pooled row changed - the bounds on nsteps * FT in test_window_lengths_host.py assume it"
    split = "a.split" in src
    warmup = False
    if split:
        assert re.search(rf"if \(nsteps < {STEPS} && part == a\.split - 1\)", src), \
            f"{src_name}: who copies changed - runs_of() and the host test assume the last part, whether its run is empty or not"
        assert re.search(r"const int per = \(nsteps \+ a\.split - 1\) / a\.split;\s*"
                         r"const int s_lo = min\(part \* per, nsteps\), s_hi = min\(s_lo \+ per, nsteps\);", src), \
            f"{src_name}: per / s_lo / s_hi changed - runs_of() restates them"
        if "s_begin" in src:
            assert re.search(r"const int s_begin = s_hi > s_lo \? \(s_lo > 0 \? s_lo - 1 : 0\) : s_hi;", src), \
                f"{src_name}: s_begin changed - runs_of(warmup=True) restates it"
            warmup = True              # gnn_fused_tk.hip has none: x2 comes from a table, a step depends on nothing before it
    else:
        assert re.search(rf"if \(nsteps < {STEPS}\)", src), f"{src_name}: who copies changed - the model assumes one workgroup per window"
    return dict(ft=ft, steps=(TOKENS + ft - 1) // ft, reach=reach, split=split, warmup=warmup)


def nsteps_of(last, ft, steps, reach):
    return max(1, min(steps, (last + 1 + reach + ft - 1) // ft))


def runs_of(nsteps, split, warmup):
    """[(s_lo, s_hi, s_begin)] of every part; a part executes the steps [s_begin, s_hi) and stores [s_lo, s_hi)."""
    per = (nsteps + split - 1) // split
    out = []
    for part in range(split):
        s_lo = min(part * per, nsteps)
        s_hi = min(s_lo + per, nsteps)
        if not warmup:
            s_begin = s_lo
        else:
            s_begin = (s_lo - 1 if s_lo > 0 else 0) if s_hi > s_lo else s_hi
        out.append((s_lo, s_hi, s_begin))
    return out


def boundary_lengths(reach=15, fts=(96, 128)):
    """Valid lengths on both sides of a change of nsteps: L = k FT - reach computes k steps, L + 1 computes k + 1; at k = STEPS - 1
    the copy shrinks to the last step and then disappears."""
    out = []
    for ft in fts:
        steps = (TOKENS + ft - 1) // ft
        for k in (1, 2, 3, 5, 31, steps - 1):
            out += [k * ft - reach, k * ft - reach + 1]
    return sorted(set(out))


def acgt(rng, shape):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, shape)]


def length_windows(lengths, seed):
    """One window per length: L seeded random ACGT bytes, then N."""
    lengths = np.asarray(lengths)
    w = acgt(np.random.default_rng(seed), (len(lengths), WINDOW))
    w[np.arange(WINDOW)[None, :] >= lengths[:, None]] = ord("N")
    return w


def planted_positions(ft, steps, reach=15):
    """Tail positions on, before and after every change of nsteps (last = k FT - reach is the first that computes k + 1 steps), for a
    plant that ends at p (one byte) or at p + 2 (three bytes), and the window's last byte."""
    ps = set()
    for k in (1, 2, 3, 31, steps - 1, steps):
        b = k * ft - reach
        ps.update(range(b - 3, b + 2))
    return sorted(p for p in ps if 0 <= p < WINDOW) + [WINDOW - 1]


def planted_cases(ft, steps, reach=15, bodies=(0, 50, 2000), plants=(1, 3)):
    """(L, p, plant): a body of L bytes, N, and `plant` ACGT bytes at p .. p + plant - 1 with at least one N between them and the
    body (so that no four consecutive ACGT bytes, hence no token, contain a planted byte)."""
    out = []
    for L in bodies:
        for p in sorted(set(planted_positions(ft, steps, reach))):
            for plant in plants:
                q = min(p, WINDOW - plant)                  # the plant at the window's end: its LAST byte is byte 5999
                if q > L and (L, q, plant) not in out:
                    out.append((L, q, plant))
    return out


def planted_window(L, p, plant, seed=29):
    """The body of length L is the same bytes for every (p, plant): seeded by L alone.  plant = 0: the unplanted window."""
    w = length_windows([L], seed + L)[0]
    if plant:
        w[p:p + plant] = acgt(np.random.default_rng(seed + 7919 * p + plant), plant)
    return w
