"""Inputs that take the region calls (gnn_regions.hip) to the limits tests/test_regions_gpu.py stays away from, the conditions each
is made for asserted on the CPU (tests/test_regions_limits_host.py), and two references that share no code with
sequence.call_regions: exact emissions over fractions, and a Viterbi pass that counts the ties it decides.  What each input pins:

  edge_values   what load_q reads: the clamp at 0 and at 1, -0.0, subnormals, +-FLT_MAX, +-inf and NaN, and the ties of rint at k + 1/2
  edge_track    one contig of ONE bin per ordered triple of edge_values: every bin is its own region, so the device's qsum row is the
                bin's q and its evidence is the bin's flag; about 10^4 contigs and as many tiles (owner_of bisects 13 deep), two
                trailing empty contigs
  tie_track     values of {0, 0.25, 0.5, 1, NaN} on contig sizes around every tile seam and around TILE_MAX: d ties at every penalty,
                so `a tie stays`, `the lowest s'` and `the lowest s with maximal d` decide states, also on the first bin of a tile
  planted_ties  four contigs whose outcome hangs on one tie each, the run that ties laid across a tile seam; the regions are written
                out by hand
  long_track    262 845 bins: 1 027 blocks of 256 (nn_scan_kernel with more than one count per thread), 1 024 tiles in one
                contig (carry_kernel, carry_back_kernel), and at the largest penalty one region whose qsum passes 2^32"""
import functools
from fractions import Fraction

import numpy as np

from genomad_amd import sequence

Q1 = 1 << 20
KEYS = ("contig", "lo", "hi", "state", "evidence", "qsum")
SIZES = (0, 1, 0, 2, 6, 0, 7, 8, 0, 14, 26, 3, 4, 5, 8, 255, 0, 256, 257, 0, 300)      # tests/test_regions_gpu.py::SIZES
TIE_SIZES = SIZES + (4095, 4096, 4097, 0)
TIE_VALUES = (0, 0.25, 0.5, 1, np.nan)
TIE_SEED = 3
TIE_PENALTIES = (0.25, 0.5, 1, 2)
TIE_TILES = (4, 7, 256)
LONG_SIZES = (0, 5, 262139, 1, 0, 700, 0)
LONG_CONTIG = 2                                         # the 262 139-bin contig of long_track


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


# ---- emissions ---------------------------------------------------------------------------------------------------------------------

def edge_values():
    """the float32 values E, NaN last"""
    f = np.float32
    half = f(2.0 ** -21)                                # half a step of 2^-20: rint's ties sit at odd multiples of it
    fmax = np.finfo(f).max
    e = [f(-0.0), f(0), f(1e-45), f(-1e-45), f(1e-39), f(-0.3),
         half, np.nextafter(half, f(1)), f(3) * half, f(5) * half, f(0.5) + half,
         f(1) - f(2.0 ** -24), f(1), np.nextafter(f(1), f(2)), f(2),
         fmax, -fmax, f(np.inf), f(-np.inf), f(np.nan)]
    return np.array(e, np.float32)


# q of edge_values() in its order, by hand: the clamp at 0, 0.5 -> 0, just above -> 1, 1.5 -> 2, 2.5 -> 2, 524288.5 -> 524288, the clamp at 1;
# a non-finite value has no q of its own (its bin is no evidence bin)
EDGE_Q = (0, 0, 0, 0, 0, 0, 0, 1, 2, 2, 524288, Q1, Q1, Q1, Q1, Q1, 0, None, None, None)


def exact_q(v):
    """q of one finite float32 in exact arithmetic: clamp to [0, 1], times 2^20, to the nearest integer, ties to even (Python's round
    of a Fraction); None for a value that is not finite"""
    v = float(v)
    if v != v or v in (float("inf"), float("-inf")):
        return None
    return int(round(min(max(Fraction(v), Fraction(0)), Fraction(1)) * Q1))


def exact_emissions(track):
    """(q int64 (n, 3), evidence bool (n,)) of a track through exact_q: a bin with a value that is not finite has q = 0 throughout"""
    t = np.asarray(track, np.float32).reshape(-1, 3)
    table = {}
    q, ev = np.zeros(t.shape, np.int64), np.zeros(len(t), bool)
    for b, row in enumerate(t.view(np.uint32).tolist()):
        vals = []
        for bits in row:
            if bits not in table:
                table[bits] = exact_q(np.array(bits, np.uint32).view(np.float32))
            vals.append(table[bits])
        if None not in vals:
            q[b], ev[b] = vals, True
    return q, ev


def edge_track():
    """(track, bin_offsets): one contig of one bin per ordered triple of edge_values(), then two empty contigs"""
    e = edge_values()
    n = len(e)
    i = np.arange(n ** 3)
    track = np.stack([e[i // (n * n)], e[(i // n) % n], e[i % n]], axis=1).astype(np.float32)
    return track, _offsets((1,) * len(track) + (0, 0))


# ---- ties --------------------------------------------------------------------------------------------------------------------------

def tie_track(seed=TIE_SEED):
    """(track, bin_offsets): TIE_SIZES filled with draws from TIE_VALUES, as tests/test_regions_host.py::_tracks does"""
    rng = np.random.default_rng(seed)
    off = _offsets(TIE_SIZES)
    values = np.array(TIE_VALUES, np.float32)
    return values[rng.integers(0, len(values), (int(off[-1]), 3))], off


@functools.lru_cache(maxsize=None)
def tie_reference(penalty):
    """sequence.call_regions on tie_track(), once per penalty in a test run"""
    return sequence.call_regions(*tie_track(), penalty)


def counting_viterbi(q, off, P):
    """The path of the definition written a second time, over candidate lists, and what it decided by a tie.  ``q``
    (n_bins, 3) integers, ``off`` the bin CSR, ``P`` the integer penalty.  Returns (state uint8, counts): counts[kind] is a list of
    (contig, contig-relative bin) ON THE PATH - the decision that gave the path its state before that bin - for kind
      "stay_tie"    the path stayed because d[s] EQUALS the best other state's d - P (a `>` in place of `>=` switches here)
      "switch_tie"  the path switched, and the two states it could come from had EQUAL d (a `>=` in place of `>` takes the higher)
    and counts["last_tie"] a list of contigs whose last bin's maximal d is shared by two or three states.  counts["cells"][kind] lists
    (contig, bin) of every (bin, state) cell of either kind, on the path or not: the device computes each of them, but only a
    decision on the path can change an output."""
    q = np.asarray(q, np.int64).tolist()
    off = [int(o) for o in off]
    state = np.zeros(off[-1], np.uint8)
    counts = {"stay_tie": [], "switch_tie": [], "last_tie": [], "cells": {"stay_tie": [], "switch_tie": []}}
    for c in range(len(off) - 1):
        a, n = off[c], off[c + 1] - off[c]
        if n == 0:
            continue
        d = list(q[a])
        back = [None]                                    # per bin: three (previous state, kind or None)
        for b in range(1, n):
            nd, row = [], []
            for s in range(3):
                cand = [d[t] - (0 if t == s else P) for t in range(3)]
                top = max(cand)
                others = [t for t in range(3) if t != s]
                if cand[s] == top:                       # staying attains the maximum: it stays
                    kind = "stay_tie" if any(cand[t] == top for t in others) else None
                    prev = s
                else:
                    prev = min(t for t in others if cand[t] == top)
                    kind = "switch_tie" if cand[others[0]] == cand[others[1]] else None
                if kind:
                    counts["cells"][kind].append((c, b))
                nd.append(q[a + b][s] + top)
                row.append((prev, kind))
            d = nd
            back.append(row)
        top = max(d)
        if sum(v == top for v in d) > 1:
            counts["last_tie"].append(c)
        s = min(t for t in range(3) if d[t] == top)
        for b in range(n - 1, 0, -1):
            state[a + b] = s
            prev, kind = back[b][s]
            if kind:
                counts[kind].append((c, b))
            s = prev
        state[a] = s
    return state, counts


def regions_of(state, q, ev, off):
    """the six region arrays of a state vector: maximal runs within a contig, with their sums (plain loops)"""
    out = {k: [] for k in KEYS}
    for c in range(len(off) - 1):
        a, e = int(off[c]), int(off[c + 1])
        lo = a
        for b in range(a + 1, e + 1):
            if b == e or state[b] != state[lo]:
                out["contig"].append(c), out["lo"].append(lo - a), out["hi"].append(b - a), out["state"].append(state[lo])
                out["evidence"].append(int(ev[lo:b].sum())), out["qsum"].append(q[lo:b].sum(axis=0))
                lo = b
    r = {k: np.asarray(out[k], np.uint8 if k == "state" else np.int64) for k in KEYS}
    r["qsum"] = r["qsum"].reshape(-1, 3)
    return r


FINE_SIZES = (1, 5, 300, 0, 64)
# penalties that are no multiple of 2^-20, with the P that rint (ties to even) gives; cutting the fraction off would give 0, 1, 2, 1, 1
FINE_PENALTIES = ((2.0 ** -21, 0), (3 * 2.0 ** -21, 2), (5 * 2.0 ** -21, 2), (1e-6, 1), (1.5e-6, 2))


def fine_track(seed=41):
    """(track, bin_offsets): q of 0 .. 4 (values k * 2^-20) with about 10 % NaN bins: d differs by single units, so P = 0, 1 and 2
    give different paths and the rounding of penalty * 2^20 shows in the states"""
    rng = np.random.default_rng(seed)
    off = _offsets(FINE_SIZES)
    track = (rng.integers(0, 5, (int(off[-1]), 3)) * 2.0 ** -20).astype(np.float32)
    track[rng.random(len(track)) < 0.1] = np.nan
    return track, off


# ---- planted ties ------------------------------------------------------------------------------------------------------------------

def planted_ties(T, penalty):
    """(track, bin_offsets, state, regions) for an integer penalty p >= 1 and a tile of T bins: four contigs of (1, 0, 0) bins around
    one run of m bins of (0, 1, 0).  Entering the run costs p and so does leaving it; every bin inside gains 1.
      0  k bins, then the run, m = p: the two final states tie, the lowest wins          one region of state 0
      1  the same, m = p + 1                                                               two regions
      2  k bins, the run, k bins, m = 2p: in and out again ties with staying, a tie stays  one region of state 0
      3  the same, m = 2p + 1                                                              three regions
    The run lies across bin X, a multiple of T past 3p + 3: it begins m // 2 bins before X (for m = 1 it IS bin X, a tile's first
    bin), so the tie is decided by an entry vector or a composed back pointer, not inside one tile.  State and regions are written
    down here from k and m, not computed."""
    p = int(penalty)
    assert p == penalty and p >= 1 and T >= 1
    X = T * -(-(3 * p + 3) // T)
    one, run = (1, 0, 0), (0, 1, 0)
    rows, sizes, state = [], [], []
    reg = {k: [] for k in KEYS}

    def region(c, lo, hi, s, n0, n1):
        reg["contig"].append(c), reg["lo"].append(lo), reg["hi"].append(hi), reg["state"].append(s)
        reg["evidence"].append(hi - lo), reg["qsum"].append((n0 * Q1, n1 * Q1, 0))

    for c, (m, closed) in enumerate(((p, False), (p + 1, False), (2 * p, True), (2 * p + 1, True))):
        k = X - m // 2
        assert k > p + 1 and k <= X < k + m + (m == 1) and (m == 1 or k < X)
        tail = k if closed else 0
        rows += [one] * k + [run] * m + [one] * tail
        sizes.append(k + m + tail)
        if c in (0, 2):                                  # the tie: all of it stays in state 0
            state += [0] * (k + m + tail)
            region(c, 0, k + m + tail, 0, k + tail, m)
        else:
            state += [0] * k + [1] * m + [0] * tail
            region(c, 0, k, 0, k, 0)
            region(c, k, k + m, 1, 0, m)
            if closed:
                region(c, k + m, k + m + tail, 0, tail, 0)
    regions = {k: np.asarray(reg[k], np.uint8 if k == "state" else np.int64) for k in KEYS}
    return np.array(rows, np.float32), _offsets(sizes), np.array(state, np.uint8), regions


# ---- a long track ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def long_track(seed=29):
    """(track, bin_offsets), read-only: LONG_SIZES of random scores with about 10 % NaN bins: 262 845 bins"""
    rng = np.random.default_rng(seed)
    off = _offsets(LONG_SIZES)
    track = rng.random((int(off[-1]), 3), dtype=np.float32)
    track[rng.random(len(track)) < 0.1] = np.nan
    track.flags.writeable = off.flags.writeable = False
    return track, off


@functools.lru_cache(maxsize=None)
def long_reference(penalty):
    """sequence.call_regions on long_track(), once per penalty in a test run (1 - 2 s each), read-only"""
    state, regions = sequence.call_regions(*long_track(), penalty)
    state.flags.writeable = False
    for a in regions.values():
        a.flags.writeable = False
    return state, regions
