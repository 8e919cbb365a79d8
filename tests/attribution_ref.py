"""Reference attention contribution maps in numpy, from the fp64 oracle's taps and the weights (TEST INFRASTRUCTURE ONLY).

The encoder ends in feat[h*128 + ch] = sum_q alpha[h][q] yp[h][q][ch]; the dense head behind it is piecewise linear, so for the window's
own ReLU pattern logit_c = g_c . feat + bias_c and

    contrib[h][q][c] = alpha[h][q] * sum_ch yp[h][q][ch] g_c[h*128 + ch],        sum_h sum_q contrib + bias_c = logit_c.

BatchNormalization is folded into the Dense before it, as the library does at gnn_load_weights.  The masks are the oracle's own
(h1 > 0, h2 > 0).  The 32-window reference of the tests is computed once per process (about 15 s of oracle time)."""
import functools

import numpy as np

from genomad_amd import synthetic
from oracle import igloo_oracle, sequence_oracle

POOLED, CH = 749, 128


def folded_head(weights, dtype=np.float64):
    """(D1, b1, D2, b2, D3, b3): y = gamma (x K + b - mean) / sqrt(var + eps) + beta = x (K s) + ((b - mean) s + beta)"""
    w = {k: np.asarray(v).astype(dtype) for k, v in weights.items() if np.asarray(v).dtype.kind == "f"}
    out = []
    for p in ("enc", "head"):
        s = w[f"{p}_bn_gamma"] / np.sqrt(w[f"{p}_bn_var"] + dtype(igloo_oracle.BN_EPS))
        out += [w[f"{p}_dense_kernel"] * s, (w[f"{p}_dense_bias"] - w[f"{p}_bn_mean"]) * s + w[f"{p}_bn_beta"]]
    return (*out, w["out_dense_kernel"], w["out_dense_bias"])


def maps_from_taps(taps, weights, dtype=np.float64):
    """taps of igloo_oracle.forward(..., return_taps=True) -> dict(contrib (n, 2, 749, 3), bias, logits, g (n, 256, 3), f (n, 256),
    pre1, pre2: the pre-activations of both hidden layers)"""
    d1, b1, d2, b2, d3, b3 = folded_head(weights, dtype)
    f, h1, h2 = (np.asarray(taps[k], dtype) for k in ("f", "h1", "h2"))
    pre1 = f @ d1 + b1
    pre2 = h1 @ d2 + b2
    v2 = (h2 > 0)[:, :, None] * d3[None]                                    # (n, 512, 3)
    v1 = (h1 > 0)[:, :, None] * np.einsum("jk,nkc->njc", d2, v2)
    g = np.einsum("ij,njc->nic", d1, v1)                                    # (n, 256, 3)
    bias = b3 + np.einsum("k,nkc->nc", b2, v2) + np.einsum("j,njc->nc", b1, v1)
    contrib = np.stack([np.asarray(taps[f"alpha{h}"], dtype)[:, :, None]
                        * np.einsum("nqd,ndc->nqc", np.asarray(taps[f"yp{h}"], dtype), g[:, i * CH:(i + 1) * CH])
                        for i, h in enumerate("AB")], axis=1)
    return dict(contrib=contrib, bias=bias, logits=np.asarray(taps["logits"], dtype), g=g, f=f, pre1=pre1, pre2=pre2)


def reference_maps(bases, weights, dtype=np.float64, batch=16):
    parts = []
    for a in range(0, len(bases), batch):
        _, taps = igloo_oracle.forward(sequence_oracle.tokenize_closed_form(bases[a:a + batch]), weights, dtype, literal=False,
                                       return_taps=True)
        parts.append(maps_from_taps(taps, weights, dtype))
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


@functools.lru_cache(maxsize=None)
def reference_32():
    """(bases, fp64 maps) of synth_windows(0, 32) under synth_weights(): what the host and the GPU tests compare against.  Read only."""
    bases = synthetic.synth_windows(0, 32)
    ref = reference_maps(bases, synthetic.synth_weights(), np.float64)
    for v in ref.values():
        v.setflags(write=False)
    return bases, ref


def margins(ref):
    """per window: the smallest |pre-activation| of both hidden layers, and max |h1|"""
    return (np.minimum(np.abs(ref["pre1"]).min(axis=1), np.abs(ref["pre2"]).min(axis=1)), np.maximum(ref["pre1"], 0).max(axis=1))


def decided(ref, tol=1e-4, scaled=False):
    """Which windows' maps are compared with the device's: those whose every pre-activation is farther from zero than the margin, so
    that no unit can legitimately sit on the other side of its ReLU.  scaled: the margin tol * max(1, max |h1|), the project's bound
    on the h1 error.  On the 32 test windows max |h1| is 5.5 .. 7.6, that margin is 5.5e-4 .. 7.6e-4 and 8 windows fall inside it
    (smallest pre-activations 9.1e-5, 1.3e-4, 1.8e-4, 3.0e-4, 4.0e-4, 4.6e-4, 5.7e-4, 5.9e-4) - more than the 2 the tests may leave
    out.  The tests therefore use the plain margin tol: every window the scaled rule compares and seven more, 1 left out.
    The price: the project's bound on the h1 error of these windows is the scaled margin, about 6.5e-4, so a unit of the seven
    extra windows (pre-activations 1.3e-4 .. 5.9e-4) may legitimately flip under another arithmetic or compiler and fail the parity
    test although nothing is wrong.  The arithmetics of today sit within 1e-5 of the oracle there and flip none."""
    small, h1max = margins(ref)
    return small > (tol * np.maximum(1.0, h1max) if scaled else tol)


def binned(contrib1, bin):
    """the map at `bin` from the bin = 1 map (n, 2, 749, 3) float32: per bin the sequential f32 sum in increasing q"""
    nb = -(-POOLED // bin)
    out = np.empty(contrib1.shape[:2] + (nb, 3), np.float32)
    for b in range(nb):
        out[:, :, b] = np.cumsum(contrib1[:, :, b * bin:min((b + 1) * bin, POOLED)], axis=2, dtype=np.float32)[:, :, -1]
    return out
