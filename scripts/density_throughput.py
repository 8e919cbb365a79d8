"""What the density clusters cost beside the cluster search: NNEngine.density_dev at min_points 5 and 50 and NNEngine.cluster_dev at the
same threshold, on the same embedding-like rows resident on one GPU, in one process, interleaved.

    python scripts/density_throughput.py [--n 262144] [--threshold 0.9] [--repeats 3] [--family 1000] [--planted 0.1] [--out FILE]

Three inputs of n rows (tests.neighbours_data.rows: ReLU of a Gaussian with one power-of-two scale per channel), those of
scripts/clusters_throughput.py:
  (a) the rows as they are: at the threshold practically no pair is an edge - the count pass raises no flag, so every workgroup of the
      link pass leaves before it loads its tile: the expectation is near parity with cluster;
  (b) the same rows with `--planted` of them replaced by families of `--family` rows (centre + 0.15 * noise: cliques at the threshold),
      scattered over all tiles: practically every workgroup holds an edge, the link pass is a full pass: the expectation is up to two
      cluster passes;
  (c) the families of (b) plus one border row per family member, at other scattered places: the member turned by a signed direction
      to the cosine 0.94 - between the threshold and the family's own 0.98.  Such a row sees its whole family (about 1 000 core rows at
      0.92 to 0.94) and a few other border rows; a member sees its family and its family's border rows, about 1 999.  At min_points
      5 and 50 all of them are core, so (c) also runs at min_points = 1.5 x family: there the members are core and the border rows are
      border rows, as many as core rows, each with about 1 000 core neighbours for the 64-bit maxima of the link pass to choose among.
      The script asserts those kinds.  No expectation was derived for it: it is a record.
Per input: one warm-up of every call (the ctx's buffers grow once), then `--repeats` rounds of [cluster, density(5), density(50)] -
and density(1.5 x family) on (c) -;
reported are the seconds of every call from the call to the synchronised stream, the HIP-event time of its kernels (gnn_profile_get,
GNN_K_NEIGHBOURS - all file theirs there, so the difference around a call is that call's), the medians, density / cluster per input
and min_points with cluster's own pass-to-pass spread ((max - min) / median) beside it, and the clusters, core, border and noise rows
found.  The script asserts that density's degrees are cluster's.  No ratio is a condition.
"""
import argparse
import json
import os
import socket
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.clusters_throughput import plant_families  # noqa: E402
from tests.neighbours_data import rows  # noqa: E402

MIN_POINTS = (5, 50)
BORDER_COSINE = 0.94


def plant_borders(data, fraction, family, seed):
    """Input (c): plant_families' families - the same rows at the same places, made again here from its generator and its permutation -
    and, at the permutation's next places, one border row per member: |m| (0.94 m / |m| + sqrt(1 - 0.94^2) w / |w|), w a signed
    Gaussian with the generator's channel scales, made orthogonal to m.  Returns (places of the members, places of the border rows)."""
    n = len(data)
    families = int(n * fraction) // family
    planted = plant_families(data, fraction, family, seed)
    assert planted == families * family and 2 * planted <= n
    extra = rows(families * (family + 1), seed)
    where = np.random.default_rng(seed + 1).permutation(n)[:2 * planted]
    rng = np.random.default_rng(seed + 2)
    for f in range(families):
        at = where[f * family:(f + 1) * family]
        m = extra[families + f * family:families + (f + 1) * family] * np.float32(0.15) + extra[f]
        assert np.array_equal(data[at], m)                      # what plant_families put there
        m = m.astype(np.float64)
        norm = np.sqrt((m * m).sum(axis=1, keepdims=True))
        w = rng.standard_normal(m.shape) * np.abs(rows(family, seed + 3 + f))
        w -= (w * m).sum(axis=1, keepdims=True) * m / norm ** 2
        w /= np.sqrt((w * w).sum(axis=1, keepdims=True))
        border = BORDER_COSINE * m + np.sqrt(1 - BORDER_COSINE ** 2) * norm * w
        data[where[planted + f * family:planted + (f + 1) * family]] = border.astype(np.float32)
    return where[:planted], where[planted:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--threshold", type=float, default=0.9)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--family", type=int, default=1000)
    ap.add_argument("--planted", type=float, default=0.1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from genomad_amd import _lib, synthetic
    from genomad_amd.engine import NNEngine

    n = args.n
    eng = NNEngine(0, synthetic.synth_weights())
    info = eng.device_info()
    eng.profile_enable(True)
    data = rows(n, 7)
    q = eng.alloc(data.nbytes)
    c_outs = [eng.alloc(n * 8) for _ in range(4)]
    d_outs = [eng.alloc(n * 8) for _ in range(4)] + [eng.alloc(n * 4), eng.alloc(n)]
    results = {}

    def timed(call):
        k0 = eng.profile_get(_lib.K_NEIGHBOURS)[0]
        t = time.perf_counter()
        call()
        eng.sync()
        wall = time.perf_counter() - t
        return wall, (eng.profile_get(_lib.K_NEIGHBOURS)[0] - k0) * 1e-3

    def cluster():
        eng.cluster_dev(q.ptr, n, args.threshold, *(b.ptr for b in c_outs))

    def density(min_points):
        return lambda: eng.density_dev(q.ptr, n, args.threshold, min_points, *(b.ptr for b in d_outs))

    try:
        for name in ("a_no_edges", "b_planted", "c_borders"):
            planted, min_points = 0, MIN_POINTS
            if name == "b_planted":
                planted = plant_families(data, args.planted, args.family, 8)
            elif name == "c_borders":                                           # over (b)'s rows: the families are planted again, as they are
                members, borders = plant_borders(data, args.planted, args.family, 8)
                planted, min_points = len(members) + len(borders), MIN_POINTS + (3 * args.family // 2,)
            q.upload(data)
            calls = {"cluster": cluster, **{f"density_{m}": density(m) for m in min_points}}
            for call in calls.values():                                         # warm-up: every buffer at its size
                timed(call)
            t = {what: [] for what in calls}
            found = {}
            for _ in range(args.repeats):                                       # interleaved: drift hits all alike
                for what, call in calls.items():
                    t[what].append(timed(call))
                    if what != "cluster" and what not in found:
                        label, degree = d_outs[0].download((n,), np.int64), d_outs[1].download((n,), np.int64)
                        kind = d_outs[5].download((n,), np.uint8)
                        found[what] = {"clusters": int((label == np.arange(n)).sum()), "core": int((kind == 3).sum()),
                                       "border": int((kind == 2).sum()), "noise": int((kind == 1).sum())}
                        assert np.array_equal(degree, c_outs[1].download((n,), np.int64)), "density's degrees are not cluster's"
                        if name == "c_borders" and what == f"density_{min_points[-1]}":
                            assert (kind[members] == 3).all() and (kind[borders] == 2).all(), "the planted kinds"
                            anchor = d_outs[3].download((n,), np.int64)
                            assert np.isin(anchor[borders], members).all() and found[what]["border"] == len(borders)
            degree = c_outs[1].download((n,), np.int64)
            r = {"planted_rows": planted, "edges": int(degree.sum()) // 2, "largest_degree": int(degree.max())}
            for what in calls:
                walls = [w for w, _ in t[what]]
                med = statistics.median(walls)
                r[what] = {"seconds": [round(w, 4) for w in walls], "kernel_seconds": [round(k, 4) for _, k in t[what]],
                           "median": round(med, 4), "spread": round((max(walls) - min(walls)) / med, 4), **found.get(what, {})}
            for m in min_points:
                r[f"density_{m}_over_cluster"] = round(r[f"density_{m}"]["median"] / r["cluster"]["median"], 3)
            results[name] = r
            print(f"{name}: n = {n}, threshold {args.threshold:g}, {r['edges']} edges: cluster {r['cluster']['median']:.3f} s (spread "
                  f"{100 * r['cluster']['spread']:.1f} %); " +
                  "; ".join(f"density({m}) {r[f'density_{m}']['median']:.3f} s = {r[f'density_{m}_over_cluster']:.2f} x, "
                            f"{r[f'density_{m}']['clusters']} clusters, {r[f'density_{m}']['core']} core, {r[f'density_{m}']['border']} "
                            f"border" for m in min_points), flush=True)
    finally:
        for b in [q] + c_outs + d_outs:
            b.free()
    out = {"box": {"device": info["name"], "cus": info["cus"], "pci_bus_id": eng.pci_bus_id(), "host": socket.gethostname()},
           "n": n, "threshold": args.threshold, "repeats": args.repeats, "family": args.family, "min_points": list(MIN_POINTS),
           "min_points_c": list(MIN_POINTS) + [3 * args.family // 2], "border_cosine": BORDER_COSINE, "results": results}
    eng.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
