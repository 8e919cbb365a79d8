"""What the cluster search costs beside the neighbour search: NNEngine.cluster_dev and NNEngine.neighbours_dev (k = 1, the self-search)
on the same embedding-like rows resident on one GPU, in one process, interleaved.

    python scripts/clusters_throughput.py [--n 262144] [--threshold 0.9] [--repeats 3] [--family 1000] [--planted 0.1] [--out FILE]

Two inputs of n rows (tests.neighbours_data.rows: ReLU of a Gaussian with one power-of-two scale per channel):
  (a) the rows as they are: at the threshold practically no pair is an edge - the cost of the upper triangle and of looking at it;
  (b) the same rows with `--planted` of them replaced by families of `--family` rows (centre + 0.15 * noise: cliques at the threshold),
      scattered: about n * planted * (family - 1) / 2 edges - what the degree counts and the union-find add.
Per input: one warm-up of either search (the ctx's buffers grow once), then `--repeats` rounds of [neighbours k = 1, cluster]; reported
are the seconds of every call from the call to the synchronised stream, the HIP-event time of its kernels (gnn_profile_get,
GNN_K_NEIGHBOURS - both searches file theirs there, so the difference around a call is that call's), the medians, cluster / neighbours
per input, (b) / (a) for cluster, pairs per second (n (n - 1) / 2 for cluster), and the clusters and edges found.  The condition of (a):
cluster is not slower than neighbours(k = 1) - it issues half the MFMAs and keeps no lists.
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

from tests.neighbours_data import rows  # noqa: E402


def plant_families(data, fraction, family, seed):
    """`fraction` of the rows, at scattered places, become families of `family` rows: centre + 0.15 * noise, centre and noise rows of
    the same generator.  Returns the number of planted rows."""
    n = len(data)
    families = int(n * fraction) // family
    if families == 0:
        return 0
    extra = rows(families * (family + 1), seed)
    where = np.random.default_rng(seed + 1).permutation(n)[:families * family]
    for f in range(families):
        data[where[f * family:(f + 1) * family]] = extra[families + f * family:families + (f + 1) * family] * np.float32(0.15) + extra[f]
    return families * family


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
    q, idx, sim = eng.alloc(data.nbytes), eng.alloc(n * 8), eng.alloc(n * 4)
    outs = [eng.alloc(n * 8) for _ in range(4)]
    results = {}

    def timed(call):
        k0 = eng.profile_get(_lib.K_NEIGHBOURS)[0]
        t = time.perf_counter()
        call()
        eng.sync()
        wall = time.perf_counter() - t
        return wall, (eng.profile_get(_lib.K_NEIGHBOURS)[0] - k0) * 1e-3

    def neighbours():
        eng.neighbours_dev(q.ptr, n, None, 0, idx.ptr, sim.ptr, 1)

    def cluster():
        eng.cluster_dev(q.ptr, n, args.threshold, *(b.ptr for b in outs))

    try:
        for name in ("a_no_edges", "b_planted"):
            planted = plant_families(data, args.planted, args.family, 8) if name == "b_planted" else 0
            q.upload(data)
            timed(neighbours), timed(cluster)                                   # warm-up: every buffer at its size
            t = {"neighbours_k1": [], "cluster": []}
            for _ in range(args.repeats):                                       # interleaved: drift hits both alike
                t["neighbours_k1"].append(timed(neighbours))
                t["cluster"].append(timed(cluster))
            label, degree = outs[0].download((n,), np.int64), outs[1].download((n,), np.int64)
            r = {"planted_rows": planted, "clusters": int((label == np.arange(n)).sum()), "edges": int(degree.sum()) // 2,
                 "largest_degree": int(degree.max())}
            for what, pairs in (("neighbours_k1", float(n) * n), ("cluster", n * (n - 1) / 2.0)):
                med = statistics.median(w for w, _ in t[what])
                r[what] = {"seconds": [round(w, 4) for w, _ in t[what]], "kernel_seconds": [round(k, 4) for _, k in t[what]],
                           "median": round(med, 4), "pairs_per_second": round(pairs / med, 1)}
            r["cluster_over_neighbours_k1"] = round(r["cluster"]["median"] / r["neighbours_k1"]["median"], 3)
            results[name] = r
            print(f"{name}: n = {n}, threshold {args.threshold:g}: neighbours(k = 1) {r['neighbours_k1']['median']:.3f} s, cluster "
                  f"{r['cluster']['median']:.3f} s = {r['cluster_over_neighbours_k1']:.2f} x; {r['edges']} edges, {r['clusters']} clusters",
                  flush=True)
        results["cluster_b_over_a"] = round(results["b_planted"]["cluster"]["median"] / results["a_no_edges"]["cluster"]["median"], 3)
    finally:
        for b in [q, idx, sim] + outs:
            b.free()
    out = {"box": {"device": info["name"], "cus": info["cus"], "pci_bus_id": eng.pci_bus_id(), "host": socket.gethostname()},
           "n": n, "threshold": args.threshold, "repeats": args.repeats, "family": args.family, "results": results}
    eng.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
