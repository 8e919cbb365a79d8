"""What the single-linkage tree costs beside one threshold's clusters: NNEngine.linkage_dev and NNEngine.cluster_dev on the same
embedding-like rows resident on one GPU, in one process, interleaved.

    python scripts/linkage_throughput.py [--n 262144] [--threshold 0.9] [--repeats 2] [--family 1000] [--planted 0.1] [--out FILE]

The two inputs of scripts/representatives_throughput.py (tests.neighbours_data.rows):
  (a) the rows as they are: practically no structure - components are scattered over the tiles, so no wave skips before the tree is
      whole and every round is a full pass over the upper triangle;
  (b) the same rows with `--planted` of them in families of `--family` rows, scattered.
Per input: one warm-up of either search (the ctx's buffers grow once), then `--repeats` rounds of [cluster, linkage]; reported are the
seconds of every call from the call to its return (linkage) or to the synchronised stream (cluster), the HIP-event time of its kernels
(gnn_profile_get, GNN_K_NEIGHBOURS - both searches file theirs there, so the difference around a call is that call's), the medians,
linkage / cluster, `rounds`, the HIP-event time of every round of the last call (gnn_debug_linkage_round_ms; the last entry is the
round that found nothing to add, where one ran), the mean round over cluster's pass, and the edges of the tree.  The expectation:
rounds x one cluster pass, rounds <= ceil(log2 n).  Nothing here is a bar.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--threshold", type=float, default=0.9)
    ap.add_argument("--repeats", type=int, default=2)
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
    cl_outs = [eng.alloc(n * 8) for _ in range(4)]
    results, state = {}, {}

    def timed(call):
        k0 = eng.profile_get(_lib.K_NEIGHBOURS)[0]
        t = time.perf_counter()
        call()
        eng.sync()
        wall = time.perf_counter() - t
        return wall, (eng.profile_get(_lib.K_NEIGHBOURS)[0] - k0) * 1e-3

    def cluster():
        eng.cluster_dev(q.ptr, n, args.threshold, *(b.ptr for b in cl_outs))

    def linkage():
        state["res"] = eng.linkage_dev(q.ptr, n)

    try:
        for name in ("a_no_structure", "b_planted"):
            planted = plant_families(data, args.planted, args.family, 8) if name == "b_planted" else 0
            q.upload(data)
            timed(cluster), timed(linkage)                                      # warm-up: every buffer at its size
            t = {"cluster": [], "linkage": []}
            for _ in range(args.repeats):                                       # interleaved: drift hits both alike
                t["cluster"].append(timed(cluster))
                t["linkage"].append(timed(linkage))
            round_ms, res = eng.linkage_round_ms(), state["res"]
            label = cl_outs[0].download((n,), np.int64)
            r = {"planted_rows": planted, "clusters_at_threshold": int((label == np.arange(n)).sum()),
                 "clusters_at_threshold_from_the_tree": int(res.cluster_counts([args.threshold])[0]), "n_edges": res.n_edges,
                 "n_valid": res.n_valid, "rounds": res.rounds, "round_ms": [round(float(m), 3) for m in round_ms]}
            for what in t:
                med = statistics.median(w for w, _ in t[what])
                r[what] = {"seconds": [round(w, 4) for w, _ in t[what]], "kernel_seconds": [round(k, 4) for _, k in t[what]],
                           "median": round(med, 4), "median_kernel_seconds": round(statistics.median(k for _, k in t[what]), 4)}
            r["linkage_over_cluster"] = round(r["linkage"]["median"] / r["cluster"]["median"], 3)
            adding = round_ms[:res.rounds]
            r["mean_round_over_cluster_pass"] = (round(float(adding.mean()) * 1e-3 / r["cluster"]["median_kernel_seconds"], 3)
                                                 if len(adding) else None)
            results[name] = r
            print(f"{name}: n = {n}: cluster at {args.threshold:g} {r['cluster']['median']:.3f} s, linkage {r['linkage']['median']:.3f} s = "
                  f"{r['linkage_over_cluster']:.2f} x in {r['rounds']} rounds (a round = {r['mean_round_over_cluster_pass']} cluster "
                  f"passes; ms per round {r['round_ms']}); {r['n_edges']} edges, {r['clusters_at_threshold']} clusters at the threshold",
                  flush=True)
    finally:
        for b in [q] + cl_outs:
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
