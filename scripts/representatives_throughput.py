"""What the greedy clustering costs beside the single-linkage one: NNEngine.representatives_dev and NNEngine.cluster_dev on the same
embedding-like rows resident on one GPU, in one process, interleaved.

    python scripts/representatives_throughput.py [--n 262144] [--threshold 0.9] [--repeats 3] [--family 1000] [--planted 0.1] [--out FILE]

The two inputs of scripts/clusters_throughput.py (tests.neighbours_data.rows; the rows are taken in index order):
  (a) the rows as they are: at the threshold practically no pair is an edge - one full pass over the upper triangle, one decide, no
      assign: the same MFMAs as cluster and a cheaper epilogue (an OR per column instead of degree counts and joins);
  (b) the same rows with `--planted` of them in families of `--family` rows (cliques at the threshold), scattered: the first round is
      the full pass, the later ones touch only tiles and column blocks that still hold live rows, then the assign pass.
Per input: one warm-up of either search (the ctx's buffers grow once), then `--repeats` rounds of [cluster, representatives]; reported
are the seconds of every call from the call to the synchronised stream, the HIP-event time of its kernels (gnn_profile_get,
GNN_K_NEIGHBOURS - both searches file theirs there, so the difference around a call is that call's), the medians, representatives /
cluster per input, `rounds`, the HIP-event time of every round of the last call (gnn_debug_representative_round_ms) and what the
rounds after the first cost as a fraction of the first.  The expectation of (a): parity with cluster - allowed the spread cluster's
own repeated passes show, plus one round's synchronise; reported as `a_within_spread`.  (b) has no bar.
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
    cl_outs = [eng.alloc(n * 8) for _ in range(4)]
    rp_outs = [eng.alloc(n * 8), eng.alloc(n * 4), eng.alloc(n * 8)]
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

    def representatives():
        state["rounds"] = eng.representatives_dev(q.ptr, n, args.threshold, *(b.ptr for b in rp_outs))

    try:
        for name in ("a_no_edges", "b_planted"):
            planted = plant_families(data, args.planted, args.family, 8) if name == "b_planted" else 0
            q.upload(data)
            timed(cluster), timed(representatives)                              # warm-up: every buffer at its size
            t = {"cluster": [], "representatives": []}
            for _ in range(args.repeats):                                       # interleaved: drift hits both alike
                t["cluster"].append(timed(cluster))
                t["representatives"].append(timed(representatives))
            round_ms = eng.representative_round_ms()
            label, rep = cl_outs[0].download((n,), np.int64), rp_outs[0].download((n,), np.int64)
            r = {"planted_rows": planted, "single_linkage_clusters": int((label == np.arange(n)).sum()),
                 "n_representatives": int((rep == np.arange(n)).sum()), "rounds": int(state["rounds"]),
                 "round_ms": [round(float(m), 3) for m in round_ms],
                 "later_rounds_over_first": round(float(round_ms[1:].sum() / round_ms[0]), 4) if len(round_ms) else None}
            for what in t:
                med = statistics.median(w for w, _ in t[what])
                r[what] = {"seconds": [round(w, 4) for w, _ in t[what]], "kernel_seconds": [round(k, 4) for _, k in t[what]],
                           "median": round(med, 4), "pairs_per_second": round(n * (n - 1) / 2.0 / med, 1)}
            r["representatives_over_cluster"] = round(r["representatives"]["median"] / r["cluster"]["median"], 3)
            results[name] = r
            print(f"{name}: n = {n}, threshold {args.threshold:g}: cluster {r['cluster']['median']:.3f} s, representatives "
                  f"{r['representatives']['median']:.3f} s = {r['representatives_over_cluster']:.2f} x in {r['rounds']} rounds "
                  f"(later rounds / first {r['later_rounds_over_first']}); {r['n_representatives']} representatives, "
                  f"{r['single_linkage_clusters']} single-linkage clusters", flush=True)
        a = results["a_no_edges"]
        spread = max(a["cluster"]["seconds"]) - min(a["cluster"]["seconds"])
        sync = a["representatives"]["median"] - statistics.median(a["representatives"]["kernel_seconds"])     # host gaps of the call
        results["a_cluster_spread_seconds"] = round(spread, 4)
        results["a_within_spread"] = bool(a["representatives"]["median"] <= a["cluster"]["median"] + spread + max(sync, 0.0))
    finally:
        for b in [q] + cl_outs + rp_outs:
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
