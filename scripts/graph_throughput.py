"""What the similarity graph costs beside the cluster search: NNEngine.graph_count_dev + graph_fill_dev and NNEngine.cluster_dev at the same
threshold on the same embedding-like rows resident on one GPU, in one process, interleaved.

    python scripts/graph_throughput.py [--n 262144] [--threshold 0.9] [--repeats 3] [--family 1000] [--planted 0.1] [--out FILE]

Two inputs of n rows (tests.neighbours_data.rows), those of scripts/clusters_throughput.py:
  (a) the rows as they are: at the threshold practically no pair is an edge - the count pass alone, the fill has nothing to visit;
  (b) the same rows with `--planted` of them replaced by families of `--family` rows (centre + 0.15 * noise: cliques at the threshold),
      scattered over all tiles: about n * planted * (family - 1) / 2 edges, and few (tile, part) workgroups without one.
Per input: one warm-up of either search (the ctx's buffers grow once), then `--repeats` rounds of [cluster, graph count, graph fill];
reported are the seconds of every call from the call to the synchronised stream, the HIP-event time of its kernels (gnn_profile_get,
GNN_K_NEIGHBOURS: the difference around a call is that call's), the count call's own split into [count pass, scan]
(gnn_debug_graph_pass_ms; the rest of its kernel time is the prepare kernel), the medians, graph / cluster and fill / count per input,
and the edges found.  The expectation to confront: count = one cluster pass (the same products, no joins), fill = that pass times the
share of (tile, part) workgroups that hold an edge: graph = 1 x cluster on (a), 2 x on (b).
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
    q, indptr = eng.alloc(data.nbytes), eng.alloc((n + 1) * 8)
    outs = [eng.alloc(n * 8) for _ in range(4)]
    edge_bufs = []
    results = {}
    state = {"total": 0, "pass_ms": []}

    def timed(call):
        k0 = eng.profile_get(_lib.K_NEIGHBOURS)[0]
        t = time.perf_counter()
        call()
        eng.sync()
        wall = time.perf_counter() - t
        return wall, (eng.profile_get(_lib.K_NEIGHBOURS)[0] - k0) * 1e-3

    def cluster():
        eng.cluster_dev(q.ptr, n, args.threshold, *(b.ptr for b in outs))

    def count():
        state["total"] = eng.graph_count_dev(q.ptr, n, args.threshold, indptr.ptr)
        state["pass_ms"] = list(eng.graph_pass_ms())

    def fill():
        eng.graph_fill_dev(q.ptr, n, args.threshold, edge_bufs[0].ptr if edge_bufs else None, edge_bufs[1].ptr if edge_bufs else None,
                           state["total"])

    try:
        for name in ("a_no_edges", "b_planted"):
            planted = plant_families(data, args.planted, args.family, 8) if name == "b_planted" else 0
            q.upload(data)
            timed(cluster), timed(count)                                        # warm-up: every buffer at its size
            for b in edge_bufs:
                b.free()
            del edge_bufs[:]
            if state["total"]:
                edge_bufs += [eng.alloc(4 * state["total"]), eng.alloc(4 * state["total"])]
            timed(fill)
            t = {"cluster": [], "count": [], "fill": []}
            passes = []
            for _ in range(args.repeats):                                       # interleaved: drift hits all alike
                t["cluster"].append(timed(cluster))
                t["count"].append(timed(count))
                passes.append(state["pass_ms"])
                t["fill"].append(timed(fill))
            degree = outs[1].download((n,), np.int64)
            ptr = indptr.download((n + 1,), np.int64)
            assert int(ptr[-1]) == state["total"] == int(degree.sum()) // 2, (int(ptr[-1]), state["total"], int(degree.sum()) // 2)
            r = {"planted_rows": planted, "edges": state["total"], "largest_segment": int(np.diff(ptr).max())}
            for what in t:
                med = statistics.median(w for w, _ in t[what])
                r[what] = {"seconds": [round(w, 4) for w, _ in t[what]], "kernel_seconds": [round(k, 4) for _, k in t[what]],
                           "median": round(med, 4)}
            r["count"]["count_pass_ms"] = [round(p[0], 3) for p in passes if len(p) == 2]
            r["count"]["scan_ms"] = [round(p[1], 3) for p in passes if len(p) == 2]
            graph = r["count"]["median"] + r["fill"]["median"]
            r["graph_over_cluster"] = round(graph / r["cluster"]["median"], 3)
            r["count_over_cluster"] = round(r["count"]["median"] / r["cluster"]["median"], 3)
            r["fill_over_count"] = round(r["fill"]["median"] / r["count"]["median"], 3)
            r["pairs_per_second"] = round(n * (n - 1) / 2.0 / graph, 1)
            results[name] = r
            print(f"{name}: n = {n}, threshold {args.threshold:g}: cluster {r['cluster']['median']:.3f} s, count {r['count']['median']:.3f} s "
                  f"(scan {statistics.median(r['count']['scan_ms'] or [0]):.3f} ms), fill {r['fill']['median']:.3f} s: graph = "
                  f"{r['graph_over_cluster']:.2f} x cluster; {r['edges']} edges", flush=True)
    finally:
        for b in [q, indptr] + outs + edge_bufs:
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
