"""What average linkage costs beside the graph it runs on: NNEngine.graph_count_dev + graph_fill_dev, then NNEngine.average_linkage_dev
on the CSR they left on the device, on embedding-like rows resident on one GPU; and SciPy's dense average linkage on the host.

    python scripts/average_linkage_throughput.py [--n 262144] [--threshold 0.9] [--cut 0.9] [--repeats 3] [--family 1000]
                                                 [--planted 0.1] [--host-n 16384] [--threads 16] [--out FILE]

The input is (b) of scripts/graph_throughput.py, as scripts/mcl_throughput.py and scripts/spread_throughput.py have it: n rows of
tests.neighbours_data.rows with `--planted` of them in families of `--family` (cliques at the threshold), scattered over all tiles.
One warm-up of the graph and of the tree (the ctx's buffers grow once), then `--repeats` rounds of average_linkage_dev with stop =
`--cut`; reported are the seconds of every call from the call to the synchronised stream, the tree's HIP-event time per pass
(gnn_debug_avglink_ms: validate + symmetrise, then every round), the pairs every round merged, how many rows the contractions took
by class (one wave, one workgroup, the accumulator in global memory) and whether the planted families come out at the cut.
The host comparison: scipy.cluster.hierarchy.linkage(method="average") on the condensed cosine distances of the first `--host-n`
rows of the same input (a 16 384-row condensed matrix is 1 GB of float64), with the BLAS that builds the distances on `--threads`
threads; SciPy's linkage itself is one thread.  `--host-n 0` leaves it out.
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
from scripts.spread_throughput import family_rows  # noqa: E402
from tests.neighbours_data import rows  # noqa: E402

RECORDS = (("parent", np.int32), ("weight", np.uint64), ("size_a", np.int32), ("size_b", np.int32), ("round", np.int32))


def host_average_linkage(data, threads):
    """SciPy's dense average linkage of the rows' cosine distances: (seconds of the distances, seconds of the linkage), or None"""
    try:
        from scipy.cluster.hierarchy import linkage
    except ImportError:
        return None
    os.environ.setdefault("OMP_NUM_THREADS", str(threads))
    t = time.perf_counter()
    r = data.astype(np.float64)
    r /= np.sqrt((r * r).sum(axis=1))[:, None]
    d = 1.0 - r @ r.T
    cond = d[np.triu_indices(len(r), 1)]
    del d
    td = time.perf_counter() - t
    t = time.perf_counter()
    linkage(cond, "average")
    return td, time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--threshold", type=float, default=0.9)
    ap.add_argument("--cut", type=float, default=0.9)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--family", type=int, default=1000)
    ap.add_argument("--planted", type=float, default=0.1)
    ap.add_argument("--host-n", type=int, default=16384)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from genomad_amd import sequence, synthetic
    from genomad_amd.engine import NNEngine

    n = args.n
    data = rows(n, 7)
    planted = plant_families(data, args.planted, args.family, 8)
    members = family_rows(n, args.planted, args.family, 8)
    eng = NNEngine(0, synthetic.synth_weights())
    info = eng.device_info()
    eng.profile_enable(True)
    q, indptr = eng.alloc(data.nbytes), eng.alloc((n + 1) * 8)
    outs = [eng.alloc(np.dtype(t).itemsize * n) for _, t in RECORDS]
    edge_bufs, state = [], {}

    def timed(call):
        t = time.perf_counter()
        call()
        eng.sync()
        return time.perf_counter() - t

    def count():
        state["total"] = eng.graph_count_dev(q.ptr, n, args.threshold, indptr.ptr)

    def fill():
        eng.graph_fill_dev(q.ptr, n, args.threshold, edge_bufs[0].ptr, edge_bufs[1].ptr, state["total"])

    def tree():
        state["res"] = eng.average_linkage_dev(indptr.ptr, edge_bufs[0].ptr, edge_bufs[1].ptr, n, state["total"], *(b.ptr for b in outs),
                                               stop=args.cut)
        state["pass_ms"] = eng.average_linkage_pass_ms()
        state["classes"] = eng.average_linkage_classes()

    try:
        q.upload(data)
        timed(count)
        edge_bufs += [eng.alloc(4 * max(state["total"], 1)), eng.alloc(4 * max(state["total"], 1))]
        timed(fill)
        g = {"count": [], "fill": []}
        for _ in range(args.repeats):
            g["count"].append(timed(count))
            g["fill"].append(timed(fill))
        graph_s = statistics.median(g["count"]) + statistics.median(g["fill"])
        timed(tree)                                                  # warm-up: every buffer at its size
        secs, passes = [], []
        for _ in range(args.repeats):
            secs.append(timed(tree))
            passes.append([round(float(x), 3) for x in state["pass_ms"]])
        res = state["res"]
        rec = {k: b.download((n,), t) for (k, t), b in zip(RECORDS, outs)}
    finally:
        for b in [q, indptr] + outs + edge_bufs:
            b.free()
    # the labels at the cut: every recorded merge reached it (stop = the cut), so a node's cluster is the end of its parent chain
    label = np.arange(n)
    absorbed = rec["parent"] >= 0
    label[absorbed] = rec["parent"][absorbed]
    while True:                                                      # ends: a chain of parents falls and stops at a cluster's id
        nxt = label[label]
        if np.array_equal(nxt, label):
            break
        label = nxt
    whole = int(sum(len(set(label[m].tolist())) == 1 and int((label == label[m[0]]).sum()) == len(m) for m in members))
    per_round = [round(statistics.median(p[1 + i] for p in passes), 3) for i in range(res.rounds)] if len(passes[0]) > 1 else []
    classes = [int(x) for x in state["classes"]]
    result = {"seconds": [round(x, 4) for x in secs], "median": round(statistics.median(secs), 4),
              "over_graph": round(statistics.median(secs) / graph_s, 3), "rounds": res.rounds, "complete": res.complete,
              "merged_per_round": res.merged_per_round.tolist(), "merges": int(absorbed.sum()),
              "setup_ms": statistics.median(p[0] for p in passes) if per_round else None, "round_ms": per_round,
              "round_ms_sum": round(sum(per_round), 3), "rows_by_class": dict(zip(("wave", "workgroup", "dense"), classes)),
              "families": len(members), "families_whole_and_alone_at_the_cut": whole, "stop_q": sequence.average_linkage_stop(args.cut)}
    print(f"average_linkage_dev {result['median']:.4f} s = {result['over_graph']:.3f} x graph ({graph_s:.4f} s); {res.rounds} rounds, "
          f"{result['merges']} merges; rows by class {result['rows_by_class']}; {whole} of {len(members)} families whole and alone at the cut",
          flush=True)
    host = None
    if args.host_n > 0:
        hs = host_average_linkage(data[:args.host_n], args.threads)
        host = None if hs is None else {"rows": args.host_n, "threads": args.threads, "distances_seconds": round(hs[0], 2),
                                        "linkage_seconds": round(hs[1], 2)}
        print(f"SciPy dense average linkage of {args.host_n} rows: {host}", flush=True)
    box = {"device": info["name"], "cus": info["cus"], "pci_bus_id": eng.pci_bus_id(), "host": socket.gethostname()}
    eng.close()
    out = {"box": box, "n": n, "threshold": args.threshold, "cut": args.cut, "repeats": args.repeats, "family": args.family,
           "planted_rows": planted, "edges": state["total"], "graph_seconds": {k: [round(x, 4) for x in v] for k, v in g.items()},
           "graph_median": round(graph_s, 4), "result": result, "host": host}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
