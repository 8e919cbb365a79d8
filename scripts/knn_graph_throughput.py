"""What the k-nearest-neighbour graph costs beside the neighbour search it starts with: NNEngine.knn_graph_count_dev + knn_graph_fill_dev in
both modes and both weights, and one NNEngine.neighbours_dev self-search at the same k, on the same embedding-like rows resident on one
GPU, in one process, interleaved.

    python scripts/knn_graph_throughput.py [--n 262144] [--ks 15,64] [--repeats 3] [--family 1000] [--planted 0.1] [--out FILE]

Two inputs of n rows (tests.neighbours_data.rows), those of scripts/graph_throughput.py:
  (a) the rows as they are: no structure, every list is noise;
  (b) the same rows with `--planted` of them replaced by families of `--family` rows (centre + 0.15 * noise), scattered over all tiles.
Per input and k: one warm-up of the search and of every (mode, weight) - the ctx's buffers grow once -, then `--repeats` rounds of
[search, then count + fill of every (mode, weight)]; reported are the seconds of every call from the call to the synchronised stream,
the medians, the call's time over the search's (count + fill, whose count holds a search of its own) and the per-pass split of the
count and the fill (gnn_debug_knn_graph_ms: [search, lists, count, scan] and [fill, order, finish]), the edges, the mutual ones and
the longest segment.  The assembly is O(n k) sparse work beside an O(n^2 512) search: the figure to confront is how far the ratio is
above 1.
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

COMBOS = (("union", "similarity"), ("union", "jaccard"), ("mutual", "similarity"), ("mutual", "jaccard"))
PASSES = ("search", "lists", "count", "scan", "fill", "order", "finish")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--ks", default="15,64")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--family", type=int, default=1000)
    ap.add_argument("--planted", type=float, default=0.1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from genomad_amd import synthetic
    from genomad_amd.engine import NNEngine

    n, ks = args.n, [int(k) for k in args.ks.split(",")]
    kmax = max(ks)
    eng = NNEngine(0, synthetic.synth_weights())
    info = eng.device_info()
    eng.profile_enable(True)
    data = rows(n, 7)
    q, indptr = eng.alloc(data.nbytes), eng.alloc((n + 1) * 8)
    idx, sim = eng.alloc(n * kmax * 8), eng.alloc(n * kmax * 4)
    col, val, flag = eng.alloc(n * kmax * 4), eng.alloc(n * kmax * 4), eng.alloc(n * kmax)       # at most n k edges: sized once
    results = {}

    def timed(call):
        t = time.perf_counter()
        out = call()
        eng.sync()
        return time.perf_counter() - t, out

    try:
        for name in ("a_no_structure", "b_planted"):
            planted = plant_families(data, args.planted, args.family, 8) if name == "b_planted" else 0
            q.upload(data)
            results[name] = {"planted_rows": planted}
            for k in ks:
                def search():
                    eng.neighbours_dev(q.ptr, n, None, 0, idx.ptr, sim.ptr, k)

                def graph(mode, weight):
                    kw = dict(k=k, mode=mode, weight=weight)
                    t_count, total = timed(lambda: eng.knn_graph_count_dev(q.ptr, n, indptr.ptr, **kw))
                    t_fill, _ = timed(lambda: eng.knn_graph_fill_dev(n, col.ptr, val.ptr, flag.ptr, n * kmax, **kw))
                    return t_count, t_fill, total, [float(x) for x in eng.knn_graph_pass_ms()]

                timed(search)                                                   # warm-up: every buffer at its size
                for mode, weight in COMBOS:
                    graph(mode, weight)
                t_search, runs = [], {c: [] for c in COMBOS}
                for _ in range(args.repeats):                                   # interleaved: drift hits all alike
                    t_search.append(timed(search)[0])
                    for c in COMBOS:
                        runs[c].append(graph(*c))
                med_search = statistics.median(t_search)
                r = {"search": {"seconds": [round(t, 4) for t in t_search], "median": round(med_search, 4)}}
                for c in COMBOS:
                    total = runs[c][-1][2]
                    ptr = indptr.download((n + 1,), np.int64) if c == COMBOS[-1] else None
                    call = statistics.median(a + b for a, b, _, _ in runs[c])
                    split = [statistics.median(p[3][i] for p in runs[c]) for i in range(len(PASSES))] if all(len(p[3]) == 7 for p in runs[c]) else []
                    r["_".join(c)] = {"count_seconds": [round(a, 4) for a, _, _, _ in runs[c]], "fill_seconds": [round(b, 4) for _, b, _, _ in runs[c]],
                                      "median": round(call, 4), "over_search": round(call / med_search, 3),
                                      "assembly_over_search": round((call - med_search) / med_search, 3), "edges": int(total),
                                      "pass_ms": {p: round(ms, 3) for p, ms in zip(PASSES, split)}}
                    if ptr is not None:
                        r["_".join(c)]["largest_segment"] = int(np.diff(ptr).max())
                    print(f"{name}, k = {k}, {c[0]} / {c[1]}: search {med_search:.3f} s, count + fill {call:.3f} s = {call / med_search:.2f} x the "
                          f"search; {total} edges; passes {r['_'.join(c)]['pass_ms']}", flush=True)
                results[name][f"k{k}"] = r
    finally:
        for b in (q, indptr, idx, sim, col, val, flag):
            b.free()
    out = {"box": {"device": info["name"], "cus": info["cus"], "pci_bus_id": eng.pci_bus_id(), "host": socket.gethostname()},
           "n": n, "ks": ks, "repeats": args.repeats, "family": args.family, "results": results}
    eng.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
