"""What modularity communities cost beside the graph they run on and beside the graph's other consumers: NNEngine.graph_count_dev +
graph_fill_dev, then NNEngine.communities_dev, mcl_dev and average_linkage_dev on the CSR they left on the device, in one process, on
embedding-like rows resident on one GPU; and networkx's Louvain on the host.

    python scripts/communities_throughput.py [--n 262144] [--threshold 0.9] [--resolution 1.0] [--repeats 3] [--family 1000]
                                             [--planted 0.1] [--host-n 16384] [--out FILE]

The input is (b) of scripts/graph_throughput.py, as scripts/mcl_throughput.py and scripts/average_linkage_throughput.py have it: n
rows of tests.neighbours_data.rows with `--planted` of them in families of `--family` (cliques at the threshold), scattered over all
tiles.  One warm-up of every call (the ctx's buffers grow once), then `--repeats` rounds; reported are the seconds of every call from
the call to the synchronised stream, the communities' HIP-event time per pass (gnn_debug_communities_ms: setup, then per level every
sweep and - behind a level with an accepted sweep - its end), the per-level counters, how many rows the want launches and the
contractions took by class (one wave, one workgroup, the accumulator in global memory) and whether the planted families come out
whole and alone.  The host figure: networkx.community.louvain_communities on the graph of the first `--host-n` rows (the graph
itself comes from the device; the seconds are Louvain's alone, one thread).  `--host-n 0` leaves it out.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.clusters_throughput import plant_families  # noqa: E402
from scripts.spread_throughput import family_rows  # noqa: E402
from tests.neighbours_data import rows  # noqa: E402

AVGLINK_RECORDS = (np.int32, np.uint64, np.int32, np.int32, np.int32)
MCL_RECORDS = (np.int64, np.int64, np.int64, np.uint32, np.uint8)


def host_louvain(eng, data, threshold, resolution):
    """networkx's Louvain on the device's graph of ``data``: (edges, seconds, communities, modularity), or None"""
    try:
        import networkx as nx
    except ImportError:
        return None
    g = eng.graph(np.ascontiguousarray(data), threshold)
    a, b, sim = g.edges()
    h = nx.Graph()
    h.add_nodes_from(range(len(data)))
    h.add_weighted_edges_from(zip(a.tolist(), b.tolist(), np.rint(sim.astype(np.float64) * (1 << 24)).tolist()))
    t = time.perf_counter()
    found = nx.community.louvain_communities(h, weight="weight", resolution=resolution, seed=0)
    secs = time.perf_counter() - t
    return len(a), secs, len(found), nx.community.modularity(h, found, weight="weight", resolution=resolution)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--threshold", type=float, default=0.9)
    ap.add_argument("--resolution", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--family", type=int, default=1000)
    ap.add_argument("--planted", type=float, default=0.1)
    ap.add_argument("--host-n", type=int, default=16384)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from genomad_amd import synthetic
    from genomad_amd.engine import NNEngine

    n = args.n
    data = rows(n, 7)
    planted = plant_families(data, args.planted, args.family, 8)
    members = family_rows(n, args.planted, args.family, 8)
    eng = NNEngine(0, synthetic.synth_weights())
    info = eng.device_info()
    eng.profile_enable(True)
    q, indptr = eng.alloc(data.nbytes), eng.alloc((n + 1) * 8)
    outs = [eng.alloc(8 * n), eng.alloc(8 * n), eng.alloc(8 * n * 32)]
    others = [eng.alloc(8 * n) for _ in range(5)]                    # the records of mcl_dev and average_linkage_dev, in turn
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

    def communities():
        state["res"] = eng.communities_dev(indptr.ptr, edge_bufs[0].ptr, edge_bufs[1].ptr, n, state["total"], *(b.ptr for b in outs),
                                           resolution=args.resolution)
        state["pass_ms"] = eng.communities_pass_ms()
        state["classes"] = eng.communities_classes()

    def mcl():
        state["mcl"] = eng.mcl_dev(indptr.ptr, edge_bufs[0].ptr, edge_bufs[1].ptr, n, state["total"], *(b.ptr for b in others))

    def avglink():
        state["avl"] = eng.average_linkage_dev(indptr.ptr, edge_bufs[0].ptr, edge_bufs[1].ptr, n, state["total"], *(b.ptr for b in others),
                                               stop=args.threshold)

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
        beside = {}
        for name, call in (("mcl_dev", mcl), ("average_linkage_dev", avglink)):
            timed(call)
            beside[name] = round(statistics.median(timed(call) for _ in range(args.repeats)), 4)
        timed(communities)                                           # warm-up: every buffer at its size
        secs, passes = [], []
        for _ in range(args.repeats):
            secs.append(timed(communities))
            passes.append([round(float(x), 3) for x in state["pass_ms"]])
        res = state["res"]
        label = outs[0].download((n,), np.int64)
    finally:
        for b in [q, indptr] + outs + others + edge_bufs:
            b.free()
    whole = int(sum(len(set(label[m].tolist())) == 1 and int((label == label[m[0]]).sum()) == len(m) for m in members))
    median = [round(statistics.median(p[i] for p in passes), 3) for i in range(len(passes[0]))]
    levels, at = [], 1
    for l in range(res.levels):                                      # [setup], then per level its sweeps and - if one was accepted - its end
        s = int(res.sweeps[l])
        sweep_ms = median[at:at + s]
        at += s
        end_ms = None
        if res.accepted[l]:
            end_ms, at = median[at], at + 1
        levels.append({**{k: int(getattr(res, k)[l]) for k in ("nodes", "communities", "sweeps", "accepted", "moved", "rejected", "split")},
                       "qnum": str(res.qnum[l]), "sweep_ms": sweep_ms, "end_ms": end_ms})
    classes = [int(x) for x in state["classes"]]
    names = ("wave", "workgroup", "dense")
    result = {"seconds": [round(x, 4) for x in secs], "median": round(statistics.median(secs), 4),
              "over_graph": round(statistics.median(secs) / graph_s, 3), "levels": res.levels, "complete": res.complete,
              "modularity": res.modularity, "communities": int(np.count_nonzero(label == np.arange(n))), "m2": res.m2,
              "setup_ms": median[0] if median else None, "per_level": levels,
              "want_rows_by_class": dict(zip(names, classes[:3])), "contraction_rows_by_class": dict(zip(names, classes[3:])),
              "families": len(members), "families_whole_and_alone": whole}
    print(f"communities_dev {result['median']:.4f} s = {result['over_graph']:.3f} x graph ({graph_s:.4f} s); beside {beside}; "
          f"{res.levels} levels, sweeps {res.sweeps.tolist()}, modularity {res.modularity:.4f}, {result['communities']} communities; "
          f"{whole} of {len(members)} families whole and alone", flush=True)
    host = None
    if args.host_n > 0:
        hs = host_louvain(eng, data[:args.host_n], args.threshold, args.resolution)
        host = None if hs is None else {"rows": args.host_n, "edges": hs[0], "louvain_seconds": round(hs[1], 2), "communities": hs[2],
                                        "modularity": hs[3]}
        print(f"networkx Louvain on {args.host_n} rows: {host}", flush=True)
    box = {"device": info["name"], "cus": info["cus"]}
    eng.close()
    out = {"box": box, "n": n, "threshold": args.threshold, "resolution": args.resolution, "repeats": args.repeats, "family": args.family,
           "planted_rows": planted, "edges": state["total"], "graph_seconds": {k: [round(x, 4) for x in v] for k, v in g.items()},
           "graph_median": round(graph_s, 4), "beside": beside, "result": result, "host": host}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
