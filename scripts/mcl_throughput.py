"""What Markov clustering costs beside the graph it runs on: NNEngine.graph_count_dev + graph_fill_dev, then NNEngine.mcl_dev on the CSR they
left on the device, on embedding-like rows resident on one GPU; and a float64 scipy.sparse MCL of the same graph on the host.

    python scripts/mcl_throughput.py [--n 262144] [--threshold 0.9] [--inflation 2] [--select 256] [--repeats 3] [--family 1000]
                                     [--planted 0.1] [--threads 16] [--host-seconds 600] [--lds-slots -1] [--out FILE]

The input is (b) of scripts/graph_throughput.py: n rows of tests.neighbours_data.rows with `--planted` of them in families of `--family`
(cliques at the threshold), scattered over all tiles.  One warm-up of the graph and of the clustering (the ctx's buffers grow once),
then `--repeats` rounds of [graph count, graph fill, mcl]; reported are the seconds of every call from the call to the synchronised
stream, the clustering's HIP-event time per pass (gnn_debug_mcl_ms: validate + symmetrise, the initial matrix, every iteration), the
columns every iteration changed, the columns every pass sent down the overflow path, and the clusters found.
The host comparison: the same loops, cutoff (1 / precision of the column's sum) and selection (the `select` largest) in float64 on
scipy.sparse CSC matrices, the expansion M @ M[:, block] spread over `--threads` threads, until no entry moves by more than 1e-9 or
`--host-seconds` are over; its seconds per iteration and whether its partition is the device's.
"""
import argparse
import json
import os
import socket
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.clusters_throughput import plant_families  # noqa: E402
from tests.neighbours_data import rows  # noqa: E402


def host_mcl(indptr, col, sim, inflation, select, precision, threads, budget):
    """float64 MCL on scipy.sparse: (labels, seconds per iteration, converged)"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    n = len(indptr) - 1
    a = np.repeat(np.arange(n), np.diff(indptr))
    keep = sim > 0
    a, b, w = a[keep], col[keep].astype(np.int64), sim[keep].astype(np.float64)
    loop = np.zeros(n)
    np.maximum.at(loop, a, w)
    np.maximum.at(loop, b, w)
    loop[loop == 0] = 1.0
    m = sp.csc_matrix((np.concatenate([w, w, loop]), (np.concatenate([a, b, np.arange(n)]), np.concatenate([b, a, np.arange(n)]))), shape=(n, n))

    def prune(m):
        m = m.tocsc()
        m.sort_indices()
        cj = np.repeat(np.arange(n), np.diff(m.indptr))
        ci, y = m.indices.astype(np.int64), m.data
        total = np.add.reduceat(y, m.indptr[:-1][np.diff(m.indptr) > 0])
        seg = np.cumsum(np.concatenate([[0], cj[1:] != cj[:-1]]))
        ok = y * precision >= total[seg]
        cj, ci, y = cj[ok], ci[ok], y[ok]
        order = np.lexsort((ci, -y, cj))
        cj, ci, y = cj[order], ci[order], y[order]
        first = np.flatnonzero(np.concatenate([[True], cj[1:] != cj[:-1]]))
        seg = np.cumsum(np.concatenate([[0], cj[1:] != cj[:-1]]))
        ok = np.arange(len(cj)) - first[seg] < select
        cj, ci, y = cj[ok], ci[ok], y[ok]
        out = sp.csc_matrix((y, (ci, cj)), shape=(n, n))
        out.sort_indices()
        s = np.asarray(out.sum(axis=0)).ravel()
        s[s == 0] = 1.0
        return out @ sp.diags(1.0 / s)

    m = prune(m)
    blocks = [(k, min(n, k + max(1, n // (4 * threads)))) for k in range(0, n, max(1, n // (4 * threads)))]
    seconds, converged, start = [], False, time.perf_counter()
    with ThreadPoolExecutor(threads) as pool:
        while time.perf_counter() - start < budget:
            t = time.perf_counter()
            parts = list(pool.map(lambda ab: m @ m[:, ab[0]:ab[1]], blocks))
            e = sp.hstack(parts, format="csc")
            top = np.maximum.reduceat(e.data, e.indptr[:-1][np.diff(e.indptr) > 0])
            e.data = (e.data / np.repeat(top, np.diff(e.indptr)[np.diff(e.indptr) > 0])) ** inflation
            nxt = prune(e)
            seconds.append(time.perf_counter() - t)
            d = abs(nxt - m)
            converged = d.nnz == 0 or d.data.max() <= 1e-9
            m = nxt
            if converged:
                break
    g = m.copy()
    g.data = (g.data > 1e-6).astype(np.float64)
    g.eliminate_zeros()
    _, comp = connected_components(g, directed=False)
    return comp, seconds, converged


def same_partition(x, y, valid) -> bool:
    """two labellings of the valid rows name the same sets"""
    x, y = x[valid], y[valid]
    fx = {}
    return all(fx.setdefault(a, b) == b for a, b in zip(x.tolist(), y.tolist())) and len(set(fx.values())) == len(fx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--threshold", type=float, default=0.9)
    ap.add_argument("--inflation", type=float, default=2.0)
    ap.add_argument("--select", type=int, default=256)
    ap.add_argument("--precision", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--family", type=int, default=1000)
    ap.add_argument("--planted", type=float, default=0.1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-seconds", type=float, default=600.0)
    ap.add_argument("--lds-slots", type=int, default=-1, help="slots of the LDS table (0: every column takes the overflow path); -1: the library's")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from genomad_amd import synthetic
    from genomad_amd.engine import NNEngine

    n = args.n
    data = rows(n, 7)
    planted = plant_families(data, args.planted, args.family, 8)
    eng = NNEngine(0, synthetic.synth_weights())
    info = eng.device_info()
    eng.profile_enable(True)
    eng.set_mcl_lds(args.lds_slots)
    q, indptr = eng.alloc(data.nbytes), eng.alloc((n + 1) * 8)
    outs = [eng.alloc(8 * n) for _ in range(3)] + [eng.alloc(4 * n), eng.alloc(n)]
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

    def mcl():
        state["res"] = eng.mcl_dev(indptr.ptr, edge_bufs[0].ptr, edge_bufs[1].ptr, n, state["total"], *(b.ptr for b in outs),
                                   inflation=args.inflation, select=args.select, precision=args.precision)
        state["pass_ms"], state["overflow"] = eng.mcl_pass_ms(), eng.mcl_overflow()

    try:
        q.upload(data)
        timed(count)
        edge_bufs += [eng.alloc(4 * max(state["total"], 1)), eng.alloc(4 * max(state["total"], 1))]
        timed(fill), timed(mcl)                                                 # warm-up: every buffer at its size
        t = {"count": [], "fill": [], "mcl": []}
        passes = []
        for _ in range(args.repeats):
            t["count"].append(timed(count))
            t["fill"].append(timed(fill))
            t["mcl"].append(timed(mcl))
            passes.append([round(float(x), 3) for x in state["pass_ms"]])
        res = state["res"]
        label = outs[0].download((n,), np.int64)
        size = outs[1].download((n,), np.int64)
        length = res.matrix()[0]
        graph = (indptr.download((n + 1,), np.int64), edge_bufs[0].download((state["total"],), np.int32),
                 edge_bufs[1].download((state["total"],), np.float32))
    finally:
        for b in [q, indptr] + outs + edge_bufs:
            b.free()
    box = {"device": info["name"], "cus": info["cus"], "pci_bus_id": eng.pci_bus_id(), "host": socket.gethostname()}
    eng.close()
    med = {k: statistics.median(v) for k, v in t.items()}
    per_iter = [statistics.median(p[2 + i] for p in passes if len(p) > 2 + i) for i in range(res.iterations)] if passes and len(passes[0]) > 2 else []
    roots = label == np.arange(n)
    r = {"planted_rows": planted, "edges": state["total"], "iterations": res.iterations, "converged": res.converged,
         "changed": res.changed.tolist(), "overflow_columns": state["overflow"].tolist(),
         "overflow_share": [round(float(x) / n, 6) for x in state["overflow"]],
         "clusters": int(roots.sum()), "clusters_of_family_size": int((size[roots] == args.family).sum()),
         "singletons": int((size[roots] == 1).sum()), "final_entries": int(length.sum()),
         "seconds": {k: [round(x, 4) for x in v] for k, v in t.items()}, "median": {k: round(v, 4) for k, v in med.items()},
         "pass_ms": passes, "setup_ms": statistics.median(p[0] for p in passes) if per_iter else None,
         "initial_ms": statistics.median(p[1] for p in passes) if per_iter else None, "iteration_ms": [round(x, 3) for x in per_iter],
         "mcl_over_graph": round(med["mcl"] / (med["count"] + med["fill"]), 3)}
    print(f"n = {n}, threshold {args.threshold:g}, {r['edges']} edges: count {med['count']:.3f} s, fill {med['fill']:.3f} s, mcl {med['mcl']:.3f} s "
          f"({res.iterations} iterations, {r['clusters']} clusters, {r['clusters_of_family_size']} of {args.family}) = "
          f"{r['mcl_over_graph']:.2f} x graph; overflow columns per pass {r['overflow_columns']}", flush=True)
    print(f"ms per iteration {r['iteration_ms']}; columns changed {r['changed']}", flush=True)
    if args.host_seconds > 0:
        th = time.perf_counter()
        comp, secs, conv = host_mcl(*graph, args.inflation, args.select, args.precision, args.threads, args.host_seconds)
        r["host"] = {"threads": args.threads, "seconds_total": round(time.perf_counter() - th, 2), "iterations": len(secs), "converged": conv,
                     "seconds_per_iteration": [round(x, 3) for x in secs], "clusters": int(len(np.unique(comp))),
                     "same_partition": bool(same_partition(comp, label, label >= 0))}
        print(f"host float64 scipy.sparse MCL on {args.threads} threads: {r['host']['seconds_total']} s, {len(secs)} iterations "
              f"({'converged' if conv else 'stopped'}), {r['host']['clusters']} clusters, the device's partition: {r['host']['same_partition']}", flush=True)
    out = {"box": box, "n": n, "threshold": args.threshold, "inflation": args.inflation, "select": args.select, "precision": args.precision,
           "lds_slots": args.lds_slots, "repeats": args.repeats, "family": args.family, "result": r}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
