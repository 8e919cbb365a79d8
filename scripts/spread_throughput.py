"""What label spreading costs beside the graph it runs on: NNEngine.graph_count_dev + graph_fill_dev, then NNEngine.spread_dev on the CSR
they left on the device, on embedding-like rows resident on one GPU; and a float64 iteration of the same recurrence on the host.

    python scripts/spread_throughput.py [--n 262144] [--threshold 0.9] [--alpha 0.5] [--classes 3 64] [--max-iter 200] [--repeats 3]
                                        [--family 1000] [--planted 0.1] [--seeds 0.01] [--threads 16] [--host-iterations 20] [--out FILE]

The input is (b) of scripts/graph_throughput.py, as scripts/mcl_throughput.py has it: n rows of tests.neighbours_data.rows with
`--planted` of them in families of `--family` (cliques at the threshold), scattered over all tiles.  `--seeds` of every family's rows
carry a label: family f is of class f % classes; the seeds are clamped.  One warm-up of the graph and of the spreading (the ctx's buffers
grow once), then per class count and with the dirty-row rule on and off `--repeats` rounds of spread_dev; reported are the seconds of
every call from the call to the synchronised stream, the spreading's HIP-event time per pass (gnn_debug_spread_ms: validate +
symmetrise, then every iteration), the rows every iteration changed and the rows that got a label.
The host comparison: F <- alpha P F + (1 - alpha) Y with clamped seeds in float64, P the random-walk rows as a scipy.sparse CSR (numpy
add.at where scipy does not import; the result says which), the product spread over `--threads` threads by row blocks, for
`--host-iterations` iterations: its seconds per iteration.
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


def family_rows(n, fraction, family, seed):
    """where plant_families(data, fraction, family, seed) put its families: (families, family) row indices"""
    families = int(n * fraction) // family
    return np.random.default_rng(seed + 1).permutation(n)[:families * family].reshape(families, family)


def host_spread(indptr, col, sim, label, n_classes, alpha, threads, iterations):
    """float64 iterations of the recurrence: (what multiplied, seconds per iteration, the labels after them)"""
    n = len(indptr) - 1
    a = np.repeat(np.arange(n), np.diff(indptr))
    keep = sim > 0
    a, b, w = a[keep], col[keep].astype(np.int64), sim[keep].astype(np.float64)
    i, j, w = np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([w, w])
    d = np.bincount(i, weights=w, minlength=n)
    w = w / d[i]
    seed = label >= 0
    Y = np.zeros((n, n_classes))
    Y[np.flatnonzero(seed), label[seed]] = 1.0
    F = np.zeros((n, n_classes))
    try:
        import scipy.sparse as sp
        P = sp.csr_matrix((w, (i, j)), shape=(n, n))
        step = max(1, n // (4 * threads))
        blocks = [P[k:k + step] for k in range(0, n, step)]
        how = "scipy.sparse"

        def product(pool, F):
            return np.concatenate(list(pool.map(lambda blk: blk @ F, blocks)))
    except ImportError:
        how = "numpy add.at"

        def product(pool, F):
            g = np.zeros_like(F)
            np.add.at(g, i, w[:, None] * F[j])
            return g
    seconds = []
    with ThreadPoolExecutor(threads) as pool:
        for _ in range(iterations):
            t = time.perf_counter()
            nxt = alpha * product(pool, F) + (1 - alpha) * Y
            nxt[seed] = Y[seed]
            seconds.append(time.perf_counter() - t)
            F = nxt
    return how, seconds, np.where(F.max(axis=1) > 0, F.argmax(axis=1), -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--threshold", type=float, default=0.9)
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--classes", type=int, nargs="+", default=[3, 64])
    ap.add_argument("--max-iter", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--family", type=int, default=1000)
    ap.add_argument("--planted", type=float, default=0.1)
    ap.add_argument("--seeds", type=float, default=0.01)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-iterations", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from genomad_amd import synthetic
    from genomad_amd.engine import NNEngine

    n = args.n
    data = rows(n, 7)
    planted = plant_families(data, args.planted, args.family, 8)
    members = family_rows(n, args.planted, args.family, 8)
    per_family = max(1, int(round(args.family * args.seeds)))
    eng = NNEngine(0, synthetic.synth_weights())
    info = eng.device_info()
    eng.profile_enable(True)
    q, indptr, lab = eng.alloc(data.nbytes), eng.alloc((n + 1) * 8), eng.alloc(8 * n)
    outs = [eng.alloc(4 * n), eng.alloc(4 * n), eng.alloc(4 * n), eng.alloc(8 * n), eng.alloc(4 * n)]
    edge_bufs, state, results = [], {}, []

    def timed(call):
        t = time.perf_counter()
        call()
        eng.sync()
        return time.perf_counter() - t

    def count():
        state["total"] = eng.graph_count_dev(q.ptr, n, args.threshold, indptr.ptr)

    def fill():
        eng.graph_fill_dev(q.ptr, n, args.threshold, edge_bufs[0].ptr, edge_bufs[1].ptr, state["total"])

    def spread(c):
        state["res"] = eng.spread_dev(indptr.ptr, edge_bufs[0].ptr, edge_bufs[1].ptr, lab.ptr, n, state["total"], c, *(b.ptr for b in outs),
                                      alpha=args.alpha, clamp=True, max_iter=args.max_iter)
        state["pass_ms"] = eng.spread_pass_ms()

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
        graph = (indptr.download((n + 1,), np.int64), edge_bufs[0].download((state["total"],), np.int32),
                 edge_bufs[1].download((state["total"],), np.float32))
        for c in args.classes:
            label = np.full(n, -1, dtype=np.int64)
            for f in range(len(members)):
                label[members[f, :per_family]] = f % c
            lab.upload(label)
            entry = {"classes": c, "seeds": int((label >= 0).sum())}
            for skip in (True, False):
                eng.set_spread_skip(skip)
                timed(lambda: spread(c))                                       # warm-up: every buffer at its size
                secs, passes = [], []
                for _ in range(args.repeats):
                    secs.append(timed(lambda: spread(c)))
                    passes.append([round(float(x), 3) for x in state["pass_ms"]])
                res = state["res"]
                best = outs[0].download((n,), np.int32)
                per_iter = [round(statistics.median(p[1 + i] for p in passes), 3) for i in range(res.iterations)] if len(passes[0]) > 1 else []
                entry["dirty_rows_on" if skip else "dirty_rows_off"] = {
                    "seconds": [round(x, 4) for x in secs], "median": round(statistics.median(secs), 4),
                    "over_graph": round(statistics.median(secs) / graph_s, 3), "iterations": res.iterations, "converged": res.converged,
                    "changed": res.changed.tolist(), "setup_ms": statistics.median(p[0] for p in passes) if per_iter else None,
                    "iteration_ms": per_iter, "iteration_ms_sum": round(sum(per_iter), 3), "labelled": int((best >= 0).sum()),
                    "family_rows_labelled_right": int(sum((best[members[f]] == f % c).sum() for f in range(len(members))))}
                print(f"{c} classes, dirty-row rule {'on' if skip else 'off'}: spread_dev {statistics.median(secs):.4f} s = "
                      f"{statistics.median(secs) / graph_s:.3f} x graph; {res.iterations} iterations "
                      f"({'converged' if res.converged else 'not converged'}), ms per iteration {per_iter}", flush=True)
                state["best"] = best
            eng.set_spread_skip(True)
            if args.host_iterations > 0:
                th = time.perf_counter()
                how, hs, hbest = host_spread(*graph, label, c, args.alpha, args.threads, args.host_iterations)
                entry["host"] = {"how": how, "threads": args.threads, "iterations": len(hs), "seconds_total": round(time.perf_counter() - th, 2),
                                 "seconds_per_iteration": [round(x, 4) for x in hs],
                                 "same_labels_as_the_device": bool(np.array_equal(hbest, state["best"]))}
                print(f"host float64 {how} on {args.threads} threads, {c} classes: {statistics.median(hs):.4f} s per iteration (median of "
                      f"{len(hs)}), the device's labels: {entry['host']['same_labels_as_the_device']}", flush=True)
            results.append(entry)
    finally:
        for b in [q, indptr, lab] + outs + edge_bufs:
            b.free()
    box = {"device": info["name"], "cus": info["cus"], "pci_bus_id": eng.pci_bus_id(), "host": socket.gethostname()}
    eng.close()
    out = {"box": box, "n": n, "threshold": args.threshold, "alpha": args.alpha, "max_iter": args.max_iter, "repeats": args.repeats,
           "family": args.family, "planted_rows": planted, "seeds_per_family": per_family, "edges": state["total"],
           "graph_seconds": {k: [round(x, 4) for x in v] for k, v in g.items()}, "graph_median": round(graph_s, 4), "results": results}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
