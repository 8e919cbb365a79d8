"""What one iteration of the exact t-SNE layout costs, beside the k-nearest-neighbour graph that feeds it: NNEngine.knn_graph_count_dev +
knn_graph_fill_dev once, then NNEngine.tsne_dev over that graph, on embedding-like rows resident on one GPU, in one process; and, for
context, scikit-learn's TSNE(method="exact") on a subset on the CPU.

    python scripts/tsne_throughput.py [--n 262144] [--k 15] [--iters 20] [--repeats 3] [--splits 0] [--sklearn 4096] [--out FILE]

The rows are tests.neighbours_data.rows with 10 % of them in families of 1 000 (scripts/clusters_throughput.plant_families), the
input (b) of scripts/knn_graph_throughput.py.  One warm-up of the graph and of the layout - the ctx's buffers grow once -, then
`--repeats` layouts of `--iters` iterations, half of them exaggerated, from the hash init.  Reported: the seconds of the graph's
count + fill, the seconds of every layout from the call to the synchronised stream, the HIP-event milliseconds of its [setup, loop,
finish] (gnn_debug_tsne_ms) and the loop's time per iteration - n^2 pairs each -, as pairs per second.  `--splits` (comma separated,
0: the library's choice) repeats the layouts for other splits of the repel pass's columns.  `--sklearn N` (0: skip it) fits
TSNE(method="exact", init="random") on the first N rows for 250 iterations, the least scikit-learn runs, and reports its seconds per
iteration; scikit-learn's affinities are perplexity-calibrated and dense, ours the graph's: the two runs share the n^2 repulsion only.
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
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--splits", default="0")
    ap.add_argument("--sklearn", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from genomad_amd import sequence, synthetic
    from genomad_amd.engine import NNEngine

    n, k, iters = args.n, args.k, args.iters
    eng = NNEngine(0, synthetic.synth_weights())
    info = eng.device_info()
    eng.profile_enable(True)
    data = rows(n, 7)
    planted = plant_families(data, 0.1, 1000, 8)
    q, indptr = eng.alloc(data.nbytes), eng.alloc((n + 1) * 8)
    col, val, flag = eng.alloc(n * k * 4), eng.alloc(n * k * 4), eng.alloc(n * k)            # at most n k edges
    init, layout, z_trace, valid = eng.alloc(n * 8), eng.alloc(n * 8), eng.alloc((iters + 1) * 8), eng.alloc(n)
    results = {"planted_rows": planted}

    def timed(call):
        t = time.perf_counter()
        out = call()
        eng.sync()
        return time.perf_counter() - t, out

    def graph():
        t_count, total = timed(lambda: eng.knn_graph_count_dev(q.ptr, n, indptr.ptr, k=k))
        t_fill, _ = timed(lambda: eng.knn_graph_fill_dev(n, col.ptr, val.ptr, flag.ptr, n * k, k=k))
        return t_count + t_fill, total

    try:
        q.upload(data)
        init.upload(sequence.tsne_init(n))
        graph()                                                                 # warm-up
        t_graph, nnz = graph()
        results["knn_graph"] = {"seconds": round(t_graph, 4), "edges": int(nnz)}
        print(f"knn_graph, k = {k}: {t_graph:.3f} s, {nnz} edges", flush=True)

        def lay(n_iter):
            return timed(lambda: eng.tsne_dev(indptr.ptr, col.ptr, val.ptr, n, int(nnz), init.ptr, layout.ptr, z_trace.ptr, valid.ptr,
                                              n_iter=n_iter, exaggeration_iter=n_iter // 2))[0]

        lay(1)                                                                  # warm-up: every buffer at its size
        for split in [int(s) for s in args.splits.split(",")]:
            eng.set_tsne_split(split)
            secs, passes = [], []
            for _ in range(args.repeats):
                secs.append(lay(iters))
                passes.append([float(x) for x in eng.tsne_pass_ms()])
            z = z_trace.download((iters + 1,), np.uint64)
            med = [statistics.median(p[i] for p in passes) for i in range(3)] if all(len(p) == 3 for p in passes) else []
            r = {"seconds": [round(t, 4) for t in secs], "median": round(statistics.median(secs), 4), "z_first": int(z[0]), "z_last": int(z[-1])}
            if med:
                per = med[1] / iters
                r.update(pass_ms={"setup": round(med[0], 3), "loop": round(med[1], 3), "finish": round(med[2], 3)},
                         ms_per_iteration=round(per, 3), pairs_per_second=round(float(n) * n / (per * 1e-3), 0),
                         iteration_over_graph=round(per * 1e-3 / t_graph, 4))
            results[f"split{split}"] = r
            print(f"tsne, split {split}: {iters} iterations in {r['median']:.3f} s; {r.get('pass_ms')}; "
                  f"{r.get('ms_per_iteration')} ms per iteration = {r.get('pairs_per_second', 0):.3g} pairs/s", flush=True)
        eng.set_tsne_split(0)
    finally:
        for b in (q, indptr, col, val, flag, init, layout, z_trace, valid):
            b.free()
    if args.sklearn > 0:
        try:
            from sklearn.manifold import TSNE
            m = min(args.sklearn, n)
            t = time.perf_counter()
            fit = TSNE(n_components=2, method="exact", init="random", random_state=0, max_iter=250, n_iter_without_progress=250).fit(data[:m])
            dt = time.perf_counter() - t
            results["sklearn_exact"] = {"rows": m, "iterations": int(fit.n_iter_), "seconds": round(dt, 3),
                                        "ms_per_iteration": round(1e3 * dt / max(int(fit.n_iter_), 1), 3), "threads": os.cpu_count()}
            print(f"scikit-learn TSNE(method='exact') on {m} rows: {dt:.1f} s for {fit.n_iter_} iterations", flush=True)
        except Exception as exc:  # noqa: BLE001  (context only: the measurement above stands without it)
            results["sklearn_exact"] = {"error": f"{type(exc).__name__}: {exc}"}
    out = {"box": {"device": info["name"], "cus": info["cus"], "pci_bus_id": eng.pci_bus_id(), "host": socket.gethostname()},
           "n": n, "k": k, "iterations": iters, "repeats": args.repeats, "results": results}
    eng.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
