"""What an iteration of the spherical k-means costs beside what a user pays today: NNEngine.kmeans_dev against one
NNEngine.neighbours_dev(rows, centroids, k=1) - the assignment of a host-side k-means, before its group sum in numpy - on the same
embedding-like rows resident on one GPU, in one process, interleaved.

    python scripts/kmeans_throughput.py [--n 262144] [--k 2 64 1024] [--iterations 3] [--repeats 3] [--init-k 2 64] [--out FILE]

Two inputs of n rows (tests.neighbours_data.rows: ReLU of a Gaussian with one power-of-two scale per channel), those of
scripts/clusters_throughput.py: (a) the rows as they are, without structure; (b) the same rows with `--planted` of them replaced by
families of `--family` rows, scattered over all tiles.  Per input and k: the init is the first k rows (given, so that the iterations
are those of the loop alone), max_iter = `--iterations`; one warm-up of every call (the ctx's buffers grow once), then `--repeats`
rounds of [neighbours_dev(k=1) against the k init rows, kmeans_dev].  Reported: the baseline's seconds from the call to the
synchronised stream, its median and spread ((max - min) / median); the HIP-event milliseconds of every iteration's assign (with the
label kernel), update, finish and prepare (gnn_debug_kmeans_pass_ms) and their medians; iteration / baseline.  At k <= 128 the update
runs twice, with its sums pre-aggregated in LDS, 16 centroids at a time (the default), and straight to memory
(gnn_debug_set_kmeans_lds 0): both are reported.  For every k of `--init-k`: the farthest-first traversal (init=None, max_iter=0),
its milliseconds per pick.  No ratio is a condition: the script asserts only that the labels of kmeans_dev at max_iter = 0 are
neighbours_dev's indices against the centroids returned.
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


def passes(ms):
    """[init, then per assignment: assign, and behind every one but the last: update, finish, prepare] -> (init, assigns, updates,
    finishes + prepares)"""
    body = list(ms[1:])
    return float(ms[0]), body[0::4], body[1::4], [f + p for f, p in zip(body[2::4], body[3::4])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--k", type=int, nargs="+", default=[2, 64, 1024])
    ap.add_argument("--init-k", type=int, nargs="*", default=[2, 64])
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--family", type=int, default=1000)
    ap.add_argument("--planted", type=float, default=0.1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from genomad_amd import synthetic
    from genomad_amd.engine import NNEngine

    n, kmax = args.n, max(args.k + args.init_k)
    eng = NNEngine(0, synthetic.synth_weights())
    info = eng.device_info()
    eng.profile_enable(True)
    data = rows(n, 7)
    q = eng.alloc(data.nbytes)
    idx, sim = eng.alloc(n * 8), eng.alloc(n * 4)
    outs = [eng.alloc(n * 8), eng.alloc(n * 4), eng.alloc(kmax * 2048), eng.alloc(kmax * 8), eng.alloc(kmax * 8)]
    results = {}
    med = statistics.median
    try:
        for name in ("a_no_structure", "b_planted"):
            if name == "b_planted":
                plant_families(data, args.planted, args.family, 8)
            q.upload(data)
            results[name] = {}
            for k in args.k:
                def baseline():
                    t = time.perf_counter()
                    eng.neighbours_dev(q.ptr, n, q.ptr, k, idx.ptr, sim.ptr, 1)          # the base: the first k rows
                    eng.sync()
                    return time.perf_counter() - t

                def kmeans(max_iter, lds=128):
                    eng.set_kmeans_lds(lds)
                    t = time.perf_counter()
                    it, conv = eng.kmeans_dev(q.ptr, n, k, *(b.ptr for b in outs), init_ptr=q.ptr, max_iter=max_iter)
                    eng.sync()
                    return time.perf_counter() - t, it, conv, passes(eng.kmeans_pass_ms())

                baseline()
                kmeans(0)                                                               # warm-up, and the one assertion
                eng.neighbours_dev(q.ptr, n, outs[2].ptr, k, idx.ptr, sim.ptr, 1)        # against the centroids returned
                eng.sync()
                assert np.array_equal(outs[0].download((n,), np.int64), idx.download((n,), np.int64)), "kmeans' labels are not neighbours'"
                kmeans(args.iterations)
                base, assign, update, finish, update_mem, walls, its = [], [], [], [], [], [], []
                for _ in range(args.repeats):                                           # interleaved: drift hits all alike
                    base.append(baseline())
                    wall, it, conv, (_, a, u, f) = kmeans(args.iterations)
                    walls.append(wall), its.append(it), assign.extend(a), update.extend(u), finish.extend(f)
                    if k <= 128:
                        update_mem.extend(kmeans(args.iterations, 0)[3][2])
                r = {"baseline_seconds": [round(b, 5) for b in base], "baseline_median": round(med(base), 5),
                     "baseline_spread": round((max(base) - min(base)) / med(base), 4), "iterations": its,
                     "kmeans_seconds": [round(w, 5) for w in walls], "assign_ms": [round(x, 3) for x in assign],
                     "update_ms": [round(x, 3) for x in update], "finish_prepare_ms": [round(x, 3) for x in finish],
                     "assign_median_ms": round(med(assign), 3), "update_median_ms": round(med(update), 3) if update else None,
                     "finish_prepare_median_ms": round(med(finish), 3) if finish else None}
                if update_mem:
                    r["update_straight_to_memory_ms"] = [round(x, 3) for x in update_mem]
                    r["update_straight_to_memory_median_ms"] = round(med(update_mem), 3)
                if update:
                    r["iteration_median_ms"] = round(med(assign) + med(update) + med(finish), 3)
                    r["iteration_over_baseline"] = round(r["iteration_median_ms"] * 1e-3 / med(base), 3)
                r["assign_over_baseline"] = round(med(assign) * 1e-3 / med(base), 3)
                results[name][f"k{k}"] = r
                print(f"{name}, k = {k}: neighbours_dev(k=1) {1e3 * med(base):.3f} ms (spread {100 * r['baseline_spread']:.1f} %); assign "
                      f"{r['assign_median_ms']} ms, update {r['update_median_ms']} ms"
                      + (f" (straight to memory {r['update_straight_to_memory_median_ms']} ms)" if update_mem else "")
                      + f", finish + prepare {r['finish_prepare_median_ms']} ms; iteration / baseline {r.get('iteration_over_baseline')}",
                      flush=True)
            for k in args.init_k:
                per_pick = []
                for _ in range(args.repeats + 1):
                    eng.kmeans_dev(q.ptr, n, k, *(b.ptr for b in outs), init_ptr=None, max_iter=0)
                    eng.sync()
                    per_pick.append(float(eng.kmeans_pass_ms()[0]) / k)
                results[name][f"init_k{k}"] = {"ms_per_pick": [round(x, 4) for x in per_pick[1:]], "median": round(med(per_pick[1:]), 4)}
                print(f"{name}, farthest-first, k = {k}: {med(per_pick[1:]):.4f} ms per pick", flush=True)
    finally:
        eng.set_kmeans_lds(128)
        for b in [q, idx, sim] + outs:
            b.free()
    out = {"box": {"device": info["name"], "cus": info["cus"], "pci_bus_id": eng.pci_bus_id(), "host": socket.gethostname()},
           "n": n, "k": args.k, "init_k": args.init_k, "max_iter": args.iterations, "repeats": args.repeats, "family": args.family,
           "planted": args.planted, "results": results}
    eng.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
