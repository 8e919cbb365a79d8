"""What the match against a reference costs beside the neighbour search: NNEngine.match_count_dev + match_fill_dev and
NNEngine.neighbours_dev(k = 1) on the same embedding-like rows resident on one GPU, in one process, alternating passes.

    python scripts/match_throughput.py [--shapes 16384x262144,262144x262144] [--threshold 0.9] [--repeats 3] [--family 1000]
                                       [--planted 0.1] [--out FILE]

Per shape (n_query x n_base) two inputs (tests.neighbours_data.rows):
  (a) base and query rows of two different draws: at the threshold no pair is a match - the count pass alone, the fill has nothing
      to visit;
  (b) the base with `--planted` of its rows replaced by families of `--family` rows (centre + 0.15 * noise: cliques at the threshold),
      scattered over all ranges, and the queries a random subset of those base rows: every query matches itself, and one in ten its
      family - about n_query * (1 + planted * (family - 1)) matches.
Per input: one warm-up of either search (the ctx's buffers grow once), then `--repeats` rounds of [neighbours, match count, match fill];
reported are the seconds of every call from the call to the synchronised stream, the HIP-event time of its kernels (gnn_profile_get,
GNN_K_NEIGHBOURS: the difference around a call is that call's), the count call's own split into [count pass, scan]
(gnn_debug_match_pass_ms; the rest of its kernel time is the two prepare kernels), the medians, the spread (max - min) of the
baseline's own repeated passes, count / neighbours per input, and the matches found.  The expectation to confront: with no match the
count pass costs no more than neighbours(k = 1) on the same shapes - the products are the same, and a compare takes the place of a sorted
list -, the margin being the baseline's own spread.
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
    ap.add_argument("--shapes", default="16384x262144,262144x262144")
    ap.add_argument("--threshold", type=float, default=0.9)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--family", type=int, default=1000)
    ap.add_argument("--planted", type=float, default=0.1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from genomad_amd import _lib, synthetic
    from genomad_amd.engine import NNEngine

    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    eng = NNEngine(0, synthetic.synth_weights())
    info = eng.device_info()
    eng.profile_enable(True)
    results = {}

    def timed(call):
        k0 = eng.profile_get(_lib.K_NEIGHBOURS)[0]
        t = time.perf_counter()
        call()
        eng.sync()
        wall = time.perf_counter() - t
        return wall, (eng.profile_get(_lib.K_NEIGHBOURS)[0] - k0) * 1e-3

    for nq, nb in shapes:
        base = rows(nb, 7)
        bufs = {"q": eng.alloc(nq * 2048), "b": eng.alloc(nb * 2048), "indptr": eng.alloc((nq + 1) * 8), "idx": eng.alloc(nq * 8),
                "sim": eng.alloc(nq * 4)}
        edge_bufs = []
        state = {"total": 0, "pass_ms": []}

        def neighbours():
            eng.neighbours_dev(bufs["q"].ptr, nq, bufs["b"].ptr, nb, bufs["idx"].ptr, bufs["sim"].ptr, 1)

        def count():
            state["total"] = eng.match_count_dev(bufs["q"].ptr, nq, bufs["b"].ptr, nb, args.threshold, bufs["indptr"].ptr)
            state["pass_ms"] = list(eng.match_pass_ms())

        def fill():
            eng.match_fill_dev(bufs["q"].ptr, nq, bufs["b"].ptr, nb, args.threshold, edge_bufs[0].ptr if edge_bufs else None,
                               edge_bufs[1].ptr if edge_bufs else None, state["total"])

        try:
            for name in ("a_no_match", "b_planted"):
                if name == "a_no_match":
                    planted, query = 0, rows(nq, 9)
                else:
                    planted = plant_families(base, args.planted, args.family, 8)
                    query = base[np.sort(np.random.default_rng(10).permutation(nb)[:nq])]
                bufs["q"].upload(np.ascontiguousarray(query))
                bufs["b"].upload(base)
                timed(neighbours), timed(count)                                     # warm-up: every buffer at its size
                for b in edge_bufs:
                    b.free()
                del edge_bufs[:]
                if state["total"]:
                    edge_bufs += [eng.alloc(4 * state["total"]), eng.alloc(4 * state["total"])]
                timed(fill)
                t = {"neighbours": [], "count": [], "fill": []}
                passes = []
                for _ in range(args.repeats):                                       # alternating: drift hits all alike
                    t["neighbours"].append(timed(neighbours))
                    t["count"].append(timed(count))
                    passes.append(state["pass_ms"])
                    t["fill"].append(timed(fill))
                ptr = bufs["indptr"].download((nq + 1,), np.int64)
                best = bufs["sim"].download((nq,), np.float32)
                assert int(ptr[-1]) == state["total"], (int(ptr[-1]), state["total"])
                # a query has a match iff its nearest neighbour reaches the threshold: both searches compute the same f32
                assert np.array_equal(np.diff(ptr) > 0, best >= np.float32(args.threshold))
                r = {"planted_rows": planted, "edges": state["total"], "largest_segment": int(np.diff(ptr).max())}
                for what in t:
                    walls = [w for w, _ in t[what]]
                    r[what] = {"seconds": [round(w, 4) for w in walls], "kernel_seconds": [round(k, 4) for _, k in t[what]],
                               "median": round(statistics.median(walls), 4), "spread": round(max(walls) - min(walls), 4)}
                r["count"]["count_pass_ms"] = [round(p[0], 3) for p in passes if len(p) == 2]
                r["count"]["scan_ms"] = [round(p[1], 3) for p in passes if len(p) == 2]
                r["count_over_neighbours"] = round(r["count"]["median"] / r["neighbours"]["median"], 3)
                r["count_pass_over_neighbours_kernels"] = round(
                    statistics.median(r["count"]["count_pass_ms"] or [0]) * 1e-3 / statistics.median(k for _, k in t["neighbours"]), 3)
                r["fill_over_count"] = round(r["fill"]["median"] / r["count"]["median"], 3)
                r["pairs_per_second"] = round(nq * nb / (r["count"]["median"] + r["fill"]["median"]), 1)
                results[f"{nq}x{nb}_{name}"] = r
                print(f"{nq} x {nb} {name}, threshold {args.threshold:g}: neighbours(k=1) {r['neighbours']['median']:.4f} s "
                      f"(spread {r['neighbours']['spread']:.4f}), count {r['count']['median']:.4f} s (pass "
                      f"{statistics.median(r['count']['count_pass_ms'] or [0]):.3f} ms, scan {statistics.median(r['count']['scan_ms'] or [0]):.3f} ms), "
                      f"fill {r['fill']['median']:.4f} s: count = {r['count_over_neighbours']:.3f} x neighbours; {r['edges']} matches", flush=True)
        finally:
            for b in list(bufs.values()) + edge_bufs:
                b.free()
    out = {"box": {"device": info["name"], "cus": info["cus"], "pci_bus_id": eng.pci_bus_id(), "host": socket.gethostname()},
           "shapes": [list(s) for s in shapes], "threshold": args.threshold, "repeats": args.repeats, "family": args.family, "results": results}
    eng.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
