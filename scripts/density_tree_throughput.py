"""What the density-aware linkage tree costs beside the single-linkage tree and the neighbour search it is made of:
NNEngine.density_tree_dev at min_points 5 and 65, NNEngine.linkage_dev and NNEngine.neighbours_dev(k = min_points - 1) on the same
embedding-like rows resident on one GPU, in one process, interleaved.

    python scripts/density_tree_throughput.py [--n 262144] [--repeats 3] [--family 1000] [--planted 0.1] [--out FILE]

The two inputs of scripts/linkage_throughput.py: (a) rows without structure, (b) the same with `--planted` of them in families of
`--family` rows.  Per input: one warm-up of every call (the ctx's buffers grow once), then `--repeats` passes of [linkage,
neighbours k = 4, density_tree m = 5, neighbours k = 64, density_tree m = 65]; reported per call are the HIP-event seconds of its
kernels (gnn_profile_get, GNN_K_NEIGHBOURS: every search files its kernels there, so the difference around a call is that call's),
the wall seconds from the call to the synchronised stream, medians, the spread (max - min) of every series - linkage's is the
baseline's own -, the rounds, and the HIP-event time of every round of the last call of each tree.  The expectation to test: a round
of the density tree costs linkage's round plus two minima and one 4-byte read per column and step, and the whole call about one
neighbours pass plus the rounds.  Nothing here is a bar.
"""
import argparse
import json
import os
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.clusters_throughput import plant_families  # noqa: E402
from tests.neighbours_data import rows  # noqa: E402

MS = (5, 65)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
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
    idx, sim = eng.alloc(n * 64 * 8), eng.alloc(n * 64 * 4)
    results, state = {}, {}

    def timed(call):
        k0 = eng.profile_get(_lib.K_NEIGHBOURS)[0]
        t = time.perf_counter()
        call()
        eng.sync()
        wall = time.perf_counter() - t
        return wall, (eng.profile_get(_lib.K_NEIGHBOURS)[0] - k0) * 1e-3

    def linkage():
        state["linkage"] = eng.linkage_dev(q.ptr, n), eng.linkage_round_ms()

    def tree(m):
        def call():
            state[f"density_tree_m{m}"] = eng.density_tree_dev(q.ptr, n, m), eng.density_tree_round_ms()
        return call

    def neighbours(m):
        return lambda: eng.neighbours_dev(q.ptr, n, None, n, idx.ptr, sim.ptr, m - 1)

    calls = [("linkage", linkage)]
    for m in MS:
        calls += [(f"neighbours_k{m - 1}", neighbours(m)), (f"density_tree_m{m}", tree(m))]
    try:
        for name in ("a_no_structure", "b_planted"):
            planted = plant_families(data, args.planted, args.family, 8) if name == "b_planted" else 0
            q.upload(data)
            for _, call in calls:                                               # warm-up: every buffer at its size
                timed(call)
            t = {what: [] for what, _ in calls}
            for _ in range(args.repeats):                                       # interleaved: drift hits all alike
                for what, call in calls:
                    t[what].append(timed(call))
            r = {"planted_rows": planted}
            for what in t:
                ks, ws = [k for _, k in t[what]], [w for w, _ in t[what]]
                r[what] = {"kernel_seconds": [round(k, 4) for k in ks], "seconds": [round(w, 4) for w in ws],
                           "median_kernel_seconds": round(statistics.median(ks), 4), "median": round(statistics.median(ws), 4),
                           "spread_kernel_seconds": round(max(ks) - min(ks), 4), "spread": round(max(ws) - min(ws), 4)}
            for what in ("linkage",) + tuple(f"density_tree_m{m}" for m in MS):
                res, round_ms = state[what]
                r[what].update(rounds=res.rounds, n_edges=res.n_edges, round_ms=[round(float(x), 3) for x in round_ms],
                               mean_adding_round_ms=round(float(round_ms[:res.rounds].mean()), 3) if res.rounds else None)
            for m in MS:
                d, nb, lk = r[f"density_tree_m{m}"], r[f"neighbours_k{m - 1}"], r["linkage"]
                d["round_over_linkage_round"] = round(d["mean_adding_round_ms"] / lk["mean_adding_round_ms"], 4)
                d["kernels_minus_rounds_over_neighbours"] = round((d["median_kernel_seconds"] - sum(d["round_ms"]) * 1e-3)
                                                                  / nb["median_kernel_seconds"], 4)
                d["over_linkage"] = round(d["median"] / lk["median"], 3)
            results[name] = r
            print(f"{name}: n = {n}: " + "; ".join(
                f"{what} {r[what]['median']:.3f} s (kernels {r[what]['median_kernel_seconds']:.3f}, spread {r[what]['spread']:.4f})"
                + (f" in {r[what]['rounds']} rounds of {r[what]['mean_adding_round_ms']} ms" if "rounds" in r[what] else "")
                for what in t), flush=True)
    finally:
        for b in (q, idx, sim):
            b.free()
    out = {"box": {"device": info["name"], "cus": info["cus"], "pci_bus_id": eng.pci_bus_id(), "host": socket.gethostname()},
           "n": n, "repeats": args.repeats, "family": args.family, "results": results}
    eng.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
