"""What the label transfer costs beside the match's count pass: NNEngine.vote_dev and NNEngine.match_count_dev on the same
embedding-like rows resident on one GPU, in one process, alternating passes, timed by HIP events.

    python scripts/votes_throughput.py [--shapes 16384x262144,262144x262144] [--dense 16384x16384] [--threshold 0.9] [--repeats 3]
                                       [--family 1000] [--planted 0.1] [--out FILE]

The baseline is the count pass of the match (gnn_debug_match_pass_ms, entry 0): existing code with the same tile skeleton and the same
edge rule.  Beside it the vote pass (gnn_debug_vote_pass_ms, entry 1: the clears and the tile kernel) in three variants: 3 classes on
the LDS path, 3 classes straight to memory (gnn_debug_set_vote_lds 0) and 64 classes (always straight to memory).  Every base row
carries a label drawn uniformly from the classes.
Per shape (n_query x n_base) two inputs (tests.neighbours_data.rows):
  (a) base and query rows of two different draws: at the threshold no pair votes - the vote pass does the count pass's work and
      nothing more;
  (b) the base with `--planted` of its rows replaced by families of `--family` rows, scattered over all ranges, and the queries a
      random subset of those base rows: every query hears itself, and one in ten its family.
and on `--dense` (c): threshold -1, where every pair votes.
Per input: one warm-up of each call, then `--repeats` rounds of [count, vote LDS, vote memory, vote 64]; reported are the HIP-event
milliseconds of every pass, the medians, the spread (max - min) of the baseline's own passes and each variant's ratio to the
baseline.  The one condition: on (a) a variant's median lies within the baseline's own spread of the baseline's median, as measured in
the same run.  On every input the script asserts that the votes are as many as the match's edges.
"""
import argparse
import json
import os
import socket
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.clusters_throughput import plant_families  # noqa: E402
from tests.neighbours_data import rows  # noqa: E402

VARIANTS = (("vote_3_lds", 3, 16), ("vote_3_memory", 3, 0), ("vote_64_memory", 64, 16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16384x262144,262144x262144")
    ap.add_argument("--dense", default="16384x16384")
    ap.add_argument("--threshold", type=float, default=0.9)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--family", type=int, default=1000)
    ap.add_argument("--planted", type=float, default=0.1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from genomad_amd import synthetic
    from genomad_amd.engine import NNEngine

    parse = lambda s: tuple(int(x) for x in s.split("x"))       # noqa: E731
    cases = [(parse(s), name, args.threshold) for s in args.shapes.split(",") if s for name in ("a_no_vote", "b_planted")]
    cases += [(parse(s), "c_every_pair", -1.0) for s in args.dense.split(",") if s]
    eng = NNEngine(0, synthetic.synth_weights())
    info = eng.device_info()
    eng.profile_enable(True)
    results = {}
    for (nq, nb), name, threshold in cases:
        base = rows(nb, 7)
        planted = 0
        if name == "a_no_vote":
            query = rows(nq, 9)
        else:
            if name == "b_planted":
                planted = plant_families(base, args.planted, args.family, 8)
            query = base[np.sort(np.random.default_rng(10).permutation(nb)[:nq])]
        cells = nq * 64
        bufs = {"q": eng.alloc(nq * 2048), "b": eng.alloc(nb * 2048), "indptr": eng.alloc((nq + 1) * 8), "label": eng.alloc(nb * 8),
                "count": eng.alloc(cells * 8), "weight": eng.alloc(cells * 8), "nearest": eng.alloc(cells * 8), "nearest_sim": eng.alloc(cells * 4)}
        state = {}

        def count():
            state["edges"] = eng.match_count_dev(bufs["q"].ptr, nq, bufs["b"].ptr, nb, threshold, bufs["indptr"].ptr)
            return float(eng.match_pass_ms()[0])

        def vote(nc, lds):
            eng.set_vote_lds(lds)
            bufs["label"].upload(np.random.default_rng(11).integers(0, nc, nb).astype(np.int64))
            eng.vote_dev(bufs["q"].ptr, nq, bufs["b"].ptr, nb, bufs["label"].ptr, nc, threshold, bufs["count"].ptr, bufs["weight"].ptr,
                         bufs["nearest"].ptr, bufs["nearest_sim"].ptr)
            ms = eng.vote_pass_ms()
            state["votes"] = int(bufs["count"].download((nq, nc), np.int64).sum())
            return float(ms[1])

        try:
            bufs["q"].upload(np.ascontiguousarray(query))
            bufs["b"].upload(base)
            count()                                                             # warm-up: every buffer at its size
            for _, nc, lds in VARIANTS:
                vote(nc, lds)
            ms = {"count_pass": []}
            for _ in range(args.repeats):                                       # alternating: drift hits all alike
                ms["count_pass"].append(count())
                for variant, nc, lds in VARIANTS:
                    ms.setdefault(variant, []).append(vote(nc, lds))
                    assert state["votes"] == state["edges"], (variant, state)   # every base row is labelled: a vote per edge
            r = {"planted_rows": planted, "threshold": threshold, "votes": state["edges"]}
            base_ms = statistics.median(ms["count_pass"])
            spread = max(ms["count_pass"]) - min(ms["count_pass"])
            for what, v in ms.items():
                r[what] = {"ms": [round(x, 3) for x in v], "median": round(statistics.median(v), 3), "spread": round(max(v) - min(v), 3)}
                if what != "count_pass":
                    r[what]["over_count_pass"] = round(statistics.median(v) / base_ms, 4)
                    r[what]["minus_count_pass_ms"] = round(statistics.median(v) - base_ms, 3)
                    if name == "a_no_vote":
                        r[what]["within_baseline_spread"] = bool(abs(statistics.median(v) - base_ms) <= spread)
            results[f"{nq}x{nb}_{name}"] = r
            print(f"{nq} x {nb} {name}, threshold {threshold:g}, {state['edges']} votes: count pass {base_ms:.3f} ms (spread {spread:.3f}); "
                  + "; ".join(f"{v} {r[v]['median']:.3f} ms = {r[v]['over_count_pass']:.4f} x" for v, _, _ in VARIANTS), flush=True)
        finally:
            eng.set_vote_lds(16)
            for b in bufs.values():
                b.free()
    out = {"box": {"device": info["name"], "cus": info["cus"], "pci_bus_id": eng.pci_bus_id(), "host": socket.gethostname()},
           "threshold": args.threshold, "repeats": args.repeats, "family": args.family, "results": results}
    eng.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
