"""What an occlusion map costs per forward pass: forward passes/s (windows + pairs) of NNEngine.occlude_contigs_dev at blocks of
500 / 100 / 20 bases against the windows/s of NNEngine.classify_contigs_dev, on one GPU and one synthetic packed buffer.

    python scripts/occlusion_throughput.py [--mbp 60] [--repeats 3] [--blocks 500,100,20] [--baseline-only] [--out FILE]

The buffer is `--mbp` Mbp of BASELINE configs[4] (contigs of 1-500 kbp synthesised in HBM, as bench.py's metagenome block) - a slice
of the workload of scripts/scan_throughput.py small enough for the smallest block (301 passes per window) to finish in seconds -
classified with the arithmetic main() would pick.  One warm-up pass of every variant (the workspaces grow once), then `--repeats`
passes with the variants interleaved (baseline, block a, block b, ..., baseline, ...: drifts of clock and power hit all alike).
Reported per variant: forward passes, the seconds of every pass, passes/s at the median, and the ratio to the baseline's windows/s;
the spread of the baseline's own passes is the yardstick for that ratio.  --baseline-only times classify_contigs_dev alone: it needs
nothing this script's own commit added, so it also runs on older checkouts.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=float, default=60.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--blocks", default="500,100,20")
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--no-kmer-tables", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from genomad_amd import synthetic
    from genomad_amd.engine import NNEngine

    eng = NNEngine(0, synthetic.synth_weights())
    info = eng.device_info()
    prec = "f16x3tk" if not args.no_kmer_tables and eng.build_kmer_tables() else "f16x3tc"
    nbytes = int(args.mbp * 1e6) // 6000 * 6000
    offs = synthetic.synth_metagenome_offsets(nbytes, seed=synthetic.DATA_SEED)
    variants = ["classify_contigs"] + ([] if args.baseline_only else [f"occlude_{int(b)}" for b in args.blocks.split(",")])
    seq = eng.alloc(nbytes)

    def sweep(variant):
        t = time.perf_counter()
        if variant == "classify_contigs":
            passes = len(eng.classify_contigs_dev(seq.ptr, offs, False, prec)[1])
        else:
            res = eng.occlude_contigs_dev(seq.ptr, offs, int(variant.split("_")[1]), False, prec)
            passes = len(res.scores) + len(res.delta)
        return time.perf_counter() - t, passes

    try:
        eng.synth_windows_dev(0, nbytes // 6000, seq.ptr)
        eng.sync()
        ts, passes = {v: [] for v in variants}, {}
        for v in variants:                               # warm-up
            sweep(v)
        for _ in range(args.repeats):
            for v in variants:
                dt, passes[v] = sweep(v)
                ts[v].append(round(dt, 4))
                print(v, passes[v], ts[v][-1], flush=True)
    finally:
        seq.free()
    res = {v: {"forward_passes": passes[v], "seconds": ts[v], "passes_per_s_at_median": round(passes[v] / statistics.median(ts[v]), 1),
               "passes_per_s_min_max": [round(passes[v] / max(ts[v]), 1), round(passes[v] / min(ts[v]), 1)]} for v in variants}
    base = res["classify_contigs"]["passes_per_s_at_median"]
    for v in variants[1:]:
        res[v]["ratio_to_classify_contigs"] = round(res[v]["passes_per_s_at_median"] / base, 4)
    lo, hi = res["classify_contigs"]["passes_per_s_min_max"]
    res["classify_contigs"]["spread_of_the_passes"] = round((hi - lo) / base, 4)
    out = {"box": {"device": info["name"], "cus": info["cus"], "pci_bus_id": eng.pci_bus_id(), "host": socket.gethostname()},
           "arithmetic": prec, "mbp": round(nbytes / 1e6, 2), "contigs": int(len(offs) - 1), "repeats": args.repeats, "results": res}
    eng.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
