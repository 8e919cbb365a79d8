"""What a scan costs per window: windows/s of NNEngine.scan_contigs_dev at strides 6000 / 2000 / 1000 against
NNEngine.classify_contigs_dev, on one GPU and one synthetic packed buffer.

    python scripts/scan_throughput.py [--gbp 3] [--repeats 3] [--strides 6000,2000,1000] [--baseline-only] [--out FILE]

The buffer is `--gbp` Gbp of BASELINE configs[4] (contigs of 1-500 kbp, chunks of 0.6 Gbp synthesised in HBM, as bench.py's
metagenome block), classified with the arithmetic main() would pick.  One warm-up pass of every variant (the workspaces grow
once), then `--repeats` passes with the variants interleaved (baseline, stride a, stride b, ..., baseline, ...: drifts of clock
and power hit all alike).  Reported per variant: windows, the seconds of every pass, windows/s at the median, and the ratio to
the baseline's windows/s; the spread of the baseline's own passes is the yardstick for that ratio.  --baseline-only times
classify_contigs_dev alone: it needs nothing this script's own commit added, so it also runs on older checkouts.
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
    ap.add_argument("--gbp", type=float, default=3.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--strides", default="6000,2000,1000")
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--no-kmer-tables", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from genomad_amd import synthetic
    from genomad_amd.engine import NNEngine

    eng = NNEngine(0, synthetic.synth_weights())
    info = eng.device_info()
    prec = "f16x3tk" if not args.no_kmer_tables and eng.build_kmer_tables() else "f16x3tc"
    chunk_bytes = int(0.6e9) // 6000 * 6000
    n_chunks = max(1, int(round(args.gbp * 1e9 / chunk_bytes)))
    offs = [synthetic.synth_metagenome_offsets(chunk_bytes, seed=synthetic.DATA_SEED + c) for c in range(n_chunks)]
    variants = ["classify_contigs"] + ([] if args.baseline_only else [f"scan_{int(s)}" for s in args.strides.split(",")])
    seq = eng.alloc(chunk_bytes)

    def sweep(variant):
        t_total, windows = 0.0, 0
        for c in range(n_chunks):
            eng.synth_windows_dev(c * (chunk_bytes // 6000), chunk_bytes // 6000, seq.ptr)
            eng.sync()
            t = time.perf_counter()                      # the synthesis of the chunk is not timed
            if variant == "classify_contigs":
                windows += len(eng.classify_contigs_dev(seq.ptr, offs[c], False, prec)[1])
            else:
                windows += len(eng.scan_contigs_dev(seq.ptr, offs[c], int(variant.split("_")[1]), False, prec).scores)
            t_total += time.perf_counter() - t
        return t_total, windows

    try:
        ts, windows = {v: [] for v in variants}, {}
        for v in variants:                               # warm-up
            sweep(v)
        for _ in range(args.repeats):
            for v in variants:
                dt, windows[v] = sweep(v)
                ts[v].append(round(dt, 4))
                print(v, windows[v], ts[v][-1], flush=True)
    finally:
        seq.free()
    res = {v: {"windows": windows[v], "seconds": ts[v], "windows_per_s_at_median": round(windows[v] / statistics.median(ts[v]), 1),
               "windows_per_s_min_max": [round(windows[v] / max(ts[v]), 1), round(windows[v] / min(ts[v]), 1)]} for v in variants}
    base = res["classify_contigs"]["windows_per_s_at_median"]
    for v in variants[1:]:
        res[v]["ratio_to_classify_contigs"] = round(res[v]["windows_per_s_at_median"] / base, 4)
    lo, hi = res["classify_contigs"]["windows_per_s_min_max"]
    res["classify_contigs"]["spread_of_the_passes"] = round((hi - lo) / base, 4)
    out = {"box": {"device": info["name"], "cus": info["cus"], "pci_bus_id": eng.pci_bus_id(), "host": socket.gethostname()},
           "arithmetic": prec, "gbp": round(n_chunks * chunk_bytes / 1e9, 2), "chunks": n_chunks,
           "contigs": int(sum(len(o) - 1 for o in offs)), "repeats": args.repeats, "results": res}
    eng.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
