"""What interval embeddings cost beside the scan of the same windows: windows/s of NNEngine.embed_intervals_dev against
NNEngine.scan_contigs_dev at the same stride, on one GPU and one synthetic packed buffer.

    python scripts/intervals_throughput.py [--mbp 300] [--repeats 3] [--strides 6000,1000] [--penalty 1] [--out FILE]

Two cases.  (1) `--mbp` Mbp of BASELINE configs[4] (contigs of 1-500 kbp, synthesised in HBM as scripts/scan_throughput.py does),
scanned at every stride of `--strides`; the intervals are the regions NNEngine.call_regions finds on that scan's track with
`--penalty`.  (2) One contig of `--worst-mbp` Mbp as a single interval at stride `--worst-stride`: the serial worst case of the
fold, every window of a slab added by one workgroup.  Per case: one warm-up pass of both variants (the workspaces grow once), then
`--repeats` passes, interleaved (scan, intervals, scan, ...: drifts of clock and power hit both alike).  Reported: windows,
intervals, the seconds of every pass, windows/s at the median, the ratio intervals / scan, the spread of the scan's own passes -
the yardstick for that ratio - and, from one further pass with profiling on, the HIP-event time of the fold and finish kernels
(gnn_profile_get, GNN_K_REGIONS) as a share of that pass.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=float, default=300.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--strides", default="6000,1000")
    ap.add_argument("--penalty", type=float, default=1.0)
    ap.add_argument("--worst-mbp", type=float, default=2.0)
    ap.add_argument("--worst-stride", type=int, default=1000)
    ap.add_argument("--worst-repeats", type=int, default=15)
    ap.add_argument("--no-kmer-tables", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from genomad_amd import _lib, synthetic
    from genomad_amd.engine import NNEngine

    eng = NNEngine(0, synthetic.synth_weights())
    info = eng.device_info()
    prec = "f16x3tk" if not args.no_kmer_tables and eng.build_kmer_tables() else "f16x3tc"
    nbytes = int(args.mbp * 1e6) // 6000 * 6000
    seq = eng.alloc(max(nbytes, int(args.worst_mbp * 1e6) // 6000 * 6000))
    eng.synth_windows_dev(0, seq.nbytes // 6000, seq.ptr)
    eng.sync()

    def case(offsets, stride, intervals, repeats):
        variants = {"scan": lambda: len(eng.scan_contigs_dev(seq.ptr, offsets, stride, False, prec).scores),
                    "intervals": lambda: int(eng.embed_intervals_dev(seq.ptr, offsets, stride, *intervals, precision=prec).count.sum())}
        ts, n = {v: [] for v in variants}, {}
        for v, f in variants.items():                    # warm-up
            f()
        for _ in range(repeats):
            for v, f in variants.items():
                t = time.perf_counter()
                n[v] = f()
                ts[v].append(round(time.perf_counter() - t, 5))
        eng.profile_enable(True)
        eng.profile_reset()
        t = time.perf_counter()
        variants["intervals"]()
        wall = time.perf_counter() - t
        kernel_ms, launches = eng.profile_get(_lib.K_REGIONS)
        eng.profile_enable(False)
        windows = n["scan"]
        med = {v: statistics.median(ts[v]) for v in variants}
        return {"stride": stride, "contigs": len(offsets) - 1, "windows": windows, "intervals": len(intervals[0]),
                "kept_windows_inside_an_interval": n["intervals"], "seconds": ts,
                "windows_per_s_at_median": {v: round(windows / med[v], 1) for v in variants},
                "ratio_intervals_to_scan": round(med["scan"] / med["intervals"], 4),
                "spread_of_the_scan_passes": round((max(ts["scan"]) - min(ts["scan"])) / med["scan"], 4),
                "fold_and_finish_kernels": {"ms": round(kernel_ms, 3), "launches": int(launches), "share_of_the_pass": round(kernel_ms * 1e-3 / wall, 5)}}

    results = []
    try:
        offsets = synthetic.synth_metagenome_offsets(nbytes, seed=synthetic.DATA_SEED)
        for stride in (int(s) for s in args.strides.split(",")):
            scan = eng.scan_contigs_dev(seq.ptr, offsets, stride, False, prec)
            reg = eng.call_regions(scan.track, scan.bin_offsets, args.penalty, offsets, stride)
            r = case(offsets, stride, (reg.region_contig, reg.start, reg.end), args.repeats)
            r["case"] = f"{round(nbytes / 1e6)} Mbp, the regions of call_regions at penalty {args.penalty:g}"
            results.append(r)
            print(json.dumps(r), flush=True)
        worst = int(args.worst_mbp * 1e6)
        one = np.array([0, worst], np.int64)
        r = case(one, args.worst_stride, (np.zeros(1, np.int64), np.zeros(1, np.int64), np.array([worst], np.int64)), args.worst_repeats)
        r["case"] = f"one contig of {args.worst_mbp:g} Mbp as a single interval"
        results.append(r)
        print(json.dumps(r), flush=True)
    finally:
        seq.free()
    out = {"box": {"device": info["name"], "cus": info["cus"], "pci_bus_id": eng.pci_bus_id(), "host": socket.gethostname()},
           "arithmetic": prec, "results": results}
    eng.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
