"""What region calls cost beside the scan that produced their track: NNEngine.call_regions against NNEngine.scan_contigs_dev on one
GPU and the synthetic metagenome buffer of scripts/scan_throughput.py.

    python scripts/regions_throughput.py [--gbp 3] [--repeats 3] [--strides 1000,100] [--penalty 1] [--single-bins 10000000] [--out FILE]

Per stride: one warm-up pass (workspaces and region buffers grow once), then `--repeats` passes in which every chunk is scanned and
its track goes through call_regions right away - the two are interleaved, so drifts of clock and power hit both alike.  Reported:
the seconds of every pass of either, call_regions from host arrays in to host arrays out, the HIP-event time of its kernels
(gnn_profile_get, GNN_K_REGIONS; copies excluded), their medians and spread, and the ratio regions / scan at the medians - the
feature's condition is a ratio of at most 0.01.  Then sequence.call_regions (numpy, the definition) on a 10^5-bin sample of the
last track, per bin, and one synthetic contig of `--single-bins` bins: the worst case of the two per-contig carries.
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


def spread(xs):
    return {"seconds": [round(x, 5) for x in xs], "median": round(statistics.median(xs), 5), "min": round(min(xs), 5), "max": round(max(xs), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbp", type=float, default=3.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--strides", default="1000,100")
    ap.add_argument("--penalty", type=float, default=1.0)
    ap.add_argument("--single-bins", type=int, default=10_000_000)
    ap.add_argument("--no-kmer-tables", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from genomad_amd import _lib, sequence, synthetic
    from genomad_amd.engine import NNEngine

    eng = NNEngine(0, synthetic.synth_weights())
    info = eng.device_info()
    prec = "f16x3tk" if not args.no_kmer_tables and eng.build_kmer_tables() else "f16x3tc"
    chunk_bytes = int(0.6e9) // 6000 * 6000
    n_chunks = max(1, int(round(args.gbp * 1e9 / chunk_bytes)))
    offs = [synthetic.synth_metagenome_offsets(chunk_bytes, seed=synthetic.DATA_SEED + c) for c in range(n_chunks)]
    seq = eng.alloc(chunk_bytes)
    eng.profile_enable(True)

    def kernel_ms():
        return eng.profile_get(_lib.K_REGIONS)[0]

    def sweep(stride):
        """every chunk: scan (timed), then call_regions on its track (timed; kernel time from the events)"""
        t_scan = t_reg = 0.0
        bins = regions = 0
        k0 = kernel_ms()
        last = None
        for c in range(n_chunks):
            eng.synth_windows_dev(c * (chunk_bytes // 6000), chunk_bytes // 6000, seq.ptr)
            eng.sync()
            t = time.perf_counter()                      # the synthesis of the chunk is not timed
            scan = eng.scan_contigs_dev(seq.ptr, offs[c], stride, False, prec)
            t_scan += time.perf_counter() - t
            t = time.perf_counter()
            res = eng.call_regions(scan.track, scan.bin_offsets, args.penalty)
            t_reg += time.perf_counter() - t
            bins += len(scan.track)
            regions += len(res.region_lo)
            last = scan
        return t_scan, t_reg, (kernel_ms() - k0) * 1e-3, bins, regions, last

    results = {}
    try:
        last = None
        for stride in (int(s) for s in args.strides.split(",")):
            sweep(stride)                                # warm-up
            scan_s, reg_s, ker_s = [], [], []
            for _ in range(args.repeats):
                a, b, k, bins, regions, last = sweep(stride)
                scan_s.append(a), reg_s.append(b), ker_s.append(k)
                print(f"stride {stride}: scan {a:.3f} s, call_regions {b:.4f} s (kernels {k:.4f} s), {bins} bins, {regions} regions", flush=True)
            ratio = statistics.median(reg_s) / statistics.median(scan_s)
            results[f"stride_{stride}"] = {
                "bins": bins, "regions": regions, "scan": spread(scan_s), "call_regions_host_to_host": spread(reg_s),
                "call_regions_kernels": spread(ker_s), "ratio_regions_to_scan_at_medians": round(ratio, 6),
                "ratio_min_max": [round(min(reg_s) / max(scan_s), 6), round(max(reg_s) / min(scan_s), 6)],
                "ns_per_bin_host_to_host": round(statistics.median(reg_s) / bins * 1e9, 2),
                "ns_per_bin_kernels": round(statistics.median(ker_s) / bins * 1e9, 2), "meets_1_percent": bool(ratio <= 0.01)}
        # the numpy definition on a sample of the last track, per bin
        n = min(100_000, len(last.track))
        t = time.perf_counter()
        sequence.call_regions(last.track[:n], np.array([0, n], np.int64), args.penalty)
        dt = time.perf_counter() - t
        results["numpy_definition"] = {"bins": n, "seconds": round(dt, 3), "us_per_bin": round(dt / n * 1e6, 3)}
        # one contig of --single-bins bins: the longest per-contig carries
        rng = np.random.default_rng(1)
        track = rng.random((args.single_bins, 3), dtype=np.float32)
        off = np.array([0, args.single_bins], np.int64)
        eng.call_regions(track, off, args.penalty)       # warm-up: the buffers grow
        one_s, one_k = [], []
        for _ in range(args.repeats):
            k0 = kernel_ms()
            t = time.perf_counter()
            res = eng.call_regions(track, off, args.penalty)
            one_s.append(time.perf_counter() - t)
            one_k.append((kernel_ms() - k0) * 1e-3)
        results["single_contig"] = {"bins": args.single_bins, "regions": len(res.region_lo), "call_regions_host_to_host": spread(one_s),
                                    "call_regions_kernels": spread(one_k),
                                    "ns_per_bin_host_to_host": round(statistics.median(one_s) / args.single_bins * 1e9, 2),
                                    "ns_per_bin_kernels": round(statistics.median(one_k) / args.single_bins * 1e9, 2)}
    finally:
        seq.free()
    out = {"box": {"device": info["name"], "cus": info["cus"], "pci_bus_id": eng.pci_bus_id(), "host": socket.gethostname()},
           "arithmetic": prec, "gbp": round(n_chunks * chunk_bytes / 1e9, 2), "chunks": n_chunks, "penalty": args.penalty,
           "contigs": int(sum(len(o) - 1 for o in offs)), "repeats": args.repeats, "results": results}
    eng.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
