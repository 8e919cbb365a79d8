"""What scoring both strands costs per window: scored windows/s of NNEngine.classify_contigs_strand_dev(both) against
NNEngine.classify_contigs_dev, on one GPU and one synthetic packed buffer.

    python scripts/strand_throughput.py [--gbp 3] [--repeats 3] [--genome-windows 906] [--genome-repeats 20] [--out FILE]

The buffer is `--gbp` Gbp of BASELINE configs[4] (contigs of 1-500 kbp, chunks of 0.6 Gbp synthesised in HBM, as
scripts/scan_throughput.py), classified with f16x3tk where the device holds the k-mer tables and f16x3tc otherwise.  One warm-up
pass of each variant (the workspaces grow once), then `--repeats` passes with the two interleaved (forward, both, forward, ...:
drifts of clock and power hit both alike).  `both` scores two windows per span, so its rate counts two per span; the bar is the
ratio of the two rates in this one run (>= 0.97), with the spread of the baseline's own passes as the yardstick.

Second figure: one genome of `--genome-windows` windows (one contig; config 1's size) - the time of `both` over the time of
`forward`.  The two strands of a slab go through the front end as ONE batch, so a genome that fills a fraction of the device
costs less than twice the forward pass.

Third: the reverse-complement kernel alone, `gnn_revcomp_spans_dev` over the spans of one chunk, as GB/s read + written (the
call also uploads the 12 B span table per window and synchronises: a lower bound of the kernel's own rate; the kernel's time
alone is in a `rocprofv3 --kernel-trace --stats` run of this script).
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
    ap.add_argument("--gbp", type=float, default=3.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--genome-windows", type=int, default=906)
    ap.add_argument("--genome-repeats", type=int, default=20)
    ap.add_argument("--no-kmer-tables", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from genomad_amd import sequence, synthetic
    from genomad_amd.engine import NNEngine

    eng = NNEngine(0, synthetic.synth_weights())
    info = eng.device_info()
    prec = "f16x3tk" if not args.no_kmer_tables and eng.build_kmer_tables() else "f16x3tc"
    chunk_bytes = int(0.6e9) // 6000 * 6000
    n_chunks = max(1, int(round(args.gbp * 1e9 / chunk_bytes)))
    offs = [synthetic.synth_metagenome_offsets(chunk_bytes, seed=synthetic.DATA_SEED + c) for c in range(n_chunks)]
    variants = ["classify_contigs", "strand_both"]
    seq = eng.alloc(chunk_bytes)

    def call(variant, off):
        """kept spans of one call"""
        if variant == "classify_contigs":
            return len(eng.classify_contigs_dev(seq.ptr, off, False, prec)[1])
        return len(eng.classify_contigs_strand_dev(seq.ptr, off, "both", False, prec)[1])

    def sweep(variant):
        t_total, spans = 0.0, 0
        for c in range(n_chunks):
            eng.synth_windows_dev(c * (chunk_bytes // 6000), chunk_bytes // 6000, seq.ptr)
            eng.sync()
            t = time.perf_counter()                      # the synthesis of the chunk is not timed
            spans += call(variant, offs[c])
            t_total += time.perf_counter() - t
        return t_total, spans

    try:
        ts, spans = {v: [] for v in variants}, {}
        for v in variants:                               # warm-up
            sweep(v)
        for _ in range(args.repeats):
            for v in variants:
                dt, spans[v] = sweep(v)
                ts[v].append(round(dt, 4))
                print(v, spans[v], ts[v][-1], flush=True)
        per_span = {"classify_contigs": 1, "strand_both": 2}
        res = {}
        for v in variants:
            n = spans[v] * per_span[v]
            res[v] = {"spans": spans[v], "scored_windows": n, "seconds": ts[v],
                      "windows_per_s_at_median": round(n / statistics.median(ts[v]), 1),
                      "windows_per_s_min_max": [round(n / max(ts[v]), 1), round(n / min(ts[v]), 1)]}
        base = res["classify_contigs"]["windows_per_s_at_median"]
        res["strand_both"]["ratio_to_classify_contigs"] = round(res["strand_both"]["windows_per_s_at_median"] / base, 4)
        lo, hi = res["classify_contigs"]["windows_per_s_min_max"]
        res["classify_contigs"]["spread_of_the_passes"] = round((hi - lo) / base, 4)

        # one genome: a single contig of --genome-windows windows in the buffer's first bytes
        g_off = np.array([0, args.genome_windows * 6000], np.int64)
        eng.synth_windows_dev(0, args.genome_windows, seq.ptr)
        eng.sync()
        g = {v: [] for v in variants}
        for v in variants:
            call(v, g_off)
        for _ in range(args.genome_repeats):
            for v in variants:
                t = time.perf_counter()
                call(v, g_off)
                g[v].append(time.perf_counter() - t)
        gm = {v: statistics.median(g[v]) for v in variants}
        genome = {"windows": args.genome_windows, "repeats": args.genome_repeats,
                  "forward_ms_at_median": round(gm["classify_contigs"] * 1e3, 3), "both_ms_at_median": round(gm["strand_both"] * 1e3, 3),
                  "both_over_forward": round(gm["strand_both"] / gm["classify_contigs"], 4)}

        # the reverse-complement kernel through its own entry point: every span of chunk 0
        eng.synth_windows_dev(0, chunk_bytes // 6000, seq.ptr)
        starts, lens, _, _ = sequence.candidate_spans(offs[0])
        out = eng.alloc(len(starts) * 6000)
        try:
            eng.revcomp_spans_dev(seq.ptr, starts, lens, out.ptr)
            rt = []
            for _ in range(5):
                t = time.perf_counter()
                eng.revcomp_spans_dev(seq.ptr, starts, lens, out.ptr)
                rt.append(time.perf_counter() - t)
        finally:
            out.free()
        moved = int(lens.sum()) + len(starts) * 6000
        revcomp = {"spans": len(starts), "bytes_read_and_written": moved, "call_ms_at_median": round(statistics.median(rt) * 1e3, 3),
                   "gb_per_s_of_the_call": round(moved / statistics.median(rt) / 1e9, 1)}
    finally:
        seq.free()
    out = {"box": {"device": info["name"], "cus": info["cus"], "pci_bus_id": eng.pci_bus_id(), "host": socket.gethostname()},
           "arithmetic": prec, "gbp": round(n_chunks * chunk_bytes / 1e9, 2), "chunks": n_chunks,
           "contigs": int(sum(len(o) - 1 for o in offs)), "repeats": args.repeats, "results": res, "one_genome": genome,
           "revcomp_spans_dev": revcomp}
    eng.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
