"""What the encoder embeddings cost: windows/s with and without them, on one GPU.

    python scripts/embed_throughput.py [--windows 65536] [--gbp 3] [--repeats 5] [--out FILE]

* window path: gnn_classify_dev vs gnn_embed_dev (f32 rows, 2 KB per window written to HBM) on `--windows` synthetic windows
  resident in HBM, for f16x3tc and f16x3tk (the latter when the device holds the k-mer tables);
* contig path: gnn_classify_contigs vs gnn_classify_contigs_embed on `--gbp` Gbp of BASELINE configs[4] (contigs of 1-500 kbp,
  chunks of 0.6 Gbp synthesised in HBM, as bench.py's metagenome block), with the arithmetic main() would pick.

One warm-up pass of each variant, then `--repeats` passes with the two variants interleaved (A B A B ...: drifts of clock and power
hit both alike); the medians are reported, with min and max.  The result names the box (device name, PCI bus id, host).
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


def _stats(ts, work):
    med = statistics.median(ts)
    return {"median_s": round(med, 5), "min_s": round(min(ts), 5), "max_s": round(max(ts), 5), "per_s_at_median": round(work / med, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=65536)
    ap.add_argument("--gbp", type=float, default=3.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    from genomad_amd import synthetic
    from genomad_amd.engine import NNEngine

    eng = NNEngine(0, synthetic.synth_weights())
    info = eng.device_info()
    out = {"box": {"device": info["name"], "cus": info["cus"], "pci_bus_id": eng.pci_bus_id(), "host": socket.gethostname()},
           "repeats": args.repeats, "window_path": {}, "contig_path": {}}
    tables = eng.build_kmer_tables()
    n = args.windows
    bases = eng.alloc(n * 6000)
    scores = eng.alloc(n * 3 * 4)
    emb = eng.alloc(n * 512 * 4)
    try:
        eng.synth_windows_dev(0, n, bases.ptr)
        eng.sync()
        for prec in ["f16x3tc"] + (["f16x3tk"] if tables else []):
            runs = {"classify_dev": lambda p=prec: eng.classify_dev(bases.ptr, n, scores.ptr, p),
                    "embed_dev": lambda p=prec: eng.embed_dev(bases.ptr, n, emb.ptr, p, scores_ptr=scores.ptr)}
            ts = {k: [] for k in runs}
            for k, f in runs.items():          # warm-up
                f()
                eng.sync()
            for _ in range(args.repeats):
                for k, f in runs.items():
                    t = time.perf_counter()
                    f()
                    eng.sync()
                    ts[k].append(time.perf_counter() - t)
            r = {k: _stats(v, n) for k, v in ts.items()}
            r["embed_cost_pct"] = round(100 * (r["embed_dev"]["median_s"] / r["classify_dev"]["median_s"] - 1), 2)
            out["window_path"][prec] = r
            print(prec, json.dumps(r), flush=True)
    finally:
        bases.free(), scores.free(), emb.free()

    prec = "f16x3tk" if tables else "f16x3tc"
    chunk_bytes = int(0.6e9) // 6000 * 6000
    n_chunks = max(1, int(round(args.gbp * 1e9 / chunk_bytes)))
    seq = eng.alloc(chunk_bytes)
    try:
        offs = [synthetic.synth_metagenome_offsets(chunk_bytes, seed=synthetic.DATA_SEED + c) for c in range(n_chunks)]

        def sweep(embed):
            t_total, windows = 0.0, 0
            for c in range(n_chunks):
                eng.synth_windows_dev(c * (chunk_bytes // 6000), chunk_bytes // 6000, seq.ptr)
                eng.sync()
                t = time.perf_counter()                  # the synthesis of the chunk is not timed
                res = (eng.embed_contigs_dev if embed else eng.classify_contigs_dev)(seq.ptr, offs[c], False, prec)
                t_total += time.perf_counter() - t
                windows += len(res[-1])
            return t_total, windows

        sweep(False), sweep(True)                        # warm-up: the contig workspaces grow once
        ts = {"classify_contigs": [], "embed_contigs": []}
        for _ in range(args.repeats):
            for k in ts:
                dt, windows = sweep(k == "embed_contigs")
                ts[k].append(dt)
        r = {k: _stats(v, windows) for k, v in ts.items()}
        r["embed_cost_pct"] = round(100 * (r["embed_contigs"]["median_s"] / r["classify_contigs"]["median_s"] - 1), 2)
        r.update(arithmetic=prec, gbp=round(n_chunks * chunk_bytes / 1e9, 2), chunks=n_chunks, windows=windows,
                 contigs=int(sum(len(o) - 1 for o in offs)))
        out["contig_path"] = r
        print("contigs", json.dumps(r), flush=True)
    finally:
        seq.free()
    eng.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
