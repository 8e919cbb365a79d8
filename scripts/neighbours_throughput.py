"""What the neighbour search costs: NNEngine.neighbours_dev, the self-search among embedding-like rows resident on one GPU.

    python scripts/neighbours_throughput.py [--sizes 65536,262144] [--ks 1,10,64] [--repeats 3] [--out FILE]

Per size: the rows (ReLU of a Gaussian with one power-of-two scale per channel, the generator of tests/neighbours_data.py) go up once;
one warm-up search (the ctx's buffers grow once), then `--repeats` searches per k.  Reported per (size, k): the seconds of every search
from the call to the synchronised stream, the HIP-event time of its kernels (gnn_profile_get, GNN_K_NEIGHBOURS: prepare, tile and merge
of every query slab), pairs per second, the executed f16 FLOP/s - three MFMA products per pair and element: 2 x 3 x 512 per pair - and
that rate as a fraction of gnn_mfma_probe_kind(kind = 1) on the same box, measured right before.  Per size: the k = 64 / k = 1 time
ratio, which is what the selection costs.  For context: numpy (float32 matmul + argpartition) on one 256-query slab of the largest size.
"""
import argparse
import ctypes as C
import json
import os
import socket
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rows(n, seed):
    rng = np.random.default_rng(seed)
    scale = np.exp2(rng.integers(-3, 3, 512)).astype(np.float32)
    out = np.empty((n, 512), np.float32)
    for a in range(0, n, 16384):                         # in pieces: the float64 normals of 262144 rows are 1 GB
        out[a:a + 16384] = np.maximum(rng.standard_normal((min(16384, n - a), 512)), 0).astype(np.float32) * scale
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,262144")
    ap.add_argument("--ks", default="1,10,64")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from genomad_amd import _lib, synthetic
    from genomad_amd.engine import NNEngine, check

    sizes = [int(s) for s in args.sizes.split(",")]
    ks = [int(k) for k in args.ks.split(",")]
    eng = NNEngine(0, synthetic.synth_weights())
    info = eng.device_info()
    eng.profile_enable(True)
    probe = C.c_double(0)
    check(eng.lib.gnn_mfma_probe_kind(eng.ctx, 1, 300, C.byref(probe)))
    results = {"mfma_probe_f16_tflops": round(probe.value, 1)}
    data = None
    for n in sizes:
        data = rows(n, 7)
        q, idx, sim = eng.alloc(data.nbytes), eng.alloc(n * max(ks) * 8), eng.alloc(n * max(ks) * 4)
        try:
            q.upload(data)
            eng.neighbours_dev(q.ptr, n, None, 0, idx.ptr, sim.ptr, max(ks))           # warm-up: every buffer at its largest
            eng.sync()
            per_k = {}
            for k in ks:
                wall, kern = [], []
                for _ in range(args.repeats):
                    k0 = eng.profile_get(_lib.K_NEIGHBOURS)[0]
                    t = time.perf_counter()
                    eng.neighbours_dev(q.ptr, n, None, 0, idx.ptr, sim.ptr, k)
                    eng.sync()
                    wall.append(time.perf_counter() - t)
                    kern.append((eng.profile_get(_lib.K_NEIGHBOURS)[0] - k0) * 1e-3)
                med = statistics.median(wall)
                flops = n * n * 2.0 * 3 * 512 / med
                per_k[f"k_{k}"] = {"seconds": [round(x, 4) for x in wall], "median": round(med, 4), "kernel_seconds": [round(x, 4) for x in kern],
                                   "pairs_per_second": round(n * n / med, 1), "executed_f16_tflops": round(flops / 1e12, 1),
                                   "fraction_of_mfma_probe": round(flops / 1e12 / probe.value, 3)}
                print(f"n = {n}, k = {k}: {med:.3f} s, {n * n / med:.3e} pairs/s, {flops / 1e12:.0f} TFLOP/s executed = "
                      f"{flops / 1e12 / probe.value:.2f} of the probe's {probe.value:.0f}", flush=True)
            if 1 in ks and 64 in ks:
                per_k["k64_over_k1"] = round(per_k["k_64"]["median"] / per_k["k_1"]["median"], 3)
            results[f"n_{n}"] = per_k
        finally:
            for b in (q, idx, sim):
                b.free()
    # numpy on one slab of 256 queries of the last size: float32 matmul, argpartition, sort of the k best
    unit = data / np.sqrt((data.astype(np.float64) ** 2).sum(axis=1))[:, None].astype(np.float32)
    t = time.perf_counter()
    s = unit[:256] @ unit.T
    part = np.argpartition(-s, 10, axis=1)[:, :10]
    np.take_along_axis(part, np.argsort(-np.take_along_axis(s, part, axis=1), axis=1), axis=1)
    dt = time.perf_counter() - t
    results["numpy_one_slab"] = {"queries": 256, "base": len(data), "k": 10, "seconds": round(dt, 3), "pairs_per_second": round(256 * len(data) / dt, 1),
                                 "threads": os.cpu_count()}
    out = {"box": {"device": info["name"], "cus": info["cus"], "pci_bus_id": eng.pci_bus_id(), "host": socket.gethostname()},
           "repeats": args.repeats, "results": results}
    eng.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
