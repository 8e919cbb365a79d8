"""What the principal components cost on one GPU, on embedding-like rows resident on the device, in one process.

    python scripts/pca_throughput.py [--n 262144] [--ncomp 2 64] [--repeats 10] [--splits 0] [--out FILE]

The rows are tests.neighbours_data.rows (ReLU of a Gaussian with one power-of-two scale per channel), as in the other throughput
scripts.  One warm-up of every call (the ctx's buffers grow once), then `--repeats` rounds.

Moments: NNEngine.pca_moments_dev - seconds from the call to the synchronised stream and the HIP-event milliseconds of its four passes
(gnn_debug_pca_pass_ms: prepare, sums, gram, mirror) - beside two baselines: the prepare pass alone (nn_prepare on the same rows: the
floor of any pass over them, taken from the same event list) and numpy's float32 X.T @ X of the unit rows on the box's host threads
(what a user does today; the normalisation is not timed).  The Gram pass is also run at every `--splits` value (rows per workgroup; 0
= the library's choice).  Reported beside the times: the pass's FLOP (2 x 10 block pairs x 128 x 128 x padded rows) over its time.

Projection: NNEngine.project_dev at every `--ncomp`, interleaved with NNEngine.neighbours_dev(rows, components, k=ncomp) - the same
values plus a selection - seconds from the call to the synchronised stream, the medians, the baseline's spread ((max - min) / median),
project / neighbours.  The script asserts that the projection's values are the neighbour search's, bit for bit, on the first 4 096
rows; no ratio is a condition of the script."""
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

from tests.neighbours_data import rows  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--ncomp", type=int, nargs="+", default=[2, 64])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--splits", type=int, nargs="*", default=[0])
    ap.add_argument("--host-repeats", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from genomad_amd import synthetic
    from genomad_amd.engine import NNEngine

    n, cmax = args.n, max(args.ncomp)
    med = statistics.median
    eng = NNEngine(0, synthetic.synth_weights())
    info = eng.device_info()
    eng.profile_enable(True)
    data = rows(n, 7)
    comp = np.ascontiguousarray(np.random.default_rng(3).standard_normal((cmax, 512)).astype(np.float32))
    q, c = eng.alloc(data.nbytes), eng.alloc(comp.nbytes)
    G, S, nv = eng.alloc(8 * 512 * 512), eng.alloc(8 * 512), eng.alloc(8)
    out, idx, sim = eng.alloc(4 * n * cmax), eng.alloc(8 * n * cmax), eng.alloc(4 * n * cmax)
    results = {"moments": {}, "project": {}}
    try:
        q.upload(data)
        c.upload(comp)

        def moments():
            t = time.perf_counter()
            eng.pca_moments_dev(q.ptr, n, G.ptr, S.ptr, nv.ptr)
            eng.sync()
            return time.perf_counter() - t, eng.pca_pass_ms()

        flop = 2.0 * 10 * 128 * 128 * ((n + 63) // 64 * 64)
        first = None
        for split in args.splits:
            eng.set_pca_split(split)
            moments()
            got = G.download((512, 512), np.int64)
            first = got if first is None else first
            assert np.array_equal(got, first), "the Gram matrix depends on the split"
            walls, passes = [], []
            for _ in range(args.repeats):
                w, ms = moments()
                walls.append(w), passes.append(list(ms))
            p = [med(x[i] for x in passes) for i in range(4)]
            r = {"seconds": [round(w, 6) for w in walls], "median_seconds": round(med(walls), 6),
                 "spread": round((max(walls) - min(walls)) / med(walls), 4),
                 "prepare_ms": round(p[0], 4), "sums_ms": round(p[1], 4), "gram_ms": round(p[2], 4), "mirror_ms": round(p[3], 4),
                 "moments_without_prepare_ms": round(p[1] + p[2] + p[3], 4), "gram_tflops": round(flop / (p[2] * 1e-3) / 1e12, 2)}
            results["moments"][f"split{split}"] = r
            print(f"moments, split {split}: {1e3 * med(walls):.3f} ms (spread {100 * r['spread']:.1f} %); prepare {p[0]:.3f} ms, sums "
                  f"{p[1]:.3f} ms, gram {p[2]:.3f} ms ({r['gram_tflops']} TF), mirror {p[3]:.3f} ms", flush=True)
        eng.set_pca_split(0)
        # the host baseline: float32 X.T @ X of the unit rows; normalising them is not timed
        unit = data / np.sqrt((data.astype(np.float64) ** 2).sum(axis=1)).astype(np.float32)[:, None]
        host = []
        for _ in range(args.host_repeats + 1):
            t = time.perf_counter()
            unit.T @ unit
            host.append(time.perf_counter() - t)
        results["moments"]["numpy_f32_seconds"] = [round(x, 4) for x in host[1:]]
        results["moments"]["numpy_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0"))
        print(f"numpy float32 X.T @ X on the host: {med(host[1:]):.3f} s", flush=True)
        for k in args.ncomp:
            def project():
                t = time.perf_counter()
                eng.project_dev(q.ptr, n, c.ptr, k, out.ptr)
                eng.sync()
                return time.perf_counter() - t, eng.pca_pass_ms()

            def baseline():
                t = time.perf_counter()
                eng.neighbours_dev(q.ptr, n, c.ptr, k, idx.ptr, sim.ptr, k)
                eng.sync()
                return time.perf_counter() - t

            project()
            baseline()
            m = min(n, 4096)
            p = out.download((n, k), np.float32)[:m]
            i, s = idx.download((n, k), np.int64)[:m], sim.download((n, k), np.float32)[:m]
            want = np.full((m, k), np.nan, np.float32)
            ok = i[:, 0] >= 0
            want[np.flatnonzero(ok)[:, None], i[ok]] = s[ok]
            assert np.array_equal(p.view(np.uint32), want.view(np.uint32)), "the projection is not the neighbour search's values"
            base, proj, kern = [], [], []
            for _ in range(args.repeats):                   # interleaved: drift hits both alike
                base.append(baseline())
                w, ms = project()
                proj.append(w), kern.append(list(ms))
            r = {"neighbours_seconds": [round(x, 6) for x in base], "neighbours_median": round(med(base), 6),
                 "neighbours_spread": round((max(base) - min(base)) / med(base), 4),
                 "project_seconds": [round(x, 6) for x in proj], "project_median": round(med(proj), 6),
                 "project_spread": round((max(proj) - min(proj)) / med(proj), 4),
                 "prepare_rows_ms": round(med(x[0] for x in kern), 4), "prepare_components_ms": round(med(x[1] for x in kern), 4),
                 "project_kernel_ms": round(med(x[2] for x in kern), 4), "project_over_neighbours": round(med(proj) / med(base), 3)}
            results["project"][f"ncomp{k}"] = r
            print(f"project, ncomp {k}: {1e3 * med(proj):.3f} ms (kernel {r['project_kernel_ms']} ms, prepare {r['prepare_rows_ms']} ms) "
                  f"against neighbours_dev(k={k}) {1e3 * med(base):.3f} ms (spread {100 * r['neighbours_spread']:.1f} %): "
                  f"{r['project_over_neighbours']} x", flush=True)
    finally:
        eng.set_pca_split(0)
        for b in (q, c, G, S, nv, out, idx, sim):
            b.free()
    res = {"box": {"device": info["name"], "cus": info["cus"], "pci_bus_id": eng.pci_bus_id(), "host": socket.gethostname()},
           "n": n, "ncomp": args.ncomp, "repeats": args.repeats, "splits": args.splits, "results": results}
    eng.close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
