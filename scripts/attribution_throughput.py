"""What the attention contribution maps cost: windows/s of NNEngine.attribute_contigs_dev at bins of 1 and 8 pooled positions against
the windows/s of NNEngine.classify_contigs_dev, in one process, on one GPU and one synthetic packed buffer.

    python scripts/attribution_throughput.py [--mbp 300] [--repeats 3] [--bins 1,8] [--step-timeout 120] [--out FILE]

The buffer is `--mbp` Mbp of BASELINE configs[4] (contigs of 1-500 kbp synthesised in HBM, as bench.py's metagenome block), classified
with the arithmetic main() would pick.  One warm-up pass of every variant (the workspaces grow once), then `--repeats` passes with the
variants interleaved (baseline, bin a, bin b, baseline, ...: drifts of clock and power hit all alike).  Reported per variant: windows,
the seconds of every pass, windows/s at the median and the ratio to the baseline; the spread of the baseline's own passes is the
yardstick for that ratio.  A last, profiled pass per bin (HIP events around every launch: not timed against the baseline) says where
the time goes: front end, back end, and the two kernels the maps add - the head's gradient and the contribution kernel.
Every GPU step (a pass of one variant, its profile read-out included) runs under its own time limit, `--step-timeout` seconds: a
step that overruns it ends the process with status 124 and nothing more is started on the GPU.  The limit is a SIGALRM handler, and
Python runs handlers between bytecodes only: a step that hangs INSIDE a library call never reaches it.  Run the script under
`timeout -k 10 N` as well, which ends that case too.
"""
import argparse
import json
import os
import signal
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class step_limit:
    """with step_limit(seconds, what): ... - SIGALRM ends the process (status 124) when the step overruns"""

    def __init__(self, seconds, what):
        self.seconds, self.what = int(seconds), what

    def _fire(self, *_):
        print(f"step {self.what!r} overran its limit of {self.seconds} s: stopping", file=sys.stderr, flush=True)
        os._exit(124)

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._fire)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=float, default=300.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--bins", default="1,8")
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--no-kmer-tables", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from genomad_amd import _lib, synthetic
    from genomad_amd.engine import NNEngine

    with step_limit(args.step_timeout, "engine and k-mer tables"):
        eng = NNEngine(0, synthetic.synth_weights())
        info = eng.device_info()
        prec = "f16x3tk" if not args.no_kmer_tables and eng.build_kmer_tables() else "f16x3tc"
    nbytes = int(args.mbp * 1e6) // 6000 * 6000
    offs = synthetic.synth_metagenome_offsets(nbytes, seed=synthetic.DATA_SEED)
    variants = ["classify_contigs"] + [f"attribute_{int(b)}" for b in args.bins.split(",")]
    seq = eng.alloc(nbytes)

    def sweep(variant, profiled=False):
        with step_limit(args.step_timeout, variant):
            if profiled:
                eng.profile_reset()
            t = time.perf_counter()
            if variant == "classify_contigs":
                windows = len(eng.classify_contigs_dev(seq.ptr, offs, False, prec)[1])
            else:
                res = eng.attribute_contigs_dev(seq.ptr, offs, int(variant.split("_")[1]), False, prec)
                windows = int(res.kept.sum())              # the windows classify_contigs reports: the same table, the same mask
            dt = time.perf_counter() - t
            if profiled:                                   # the read-out synchronises: inside the step's limit
                profile[variant] = {k: round(eng.profile_get(i)[0], 3) for k, i in kernels.items()}
            return dt, windows

    profile = {}
    kernels = {"front_end": _lib.K_FUSED, "back_end": _lib.K_BACKEND, "attr_head": _lib.K_ATTR_HEAD, "attr_contrib": _lib.K_ATTR_CONTRIB}
    try:
        with step_limit(args.step_timeout, "synthesise the buffer"):
            eng.synth_windows_dev(0, nbytes // 6000, seq.ptr)
            eng.sync()
        ts, windows = {v: [] for v in variants}, {}
        for v in variants:                               # warm-up
            sweep(v)
        for _ in range(args.repeats):
            for v in variants:
                dt, windows[v] = sweep(v)
                ts[v].append(round(dt, 4))
                print(v, windows[v], ts[v][-1], flush=True)
        eng.profile_enable(True)
        for v in variants:
            sweep(v, profiled=True)
        eng.profile_enable(False)
    finally:
        seq.free()
    res = {v: {"windows": windows[v], "seconds": ts[v], "windows_per_s_at_median": round(windows[v] / statistics.median(ts[v]), 1),
               "windows_per_s_min_max": [round(windows[v] / max(ts[v]), 1), round(windows[v] / min(ts[v]), 1)]} for v in variants}
    base = res["classify_contigs"]["windows_per_s_at_median"]
    for v in variants[1:]:
        res[v]["ratio_to_classify_contigs"] = round(res[v]["windows_per_s_at_median"] / base, 4)
    for v in variants:
        res[v]["profiled_pass_ms"] = profile[v]
    lo, hi = res["classify_contigs"]["windows_per_s_min_max"]
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
