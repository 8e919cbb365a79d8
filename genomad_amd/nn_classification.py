"""Drop-in replacement for ``genomad.modules.nn_classification`` on MI355X.

    genomad_amd.nn_classification.main(input_path, output_path, single_window, batch_size,
                                       restart, threads, verbose, cleanup)

has the signature, the on-disk outputs, the resume rules and the error behaviour of the
reference's ``main`` (genomad/modules/nn_classification.py:21-427); ``install()`` rebinds
``genomad.nn_classification`` / ``genomad.modules.nn_classification`` so that ``genomad
nn-classification`` and ``genomad end-to-end`` (cli.py:772, :1367-1376) pick it up unchanged.

What differs inside: windows are tokenised and classified by libgenomad_nn_hip.so (no TensorFlow,
no TFRecord round trip).  ``<prefix>_encoded_sequences/`` holds ``<prefix>_seq_window_id.npz``
(same keys as the reference) and the padded windows as ``<n>.win.npy`` instead of ``*.tfrec``.
``threads`` is accepted and ignored (it only sized TensorFlow's pools, :39-40); ``batch_size``
bounds the windows per GPU launch (results do not depend on it).

Weights: ``$GENOMAD_AMD_WEIGHTS`` or ``<genomad data dir>/nn_classifier.npz`` in the schema of
genomad_amd/weights.py.  With WORLD_SIZE > 1 (one process per GPU, e.g. started by
``python -m torch.distributed.run`` — used only as a process launcher) the contigs are sharded across
ranks, the per-contig scores are collected with one RCCL gather (genomad_amd/rccl.py, no torch) and rank 0
writes the files.
"""
import concurrent.futures
import functools
import hashlib
import json
import os
import shutil
import sys
import threading
import time
from collections import namedtuple
from datetime import datetime, timezone
from pathlib import Path
from types import SimpleNamespace

import numpy as np

from . import sequence
from ._lib import DEFAULT_PRECISION, GnnError

# arithmetic of the fused front end (GENOMAD_AMD_PRECISION overrides): "f16x3tc" = split-f16 limbs with conv2 / conv3 by Toom-Cook
# minimal filtering, f32-class accuracy - the default, because the TSV prints four decimals and the 1e-4 tolerance has to hold
# with margin on inputs and weights nobody has measured; "f16x3" = the direct three-pass form (round 3's default, 0.82x the
# speed); "f16c6" / "f16c8" = f16 MFMA + MX-fp6 / fp8 corrections (faster, no head-room: DESIGN.md section 2); "bf16x3" =
# split-bf16 three passes (f32 range); "f32" = exact f32 reference kernels
MODULE_NAME = "nn_classification"   # utils.write_execution_info("nn_classification", ...) :207-212
TSV_HEADER = "seq_name\tchromosome_score\tplasmid_score\tvirus_score\n"   # :345


class Outputs:
    """File naming contract, genomad/_paths.py:188-236 (+ the find-proviruses files that
    utils.check_provirus_execution reads, utils.py:280-297)."""

    def __init__(self, prefix: str, output_dir: Path):
        o, p = Path(output_dir), prefix
        self.nn_classification_log = o / f"{p}_nn_classification.log"
        d = self.nn_classification_dir = o / f"{p}_nn_classification"
        self.nn_classification_execution_info = d / f"{p}_nn_classification.json"
        self.encoded_sequences_dir = d / f"{p}_encoded_sequences"
        self.seq_window_id_output = self.encoded_sequences_dir / f"{p}_seq_window_id.npz"
        self.nn_classification_output = d / f"{p}_nn_classification.tsv"
        self.nn_classification_npz_output = d / f"{p}_nn_classification.npz"
        self.encoded_proviruses_dir = d / f"{p}_encoded_proviruses"
        self.provirus_window_id_output = self.encoded_proviruses_dir / f"{p}_provirus_window_id.npz"
        self.provirus_nn_classification_output = d / f"{p}_provirus_nn_classification.tsv"
        self.provirus_nn_classification_npz_output = d / f"{p}_provirus_nn_classification.npz"
        # written only when GENOMAD_AMD_EMBEDDINGS=1 (encoder embeddings per contig; no counterpart in the reference)
        self.nn_embeddings_output = d / f"{p}_nn_embeddings.npz"
        self.provirus_nn_embeddings_output = d / f"{p}_provirus_nn_embeddings.npz"
        # written only when GENOMAD_AMD_SCAN_STRIDE is set (score tracks along the contigs; no counterpart in the reference)
        self.nn_scan_output = d / f"{p}_nn_scan.npz"
        self.provirus_nn_scan_output = d / f"{p}_provirus_nn_scan.npz"
        # written only when GENOMAD_AMD_STRAND is reverse or both (each strand's contig scores; no counterpart in the reference)
        self.nn_strand_output = d / f"{p}_nn_strand.npz"
        self.provirus_nn_strand_output = d / f"{p}_provirus_nn_strand.npz"
        # written only when GENOMAD_AMD_OCCLUSION_BLOCK is set (occlusion maps of the contigs; no counterpart in the reference)
        self.nn_occlusion_output = d / f"{p}_nn_occlusion.npz"
        self.provirus_nn_occlusion_output = d / f"{p}_provirus_nn_occlusion.npz"
        # written only when GENOMAD_AMD_ATTRIBUTION_BIN is set (attention contribution maps of the windows; no counterpart in the reference)
        self.nn_attribution_output = d / f"{p}_nn_attribution.npz"
        self.provirus_nn_attribution_output = d / f"{p}_provirus_nn_attribution.npz"
        # written only when GENOMAD_AMD_REGION_PENALTY is set (region calls along the score tracks; no counterpart in the reference)
        self.nn_regions_output = d / f"{p}_nn_regions.npz"
        self.nn_regions_tsv_output = d / f"{p}_nn_regions.tsv"
        self.provirus_nn_regions_output = d / f"{p}_provirus_nn_regions.npz"
        self.provirus_nn_regions_tsv_output = d / f"{p}_provirus_nn_regions.tsv"
        # written only when GENOMAD_AMD_REGION_EMBEDDINGS=1 (encoder embeddings per called region; no counterpart in the reference)
        self.nn_region_embeddings_output = d / f"{p}_nn_region_embeddings.npz"
        self.provirus_nn_region_embeddings_output = d / f"{p}_provirus_nn_region_embeddings.npz"
        # written only when the analysis is requested (the analyses of the per-contig embeddings, ANALYSES below: <stem>.npz and,
        # for all but the neighbours, <stem>.tsv; no counterpart in the reference)
        for stage in self._STAGE.values():
            for a in ANALYSES_RUN:
                setattr(self, f"{stage}nn_{a.name}_output", d / f"{p}_{stage}nn_{a.name}.npz")
                if a.tsv:
                    setattr(self, f"{stage}nn_{a.name}_tsv_output", d / f"{p}_{stage}nn_{a.name}.tsv")
        f = o / f"{p}_find_proviruses"
        self.find_proviruses_execution_info = f / f"{p}_find_proviruses.json"
        self.find_proviruses_output = f / f"{p}_provirus.tsv"
        self.find_proviruses_nucleotide_output = f / f"{p}_provirus.fna"
        self.find_proviruses_proteins_output = f / f"{p}_provirus_proteins.faa"
        self.find_proviruses_genes_output = f / f"{p}_provirus_genes.tsv"

    _STAGE = {"sequence": "", "provirus": "provirus_"}          # main()'s name of a stage -> what its files' names carry

    def files(self, what, name):
        """(npz, tsv or None) of a stage's output ``name`` - "strand", "regions", ..., or one of the ANALYSES"""
        stem = f"{self._STAGE[what]}nn_{name}"
        return getattr(self, f"{stem}_output"), getattr(self, f"{stem}_tsv_output", None)

    def classification_files(self, what):
        """(directory of the encoded windows, window ids, scores npz, scores tsv) of a stage"""
        if what == "sequence":
            return self.encoded_sequences_dir, self.seq_window_id_output, self.nn_classification_npz_output, self.nn_classification_output
        return (self.encoded_proviruses_dir, self.provirus_window_id_output, self.provirus_nn_classification_npz_output,
                self.provirus_nn_classification_output)


class Console:
    """Minimal stand-in for utils.HybridConsole (utils.py:42-123): messages go to stdout (unless
    quiet) and are appended to the log file, which is deleted at construction if it exists."""

    def __init__(self, output_file=None, verbose=True):
        self.output_file, self.verbose = output_file, verbose
        if output_file and Path(output_file).exists():
            Path(output_file).unlink()

    def _emit(self, msg, stream):
        line = f"[{datetime.now().strftime('%X')}] {msg}"
        if stream is not None:
            print(line, file=stream, flush=True)
        if self.output_file:
            with open(self.output_file, "a") as fout:
                fout.write(line + "\n")

    def log(self, msg, **_):
        self._emit(msg, sys.stdout if self.verbose else None)

    def error(self, msg, **_):
        self._emit(msg, sys.stderr)


def _md5_of(path, size=1 << 22) -> str:   # utils.py:216-223 (same digest; bigger blocks)
    m = hashlib.md5()
    with open(path, "rb") as fin:
        for block in iter(lambda: fin.read(size), b""):
            m.update(block)
    return m.hexdigest()


_MD5_FUTURES = {}
_MD5_LOCK = threading.Lock()


def md5_async(path) -> "concurrent.futures.Future":
    """The md5 of ``path`` as a future, computed once per (path, size, mtime) on a background thread.
    The reference hashes the input up to three times per run (utils.py:241, :277, :284) at
    ≈ 0.9 GB/s — comparable to the whole GPU classification of the same file — so main() starts it
    first and everything that needs the digest waits on the same future (hashlib releases the GIL)."""
    st = os.stat(path)
    key = (str(Path(path).resolve()), st.st_size, st.st_mtime_ns)
    with _MD5_LOCK:
        fut = _MD5_FUTURES.get(key)
        if fut is None:
            if len(_MD5_FUTURES) > 8:
                _MD5_FUTURES.clear()
            fut = concurrent.futures.Future()
            _MD5_FUTURES[key] = fut

            def work():
                try:
                    fut.set_result(_md5_of(path))
                except BaseException as exc:  # noqa: BLE001
                    fut.set_exception(exc)
            threading.Thread(target=work, name="genomad-amd-md5").start()
    return fut


def get_md5(path, size=None) -> str:      # utils.py:216-223
    return md5_async(path).result()


def write_execution_info(module_name, input_file: Path, parameters: dict, output_file: Path, start_time=None):
    """utils.py:238-254, byte for byte (indent=4, trailing newline, local-tz ISO start time)."""
    start_time = start_time or datetime.now(timezone.utc).astimezone().isoformat()
    dump = json.dumps({"module": module_name, "input": Path(input_file).name,
                       "input_md5": get_md5(input_file),
                       "start_time": start_time,
                       "parameters": parameters}, indent=4)
    tmp = Path(f"{output_file}.tmp{os.getpid()}")      # never leave a half-written JSON for a concurrent reader
    with open(tmp, "w") as fout:
        fout.write(f"{dump}\n")
    os.replace(tmp, output_file)


def compare_executions(input_file, parameters, execution_info_file) -> bool:   # utils.py:266-277
    with open(execution_info_file) as fin:
        info = json.load(fin)
    return parameters == info["parameters"] and get_md5(input_file) == info["input_md5"]


def check_provirus_execution(outputs: Outputs, input_file) -> bool:   # utils.py:280-297
    if not outputs.find_proviruses_execution_info.exists():
        return False
    with open(outputs.find_proviruses_execution_info) as fin:
        if get_md5(input_file) != json.load(fin)["input_md5"]:
            return False
    required = [outputs.find_proviruses_output, outputs.find_proviruses_nucleotide_output,
                outputs.find_proviruses_proteins_output, outputs.find_proviruses_genes_output]
    if not all(p.exists() for p in required):
        return False
    with sequence.open_text(outputs.find_proviruses_output) as fin:
        next(fin, None)
        return sum(1 for _ in fin) > 0


def write_tsv(path, names, predictions):
    """nn_classification.py:344-348: '%.4f' columns joined by tabs, no trailing tab."""
    p = np.asarray(predictions)
    with open(path, "w") as fout:
        fout.write(TSV_HEADER)
        if p.ndim == 2 and p.shape[1] == 3:      # the module's only shape: one formatted write per 64 Ki contigs
            cols = [p[:, j].tolist() for j in range(3)]        # exact float32 -> float conversions: the same digits
            for lo in range(0, len(p), 1 << 16):
                hi = lo + (1 << 16)
                fout.write("".join(f"{n}\t{a:.4f}\t{b:.4f}\t{c:.4f}\n" for n, a, b, c in
                                   zip(names[lo:hi], cols[0][lo:hi], cols[1][lo:hi], cols[2][lo:hi])))
        else:
            for name, scores in zip(names, p):
                row = "\t".join(f"{x:.4f}" for x in scores)
                fout.write(f"{name}\t{row}\n")


def find_weights() -> Path:
    cand = []
    if os.environ.get("GENOMAD_AMD_WEIGHTS"):
        cand.append(Path(os.environ["GENOMAD_AMD_WEIGHTS"]))
    try:
        from genomad._paths import GenomadData   # only when the reference package is installed
        cand.append(Path(GenomadData.nn_model_file).with_suffix(".npz"))
        cand.append(Path(GenomadData.nn_model_file))          # the reference's own Keras HDF5 blob
    except Exception:  # noqa: BLE001
        pass
    for c in cand:
        if c.is_file():
            return c
    raise FileNotFoundError(
        "nn classifier weights not found: set GENOMAD_AMD_WEIGHTS to an .npz in the schema of "
        "genomad_amd/weights.py, or to the reference's nn_classifier.h5 (read through libhdf5, "
        "see genomad_amd/h5weights.py)")


def load_weights_file(path: Path) -> dict:
    """``.npz`` in the repo schema, or the reference's Keras HDF5 (genomad/data/nn_classifier.h5)."""
    from . import weights as W
    if Path(path).suffix.lower() in (".h5", ".hdf5"):
        from . import h5weights
        return h5weights.load_h5(path)
    return W.load_npz(path)


_ENGINE = None


def _engine():
    """One engine per process (the reference builds its Keras model twice, :309 and :379; here the
    weights are uploaded once and reused for the provirus pass)."""
    global _ENGINE
    if _ENGINE is None:
        from . import rccl
        from .engine import NNEngine
        # the reference module sets CUDA_VISIBLE_DEVICES=-1 at import (nn_classification.py:8), which
        # HIP honours; undo it before the HIP runtime is initialised (main() and install() do so as well)
        rccl.prepare_env()
        device = int(os.environ.get("GENOMAD_AMD_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        _ENGINE = NNEngine(device, load_weights_file(find_weights()))
    return _ENGINE




def configured_precision() -> str:
    """GENOMAD_AMD_PRECISION if set (one of the library's arithmetic names), else the default; an unknown name is an error
    before anything is read or written, not a KeyError in the middle of a run."""
    from ._lib import OUT_OF_TOLERANCE, PRECISIONS
    name = os.environ.get("GENOMAD_AMD_PRECISION", DEFAULT_PRECISION)
    if name not in PRECISIONS:
        raise ValueError(f"GENOMAD_AMD_PRECISION={name!r}: expected one of {sorted(PRECISIONS)} (default {DEFAULT_PRECISION})")
    if name in OUT_OF_TOLERANCE and os.environ.get("GENOMAD_AMD_ALLOW_OUT_OF_TOLERANCE") != "1":
        raise ValueError(f"GENOMAD_AMD_PRECISION={name!r} is a measurement mode: max |dscore| {OUT_OF_TOLERANCE[name]:.1e} against the reference "
                         f"arithmetic on 10^6 windows, outside the 1e-4 tolerance; set GENOMAD_AMD_ALLOW_OUT_OF_TOLERANCE=1 to use it anyway")
    return name


def _warn_out_of_tolerance(console, name):
    """One log line per run for an arithmetic that was let through by GENOMAD_AMD_ALLOW_OUT_OF_TOLERANCE=1."""
    from ._lib import OUT_OF_TOLERANCE
    if name in OUT_OF_TOLERANCE and ("oot", name) not in _WARNED:
        _WARNED.add(("oot", name))
        msg = (f"WARNING: arithmetic {name} is OUTSIDE the 1e-4 score tolerance at scale (measured {OUT_OF_TOLERANCE[name]:.1e} on 10^6 "
               f"windows); it runs only because GENOMAD_AMD_ALLOW_OUT_OF_TOLERANCE=1 is set.  The 64-window parity sentinel cannot see a 1-in-10^5 tail.")
        (console.log if console is not None else print)(msg)
_WARNED = set()


# what to recompute a batch with when an f16-operand arithmetic returns non-finite scores: the Toom-Cook form's transformed
# activations leave the f16 range first (|activation| > ~2 000), the direct f16 forms at 65 504, bf16x3 has the f32 range
RANGE_FALLBACKS = {"f16x3tk": ("f16x3", "bf16x3"), "f16x3tc": ("f16x3", "bf16x3"), "f16x3": ("bf16x3",), "f16c6": ("bf16x3",)}

# ---- the k-mer tables of "f16x3tk" (gnn_fused_tk.hip): conv2 as a 137 GB table of all 14-mers, head A's pair products as an 8.8 GB
# (entry, 9-mer) table.  1.4x the default arithmetic's speed, the same scores to 1e-6 - and 1.5 .. 6 seconds of hipMalloc to set up,
# which a window costing 5 us repays after a few million windows.  GENOMAD_AMD_KMER_TABLES: "auto" (default) builds them when the
# run's input is at least GENOMAD_AMD_KMER_TABLES_MIN_GB (default 18 = 3 M windows) of FASTA or the engine already has them,
# "1" always, "0" never.  A device that cannot hold them (156 GB + workspaces) keeps the default arithmetic; so does the whole
# run when ANY rank cannot (the scores must not depend on which rank classified a contig).  The decision depends on the input,
# never on the number of ranks: a run gives the same bits on 1 GPU and on 8.
KMER_TABLES_MIN_GB = 18.0


def select_arithmetic(eng, precision: str, input_bytes: int, comm=None, console=None) -> str:
    """The arithmetic main() classifies with: ``precision`` (configured_precision()), promoted from "f16x3tc" to "f16x3tk" when the
    k-mer tables are there or worth building (see above).  An explicit GENOMAD_AMD_PRECISION=f16x3tk that cannot be served is an
    error; every other arithmetic is returned as it is."""
    if precision not in ("f16x3tc", "f16x3tk") or not hasattr(eng, "build_kmer_tables"):
        return precision
    policy = os.environ.get("GENOMAD_AMD_KMER_TABLES", "auto").lower()
    if policy not in ("auto", "0", "1"):
        raise ValueError(f"GENOMAD_AMD_KMER_TABLES={policy!r}: expected auto, 0 or 1")
    explicit = precision == "f16x3tk"
    min_bytes = float(os.environ.get("GENOMAD_AMD_KMER_TABLES_MIN_GB", KMER_TABLES_MIN_GB)) * 1e9
    want = explicit or policy == "1" or (policy == "auto" and (eng.has_kmer_tables() or input_bytes >= min_bytes))
    if comm is not None:                       # eng.has_kmer_tables() is per process: every rank follows what ANY rank wants
        want = bool(np.asarray(comm.allgather_i64([1 if want else 0])).any())
    ok = False
    if want:
        t = time.perf_counter()
        had = eng.has_kmer_tables()
        ok = eng.build_kmer_tables()
        if ok and not had and console is not None:
            console.log(f"k-mer tables built on the device in {time.perf_counter() - t:.1f} s (14-mer table of conv2, 9-mer table of head A's pair products).")
    if comm is not None:                       # ... and what EVERY rank could build (allgather_i64: the transport every comm of sharding.py has)
        ok = bool(np.asarray(comm.allgather_i64([1 if ok else 0])).all())
    if want and not ok:
        if explicit:
            raise RuntimeError("GENOMAD_AMD_PRECISION=f16x3tk: the device cannot hold the k-mer tables (156 GB + workspaces); "
                               "unset it to run the default arithmetic")
        if console is not None:
            console.log("k-mer tables not built (device memory): classifying with the default arithmetic f16x3tc.")
    return "f16x3tk" if ok else "f16x3tc"


def _range_fallback(console, what, to):
    """The f16-operand modes cannot represent activations beyond their range; scores that come back
    non-finite are recomputed with the next arithmetic of RANGE_FALLBACKS.  ``what`` is the arithmetic that just
    returned the non-finite scores (on the second hop of a chain: the first fallback, not the configured one).
    Said once per run and pair."""
    if (what, to) not in _WARNED:
        _WARNED.add((what, to))
        msg = (f"Non-finite class scores from the f16 arithmetic ({what}): activations left its range; "
               f"recomputing the affected batch with {to}.")
        (console.log if console is not None else print)(msg)


def _with_range_fallback(run, precision, console=None):
    """``run(arithmetic)`` -> (scores, extra); walks RANGE_FALLBACKS[precision] while the scores are non-finite.
    Returns (scores, extra, arithmetic that produced them)."""
    used = precision
    pr, extra = run(used)
    for nxt in RANGE_FALLBACKS.get(precision, ()):
        if np.isfinite(pr).all():
            break
        _range_fallback(console, used, nxt)
        used = nxt
        pr, extra = run(used)
    return pr, extra, used


def classify_contigs_safely(eng, seq, offsets, single_window, precision, console=None):
    """NNEngine.classify_contigs with the range fallback of :func:`_range_fallback`."""
    pr, wid, _ = _with_range_fallback(lambda a: eng.classify_contigs(seq, offsets, single_window, a), precision, console)
    return pr, wid


def embed_contigs_safely(eng, seq, offsets, single_window, precision, console=None):
    """NNEngine.embed_contigs with the range fallback of :func:`_range_fallback`: a piece whose scores come back non-finite is
    recomputed with the next arithmetic, and its embeddings are those of that same recomputation.  (scores, embeddings, ids)."""
    def run(a):
        pr, emb, wid = eng.embed_contigs(seq, offsets, single_window, a)
        return pr, (emb, wid)
    pr, (emb, wid), _ = _with_range_fallback(run, precision, console)
    return pr, emb, wid


def _env_similarity(name, meaning):
    """The switch ``name`` as a cosine similarity: a float in [-1, 1], returned as it is compared - the float32 it rounds to; unset or
    empty: None.  Any other value is a ``ValueError`` that ends with ``meaning``."""
    v = os.environ.get(name, "").strip()
    if not v:
        return None
    try:
        t = float(v)
    except ValueError:
        t = float("nan")
    if not -1.0 <= t <= 1.0:                             # a NaN fails both comparisons
        raise ValueError(f"{name}={v!r}: expected a float in [-1, 1] {meaning}")
    return float(np.float32(t))


def _env_int(name, lo, hi, meaning, default=None):
    """The switch ``name`` as an integer in [lo, hi] (``hi`` None: no upper bound); unset or empty: ``default``.  Any other value is a
    ``ValueError`` that ends with ``meaning``."""
    v = os.environ.get(name, "").strip()
    if not v:
        return default
    try:
        k = int(v)
    except ValueError:
        k = lo - 1
    if k < lo or (hi is not None and k > hi):
        bounds = f"in [{lo}, {hi}]" if hi is not None and hi < (1 << 31) - 1 else f">= {lo}"      # the int32 limit is not spelt out
        raise ValueError(f"{name}={v!r}: expected an integer {bounds} {meaning}")
    return k


def _env_refines(name, other, advice):
    """``name`` only refines the request of ``other``: set without it, it is a ``ValueError``"""
    m = os.environ.get(name, "").strip()
    if m:
        raise ValueError(f"{name}={m!r} needs {other}: {advice} {name}")


def _strand_entry(strand) -> dict:
    """the ``strand`` entry of an output file, which only reverse / both write (:func:`_npz_strand`)"""
    return {"strand": np.array(strand)} if strand != "forward" else {}


_UNREADABLE = object()        # what _request_of_file says of a file it cannot read: equal to no request, so the stage runs again


def _request_of_file(path, keys):
    """The request an output file of a stage was computed with, as it spells it: the value of its entry ``keys`` = ((name, cast),),
    or the tuple of several; no file = None (nothing was asked for); a file that cannot be read = ``_UNREADABLE``."""
    if not Path(path).exists():
        return None
    try:
        z = np.load(path)
        got = tuple(cast(z[k]) for k, cast in keys)
    except Exception:  # noqa: BLE001
        return _UNREADABLE
    return got[0] if len(got) == 1 else got


def embeddings_requested() -> bool:
    """GENOMAD_AMD_EMBEDDINGS=1: main() also writes the per-contig encoder embeddings (<prefix>_nn_embeddings.npz); unset or 0:
    nothing changes.  Any other value is an error."""
    v = os.environ.get("GENOMAD_AMD_EMBEDDINGS", "0").strip()
    if v not in ("", "0", "1"):
        raise ValueError(f"GENOMAD_AMD_EMBEDDINGS={v!r}: expected 1 (write the embeddings) or 0")
    return v == "1"


def scan_contigs_safely(eng, seq, offsets, stride, single_window, precision, console=None):
    """NNEngine.scan_contigs with the range fallback of :func:`_range_fallback`: a piece with a non-finite window score is scanned
    again with the next arithmetic, and everything returned is that scan's."""
    def run(a):
        res = eng.scan_contigs(seq, offsets, stride, single_window, a)
        return res.scores, res
    _, res, _ = _with_range_fallback(run, precision, console)
    return res


def scan_stride_requested():
    """GENOMAD_AMD_SCAN_STRIDE=<int in [1, 6000]>: main() also writes the score tracks along the contigs (<prefix>_nn_scan.npz),
    windows every that many bases; unset or empty: nothing changes (None).  Any other value is an error."""
    return _env_int("GENOMAD_AMD_SCAN_STRIDE", 1, sequence.WINDOW, "(bases between window starts)")


def _scan_file_has_stride(path, stride) -> bool:
    try:
        return int(np.load(path)["stride"]) == stride
    except Exception:  # noqa: BLE001  (missing or unreadable: scan again)
        return False


def occlude_contigs_safely(eng, seq, offsets, block, single_window, precision, console=None):
    """NNEngine.occlude_contigs with the range fallback of :func:`_range_fallback`: a piece with a non-finite window score or delta is
    occluded again with the next arithmetic, and everything returned is that run's."""
    def run(a):
        res = eng.occlude_contigs(seq, offsets, block, single_window, a)
        return np.concatenate([res.scores.reshape(-1), res.delta.reshape(-1)]), res
    _, res, _ = _with_range_fallback(run, precision, console)
    return res


def occlusion_block_requested():
    """GENOMAD_AMD_OCCLUSION_BLOCK=<int in [1, 6000]>: main() also writes the occlusion maps of the contigs (<prefix>_nn_occlusion.npz):
    every window scored again with each block of that many bases set to N; unset or empty: nothing changes (None).  Any other value
    is an error."""
    return _env_int("GENOMAD_AMD_OCCLUSION_BLOCK", 1, sequence.WINDOW, "(bases per occluded block)")


def attribute_contigs_safely(eng, seq, offsets, bin, single_window, precision, console=None):
    """NNEngine.attribute_contigs with the range fallback of :func:`_range_fallback`: a piece with a non-finite window score is
    attributed again with the next arithmetic, and everything returned is that run's."""
    def run(a):
        res = eng.attribute_contigs(seq, offsets, bin, single_window, a)
        return res.window_scores, res
    _, res, _ = _with_range_fallback(run, precision, console)
    return res


ATTRIBUTION_POSITIONS = 749          # pooled positions per attention head (GNN_POOLED)


def attribution_bin_requested():
    """GENOMAD_AMD_ATTRIBUTION_BIN=<int in [1, 749]>: main() also writes the attention contribution maps of the windows
    (<prefix>_nn_attribution.npz): each bin of that many pooled positions' share of every window's logits, computed in the pass that
    scores the window; unset or empty: nothing changes (None).  Any other value is an error."""
    return _env_int("GENOMAD_AMD_ATTRIBUTION_BIN", 1, ATTRIBUTION_POSITIONS, "(pooled positions per bin of the map)")


def region_penalty_requested():
    """GENOMAD_AMD_REGION_PENALTY=<float in [0, 4096]>: main() also calls regions along the score tracks of GENOMAD_AMD_SCAN_STRIDE
    (<prefix>_nn_regions.npz and .tsv): a Viterbi segmentation in which a switch between classes costs that many score x bins;
    unset or empty: nothing changes (None).  Any other value is an error."""
    v = os.environ.get("GENOMAD_AMD_REGION_PENALTY", "").strip()
    if not v:
        return None
    try:
        penalty = float(v)
    except ValueError:
        penalty = -1.0
    if not 0.0 <= penalty <= sequence.REGION_PENALTY_MAX:
        raise ValueError(f"GENOMAD_AMD_REGION_PENALTY={v!r}: expected a number in [0, {sequence.REGION_PENALTY_MAX:g}] (the cost of a switch "
                         "between classes, in score x bins)")
    return penalty


def embed_intervals_safely(eng, seq, offsets, stride, contig, start, end, strand, single_window, precision, console=None):
    """NNEngine.embed_intervals with the range fallback of :func:`_range_fallback`: a piece with a non-finite interval score or
    embedding is folded again with the next arithmetic, and everything returned is that pass's."""
    def run(a):
        res = eng.embed_intervals(seq, offsets, stride, contig, start, end, strand, single_window, a)
        return np.concatenate([res.scores.ravel(), res.embedding.ravel()]), res
    _, res, _ = _with_range_fallback(run, precision, console)
    return res


def region_embeddings_requested() -> bool:
    """GENOMAD_AMD_REGION_EMBEDDINGS=1: main() also writes one encoder embedding per region called under GENOMAD_AMD_REGION_PENALTY
    (<prefix>_nn_region_embeddings.npz: the mean over the scan windows centred in the region, their mean scores, their number and
    the coherence of their rows); unset or 0: nothing changes.  Any other value is an error."""
    v = os.environ.get("GENOMAD_AMD_REGION_EMBEDDINGS", "0").strip()
    if v not in ("", "0", "1"):
        raise ValueError(f"GENOMAD_AMD_REGION_EMBEDDINGS={v!r}: expected 1 (write the region embeddings) or 0")
    return v == "1"


NEIGHBOUR_METRIC = "cosine"          # what main() searches with


def neighbours_requested():
    """GENOMAD_AMD_NEIGHBOURS=<int in [1, 64]>: main() also writes every contig's that many nearest neighbours among the per-contig
    encoder embeddings of GENOMAD_AMD_EMBEDDINGS=1 (<prefix>_nn_neighbours.npz: cosine similarity, the contig itself excluded);
    unset or empty: nothing changes (None).  Any other value is an error."""
    return _env_int("GENOMAD_AMD_NEIGHBOURS", 1, sequence.NEIGHBOUR_K_MAX, "(neighbours per contig)")


def write_neighbours(npz_path, names_key, names, res, k, strand="forward"):
    """The neighbour file of a stage: the (idx, sim) of NNEngine.neighbours with the contig names."""
    idx, sim = res
    np.savez_compressed(npz_path, **{names_key: names, "k": np.int64(k), "metric": np.array(NEIGHBOUR_METRIC), "idx": idx, "sim": sim,
                                     **_strand_entry(strand)})


def clusters_requested():
    """GENOMAD_AMD_CLUSTERS=<float in [-1, 1]>: main() also writes the single-linkage clusters of the contigs at that cosine similarity
    of the per-contig encoder embeddings of GENOMAD_AMD_EMBEDDINGS=1 (<prefix>_nn_clusters.npz and .tsv); unset or empty: nothing
    changes (None).  Any other value is an error.  Returns the threshold as it is compared: the float32 it rounds to."""
    return _env_similarity("GENOMAD_AMD_CLUSTERS", "(the cosine similarity at which two contigs are joined)")


CLUSTER_TSV_HEADER = "seq_name\tcluster\tcluster_size\trepresentative\tdegree\n"


def write_clusters_tsv(path, names, res):
    """One line per contig of a ClusterResult: the name of its cluster's label contig, the cluster's size, the name of its
    representative and the contig's own degree; a contig without a valid embedding has NA, 0, NA, 0."""
    with open(path, "w") as fout:
        fout.write(CLUSTER_TSV_HEADER)
        for i, name in enumerate(names):
            if res.label[i] < 0:
                fout.write(f"{name}\tNA\t0\tNA\t0\n")
            else:
                fout.write(f"{name}\t{names[res.label[i]]}\t{res.size[i]}\t{names[res.rep[i]]}\t{res.degree[i]}\n")


def write_clusters(npz_path, tsv_path, names_key, names, res, threshold, strand="forward"):
    """Both cluster files of a stage: the arrays of a ClusterResult with the contig names, and one line per contig."""
    np.savez_compressed(npz_path, **{names_key: names, "threshold": np.float64(threshold), "metric": np.array(NEIGHBOUR_METRIC),
                                     "label": res.label, "degree": res.degree, "size": res.size, "rep": res.rep, **_strand_entry(strand)})
    write_clusters_tsv(tsv_path, names, res)


DENSITY_MIN_POINTS_DEFAULT = 5


def density_requested():
    """GENOMAD_AMD_DENSITY=<float in [-1, 1]>: main() also writes the density clusters (DBSCAN) of the contigs at that cosine similarity
    of the per-contig encoder embeddings of GENOMAD_AMD_EMBEDDINGS=1 (<prefix>_nn_density.npz and .tsv); unset or empty: nothing
    changes (None).  GENOMAD_AMD_DENSITY_MIN_POINTS=<integer >= 1> (default 5) is how many contigs, itself included, a contig needs
    within the threshold to be a core contig; it is an error without GENOMAD_AMD_DENSITY.  Any other value of either is an error.
    Returns (the threshold as it is compared: the float32 it rounds to, min_points), or None."""
    t = _env_similarity("GENOMAD_AMD_DENSITY", "(the cosine similarity within which contigs count towards each other's density)")
    if t is None:
        _env_refines("GENOMAD_AMD_DENSITY_MIN_POINTS", "GENOMAD_AMD_DENSITY", "set the threshold of the density clusters or unset")
        return None
    return t, _env_int("GENOMAD_AMD_DENSITY_MIN_POINTS", 1, sequence.DENSITY_MIN_POINTS_END - 1,
                       "(below 2^31): the contigs, itself included, that a core contig has within the threshold", DENSITY_MIN_POINTS_DEFAULT)


DENSITY_TSV_HEADER = "seq_name\tcluster\tcluster_size\tkind\tanchor\tsimilarity\tdegree\n"


def write_density_tsv(path, names, res):
    """One line per contig of a DensityResult: the name of its cluster's label contig, the cluster's size, core | border | noise |
    invalid, the name of its anchor (a core contig's is its own), a border contig's similarity to its anchor and the contig's own
    degree; NA wherever there is none."""
    with open(path, "w") as fout:
        fout.write(DENSITY_TSV_HEADER)
        for i, name in enumerate(names):
            kind = sequence.DENSITY_KINDS[int(res.kind[i])]
            cluster = names[res.label[i]] if res.label[i] >= 0 else "NA"
            anchor = names[res.anchor[i]] if res.anchor[i] >= 0 else "NA"
            sim = f"{res.sim[i]:.6f}" if kind == "border" else "NA"
            fout.write(f"{name}\t{cluster}\t{res.size[i]}\t{kind}\t{anchor}\t{sim}\t{res.degree[i]}\n")


def write_density(npz_path, tsv_path, names_key, names, res, strand="forward"):
    """Both density files of a stage: the arrays of a DensityResult with the contig names, and one line per contig."""
    np.savez_compressed(npz_path, **{names_key: names, "threshold": np.float64(res.threshold), "min_points": np.int64(res.min_points),
                                     "metric": np.array(res.metric), "label": res.label, "degree": res.degree, "size": res.size,
                                     "anchor": res.anchor, "sim": res.sim, "kind": res.kind, **_strand_entry(strand)})
    write_density_tsv(tsv_path, names, res)


def hdbscan_requested():
    """GENOMAD_AMD_HDBSCAN=<integer >= 2>: main() also writes the HDBSCAN clusters of the contigs - the density-aware linkage tree
    under the cosine similarity of the per-contig encoder embeddings of GENOMAD_AMD_EMBEDDINGS=1, condensed with that minimum
    cluster size and cut by excess of mass (<prefix>_nn_hdbscan.npz and .tsv); unset or empty: nothing changes (None).
    GENOMAD_AMD_HDBSCAN_MIN_POINTS=<integer in [1, 65]> (default: the minimum cluster size, 65 at the most) is how many contigs,
    itself included, a contig's core similarity looks at; it is an error without GENOMAD_AMD_HDBSCAN.  Any other value of either
    is an error.  Returns (min_cluster_size, min_points), or None."""
    size = _env_int("GENOMAD_AMD_HDBSCAN", 2, (1 << 31) - 1, "(below 2^31): the contigs a cluster has at the least")
    if size is None:
        _env_refines("GENOMAD_AMD_HDBSCAN_MIN_POINTS", "GENOMAD_AMD_HDBSCAN", "set the minimum cluster size or unset")
        return None
    return size, _env_int("GENOMAD_AMD_HDBSCAN_MIN_POINTS", 1, sequence.DENSITY_TREE_MIN_POINTS_MAX,
                          "(the contigs, itself included, that a contig's core similarity looks at)",
                          min(size, sequence.DENSITY_TREE_MIN_POINTS_MAX))


HDBSCAN_TSV_HEADER = "seq_name\tcluster\tcluster_size\tcore_similarity\tlambda_out\n"


def write_hdbscan_tsv(path, names, tree, found):
    """One line per contig: the name of its cluster's label contig and the cluster's size (NA, 0 for noise), its core similarity and
    the lambda at which it left the deepest cluster it was in; a contig without a valid embedding has NA, 0, NA, NA."""
    label = found["label"]
    size = np.bincount(label[label >= 0], minlength=len(names))
    with open(path, "w") as fout:
        fout.write(HDBSCAN_TSV_HEADER)
        for i, name in enumerate(names):
            if not tree.valid[i]:
                fout.write(f"{name}\tNA\t0\tNA\tNA\n")
                continue
            cluster = names[label[i]] if label[i] >= 0 else "NA"
            core = f"{tree.core[i]:.6f}" if np.isfinite(tree.core[i]) else "NA"
            fout.write(f"{name}\t{cluster}\t{size[label[i]] if label[i] >= 0 else 0}\t{core}\t{found['lambda_out'][i]:.6g}\n")


def write_hdbscan(npz_path, tsv_path, names_key, names, res, min_cluster_size, strand="forward"):
    """Both HDBSCAN files of a stage: the DensityTreeResult's tree and core similarities, the labels and the cluster table of
    ``sequence.hdbscan_clusters`` with the contig names, and one line per contig."""
    tree, found = res
    np.savez_compressed(npz_path, **{names_key: names, "min_cluster_size": np.int64(min_cluster_size), "min_points": np.int64(tree.min_points),
                                     "metric": np.array(tree.metric), "a": tree.a, "b": tree.b, "sim": tree.sim, "core": tree.core,
                                     "valid": tree.valid, "rounds": np.int64(tree.rounds), "label": found["label"],
                                     "lambda_out": found["lambda_out"],
                                     **{"cluster_" + k: found[k] for k in ("parent", "birth", "stability", "size", "selected")},
                                     "cluster": found["cluster"], **_strand_entry(strand)})
    write_hdbscan_tsv(tsv_path, names, tree, found)


def _run_hdbscan(eng, emb, request):
    tree = eng.density_tree(emb, request[1], NEIGHBOUR_METRIC)
    return tree, tree.hdbscan(request[0])


def kmeans_requested():
    """GENOMAD_AMD_KMEANS=<integer in [1, 65535]>: main() also writes the spherical k-means of the contigs - exactly that many groups
    under the cosine similarity of the per-contig encoder embeddings of GENOMAD_AMD_EMBEDDINGS=1, and one centroid per group
    (<prefix>_nn_kmeans.npz and .tsv); unset or empty: nothing changes (None).  GENOMAD_AMD_KMEANS_MAX_ITER=<integer in [0, 1000]>
    (default 50) bounds the updates; it is an error without GENOMAD_AMD_KMEANS.  Any other value of either is an error.  Returns
    (k, max_iter), or None."""
    k = _env_int("GENOMAD_AMD_KMEANS", 1, sequence.KMEANS_K_MAX, "(the number of groups)")
    if k is None:
        _env_refines("GENOMAD_AMD_KMEANS_MAX_ITER", "GENOMAD_AMD_KMEANS", "set the number of groups or unset")
        return None
    return k, _env_int("GENOMAD_AMD_KMEANS_MAX_ITER", 0, sequence.KMEANS_MAX_ITER_MAX, "(the centroid updates at the most)",
                       sequence.KMEANS_MAX_ITER_DEFAULT)


KMEANS_TSV_HEADER = "seq_name\tcluster\tcluster_size\tsimilarity\n"


def write_kmeans_tsv(path, names, res):
    """One line per contig of a KMeansResult: the index of its cluster, the cluster's size and the contig's similarity to the
    cluster's centroid; a contig without a valid embedding has NA, 0, NA."""
    with open(path, "w") as fout:
        fout.write(KMEANS_TSV_HEADER)
        for i, name in enumerate(names):
            if res.label[i] < 0:
                fout.write(f"{name}\tNA\t0\tNA\n")
            else:
                fout.write(f"{name}\t{res.label[i]}\t{res.size[res.label[i]]}\t{res.sim[i]:.6f}\n")


def write_kmeans(npz_path, tsv_path, names_key, names, res, max_iter, strand="forward"):
    """Both k-means files of a stage: the arrays of a KMeansResult with the contig names, and one line per contig."""
    np.savez_compressed(npz_path, **{names_key: names, "k": np.int64(res.k), "max_iter": np.int64(max_iter), "metric": np.array("cosine"),
                                     "label": res.label, "sim": res.sim, "centroids": res.centroids, "size": res.size,
                                     "iterations": np.int64(res.iterations), "converged": np.bool_(res.converged),
                                     "init_rows": res.init_rows, "objective": np.float64(res.objective), **_strand_entry(strand)})
    write_kmeans_tsv(tsv_path, names, res)


def pca_requested():
    """GENOMAD_AMD_PCA=<integer in [1, 64]>: main() also writes that many principal components of the contigs' per-contig encoder
    embeddings of GENOMAD_AMD_EMBEDDINGS=1 - of their unit vectors, the geometry every search works in - and every contig's scores
    on them (<prefix>_nn_pca.npz and .tsv); unset or empty: nothing changes (None).  Any other value is an error.  Returns the
    number of components, or None."""
    return _env_int("GENOMAD_AMD_PCA", 1, sequence.PCA_COMPONENTS_MAX, "(the number of components)")


def write_pca_tsv(path, names, res):
    """One line per contig of a PCAResult: its scores on the components; NA for a contig without a valid embedding."""
    c = res.n_components
    with open(path, "w") as fout:
        fout.write("seq_name\t" + "\t".join(f"pc{j + 1}" for j in range(c)) + "\n")
        for i, name in enumerate(names):
            if res.valid[i]:
                fout.write(f"{name}\t" + "\t".join(f"{x:.6f}" for x in res.projection[i]) + "\n")
            else:
                fout.write(f"{name}\t" + "\t".join(["NA"] * c) + "\n")


def write_pca(npz_path, tsv_path, names_key, names, res, strand="forward"):
    """Both PCA files of a stage: the arrays of a PCAResult with the contig names, and one line per contig."""
    np.savez_compressed(npz_path, **{names_key: names, "n_components": np.int64(res.n_components), "metric": np.array("cosine"),
                                     "mean": res.mean, "components": res.components, "explained_variance": res.explained_variance,
                                     "explained_variance_ratio": res.explained_variance_ratio,
                                     "total_variance": np.float64(res.total_variance), "n_valid": np.int64(res.n_valid),
                                     "projection": res.projection, **_strand_entry(strand)})
    write_pca_tsv(tsv_path, names, res)


def representatives_requested():
    """GENOMAD_AMD_REPRESENTATIVES=<float in [-1, 1]>: main() also writes the greedy clusters of the contigs at that cosine similarity of
    the per-contig encoder embeddings of GENOMAD_AMD_EMBEDDINGS=1 - contigs walked by their number of kept windows, the larger first,
    every contig within the threshold of its representative (<prefix>_nn_representatives.npz and .tsv); unset or empty: nothing changes
    (None).  Any other value is an error.  Returns the threshold as it is compared: the float32 it rounds to."""
    return _env_similarity("GENOMAD_AMD_REPRESENTATIVES", "(the cosine similarity at which a contig joins a representative)")


REPRESENTATIVE_TSV_HEADER = "seq_name\trepresentative\tsimilarity\tcluster_size\tis_representative\n"


def write_representatives_tsv(path, names, res):
    """One line per contig of a RepresentativeResult: the name of its representative, its similarity to it (NA for a representative),
    the cluster's size and whether the contig is the representative; a contig without a valid embedding has NA, NA, 0, False."""
    with open(path, "w") as fout:
        fout.write(REPRESENTATIVE_TSV_HEADER)
        for i, name in enumerate(names):
            if res.rep[i] < 0:
                fout.write(f"{name}\tNA\tNA\t0\tFalse\n")
            elif res.rep[i] == i:
                fout.write(f"{name}\t{name}\tNA\t{res.size[i]}\tTrue\n")
            else:
                fout.write(f"{name}\t{names[res.rep[i]]}\t{res.sim[i]:.6f}\t{res.size[i]}\tFalse\n")


def write_representatives(npz_path, tsv_path, names_key, names, res, threshold, weight, strand="forward"):
    """Both representative files of a stage: the arrays of a RepresentativeResult with the contig names and the ``weight`` the contigs
    were walked by, and one line per contig."""
    np.savez_compressed(npz_path, **{names_key: names, "threshold": np.float64(threshold), "metric": np.array(NEIGHBOUR_METRIC),
                                     "weight": weight, "rep": res.rep, "sim": res.sim, "size": res.size, "rank": res.rank,
                                     "rounds": np.int64(res.rounds), **_strand_entry(strand)})
    write_representatives_tsv(tsv_path, names, res)


def linkage_requested() -> bool:
    """GENOMAD_AMD_LINKAGE=1: main() also writes the single-linkage tree of the contigs under the cosine similarity of the per-contig
    encoder embeddings of GENOMAD_AMD_EMBEDDINGS=1 - the merges that answer GENOMAD_AMD_CLUSTERS at every threshold at once
    (<prefix>_nn_linkage.npz and .tsv); unset, empty or 0: nothing changes.  Any other value is an error."""
    v = os.environ.get("GENOMAD_AMD_LINKAGE", "").strip()
    if v in ("", "0"):
        return False
    if v != "1":
        raise ValueError(f"GENOMAD_AMD_LINKAGE={v!r}: expected 1 (write the single-linkage tree of the contigs), 0 or nothing")
    return True


LINKAGE_TSV_HEADER = "rank\tcontig_a\tcontig_b\tsimilarity\tclusters_left\n"


def write_linkage_tsv(path, names, res):
    """One line per merge of a LinkageResult, best first: its rank (from 1), the names of the two contigs whose edge joins two
    clusters, the edge's similarity and the clusters left among the contigs with a valid embedding once it is made."""
    with open(path, "w") as fout:
        fout.write(LINKAGE_TSV_HEADER)
        for m in res.table(names):
            fout.write(f"{m['rank']}\t{m['a']}\t{m['b']}\t{m['sim']:.6f}\t{m['clusters_left']}\n")


def write_linkage(npz_path, tsv_path, names_key, names, res, strand="forward"):
    """Both linkage files of a stage: the arrays of a LinkageResult with the contig names, and the table of its merges."""
    np.savez_compressed(npz_path, **{names_key: names, "metric": np.array(res.metric), "a": res.a, "b": res.b, "sim": res.sim,
                                     "valid": res.valid, "rounds": np.int64(res.rounds), **_strand_entry(strand)})
    write_linkage_tsv(tsv_path, names, res)


def graph_requested():
    """GENOMAD_AMD_GRAPH=<float in [-1, 1]>: main() also writes the similarity graph of the contigs - every pair whose per-contig encoder
    embeddings of GENOMAD_AMD_EMBEDDINGS=1 have at least that cosine similarity, the edges GENOMAD_AMD_CLUSTERS joins at the same value
    (<prefix>_nn_graph.npz and .tsv); unset or empty: nothing changes (None).  Any other value is an error.  Returns the threshold as
    it is compared: the float32 it rounds to."""
    return _env_similarity("GENOMAD_AMD_GRAPH", "(the cosine similarity at which two contigs share an edge)")


GRAPH_TSV_HEADER = "contig_a\tcontig_b\tsimilarity\n"


def write_graph_tsv(path, names, res):
    """One line per edge of a GraphResult, in its order (rows ascending, a row's partners ascending): the names of the two contigs and
    their similarity - the label-label-weight ("abc") format graph tools read, behind one header line."""
    with open(path, "w") as fout:
        fout.write(GRAPH_TSV_HEADER)
        for e in res.table(names):
            fout.write(f"{e['a']}\t{e['b']}\t{e['sim']:.6f}\n")


def write_graph(npz_path, tsv_path, names_key, names, res, strand="forward"):
    """Both graph files of a stage: the arrays of a GraphResult with the contig names, and its edge list."""
    np.savez_compressed(npz_path, **{names_key: names, "threshold": np.float64(res.threshold), "metric": np.array(res.metric),
                                     "indptr": res.indptr, "col": res.col, "sim": res.sim, **_strand_entry(strand)})
    write_graph_tsv(tsv_path, names, res)


def _env_name(name, choices, default, meaning):
    """The switch ``name`` as one of the names ``choices``; unset or empty: ``default``.  Any other value is a ``ValueError`` that ends
    with ``meaning``."""
    v = os.environ.get(name, "").strip()
    if not v:
        return default
    if v not in choices:
        raise ValueError(f"{name}={v!r}: expected one of {', '.join(choices)} {meaning}")
    return v


def knn_graph_requested():
    """GENOMAD_AMD_KNN_GRAPH=<int in [1, 64]>: main() also writes the k-nearest-neighbour graph of the contigs - every pair of which one
    lists the other among its that many nearest neighbours by the per-contig encoder embeddings of GENOMAD_AMD_EMBEDDINGS=1
    (<prefix>_nn_knn_graph.npz and .tsv); unset or empty: nothing changes (None).  GENOMAD_AMD_KNN_GRAPH_MODE=union|mutual (default
    union: either lists the other; mutual: both do) and GENOMAD_AMD_KNN_GRAPH_WEIGHT=similarity|jaccard (default similarity; jaccard:
    the overlap of the two neighbourhoods) refine it; each is an error without GENOMAD_AMD_KNN_GRAPH.  Any other value of the three is
    an error.  Returns (k, mode, weight), or None."""
    k = _env_int("GENOMAD_AMD_KNN_GRAPH", 1, sequence.NEIGHBOUR_K_MAX, "(neighbours per contig)")
    if k is None:
        for companion in ("GENOMAD_AMD_KNN_GRAPH_MODE", "GENOMAD_AMD_KNN_GRAPH_WEIGHT"):
            _env_refines(companion, "GENOMAD_AMD_KNN_GRAPH", "set the neighbours per contig or unset")
        return None
    return (k, _env_name("GENOMAD_AMD_KNN_GRAPH_MODE", sequence.KNN_GRAPH_MODES, "union", "(which pairs are edges)"),
            _env_name("GENOMAD_AMD_KNN_GRAPH_WEIGHT", sequence.KNN_GRAPH_WEIGHTS, "similarity", "(what an edge weighs)"))


KNN_GRAPH_TSV_HEADER = "contig_a\tcontig_b\tweight\n"


def write_knn_graph(npz_path, tsv_path, names_key, names, res, strand="forward"):
    """Both files of a stage's k-nearest-neighbour graph: the arrays of a KNNGraphResult with the contig names, and its edge list - one
    line per edge in the CSR's order, the names of the two contigs and the weight, the label-label-weight ("abc") format graph tools
    read, behind one header line."""
    np.savez_compressed(npz_path, **{names_key: names, "k": np.int64(res.k), "mode": np.array(res.mode), "weight": np.array(res.weight),
                                     "metric": np.array(res.metric), "indptr": res.indptr, "col": res.col, "sim": res.sim,
                                     "mutual": res.mutual, "valid": res.valid, **_strand_entry(strand)})
    with open(tsv_path, "w") as fout:
        fout.write(KNN_GRAPH_TSV_HEADER)
        for e in res.table(names):
            fout.write(f"{e['a']}\t{e['b']}\t{e['weight']:.6f}\n")


def tsne_requested():
    """GENOMAD_AMD_TSNE=<integer in [1, 100000]>: main() also writes the exact t-SNE layout of the contigs - that many iterations (the
    first 250 exaggerated) over the k-nearest-neighbour graph of GENOMAD_AMD_KNN_GRAPH, from the first two principal components of
    the per-contig encoder embeddings (<prefix>_nn_tsne.npz and .tsv); unset or empty: nothing changes (None).  It lays out the graph
    of GENOMAD_AMD_KNN_GRAPH=<k>, which must be set with it (main() refuses the one without the other).  Any other value is an error.
    Returns (n_iter, k, mode, weight) - the last three the graph's request, None without one -, or None."""
    n_iter = _env_int("GENOMAD_AMD_TSNE", 1, sequence.TSNE_ITER_MAX, "(the iterations of the layout)")
    if n_iter is None:
        return None
    return (n_iter,) + (knn_graph_requested() or (None, None, None))


TSNE_TSV_HEADER = "seq_name\tx\ty\n"


def write_tsne(npz_path, tsv_path, names_key, names, res, request, strand="forward"):
    """Both layout files of a stage: the arrays of a TSNEResult with the contig names and the request, and one line per contig - its
    name and its two coordinates, NA for a contig without a valid embedding."""
    np.savez_compressed(npz_path, **{names_key: names, "n_iter": np.int64(request[0]), "k": np.int64(request[1]), "mode": np.array(request[2]),
                                     "weight": np.array(request[3]), "metric": np.array(NEIGHBOUR_METRIC), "init": np.array("pca"),
                                     "exaggeration_iter": np.int64(res.exaggeration_iter), "exaggeration": np.float64(res.exaggeration),
                                     "learning_rate": np.float64(res.learning_rate), "layout": res.layout, "z_trace": res.z_trace,
                                     "kl_divergence": np.float64(res.kl_divergence), "valid": res.valid, **_strand_entry(strand)})
    with open(tsv_path, "w") as fout:
        fout.write(TSNE_TSV_HEADER)
        for name, xy, ok in zip(names, res.layout, res.valid):
            fout.write(f"{name}\t{xy[0]:.6f}\t{xy[1]:.6f}\n" if ok else f"{name}\tNA\tNA\n")


MCL_SELECT_DEFAULT = 256


def mcl_requested():
    """GENOMAD_AMD_MCL=<a multiple of 0.25 in [1.25, 8]>: main() also writes the Markov clusters (MCL) of the contigs - the families the
    flow through the similarity graph of GENOMAD_AMD_GRAPH settles in at that inflation (<prefix>_nn_mcl.npz and .tsv); unset or empty:
    nothing changes (None).  It clusters the graph of GENOMAD_AMD_GRAPH=<threshold>, which must be set with it (main() refuses the one
    without the other).  GENOMAD_AMD_MCL_SELECT=<integer in [1, 1024]> (default 256) is how many entries a column of the flow matrix
    keeps at the most; it is an error without GENOMAD_AMD_MCL.  Any other value of either is an error.  Returns (inflation, the graph's
    threshold as it is compared or None, select), or None."""
    v = os.environ.get("GENOMAD_AMD_MCL", "").strip()
    if not v:
        _env_refines("GENOMAD_AMD_MCL_SELECT", "GENOMAD_AMD_MCL", "set the inflation of the Markov clusters or unset")
        return None
    try:
        inflation = float(v)
        sequence.mcl_inflation(inflation)
    except ValueError:
        raise ValueError(f"GENOMAD_AMD_MCL={v!r}: expected a multiple of 0.25 in [1.25, 8] (the inflation: the larger, the smaller the "
                         "clusters)") from None
    return inflation, graph_requested(), _env_int("GENOMAD_AMD_MCL_SELECT", 1, sequence.MCL_SELECT_MAX,
                                                  "(the entries a column of the flow matrix keeps at the most)", MCL_SELECT_DEFAULT)


def _run_mcl(eng, emb, request):
    """the graph at the request's threshold, computed again, and its Markov clusters"""
    inflation, threshold, select = request
    g = eng.graph(emb, threshold, NEIGHBOUR_METRIC)
    return eng.mcl(g.indptr, g.col, g.sim, g.valid, inflation=inflation, select=select), g.n_edges


MCL_TSV_HEADER = "seq_name\tcluster\tcluster_size\tattractor\tflow\n"


def write_mcl_tsv(path, names, res):
    """One line per contig of an MCLResult: the name of its cluster's label contig, the cluster's size, the name of its attractor
    (the contig most of its flow ends at) and that share of its flow; a contig without a valid embedding has NA, 0, NA, NA."""
    with open(path, "w") as fout:
        fout.write(MCL_TSV_HEADER)
        for i, name in enumerate(names):
            if res.label[i] < 0:
                fout.write(f"{name}\tNA\t0\tNA\tNA\n")
            else:
                fout.write(f"{name}\t{names[res.label[i]]}\t{res.size[i]}\t{names[res.attractor[i]]}\t{int(res.flow[i]) / sequence.MCL_ONE:.6f}\n")


def write_mcl(npz_path, tsv_path, names_key, names, res, request, strand="forward"):
    """Both Markov-cluster files of a stage: the arrays of an MCLResult with the contig names and the request, and one line per contig."""
    np.savez_compressed(npz_path, **{names_key: names, "inflation": np.float64(request[0]), "threshold": np.float64(request[1]),
                                     "select": np.int64(request[2]), "precision": np.int64(res.precision), "metric": np.array(NEIGHBOUR_METRIC),
                                     "label": res.label, "size": res.size, "attractor": res.attractor, "flow": res.flow,
                                     "is_attractor": res.is_attractor, "iterations": np.int64(res.iterations),
                                     "converged": np.bool_(res.converged), "changed": res.changed, **_strand_entry(strand)})
    write_mcl_tsv(tsv_path, names, res)


def average_linkage_requested():
    """GENOMAD_AMD_AVERAGE_LINKAGE=<cut similarity in (0, 1]>: main() also writes the average-linkage (UPGMA) clusters of the contigs -
    groups merge by the *mean* similarity between them over the similarity graph of GENOMAD_AMD_GRAPH, a pair without an edge counting
    as 0, down to that mean (<prefix>_nn_average_linkage.npz and .tsv); unset or empty: nothing changes (None).  It needs
    GENOMAD_AMD_GRAPH=<threshold>, which must be set with it (main() refuses the one without the other).  Any other value is an error.
    Returns (the cut as it is compared: a multiple of 2^-24, the graph's threshold as it is compared or None), or None."""
    v = os.environ.get("GENOMAD_AMD_AVERAGE_LINKAGE", "").strip()
    if not v:
        return None
    try:
        cut = float(v)
        if not 0.0 < cut <= 1.0:                         # a NaN fails both comparisons
            raise ValueError
        cut = sequence.average_linkage_stop(cut) / sequence.MCL_W
    except ValueError:
        raise ValueError(f"GENOMAD_AMD_AVERAGE_LINKAGE={v!r}: expected a float in (0, 1] (the mean cosine similarity between two groups "
                         "down to which they merge)") from None
    return cut, graph_requested()


def _run_average_linkage(eng, emb, request):
    """the graph at the request's threshold, computed again, and its average-linkage tree down to the cut"""
    cut, threshold = request
    g = eng.graph(emb, threshold, NEIGHBOUR_METRIC)
    return eng.average_linkage(g.indptr, g.col, g.sim, g.valid, stop=cut), g.n_edges


AVERAGE_LINKAGE_TSV_HEADER = "seq_name\tcluster\tcluster_size\n"


def write_average_linkage(npz_path, tsv_path, names_key, names, res, request, strand="forward"):
    """Both average-linkage files of a stage: the merges of an AverageLinkageResult with the contig names, the request and the labels
    at the cut, and one line per contig - the name of its cluster's label contig and the cluster's size; a contig without a valid
    embedding has NA and 0."""
    label = res.cut(request[0])
    size = np.where(label >= 0, np.bincount(label[label >= 0], minlength=len(label))[np.maximum(label, 0)], 0).astype(np.int64)
    np.savez_compressed(npz_path, **{names_key: names, "cut": np.float64(request[0]), "threshold": np.float64(request[1]),
                                     "metric": np.array(NEIGHBOUR_METRIC), "a": res.a, "b": res.b, "weight": res.weight, "size_a": res.size_a,
                                     "size_b": res.size_b, "round": res.round, "sim": res.sim, "valid": res.valid, "label": label, "size": size,
                                     "rounds": np.int64(res.rounds), "merged_per_round": res.merged_per_round,
                                     "complete": np.bool_(res.complete), **_strand_entry(strand)})
    with open(tsv_path, "w") as fout:
        fout.write(AVERAGE_LINKAGE_TSV_HEADER)
        for i, name in enumerate(names):
            fout.write(f"{name}\tNA\t0\n" if label[i] < 0 else f"{name}\t{names[label[i]]}\t{size[i]}\n")


def communities_requested():
    """GENOMAD_AMD_COMMUNITIES=<resolution, a multiple of 1/64 in [1/64, 4]>: main() also writes the modularity communities (Louvain's
    levels) of the contigs over the similarity graph of GENOMAD_AMD_GRAPH - a partition that scores itself, 1 being the natural
    resolution (<prefix>_nn_communities.npz and .tsv); unset or empty: nothing changes (None).  It needs GENOMAD_AMD_GRAPH=<threshold>,
    which must be set with it (main() refuses the one without the other).  GENOMAD_AMD_COMMUNITIES_MAX_LEVELS=<integer in [1, 32]>
    (default 32) caps the levels; it is an error without GENOMAD_AMD_COMMUNITIES.  Any other value of either is an error.  Returns
    (resolution, the graph's threshold as it is compared or None, max_levels), or None."""
    v = os.environ.get("GENOMAD_AMD_COMMUNITIES", "").strip()
    if not v:
        _env_refines("GENOMAD_AMD_COMMUNITIES_MAX_LEVELS", "GENOMAD_AMD_COMMUNITIES", "set the resolution of the communities or unset")
        return None
    try:
        resolution = float(v)
        sequence.communities_resolution(resolution)
    except ValueError:
        raise ValueError(f"GENOMAD_AMD_COMMUNITIES={v!r}: expected a multiple of 1/64 in [1/64, 4] (the resolution: the larger, the smaller "
                         "the communities; 1 is modularity itself)") from None
    return resolution, graph_requested(), _env_int("GENOMAD_AMD_COMMUNITIES_MAX_LEVELS", 1, sequence.COMM_LEVELS_MAX,
                                                   "(the levels of the hierarchy at the most)", sequence.COMM_LEVELS_MAX)


def _run_communities(eng, emb, request):
    """the graph at the request's threshold, computed again, and its modularity communities"""
    resolution, threshold, max_levels = request
    g = eng.graph(emb, threshold, NEIGHBOUR_METRIC)
    return eng.communities(g.indptr, g.col, g.sim, g.valid, resolution=resolution, max_levels=max_levels), g.n_edges


COMMUNITIES_TSV_HEADER = "seq_name\tcommunity\tcommunity_size\n"


def write_communities(npz_path, tsv_path, names_key, names, res, request, strand="forward"):
    """Both community files of a stage: every array of a CommunityResult with the contig names and the request (Qnum as the device's
    two words per level), and one line per contig - the name of its community's label contig and the community's size; a contig
    without a valid embedding has NA and 0."""
    np.savez_compressed(npz_path, **{names_key: names, "resolution": np.float64(request[0]), "threshold": np.float64(request[1]),
                                     "max_levels": np.int64(request[2]), "metric": np.array(NEIGHBOUR_METRIC), "label": res.label,
                                     "size": res.size, "level_label": res.level_label, "valid": res.valid,
                                     **{k: getattr(res, k) for k in sequence.COMM_LEVEL_FIELDS}, "qnum_words": res.qnum_words,
                                     "levels": np.int64(res.levels), "complete": np.bool_(res.complete), "m2": np.uint64(res.m2),
                                     "modularity": np.float64(res.modularity), **_strand_entry(strand)})
    with open(tsv_path, "w") as fout:
        fout.write(COMMUNITIES_TSV_HEADER)
        for i, name in enumerate(names):
            fout.write(f"{name}\tNA\t0\n" if res.label[i] < 0 else f"{name}\t{names[res.label[i]]}\t{res.size[i]}\n")


def match_requested():
    """GENOMAD_AMD_MATCH=<float in [-1, 1]>: main() also writes, for every contig, ALL the rows of the reference named by
    GENOMAD_AMD_MATCH_BASE whose encoder embedding has at least that cosine similarity to the contig's per-contig embedding of
    GENOMAD_AMD_EMBEDDINGS=1 (<prefix>_nn_matches.npz and .tsv); unset or empty: nothing changes (None).  Any other value is an error.
    Returns the threshold as it is compared: the float32 it rounds to."""
    return _env_similarity("GENOMAD_AMD_MATCH", "(the cosine similarity at which a contig matches a reference row)")


def match_base_requested():
    """GENOMAD_AMD_MATCH_BASE=<path>: the reference GENOMAD_AMD_MATCH matches against - an .npz as GENOMAD_AMD_EMBEDDINGS=1 writes it
    (:func:`load_match_base`); unset or empty: None."""
    v = os.environ.get("GENOMAD_AMD_MATCH_BASE", "").strip()
    return Path(v) if v else None


def load_match_base(path, strand="forward"):
    """(names, embeddings float32 (n, 512)) of a reference file: ``embeddings`` of shape (n, 512), ONE other 1-D array of n entries -
    the names, under whatever key (contig_names, provirus_names) - and an optional ``strand``, which must be the run's mode (a file
    without it is forward).  ``ValueError`` with the reason for anything else."""
    what = f"GENOMAD_AMD_MATCH_BASE={str(path)!r}"
    if not Path(path).is_file():
        raise ValueError(f"{what}: no such file")
    try:
        z = np.load(path)
        files = list(z.files)
        emb = z["embeddings"] if "embeddings" in files else None
        others = {k: z[k] for k in files if k not in ("embeddings", "strand")}
        base_strand = str(z["strand"]) if "strand" in files else "forward"
    except Exception as e:  # noqa: BLE001  (not an .npz, or one that cannot be read)
        raise ValueError(f"{what}: not a readable .npz ({e})") from None
    if emb is None or emb.ndim != 2 or emb.shape[1] != sequence.NEIGHBOUR_DIM or emb.dtype.kind != "f":
        raise ValueError(f"{what}: it must hold 'embeddings' of shape (n, {sequence.NEIGHBOUR_DIM}) as GENOMAD_AMD_EMBEDDINGS=1 writes them"
                         + ("" if emb is None else f", not {emb.dtype} {emb.shape}"))
    names = [k for k, v in others.items() if v.ndim == 1 and len(v) == len(emb) and v.dtype.kind in "US"]
    if len(names) != 1:
        raise ValueError(f"{what}: it must hold one 1-D array of the {len(emb)} names beside 'embeddings' (found: {sorted(others)})")
    if base_strand != strand:
        raise ValueError(f"{what}: its embeddings were computed under GENOMAD_AMD_STRAND={base_strand}, this run's are under {strand}: "
                         "embeddings of different strand modes are not comparable")
    return others[names[0]], np.ascontiguousarray(emb, dtype=np.float32)


MATCH_TSV_HEADER = "seq_name\treference\tsimilarity\n"


def write_matches_tsv(path, names, base_names, res):
    """One line per match of a MatchResult, in its order (contigs ascending, a contig's reference rows ascending): the contig's name,
    the reference row's name and their similarity, behind one header line."""
    with open(path, "w") as fout:
        fout.write(MATCH_TSV_HEADER)
        for e in res.table(names, base_names):
            fout.write(f"{e['query']}\t{e['base']}\t{e['sim']:.6f}\n")


def write_matches(npz_path, tsv_path, names_key, names, base_names, res, strand="forward"):
    """Both match files of a stage: the arrays of a MatchResult with the names of both sides, and its list of matches."""
    np.savez_compressed(npz_path, **{names_key: names, "base_names": base_names, "threshold": np.float64(res.threshold),
                                     "metric": np.array(res.metric), "indptr": res.indptr, "col": res.col, "sim": res.sim,
                                     **_strand_entry(strand)})
    write_matches_tsv(tsv_path, names, base_names, res)


def vote_requested():
    """GENOMAD_AMD_VOTE=<float in [-1, 1]>: main() also writes, for every contig and every class of the labelled reference named by
    GENOMAD_AMD_VOTE_BASE, how many of the class's rows have at least that cosine similarity to the contig's per-contig embedding of
    GENOMAD_AMD_EMBEDDINGS=1, their similarity sum and the most similar one, and the label they vote for (<prefix>_nn_votes.npz and
    .tsv); unset or empty: nothing changes (None).  Any other value is an error.  Returns the threshold as it is compared: the
    float32 it rounds to."""
    return _env_similarity("GENOMAD_AMD_VOTE", "(the cosine similarity at which a labelled reference row votes on a contig)")


def vote_base_requested():
    """GENOMAD_AMD_VOTE_BASE=<path>: the labelled reference GENOMAD_AMD_VOTE takes its voters from (:func:`load_vote_base`); unset or
    empty: None."""
    v = os.environ.get("GENOMAD_AMD_VOTE_BASE", "").strip()
    return Path(v) if v else None


def vote_min_votes_requested() -> int:
    """GENOMAD_AMD_VOTE_MIN_VOTES=<integer >= 1>: the voters a contig needs within the threshold to get a label; unset or empty: 1.
    Any other value is an error."""
    return _env_int("GENOMAD_AMD_VOTE_MIN_VOTES", 1, None, "(the voters a contig needs to get a label)", 1)


def load_vote_base(path, strand="forward", switch="GENOMAD_AMD_VOTE_BASE"):
    """(names, embeddings float32 (n, 512), classes, label int64 (n,)) of a labelled reference file (``switch``: the variable that
    named it, for the messages): an embeddings file as
    GENOMAD_AMD_EMBEDDINGS=1 writes it - ``embeddings`` of shape (n, 512), ONE 1-D array of the n names under whatever key, an
    optional ``strand``, which must be the run's mode - plus ``labels``, a 1-D array of n strings: "" means unlabelled (label -1), the
    classes are the sorted distinct non-empty strings (at most 1024) and a row's label is its class's place among them.
    ``ValueError`` with the reason for anything else."""
    what = f"{switch}={str(path)!r}"
    if not Path(path).is_file():
        raise ValueError(f"{what}: no such file")
    try:
        z = np.load(path)
        files = list(z.files)
        emb = z["embeddings"] if "embeddings" in files else None
        labels = z["labels"] if "labels" in files else None
        others = {k: z[k] for k in files if k not in ("embeddings", "strand", "labels")}
        base_strand = str(z["strand"]) if "strand" in files else "forward"
    except Exception as e:  # noqa: BLE001  (not an .npz, or one that cannot be read)
        raise ValueError(f"{what}: not a readable .npz ({e})") from None
    if emb is None or emb.ndim != 2 or emb.shape[1] != sequence.NEIGHBOUR_DIM or emb.dtype.kind != "f":
        raise ValueError(f"{what}: it must hold 'embeddings' of shape (n, {sequence.NEIGHBOUR_DIM}) as GENOMAD_AMD_EMBEDDINGS=1 writes them"
                         + ("" if emb is None else f", not {emb.dtype} {emb.shape}"))
    if labels is None or labels.ndim != 1 or len(labels) != len(emb) or labels.dtype.kind not in "US":
        raise ValueError(f"{what}: it must hold 'labels', a 1-D array of the {len(emb)} class names (\"\" for an unlabelled row)"
                         + ("" if labels is None else f", not {labels.dtype} {labels.shape}"))
    names = [k for k, v in others.items() if v.ndim == 1 and len(v) == len(emb) and v.dtype.kind in "US"]
    if len(names) != 1:
        raise ValueError(f"{what}: it must hold one 1-D array of the {len(emb)} names beside 'embeddings' and 'labels' (found: {sorted(others)})")
    if base_strand != strand:
        raise ValueError(f"{what}: its embeddings were computed under GENOMAD_AMD_STRAND={base_strand}, this run's are under {strand}: "
                         "embeddings of different strand modes are not comparable")
    labels = labels.astype(str)
    classes = np.array(sorted(set(labels.tolist()) - {""}), dtype=str)
    if not len(classes):
        raise ValueError(f"{what}: no row has a label: every entry of 'labels' is \"\"")
    if len(classes) > sequence.VOTE_CLASSES_MAX:
        raise ValueError(f"{what}: 'labels' names {len(classes)} classes, more than {sequence.VOTE_CLASSES_MAX}")
    label = np.where(labels == "", -1, np.searchsorted(classes, labels)).astype(np.int64)
    return others[names[0]], np.ascontiguousarray(emb, dtype=np.float32), classes, label


VOTE_TSV_HEADER = "seq_name\tlabel\tconfidence\tvotes\ttotal_votes\tnearest\tsimilarity\n"
VOTE_RULE = "weight"                    # the rule of the labels main() writes


def write_votes_tsv(path, names, classes, base_names, res, min_votes=1):
    """One line per contig of a VoteResult: its name, the class its voters' similarity sum is largest for, that class's share of the
    sum, its voters, the voters of all classes, the most similar voter of the winning class and its similarity, behind one header
    line; NA where the contig has no label (and for a share that is not defined)."""
    with open(path, "w") as fout:
        fout.write(VOTE_TSV_HEADER)
        for e in res.table(names, classes, base_names, VOTE_RULE, min_votes):
            if e["label"] is None:
                fout.write(f"{e['query']}\tNA\tNA\t0\t{e['total_votes']}\tNA\tNA\n")
            else:
                conf = "NA" if e["confidence"] is None else f"{e['confidence']:.6f}"
                fout.write(f"{e['query']}\t{e['label']}\t{conf}\t{e['votes']}\t{e['total_votes']}\t{e['nearest']}\t{e['similarity']:.6f}\n")


def write_votes(npz_path, tsv_path, names_key, names, classes, base_names, base_label, res, min_votes=1, strand="forward"):
    """Both vote files of a stage: the arrays of a VoteResult with the names of the contigs, the classes and the reference rows (and
    the rows' labels), the labels of rule ``weight``, and one line per contig."""
    label, confidence, margin = res.predict(VOTE_RULE, min_votes)
    np.savez_compressed(npz_path, **{names_key: names, "base_names": base_names, "base_label": np.asarray(base_label, dtype=np.int64),
                                     "classes": classes, "threshold": np.float64(res.threshold),
                                     "min_votes": np.int64(min_votes), "count": res.count, "weight": res.weight, "nearest": res.nearest,
                                     "nearest_sim": res.nearest_sim, "label": label, "confidence": confidence, "margin": margin,
                                     **_strand_entry(strand)})
    write_votes_tsv(tsv_path, names, classes, base_names, res, min_votes)


SPREAD_MAX_ITER_DEFAULT = 200
SPREAD_SCORE_CLASSES = 64               # the score matrix is written for up to this many classes


def spread_requested():
    """GENOMAD_AMD_SPREAD=<alpha, a multiple of 1/64 in (0, 1)>: main() also spreads the labels of the reference named by
    GENOMAD_AMD_SPREAD_BASE (a labelled embeddings file, the format of GENOMAD_AMD_VOTE_BASE) along the similarity graph of the
    reference's rows and the contigs' per-contig embeddings at the threshold of GENOMAD_AMD_GRAPH, which must be set with it - a contig
    gets a label through any number of unlabelled contigs, where GENOMAD_AMD_VOTE crosses one edge (<prefix>_nn_spread.npz and .tsv);
    unset or empty: nothing changes (None).  GENOMAD_AMD_SPREAD_MAX_ITER=<integer in [1, 10000]> (default 200) bounds the iterations;
    it is an error without GENOMAD_AMD_SPREAD.  Any other value of either is an error.  Returns (alpha, the graph's threshold as it is
    compared or None, max_iter), or None."""
    v = os.environ.get("GENOMAD_AMD_SPREAD", "").strip()
    if not v:
        _env_refines("GENOMAD_AMD_SPREAD_MAX_ITER", "GENOMAD_AMD_SPREAD", "set the alpha of the label spreading or unset")
        return None
    try:
        alpha = float(v)
        sequence.spread_alpha(alpha)
    except ValueError:
        raise ValueError(f"GENOMAD_AMD_SPREAD={v!r}: expected a multiple of 1/64 in (0, 1) (alpha: the share of its score a contig takes "
                         "from its neighbours)") from None
    return alpha, graph_requested(), _env_int("GENOMAD_AMD_SPREAD_MAX_ITER", 1, sequence.SPREAD_MAX_ITER_MAX,
                                              "(the iterations the label spreading runs at the most)", SPREAD_MAX_ITER_DEFAULT)


def spread_base_requested():
    """GENOMAD_AMD_SPREAD_BASE=<path>: the labelled reference GENOMAD_AMD_SPREAD takes its seeds from (:func:`load_vote_base`); unset
    or empty: None."""
    v = os.environ.get("GENOMAD_AMD_SPREAD_BASE", "").strip()
    return Path(v) if v else None


def _run_spread(eng, emb, request, base):
    """the graph over [the reference's rows; the contigs' rows] at the request's threshold, and the reference's labels spread along it
    as clamped seeds: (the SpreadResult of all rows, the graph's edges, the reference's rows)"""
    alpha, threshold, max_iter = request
    _, base_emb, classes, base_label = base
    g = eng.graph(np.concatenate([base_emb, np.asarray(emb, dtype=np.float32)]), threshold, NEIGHBOUR_METRIC)
    label = np.concatenate([np.asarray(base_label, dtype=np.int64), np.full(len(emb), -1, dtype=np.int64)])
    res = eng.spread(g.indptr, g.col, g.sim, label, len(classes), valid=g.valid, alpha=alpha, clamp=True, max_iter=max_iter,
                     scores=len(classes) <= SPREAD_SCORE_CLASSES)
    return res, g.n_edges, len(base_emb)


SPREAD_TSV_HEADER = "seq_name\tlabel\tconfidence\tscore\ttotal_score\tfirst\n"


def write_spread_tsv(path, names, classes, arrays):
    """One line per contig of the contigs' part of a SpreadResult: its name, the class with the largest score, that score's share of
    the contig's total, the score, the total and the first iteration that brought the contig any score, behind one header line; NA
    where the contig has no label."""
    with open(path, "w") as fout:
        fout.write(SPREAD_TSV_HEADER)
        for e in sequence.spread_table(*(arrays[k] for k in sequence.SPREAD_FIELDS[1:]), names, classes):
            if e["label"] is None:
                fout.write(f"{e['row']}\tNA\tNA\tNA\t{e['total_score']:.6f}\tNA\n")
            else:
                fout.write(f"{e['row']}\t{e['label']}\t{e['confidence']:.6f}\t{e['score']:.6f}\t{e['total_score']:.6f}\t{e['first']}\n")


def write_spread(npz_path, tsv_path, names_key, names, base, res, request, strand="forward"):
    """Both label-spreading files of a stage: the contigs' part of the arrays of a SpreadResult (the reference's rows come first in
    it) with the names of the contigs, the classes and the reference rows (and the rows' labels), the request, the labels, and one
    line per contig."""
    res, n_edges, nb = res
    base_names, _, classes, base_label = base
    arrays = {k: getattr(res, k)[nb:] for k in sequence.SPREAD_FIELDS[1:]}
    label, confidence, margin = sequence.spread_predict(*(arrays[k] for k in sequence.SPREAD_FIELDS[1:5]))
    score = {"score": res.score[nb:]} if res.score is not None else {}
    np.savez_compressed(npz_path, **{names_key: names, "base_names": base_names, "base_label": np.asarray(base_label, dtype=np.int64),
                                     "classes": classes, "alpha": np.float64(request[0]), "threshold": np.float64(request[1]),
                                     "max_iter": np.int64(request[2]), "metric": np.array(NEIGHBOUR_METRIC), **arrays, **score,
                                     "label": label, "confidence": confidence, "margin": margin, "iterations": np.int64(res.iterations),
                                     "converged": np.bool_(res.converged), "changed": res.changed, "n_edges": np.int64(n_edges),
                                     **_strand_entry(strand)})
    write_spread_tsv(tsv_path, names, classes, arrays)


REGION_TSV_HEADER = ("seq_name\tstart\tend\tclass\tn_bins\tevidence_bins\t"
                     + "\t".join("mean_" + c[:-len("_score")] for c in TSV_HEADER.split()[1:]) + "\tmargin\n")


def write_regions_tsv(path, names, res):
    """One line per region of a RegionResult with its table: coordinates 0-based half-open, floats '%.4f', the class names those of
    the classification TSV's header."""
    classes = [c[:-len("_score")] for c in TSV_HEADER.split()[1:]]
    with open(path, "w") as fout:
        fout.write(REGION_TSV_HEADER)
        for i in range(len(res.region_contig)):
            mean = "\t".join(f"{x:.4f}" for x in res.mean[i])
            fout.write(f"{names[res.region_contig[i]]}\t{res.start[i]}\t{res.end[i]}\t{classes[res.region_state[i]]}\t"
                       f"{res.region_hi[i] - res.region_lo[i]}\t{res.region_evidence[i]}\t{mean}\t{res.margin[i]:.4f}\n")


def strand_contigs_safely(eng, seq, offsets, strand, single_window, precision, embed=False, console=None):
    """NNEngine.classify_contigs_strand, asking for each strand's own scores, with the range fallback of :func:`_range_fallback`:
    a non-finite score on EITHER strand sends the piece to the next arithmetic.  (scores, embeddings or None, ids, forward, reverse)."""
    def run(a):
        pr, wid, emb, fwd, rev = eng.classify_contigs_strand(seq, offsets, strand, single_window, a, embed)
        return np.stack([pr, fwd, rev]), (pr, emb, wid, fwd, rev)
    _, out, _ = _with_range_fallback(run, precision, console)
    return out


def scan_contigs_strand_safely(eng, seq, offsets, stride, strand, single_window, precision, console=None):
    """NNEngine.scan_contigs_strand with the range fallback: a non-finite window score on either strand scans the piece again."""
    def run(a):
        res = eng.scan_contigs_strand(seq, offsets, stride, strand, single_window, a)
        return np.stack([res.scores, res.scores_fwd, res.scores_rev]), res
    _, res, _ = _with_range_fallback(run, precision, console)
    return res


def strand_requested() -> str:
    """GENOMAD_AMD_STRAND=forward|reverse|both: which strand of every window main() scores (``both``: the f32 mean of the two);
    unset, empty or ``forward``: nothing changes.  Any other value is an error."""
    v = os.environ.get("GENOMAD_AMD_STRAND", "").strip()
    if not v:
        return "forward"
    if v not in sequence.STRANDS:
        raise ValueError(f"GENOMAD_AMD_STRAND={v!r}: expected one of forward, reverse, both (the strand of every window that is scored)")
    return v


def _strand_of_file(path) -> str:
    """The mode a stage's outputs were computed under: what its strand file says; no file = forward."""
    if not Path(path).exists():
        return "forward"
    try:
        return str(np.load(path)["strand"])
    except Exception:  # noqa: BLE001  (unreadable: no mode matches, the stage runs again)
        return "?"


def _npz_strand(path) -> str:
    """The mode an embeddings or scan file was computed under: its ``strand`` entry, which only reverse / both write."""
    try:
        z = np.load(path)
        return str(z["strand"]) if "strand" in z.files else "forward"
    except Exception:  # noqa: BLE001  (missing or unreadable: no mode matches)
        return "?"


# ---- runtime parity sentinel ---------------------------------------------------------------------
# The 1e-4 claim of the production arithmetic has only ever met synthetic weights (the trained nn_classifier.h5 is not in the
# checkout).  So every run of main() classifies its first windows a second time with the exact-f32 device path (GNN_PREC_F32:
# unfused f32 FMA kernels, the parity anchor of tests/ and bench.py) and compares: the only parity evidence a user with the real
# weights ever gets, and what turns the range / precision assumptions of the f16 limb arithmetic (activations neither beyond
# ~2 000 nor so small that the low limbs go subnormal) into checked ones.  Cost: one 64-window launch of the f32 path, 6 ms
# including its 0.6 GB activation workspace (tests/test_gpu_parity.py::test_parity_sentinel_... prints it).  GENOMAD_AMD_NO_SENTINEL=1 opts out.
SENTINEL_WINDOWS = 64
SENTINEL_TOL = 1e-4            # BASELINE.json north_star: per-class scores within 1e-4 absolute of the reference path


def sentinel_windows(seq, offsets, single_window, limit=SENTINEL_WINDOWS) -> np.ndarray:
    """The first ``limit`` candidate windows of a packed contig buffer as (k, 6000) upper-cased, N-padded bytes
    (nn_classification.py:68-72; the N-content rule is irrelevant for a parity sample)."""
    starts, lens, _, _ = sequence.candidate_spans(np.asarray(offsets, np.int64), single_window)
    k = int(min(len(starts), limit))
    win = np.full((k, sequence.WINDOW), ord("N"), dtype=np.uint8)
    for i in range(k):
        w = np.asarray(seq[int(starts[i]):int(starts[i]) + int(lens[i])], dtype=np.uint8)
        win[i, :len(w)] = np.where((w >= 97) & (w <= 122), w - 32, w)          # sequence.py:35-36 upper()
    return win


def parity_sentinel(eng, windows, precision, console=None):
    """max |dscore| of the production arithmetic (after its range fallbacks) against GNN_PREC_F32 on ``windows``;
    None when switched off, for the exact arithmetic itself, or without windows.  Logs one line."""
    if os.environ.get("GENOMAD_AMD_NO_SENTINEL") == "1" or precision == "f32" or not len(windows):
        return None
    from ._lib import GnnError
    log = console.log if console is not None else print
    exact = None
    for k in (len(windows), 16, 4):          # the exact path keeps 3 x 3 MB of f32 activations per window: on a short device try fewer
        try:
            exact = eng.classify(windows[:k], "f32")
            windows = windows[:k]
            break
        except GnnError as exc:              # the production arithmetic may well fit where the exact one does not (shared / partitioned GPUs)
            if "hipMalloc" not in str(exc) and "memory" not in str(exc).lower():
                raise
    if exact is None:
        log("Parity sentinel skipped: no device memory for the exact-f32 path (4 windows need 37 MB of activations).")
        return None
    got, _, used = _with_range_fallback(lambda a: (eng.classify(windows, a), None), precision, console)
    d = float(np.abs(got.astype(np.float64) - exact).max()) if np.isfinite(got).all() and np.isfinite(exact).all() else float("inf")
    log(f"Parity sentinel: max |dscore| of {used} against the exact-f32 path on the first {len(windows)} windows = {d:.2e} "
        f"(tolerance {SENTINEL_TOL:.0e}).")
    return d


def sentinel_verdict(comm, d, console, precision):
    """Every rank brings its own sentinel result (None = nothing to check); all ranks leave together if any failed."""
    bad = d is not None and not d <= SENTINEL_TOL
    if comm is not None:
        bad = bool(np.asarray(comm.allgather_i64([int(bad)]))[:, 0].any())
    if bad:
        console.error(
            f"Parity sentinel FAILED: the {precision} arithmetic differs from the exact-f32 device path by more than {SENTINEL_TOL:.0e} "
            "on this run's first windows (weights whose activations leave the range the f16 limb arithmetic was validated for). "
            "Re-run with GENOMAD_AMD_PRECISION=bf16x3 (f32 range) or GENOMAD_AMD_PRECISION=f32 (exact, slow); "
            "GENOMAD_AMD_NO_SENTINEL=1 disables this check.")
        sys.exit(1)


class GpuBackend:
    """Scores windows and averages them per contig on the GPU (libgenomad_nn_hip.so)."""

    def __init__(self, batch_size: int, console=None):
        self.eng = _engine()
        self.chunk = max(int(batch_size), 4096)
        self.precision = configured_precision()
        if (self.precision == "f16x3tc" and getattr(self.eng, "has_kmer_tables", lambda: False)()
                and os.environ.get("GENOMAD_AMD_KMER_TABLES", "auto") != "0"):
            self.precision = "f16x3tk"          # an engine that already holds the tables (a long-lived process) uses them
        self.console = console
        self.sentinel = None          # max |dscore| of the first windows this backend scored (parity_sentinel)
        self._sentinel_done = False

    def score(self, windows: np.ndarray) -> np.ndarray:
        if not self._sentinel_done:
            self._sentinel_done = True
            self.sentinel = parity_sentinel(self.eng, windows[:SENTINEL_WINDOWS], self.precision, self.console)
        out = []
        for a in range(0, len(windows), self.chunk):
            s, _, _ = _with_range_fallback(lambda p, a=a: (self.eng.classify(windows[a:a + self.chunk], p), None),
                                           self.precision, self.console)
            out.append(s)
        return np.concatenate(out) if out else np.zeros((0, 3), np.float32)

    def segment_mean(self, scores, ids, n_segments) -> np.ndarray:
        return self.eng.segment_mean(scores, ids, n_segments)


def classify_windows(windows: np.ndarray, contig_ids: np.ndarray, n_contigs: int, backend, comm=None):
    """Window scores -> per-contig mean (nn_classification.py:316-320), sharded over the ranks of ``comm``
    (rank 0 gets the result, other ranks None)."""
    from . import sharding
    scores = sharding.classify_sharded(windows, backend.score, comm)
    if scores is None:
        return None
    return backend.segment_mean(scores, contig_ids, n_contigs)


def _encode(fasta_path, enc_dir: Path, window_id_path: Path, single_window: bool, names_key: str, ids_key: str):
    names, ids, windows = sequence.encode_fasta(fasta_path, single_window)
    np.save(enc_dir / f"{len(windows)}.win.npy", windows)
    np.savez_compressed(window_id_path, **{names_key: names, ids_key: ids})
    return names, ids, windows


# ---- the analyses of the gathered per-contig embeddings ------------------------------------------------------------------------------
# Seventeen analyses (ANALYSES_RUN) follow one rule in main() (the docstring of its stage_device); a record of ANALYSES holds what differs between them:
#   name      the stem of its files, <prefix>_nn_<name>.npz and - where ``tsv`` - .tsv
#   switch    the environment variable that requests it; ``request()`` reads it (and its companions): the request, or None
#   needs     the middle clause of the message that refuses the switch without GENOMAD_AMD_EMBEDDINGS=1
#   keys      the npz entries that spell the request, with their casts (:func:`_request_of_file`)
#   title     the head of its log line, before " (<summary>) written to ..."; {what} is "sequence" or "provirus", {base} the reference file
#   run(eng, embeddings, request, ctx) -> the result; ``ctx`` holds what only some need: what, names, ids (the gathered window ids),
#             request, base (what the reference's loader returned) and base_path
#   write(npz, tsv, names_key, names, res, strand, ctx) and summary(res, request, what, ctx): its files and its log line's middle
#   errors    the exceptions of ``run`` that end the run with status 1 and one line, "<switch>=<request>: <error>. <advice>"
#   base      for an analysis against a reference (AnalysisBase): ``request()`` its path, ``load(path, strand)``, the ``hint`` of the
#             message about a file that cannot be loaded, and ``same(npz, base)``: the file was computed against this very reference
#   after     the name of the analysis whose switch it needs as well (its request then holds that one's too), or None
Analysis = namedtuple("Analysis", "name switch request needs keys title run write summary tsv errors advice base after",
                      defaults=(True, (), "", None, None))
AnalysisBase = namedtuple("AnalysisBase", "request load hint same")
_SIMILARITY = f"{NEIGHBOUR_METRIC} similarity of the encoder embeddings"


def _kept_windows(ctx):
    """the representatives' weight: every contig's number of kept windows, counted in the gathered window ids (no further collective)"""
    return np.bincount(np.asarray(ctx.ids, dtype=np.int64), minlength=len(ctx.names)).astype(np.int64)


def _vote_request():
    t, m = vote_requested(), vote_min_votes_requested()          # a bad GENOMAD_AMD_VOTE_MIN_VOTES is an error with or without the threshold
    return None if t is None else (t, m)


def _same_vote_base(z, base) -> bool:
    """the reference's names, classes and labels are those the vote file was computed against"""
    return all(np.array_equal(z[k], base[i]) for k, i in (("base_names", 0), ("classes", 2), ("base_label", 3)))


ANALYSES = (        # in the order they run, which is the order of the log lines and of what is on disk when one of them ends the run
    Analysis("neighbours", "GENOMAD_AMD_NEIGHBOURS", neighbours_requested,
             "neighbours are searched among the per-contig encoder embeddings", (("k", int),), "Nearest neighbours of the {what}s",
             lambda eng, emb, k, ctx: eng.neighbours(emb, None, k, NEIGHBOUR_METRIC),          # the self-search: a contig is not its own neighbour
             lambda npz, tsv, key, names, res, strand, ctx: write_neighbours(npz, key, names, res, ctx.request, strand),
             lambda res, k, what, ctx: f"{k} per {what}, {_SIMILARITY}", tsv=False),
    Analysis("clusters", "GENOMAD_AMD_CLUSTERS", clusters_requested,
             "clusters are formed among the per-contig encoder embeddings", (("threshold", float),), "Clusters of the {what}s",
             lambda eng, emb, t, ctx: eng.cluster(emb, t, NEIGHBOUR_METRIC),
             lambda npz, tsv, key, names, res, strand, ctx: write_clusters(npz, tsv, key, names, res, ctx.request, strand),
             lambda res, t, what, ctx: f"{_SIMILARITY} >= {t:g}, single linkage: {res.n_clusters} clusters, {res.n_edges} edges"),
    Analysis("representatives", "GENOMAD_AMD_REPRESENTATIVES", representatives_requested,
             "representatives are chosen among the per-contig encoder embeddings", (("threshold", float),), "Representatives of the {what}s",
             lambda eng, emb, t, ctx: eng.representatives(emb, t, _kept_windows(ctx), NEIGHBOUR_METRIC),      # ties in FASTA order
             lambda npz, tsv, key, names, res, strand, ctx: write_representatives(npz, tsv, key, names, res, ctx.request, _kept_windows(ctx),
                                                                                  strand),
             lambda res, t, what, ctx: f"{_SIMILARITY} >= {t:g}, greedy by kept windows: {res.n_clusters} clusters in {res.rounds} rounds"),
    Analysis("linkage", "GENOMAD_AMD_LINKAGE", lambda: () if linkage_requested() else None,      # its request is its files' existence
             "the tree is built among the per-contig encoder embeddings", (), "Single-linkage tree of the {what}s",
             lambda eng, emb, _, ctx: eng.linkage(emb, NEIGHBOUR_METRIC),
             lambda npz, tsv, key, names, res, strand, ctx: write_linkage(npz, tsv, key, names, res, strand),
             lambda res, _, what, ctx: f"{_SIMILARITY}: {res.n_edges} merges among {res.n_valid} {what}s in {res.rounds} rounds"),
    Analysis("graph", "GENOMAD_AMD_GRAPH", graph_requested,
             "the graph's edges are found among the per-contig encoder embeddings", (("threshold", float),), "Similarity graph of the {what}s",
             lambda eng, emb, t, ctx: eng.graph(emb, t, NEIGHBOUR_METRIC),
             lambda npz, tsv, key, names, res, strand, ctx: write_graph(npz, tsv, key, names, res, strand),
             lambda res, t, what, ctx: f"{_SIMILARITY} >= {t:g}: {res.n_edges} edges among {int(res.valid.sum())} {what}s",
             errors=ValueError, advice="Raise GENOMAD_AMD_GRAPH or unset it."),      # more edges than NNEngine.graph's cap: none was allocated
    Analysis("mcl", "GENOMAD_AMD_MCL", mcl_requested,
             "the flow runs on the similarity graph of the per-contig encoder embeddings", (("inflation", float), ("threshold", float), ("select", int)),
             "Markov clusters of the {what}s",
             lambda eng, emb, r, ctx: _run_mcl(eng, emb, r),
             lambda npz, tsv, key, names, res, strand, ctx: write_mcl(npz, tsv, key, names, res[0], ctx.request, strand),
             lambda res, r, what, ctx: (f"{_SIMILARITY} >= {r[1]:g}, {res[1]} edges, inflation {r[0]:g}, at most {r[2]} entries per column: "
                                        f"{res[0].n_clusters} clusters in {res[0].iterations} iterations, "
                                        f"{'converged' if res[0].converged else 'not converged'}"),
             errors=(ValueError, GnnError), advice="Raise GENOMAD_AMD_GRAPH or unset GENOMAD_AMD_MCL.", after="graph"),      # the graph's cap on its edges
    Analysis("average_linkage", "GENOMAD_AMD_AVERAGE_LINKAGE", average_linkage_requested,
             "the groups merge by their mean similarity over the similarity graph of the per-contig encoder embeddings",
             (("cut", float), ("threshold", float)), "Average-linkage clusters of the {what}s",
             lambda eng, emb, r, ctx: _run_average_linkage(eng, emb, r),
             lambda npz, tsv, key, names, res, strand, ctx: write_average_linkage(npz, tsv, key, names, res[0], ctx.request, strand),
             lambda res, r, what, ctx: (f"{_SIMILARITY} >= {r[1]:g}, {res[1]} edges, mean similarity >= {r[0]:g}, a pair without an edge "
                                        f"counting as 0: {int(res[0].valid.sum()) - len(res[0].a)} clusters, {len(res[0].a)} merges in "
                                        f"{res[0].rounds} rounds"),
             errors=(ValueError, GnnError), advice="Raise GENOMAD_AMD_GRAPH or unset GENOMAD_AMD_AVERAGE_LINKAGE.", after="graph"),
    Analysis("density", "GENOMAD_AMD_DENSITY", density_requested,
             "density clusters are formed among the per-contig encoder embeddings", (("threshold", float), ("min_points", int)),
             "Density clusters of the {what}s",
             lambda eng, emb, r, ctx: eng.density(emb, r[0], r[1], NEIGHBOUR_METRIC),
             lambda npz, tsv, key, names, res, strand, ctx: write_density(npz, tsv, key, names, res, strand),
             lambda res, r, what, ctx: (f"{_SIMILARITY} >= {r[0]:g}, at least {r[1]} {what}s for a core: {res.n_clusters} clusters, "
                                        f"{res.n_core} core, {res.n_border} border, {res.n_noise} noise")),
    Analysis("hdbscan", "GENOMAD_AMD_HDBSCAN", hdbscan_requested,
             "the density-aware tree is built among the per-contig encoder embeddings", (("min_cluster_size", int), ("min_points", int)),
             "HDBSCAN clusters of the {what}s",
             lambda eng, emb, r, ctx: _run_hdbscan(eng, emb, r),
             lambda npz, tsv, key, names, res, strand, ctx: write_hdbscan(npz, tsv, key, names, res, ctx.request[0], strand),
             lambda res, r, what, ctx: (f"{_SIMILARITY}, at least {r[0]} {what}s per cluster, core similarity over {r[1]}: "
                                        f"{int(res[1]['selected'].sum())} clusters, {int((res[1]['label'] < 0).sum() - (res[0].n - res[0].n_valid))} "
                                        f"noise, tree in {res[0].rounds} rounds")),
    Analysis("kmeans", "GENOMAD_AMD_KMEANS", kmeans_requested,
             "the groups are formed among the per-contig encoder embeddings", (("k", int), ("max_iter", int)), "Spherical k-means of the {what}s",
             lambda eng, emb, r, ctx: eng.kmeans(emb, r[0], None, r[1]),                       # farthest-first init
             lambda npz, tsv, key, names, res, strand, ctx: write_kmeans(npz, tsv, key, names, res, ctx.request[1], strand),
             lambda res, r, what, ctx: (f"{_SIMILARITY}: {r[0]} groups, {res.iterations} updates, "
                                        f"{'converged' if res.converged else 'not converged'}, objective {res.objective:.3f}"),
             errors=(ValueError, GnnError), advice="Lower GENOMAD_AMD_KMEANS or unset it."),   # more groups than contigs with a valid embedding
    Analysis("pca", "GENOMAD_AMD_PCA", pca_requested,
             "the components are those of the per-contig encoder embeddings", (("n_components", int),), "Principal components of the {what}s",
             lambda eng, emb, c, ctx: eng.pca(emb, c),
             lambda npz, tsv, key, names, res, strand, ctx: write_pca(npz, tsv, key, names, res, strand),
             lambda res, c, what, ctx: (f"unit encoder embeddings: {c} components of {res.n_valid} {what}s, "
                                        f"{float(np.nansum(res.explained_variance_ratio)):.3f} of the variance"),
             errors=(ValueError, GnnError), advice="Unset GENOMAD_AMD_PCA."),                  # fewer than two contigs with a valid embedding
    Analysis("matches", "GENOMAD_AMD_MATCH", match_requested,
             "the per-contig encoder embeddings are matched against the reference's at that threshold", (("threshold", float),),
             "Matches of the {what}s against {base}",
             lambda eng, emb, t, ctx: eng.match(emb, ctx.base[1], t, NEIGHBOUR_METRIC),        # query: the contigs; base: the reference
             lambda npz, tsv, key, names, res, strand, ctx: write_matches(npz, tsv, key, names, ctx.base[0], res, strand),
             lambda res, t, what, ctx: (f"{_SIMILARITY} >= {t:g}: {res.n_edges} matches of {int((res.hits() > 0).sum())} {what}s among "
                                        f"{res.n_base} reference rows"),
             errors=ValueError, advice="Raise GENOMAD_AMD_MATCH or unset it.",                 # more matches than NNEngine.match's cap
             base=AnalysisBase(match_base_requested, load_match_base, "", lambda z, base: np.array_equal(z["base_names"], base[0]))),
    Analysis("votes", "GENOMAD_AMD_VOTE", _vote_request,
             "the labelled reference's embeddings vote on the per-contig encoder embeddings at that threshold",
             (("threshold", float), ("min_votes", int)), "Votes of {base} on the {what}s",
             lambda eng, emb, r, ctx: eng.vote(emb, ctx.base[1], ctx.base[3], len(ctx.base[2]), r[0]),
             lambda npz, tsv, key, names, res, strand, ctx: write_votes(npz, tsv, key, names, ctx.base[2], ctx.base[0], ctx.base[3], res,
                                                                        ctx.request[1], strand),
             lambda res, r, what, ctx: (f"{_SIMILARITY} >= {r[0]:g}, {len(ctx.base[2])} classes: "
                                        f"{int((res.predict(VOTE_RULE, r[1])[0] >= 0).sum())} of {len(ctx.names)} {what}s got a label"),
             base=AnalysisBase(vote_base_requested, load_vote_base, ", with 'labels' added", _same_vote_base)),
    Analysis("spread", "GENOMAD_AMD_SPREAD", spread_requested,
             "the labelled reference's labels spread along the similarity graph of its embeddings and the per-contig encoder embeddings",
             (("alpha", float), ("threshold", float), ("max_iter", int)), "Labels of {base} spread to the {what}s",
             lambda eng, emb, r, ctx: _run_spread(eng, emb, r, ctx.base),
             lambda npz, tsv, key, names, res, strand, ctx: write_spread(npz, tsv, key, names, ctx.base, res, ctx.request, strand),
             lambda res, r, what, ctx: (f"{_SIMILARITY} >= {r[1]:g}, {res[1]} edges among {res[2]} reference rows and {len(ctx.names)} {what}s, "
                                        f"alpha {r[0]:g}, {len(ctx.base[2])} classes: {int((res[0].best[res[2]:] >= 0).sum())} of "
                                        f"{len(ctx.names)} {what}s got a label in {res[0].iterations} iterations, "
                                        f"{'converged' if res[0].converged else 'not converged'}"),
             errors=(ValueError, GnnError), advice="Raise GENOMAD_AMD_GRAPH or unset GENOMAD_AMD_SPREAD.",      # the graph's cap on its edges
             base=AnalysisBase(spread_base_requested, functools.partial(load_vote_base, switch="GENOMAD_AMD_SPREAD_BASE"),
                               ", with 'labels' added", _same_vote_base), after="graph"),
)

# The fifteenth analysis.  It stands in a table of its own behind ANALYSES, so that table stays what the earlier analyses' tests
# count; main() walks ANALYSES_RUN (below), and everything said of a record above holds for these.
MORE_ANALYSES = (
    Analysis("communities", "GENOMAD_AMD_COMMUNITIES", communities_requested,
             "modularity is optimised over the similarity graph of the per-contig encoder embeddings",
             (("resolution", float), ("threshold", float), ("max_levels", int)), "Modularity communities of the {what}s",
             lambda eng, emb, r, ctx: _run_communities(eng, emb, r),
             lambda npz, tsv, key, names, res, strand, ctx: write_communities(npz, tsv, key, names, res[0], ctx.request, strand),
             lambda res, r, what, ctx: (f"{_SIMILARITY} >= {r[1]:g}, {res[1]} edges, resolution {r[0]:g}: {res[0].n_communities} communities, "
                                        f"modularity {res[0].modularity:.4f}, {res[0].levels} levels, "
                                        f"{'complete' if res[0].complete else 'not complete'}"),
             errors=(ValueError, GnnError), advice="Raise GENOMAD_AMD_GRAPH or unset GENOMAD_AMD_COMMUNITIES.", after="graph"),
)
ALL_ANALYSES = ANALYSES + MORE_ANALYSES

# The sixteenth analysis, in a third table for the same reason: ALL_ANALYSES stays what the communities' tests count.  main() and the
# file table of Outputs walk ANALYSES_RUN (below), and everything said of a record above holds for this one.
KNN_ANALYSES = (
    Analysis("knn_graph", "GENOMAD_AMD_KNN_GRAPH", knn_graph_requested,
             "the neighbour lists are those of the per-contig encoder embeddings", (("k", int), ("mode", str), ("weight", str)),
             "k-nearest-neighbour graph of the {what}s",
             lambda eng, emb, r, ctx: eng.knn_graph(emb, r[0], r[1], r[2], NEIGHBOUR_METRIC),
             lambda npz, tsv, key, names, res, strand, ctx: write_knn_graph(npz, tsv, key, names, res, strand),
             lambda res, r, what, ctx: (f"{r[0]} neighbours per {what}, {_SIMILARITY}, {r[1]}, weighted by {r[2]}: {res.n_edges} edges among "
                                        f"{int(res.valid.sum())} {what}s, {int(np.asarray(res.mutual).sum())} of them mutual")),
)
EVERY_ANALYSIS = ALL_ANALYSES + KNN_ANALYSES

# The seventeenth analysis and the first consumer of the k-nearest-neighbour graph, in a fourth table for the same reason:
# EVERY_ANALYSIS stays what the graph's tests count.  main() and the file table of Outputs walk ANALYSES_RUN, and everything said of a
# record above holds for this one.
TSNE_ANALYSES = (
    Analysis("tsne", "GENOMAD_AMD_TSNE", tsne_requested,
             "the layout is that of the k-nearest-neighbour graph of the per-contig encoder embeddings",
             (("n_iter", int), ("k", int), ("mode", str), ("weight", str)), "t-SNE layout of the {what}s",
             lambda eng, emb, r, ctx: eng.tsne_rows(emb, r[1], r[2], r[3], n_iter=r[0]),      # the graph computed again, the init by PCA
             lambda npz, tsv, key, names, res, strand, ctx: write_tsne(npz, tsv, key, names, res, ctx.request, strand),
             lambda res, r, what, ctx: (f"{r[0]} iterations over the {r[1]}-nearest-neighbour graph, {r[2]}, weighted by {r[3]}, from the first "
                                        f"two principal components: {int(np.asarray(res.valid).sum())} {what}s placed, "
                                        f"Kullback-Leibler divergence {res.kl_divergence:.4f}"),
             errors=(ValueError, GnnError), advice="Unset GENOMAD_AMD_TSNE.", after="knn_graph"),      # fewer than two valid embeddings; more than 2^21 contigs
)
ANALYSES_RUN = EVERY_ANALYSIS + TSNE_ANALYSES


def _resumes(a, npz, tsv, request, strand, base) -> bool:
    """Analysis ``a``'s files of a stage are what a run with ``request`` would write: the npz spells the request (no file: none), the tsv
    is there iff there is a request, and a requested file was computed under this strand mode and against this reference."""
    if _request_of_file(npz, a.keys) != request or (tsv is not None and tsv.exists() != (request is not None)):
        return False
    if request is None:
        return True
    try:
        return _npz_strand(npz) == strand and (a.base is None or bool(a.base.same(np.load(npz), base)))
    except Exception:  # noqa: BLE001  (the entries of the reference are not there: the stage runs again)
        return False


def main(input_path, output_path, single_window, batch_size, restart, threads, verbose, cleanup,
         _backend=None, _comm=None):
    """``_backend`` (tests only) replaces the GPU engine with an object offering score() and
    segment_mean(); ``_comm`` (tests only) replaces the RCCL transport with another implementation of the
    sharding.py transport interface.  The product path always builds a :class:`GpuBackend` and an
    :class:`genomad_amd.rccl.RcclComm`, and fails without a GPU."""
    from . import rccl, sharding
    rccl.prepare_env()        # before ANY HIP call: drops the reference's CUDA_VISIBLE_DEVICES=-1 (:8)
    configured_precision()    # a mistyped GENOMAD_AMD_PRECISION stops here
    embeddings = embeddings_requested()
    scan_stride = scan_stride_requested()
    strand = strand_requested()
    occlusion_block = occlusion_block_requested()
    attribution_bin = attribution_bin_requested()
    region_penalty = region_penalty_requested()
    region_embeddings = region_embeddings_requested()
    requests = {a.name: a.request() for a in ANALYSES_RUN}
    base_paths = {a.name: a.base.request() for a in ANALYSES_RUN if a.base is not None}
    input_path, output_path = Path(input_path), Path(output_path)
    if _comm is not None:
        comm = _comm
    elif _backend is None and rccl.world_from_env()[1] > 1:
        comm = rccl.comm_for(_engine())      # one process per GPU: RCCL communicator of this rank's engine
    else:
        comm = None
    rank, world = (comm.rank, comm.world) if comm is not None else (0, 1)
    rank0 = rank == 0
    if not output_path.is_dir():
        output_path.mkdir(exist_ok=True)
    prefix = sequence.prefix_of(input_path)
    outputs = Outputs(prefix, output_path)
    console = Console(output_file=outputs.nn_classification_log if rank0 else None, verbose=verbose and rank0)
    parameter_dict = {"single_window": single_window}
    md5_async(input_path)            # starts hashing now; check_fasta and the stages overlap with it
    device_front_end = _backend is None and os.environ.get("GENOMAD_AMD_FRONT_END", "device") == "device"
    if embeddings and not device_front_end:
        # the per-window host path (GpuBackend) has no embedding output: stop rather than leave the requested file out
        console.error("GENOMAD_AMD_EMBEDDINGS=1 needs the device front end: the host front end (GENOMAD_AMD_FRONT_END=host) does "
                      "not compute encoder embeddings. Unset GENOMAD_AMD_FRONT_END or GENOMAD_AMD_EMBEDDINGS.")
        sys.exit(1)
    if scan_stride is not None and not device_front_end:
        console.error("GENOMAD_AMD_SCAN_STRIDE needs the device front end: the host front end (GENOMAD_AMD_FRONT_END=host) does "
                      "not scan contigs. Unset GENOMAD_AMD_FRONT_END or GENOMAD_AMD_SCAN_STRIDE.")
        sys.exit(1)
    if region_penalty is not None and scan_stride is None:
        console.error("GENOMAD_AMD_REGION_PENALTY needs GENOMAD_AMD_SCAN_STRIDE: regions are called along the score tracks of a scan. "
                      "Set GENOMAD_AMD_SCAN_STRIDE or unset GENOMAD_AMD_REGION_PENALTY.")
        sys.exit(1)
    if region_embeddings and region_penalty is None:
        console.error("GENOMAD_AMD_REGION_EMBEDDINGS=1 needs GENOMAD_AMD_REGION_PENALTY: the embeddings are those of the regions called "
                      "along the score tracks. Set GENOMAD_AMD_REGION_PENALTY or unset GENOMAD_AMD_REGION_EMBEDDINGS.")
        sys.exit(1)
    for a in ANALYSES_RUN:
        requested = requests[a.name] is not None
        if a.base is None and requested and not embeddings:
            console.error(f"{a.switch} needs GENOMAD_AMD_EMBEDDINGS=1: {a.needs}. Set GENOMAD_AMD_EMBEDDINGS=1 or unset {a.switch}.")
            sys.exit(1)
        if requested and a.after is not None and requests[a.after] is None:
            other = next(b.switch for b in ANALYSES_RUN if b.name == a.after)
            console.error(f"{a.switch} needs {other}: {a.needs}. Set {other} or unset {a.switch}.")
            sys.exit(1)
        if a.base is not None and (requested != (base_paths[a.name] is not None) or (requested and not embeddings)):
            console.error(f"{a.switch} and {a.switch}_BASE need each other and GENOMAD_AMD_EMBEDDINGS=1: {a.needs}. Set all three or unset both.")
            sys.exit(1)

    if strand != "forward" and not device_front_end:
        console.error("GENOMAD_AMD_STRAND needs the device front end: the host front end (GENOMAD_AMD_FRONT_END=host) does "
                      "not cut reverse-complement windows. Unset GENOMAD_AMD_FRONT_END or GENOMAD_AMD_STRAND.")
        sys.exit(1)

    if occlusion_block is not None and not device_front_end:
        console.error("GENOMAD_AMD_OCCLUSION_BLOCK needs the device front end: the host front end (GENOMAD_AMD_FRONT_END=host) does "
                      "not occlude windows. Unset GENOMAD_AMD_FRONT_END or GENOMAD_AMD_OCCLUSION_BLOCK.")
        sys.exit(1)
    if occlusion_block is not None and strand != "forward":
        console.error(f"GENOMAD_AMD_OCCLUSION_BLOCK is forward-strand only: it cannot be combined with GENOMAD_AMD_STRAND={strand}. "
                      "Unset GENOMAD_AMD_STRAND or GENOMAD_AMD_OCCLUSION_BLOCK.")
        sys.exit(1)

    if attribution_bin is not None and not device_front_end:
        console.error("GENOMAD_AMD_ATTRIBUTION_BIN needs the device front end: the host front end (GENOMAD_AMD_FRONT_END=host) does "
                      "not compute contribution maps. Unset GENOMAD_AMD_FRONT_END or GENOMAD_AMD_ATTRIBUTION_BIN.")
        sys.exit(1)
    if attribution_bin is not None and configured_precision() == "f16c6":
        console.error("GENOMAD_AMD_ATTRIBUTION_BIN cannot be combined with GENOMAD_AMD_PRECISION=f16c6: the maps are the gradient of the "
                      "exact f32 dense head, which that arithmetic does not run. Unset GENOMAD_AMD_PRECISION or GENOMAD_AMD_ATTRIBUTION_BIN.")
        sys.exit(1)
    if attribution_bin is not None and strand != "forward":
        console.error(f"GENOMAD_AMD_ATTRIBUTION_BIN is forward-strand only: it cannot be combined with GENOMAD_AMD_STRAND={strand}. "
                      "Unset GENOMAD_AMD_STRAND or GENOMAD_AMD_ATTRIBUTION_BIN.")
        sys.exit(1)

    bases = {}                       # what every requested reference's loader returned, read before any classification starts
    for a in ANALYSES_RUN:
        if a.base is not None and requests[a.name] is not None:
            try:
                bases[a.name] = a.base.load(base_paths[a.name], strand)
            except ValueError as e:
                console.error(f"{e}. Name a file that GENOMAD_AMD_EMBEDDINGS=1 wrote under the same GENOMAD_AMD_STRAND{a.base.hint}, or unset "
                              f"{a.switch} and {a.switch}_BASE.")
                sys.exit(1)

    def everywhere(*flags):
        """Decisions read from files that rank 0 is about to rewrite are taken on rank 0 and made known to
        the other ranks, so that all of them walk through the same gathers."""
        return [bool(f) for f in sharding.broadcast_flags(comm, flags)] if comm is not None else [bool(f) for f in flags]

    (classify_proviruses,) = everywhere(check_provirus_execution(outputs, input_path) if rank0 else False)
    output_files = [outputs.nn_classification_execution_info, outputs.encoded_sequences_dir,
                    outputs.nn_classification_output, outputs.nn_classification_npz_output]
    if classify_proviruses:
        output_files += [outputs.encoded_proviruses_dir, outputs.provirus_nn_classification_output,
                         outputs.provirus_nn_classification_npz_output]
    console.log(f"Executing geNomad nn-classification (genomad_amd, MI355X). Outputs in {outputs.nn_classification_dir}.")

    def fail_on_bad_fasta(ok: bool):                                           # :164-170
        if not ok:
            console.error(f"{input_path} is either empty or contains multiple entries with the same identifier. "
                          "Please check your input FASTA file and execute genomad nn-classification again.")
            sys.exit(1)

    # The FASTA is validated once, on rank 0 (in bounded memory: sequence.check_fasta), and the verdict is
    # shared.  The device front end runs it on a helper thread while the GPU already classifies; nothing is
    # written (no outputs, no execution info) before ``gate()`` has seen the verdict, so an invalid input
    # leaves the same state behind as in the reference, which checks first.
    skip, changed = False, False                                               # :175-197
    if rank0 and (outputs.nn_classification_execution_info.exists() and any(p.exists() for p in output_files)
                  and not restart):
        skip = compare_executions(input_path, parameter_dict, outputs.nn_classification_execution_info)
        changed = not skip
    skip, changed = everywhere(skip, changed)
    # With several ranks the validation is sharded like the classification: every rank collects the accessions of the records
    # of ITS share while it reads it (no second pass over the file), and one gather of 64-bit digests decides
    # (sharding.fasta_verdict).  Only when the main stage really reads the file: a resumed run that finds the scores on disk
    # validates as before, on rank 0.
    (sharded_check,) = everywhere(device_front_end and world > 1 and rank0
                                  and not (skip and outputs.nn_classification_npz_output.exists()))
    check_pool = concurrent.futures.ThreadPoolExecutor(max_workers=1) if (device_front_end and rank0 and not sharded_check) else None
    check_future = check_pool.submit(sequence.check_fasta, input_path) if check_pool else None
    if not device_front_end:
        fail_on_bad_fasta(everywhere(sequence.check_fasta(input_path) if rank0 else True)[0])
    if skip:
        console.log("Previous execution detected. Steps will be skipped unless their outputs are not found. "
                    "Use the --restart option to force the execution of all the steps again.")
    elif changed:
        console.log("The input file or the parameters changed since the last execution. "
                    "Previous outputs will be overwritten.")
    state = {"info_writer": None, "gated": False, "verdict": None}
    start_time = datetime.now(timezone.utc).astimezone().isoformat()

    def gate():
        """First call (every rank, at the same point of the program): wait for the FASTA verdict, then start
        writing the execution info (as soon as the digest is ready; a non-daemon thread, so it also
        completes if a stage ends the run with sys.exit).  Every writer of an output file calls this first."""
        if state["gated"]:
            return
        state["gated"] = True
        if device_front_end and sharded_check:
            if state["verdict"] is None:                         # gate() before the main stage ran fasta_verdict: a bug, not a bad FASTA
                raise RuntimeError("internal error: gate() was reached before the sharded FASTA verdict was computed")
            fail_on_bad_fasta(state["verdict"])                  # decided by all ranks together in the main stage
        elif device_front_end:
            fail_on_bad_fasta(everywhere(check_future.result() if rank0 else True)[0])
        if rank0:
            outputs.nn_classification_dir.mkdir(exist_ok=True)
            state["info_writer"] = threading.Thread(
                target=write_execution_info, name="genomad-amd-execution-info",
                args=(MODULE_NAME, input_path, parameter_dict, outputs.nn_classification_execution_info, start_time))
            state["info_writer"].start()

    if not device_front_end:
        gate()

    def stage(fasta, enc_dir, wid_path, npz_path, tsv_path, names_key, ids_key, what):
        windows = None
        (have_enc,) = everywhere(rank0 and skip and wid_path.exists() and bool(
            len(list(enc_dir.glob("*.win.npy"))) or len(list(enc_dir.glob("*.tfrec")))))       # :215-225
        if have_enc:
            console.log(f"{enc_dir.name} was found. Skipping {what} encoding.")
            z = np.load(wid_path)
            names, ids = z[names_key], z[ids_key]
        else:
            if rank0:
                if enc_dir.is_dir():
                    shutil.rmtree(enc_dir)
                enc_dir.mkdir()
                names, ids, windows = _encode(fasta, enc_dir, wid_path, single_window, names_key, ids_key)
            else:
                names, ids, windows = sequence.encode_fasta(fasta, single_window)
            console.log(f"Encoded {what} data written to {enc_dir.name}.")
        (have_npz,) = everywhere(rank0 and skip and npz_path.exists())                   # :284-292
        predictions = None
        if have_npz:
            console.log(f"{npz_path.name} was found. Skipping {what} classification.")
            if rank0:
                z = np.load(npz_path)
                names, predictions = z[names_key], z["predictions"]
        else:
            if windows is None:
                files = sorted(enc_dir.glob("*.win.npy"))
                if files:
                    windows = np.concatenate([np.load(f) for f in files])
                else:
                    # a directory encoded by the reference itself (TFRecords of tokens, :43-52): rebuild
                    # windows that tokenise to exactly those tokens
                    from . import tfrecord
                    windows = tfrecord.tokens_to_bases(tfrecord.read_dir(enc_dir))
            if not len(windows):                                                     # :297-299
                console.error("No sequences were found. Please check your input FASTA.")
                sys.exit(1)
            backend = _backend if _backend is not None else GpuBackend(batch_size, console)
            predictions = classify_windows(windows, ids, len(names), backend, comm)
            if _backend is None:
                sentinel_verdict(comm, getattr(backend, "sentinel", None), console, getattr(backend, "precision", "?"))
            console.log(f"{what.capitalize()}s classified.")
            if rank0:
                np.savez_compressed(npz_path, **{names_key: names, "predictions": predictions})   # :326-330
        if cleanup and rank0 and enc_dir.is_dir():                                   # :335-337
            console.log(f"Deleting encoded {what} data.")
            shutil.rmtree(enc_dir)
        if rank0:
            write_tsv(tsv_path, names, predictions)                                  # :340-352 (always rewritten)

    def stage_device(fasta, what, names_key, ids_key):
        """Product path: the contig front end (NNEngine.classify_contigs) does windowing, the N rule,
        tokenising, classification and the per-contig mean on the GPU, so encoding and classification
        are one step; ``<prefix>_seq_window_id.npz`` is still written.  With several ranks the CONTIGS are
        sharded: every rank reads and packs only its own record-aligned byte range of the file (for
        compressed inputs: every world-th record-aligned chunk of the decompressed stream), classifies it
        on its GPU, and rank 0 collects the per-contig scores with one gather and writes the files —
        results are bit-identical for any number of ranks.  Every path is that of stage ``what`` in ``outputs``.
        ``emb_path`` (GENOMAD_AMD_EMBEDDINGS=1): the per-contig encoder
        embeddings are computed in the same pass and written there; a run that finds the scores but not that file classifies again.
        ``scan_path`` (GENOMAD_AMD_SCAN_STRIDE): every piece is also scanned at that stride (NNEngine.scan_contigs) and the score
        tracks are written there; a run that finds the scores but no scan file of that stride runs the stage again.
        ``strand_path`` (GENOMAD_AMD_STRAND): under ``reverse`` or ``both`` every score, embedding and track carries that mode and each
        strand's contig scores are written there; the file also says which mode the stage's outputs were computed under (absent:
        forward), and a run that asks for another mode runs the stage again.  Embeddings and scan files of reverse / both carry the
        mode as well, so one left behind by an earlier run is not taken for another mode's.
        ``occ_path`` (GENOMAD_AMD_OCCLUSION_BLOCK): after its normal classification every piece is also occluded with blocks of that
        size (NNEngine.occlude_contigs) and the maps are written there.  The file follows the strand file's rule: it says which block
        size the stage was run with (absent: none), a run that asks for another runs the stage again, and one that asks for none
        removes it.
        ``attr_path`` (GENOMAD_AMD_ATTRIBUTION_BIN): after its normal classification every piece also goes through
        NNEngine.attribute_contigs with bins of that many pooled positions, and the maps are written there.  The file follows the
        occlusion file's rule, with the bin in place of the block.
        ``regions_path``, ``regions_tsv_path`` (GENOMAD_AMD_REGION_PENALTY): rank 0 calls regions (NNEngine.call_regions) on the gathered
        track - regions are per contig, so the result does not depend on the number of ranks - and writes both files.  They follow the
        occlusion file's rule, with (stride, penalty) in place of the block.
        ``region_emb_path`` (GENOMAD_AMD_REGION_EMBEDDINGS=1, which needs the regions): right after a piece's scan, while its
        sequence is in memory, the piece's own track is segmented (regions are per contig and exact integers: they are the ones
        rank 0 calls on the gathered track, which rank 0 checks) and NNEngine.embed_intervals folds the scan windows' encoder
        embeddings into the regions, in the run's arithmetic and strand mode.  The file follows the occlusion file's rule, with
        (stride, penalty, strand) in place of the block.
        The ANALYSES (each needs the embeddings): rank 0 runs every requested one, in the table's order, on the gathered per-contig
        embeddings - of the strand mode the stage ran under - and writes its npz and its tsv.  The files follow the occlusion file's
        rule (:func:`_resumes`): the npz spells the request it was computed with (absent: none), the tsv is there iff the npz is, a
        file of reverse / both carries the mode, and one computed against a reference holds the reference's identity; a run that asks
        for anything else runs the stage again, and one that asks for none removes both files."""
        enc_dir, wid_path, npz_path, tsv_path = outputs.classification_files(what)
        emb_path = outputs.files(what, "embeddings")[0] if embeddings else None
        scan_path = outputs.files(what, "scan")[0] if scan_stride is not None else None
        strand_path, occ_path, attr_path = (outputs.files(what, name)[0] for name in ("strand", "occlusion", "attribution"))
        regions_path, regions_tsv_path = outputs.files(what, "regions")
        region_emb_file = outputs.files(what, "region_embeddings")[0]
        region_emb_path = region_emb_file if region_embeddings else None
        region_emb_request = None if region_emb_path is None else (scan_stride, region_penalty, strand)
        regions_request = None if region_penalty is None else (scan_stride, region_penalty)
        (have_npz,) = everywhere(rank0 and skip and npz_path.exists() and _strand_of_file(strand_path) == strand
                                 and _request_of_file(occ_path, (("block", int),)) == occlusion_block
                                 and _request_of_file(attr_path, (("bin", int),)) == attribution_bin
                                 and _request_of_file(regions_path, (("stride", int), ("penalty", float))) == regions_request
                                 and (regions_request is None) == (not regions_tsv_path.exists())
                                 and _request_of_file(region_emb_file, (("stride", int), ("penalty", float), ("strand", str))) == region_emb_request
                                 and all(_resumes(a, *outputs.files(what, a.name), requests[a.name], strand, bases.get(a.name)) for a in ANALYSES_RUN)
                                 and (emb_path is None or (emb_path.exists() and _npz_strand(emb_path) == strand))
                                 and (scan_path is None or (_scan_file_has_stride(scan_path, scan_stride)
                                                            and _npz_strand(scan_path) == strand)))   # :284-292
        names = predictions = None
        if have_npz:
            gate()
            console.log(f"{npz_path.name} was found. Skipping {what} classification.")
            if rank0:
                z = np.load(npz_path)
                names, predictions = z[names_key], z["predictions"]
        else:
            precision = configured_precision()
            _warn_out_of_tolerance(console, precision)
            eng = _engine()
            size = Path(fasta).stat().st_size * (1 if sequence.compression_of(fasta) == "uncompressed" else 4)
            precision = select_arithmetic(eng, precision, size, comm, console)
            parts, emb_parts, scan_parts, strand_parts, occ_parts, attr_parts, region_emb_parts = [], [], [], [], [], [], []
            sentinel = {"d": None, "done": False}

            def classify(key, nm, sq, off):
                pr, emb, wid = classify_piece(key, sq, off)
                parts.append((key, nm, pr, wid))
                emb_parts.append((key, emb))
                if scan_path is not None:       # after the normal classification, with the arithmetic the run selected
                    sc = (scan_contigs_safely(eng, sq, off, scan_stride, single_window, precision, console) if strand == "forward" else
                          scan_contigs_strand_safely(eng, sq, off, scan_stride, strand, single_window, precision, console))
                    if region_emb_path is not None:                     # while the piece's sequence is in memory
                        region_emb_parts.append((key, region_embeddings_of_piece(sc, sq, off)))
                    if region_penalty is not None:                      # the region table needs every contig's length on rank 0
                        sc = dict(sc.asdict(), contig_len=np.diff(np.asarray(off, np.int64)))
                    scan_parts.append((key, sc))
                if occlusion_block is not None:                         # likewise after, and beside, the normal classification
                    occ_parts.append((key, occlude_contigs_safely(eng, sq, off, occlusion_block, single_window, precision, console)))
                if attribution_bin is not None:
                    attr_parts.append((key, attribute_contigs_safely(eng, sq, off, attribution_bin, single_window, precision, console)))

            def region_embeddings_of_piece(sc, sq, off):
                """the piece's regions, called on its own track, and their interval embeddings: the fields of
                sharding.gather_contig_region_embeddings"""
                off = np.asarray(off, np.int64)
                reg = eng.call_regions(sc.track, sc.bin_offsets, region_penalty, off, scan_stride)
                iv = embed_intervals_safely(eng, sq, off, scan_stride, reg.region_contig, reg.start, reg.end, strand, single_window,
                                            precision, console)
                per_contig = np.bincount(reg.region_contig, minlength=len(off) - 1)
                return {"region_offsets": np.concatenate([[0], np.cumsum(per_contig)]).astype(np.int64), "start": reg.start,
                        "end": reg.end, "state": reg.region_state, "count": iv.count, "embedding": iv.embedding,
                        "coherence": iv.coherence, "scores": iv.scores}

            def classify_piece(key, sq, off):
                if not sentinel["done"] and len(off) > 1:           # this rank's first piece with a contig: the run's parity sample
                    sentinel["done"] = True
                    sentinel["d"] = parity_sentinel(eng, sentinel_windows(sq, off, single_window), precision, console)
                    if comm is None:                                # one rank: a failed check stops the run here, not after the whole
                        sentinel_verdict(None, sentinel["d"], console, precision)       # file (several ranks leave together below)
                if strand != "forward":
                    pr, emb, wid, fwd, rev = strand_contigs_safely(eng, sq, off, strand, single_window, precision, emb_path is not None, console)
                    strand_parts.append((key, fwd, rev))
                    return pr, emb, wid
                if emb_path is not None:
                    return embed_contigs_safely(eng, sq, off, single_window, precision, console)
                pr, wid = classify_contigs_safely(eng, sq, off, single_window, precision, console)
                return pr, None, wid

            validate = sharded_check and fasta is input_path        # the provirus FASTA is geNomad's own output: never validated
            seen = []                                               # digests of the accessions of ALL records of this rank's share (validate)

            def pack(text):
                if validate:                                        # one native pass, before the in-place pack consumes the text
                    seen.append(sequence.accession_digests_of_text(text))
                return sequence.pack_text(text, strip_n=True)

            if sequence.compression_of(fasta) == "uncompressed":
                # this rank's record-aligned share of the file, in pieces of about 128 MB: piece k+1
                # is read and packed on a helper thread while the GPU classifies piece k
                share = Path(fasta).stat().st_size // world
                pieces = int(min(64, max(1, -(-share // (128 << 20)))))
                read = lambda k: pack(sequence._read_text_array(  # noqa: E731
                    fasta, sequence.record_aligned_range(fasta, rank, world, k, pieces)))
                with concurrent.futures.ThreadPoolExecutor(max_workers=1) as pool:
                    nxt = pool.submit(read, 0)
                    for k in range(pieces):
                        nm, sq, off = nxt.result()
                        if k + 1 < pieces:
                            nxt = pool.submit(read, k + 1)
                        classify(rank * 64 + k, nm, sq, off)
            else:
                # compressed streams cannot be read by byte range: every rank decompresses the stream
                # chunk by chunk (bounded memory) and packs + classifies every world-th chunk
                for i, chunk in enumerate(sequence.iter_text_chunks(fasta)):
                    if i % world != rank:
                        continue
                    nm, sq, off = pack(chunk)
                    classify(i, nm, sq, off)
            if validate:
                digests = np.concatenate(seen) if seen else np.zeros(0, dtype="<u8")
                state["verdict"] = sharding.fasta_verdict(comm, digests, lambda: sequence.check_fasta(input_path))
            sentinel_verdict(comm, sentinel["d"], console, precision)      # before anything is written
            names, predictions, ids, n_windows = sharding.gather_contig_parts(comm, parts)
            embeddings_all = sharding.gather_contig_embeddings(comm, emb_parts) if emb_path is not None else None
            strand_fields = sharding.SCAN_STRAND_FIELDS if strand != "forward" else ()
            length_fields = sharding.SCAN_LENGTH_FIELDS if region_penalty is not None else ()
            scans_all = (sharding.gather_contig_scans(comm, scan_parts, extra_window_fields=strand_fields, extra_contig_fields=length_fields)
                         if scan_path is not None else None)
            strands_all = sharding.gather_contig_strand_scores(comm, strand_parts) if strand != "forward" else None
            occ_all = sharding.gather_contig_occlusions(comm, occ_parts) if occlusion_block is not None else None
            attr_all = (sharding.gather_contig_attributions(comm, attr_parts, -(-ATTRIBUTION_POSITIONS // attribution_bin))
                        if attribution_bin is not None else None)
            region_emb_all = sharding.gather_contig_region_embeddings(comm, region_emb_parts) if region_emb_path is not None else None
            gate()
            if not n_windows:                                                        # :297-299
                console.error("No sequences were found. Please check your input FASTA.")
                sys.exit(1)
            if rank0:
                if enc_dir.is_dir():
                    shutil.rmtree(enc_dir)
                enc_dir.mkdir()
                np.savez_compressed(wid_path, **{names_key: names, ids_key: ids})
                console.log(f"{what.capitalize()}s classified ({len(ids)} windows).")
                np.savez_compressed(npz_path, **{names_key: names, "predictions": predictions})
                if emb_path is not None:
                    np.savez_compressed(emb_path, **{names_key: names, "embeddings": embeddings_all, **_strand_entry(strand)})
                    console.log(f"Encoder embeddings of the {what}s written to {emb_path.name}.")
                if scan_path is not None:
                    sc = scans_all
                    np.savez_compressed(scan_path, **{names_key: names, "stride": np.int64(scan_stride), "win_offsets": sc["win_offsets"],
                                                      "window_start": sc["starts"], "window_len": sc["lens"], "window_kept": sc["kept"],
                                                      "window_scores": sc["scores"], "bin_offsets": sc["bin_offsets"],
                                                      "track": sc["track"], "cover": sc["cover"],
                                                      **({"strand": np.array(strand), "window_scores_fwd": sc["scores_fwd"],
                                                          "window_scores_rev": sc["scores_rev"]} if strand != "forward" else {})})
                    console.log(f"Score tracks of the {what}s (stride {scan_stride}, {len(sc['starts'])} windows) written to {scan_path.name}.")
                if strand != "forward":
                    fwd, rev = strands_all
                    np.savez_compressed(strand_path, **{names_key: names, "strand": np.array(strand), "scores_fwd": fwd, "scores_rev": rev,
                                                        "max_abs_diff": np.abs(fwd - rev).max(axis=1) if len(fwd) else np.zeros(0, np.float32)})
                    console.log(f"Strand mode {strand}: forward and reverse scores of the {what}s written to {strand_path.name} "
                                f"(largest per-{what} |forward - reverse| {float(np.abs(fwd - rev).max()) if len(fwd) else 0.0:.4f}).")
                elif strand_path.exists():          # these outputs are forward ones again: the file that said otherwise goes
                    strand_path.unlink()
                if occlusion_block is not None:
                    np.savez_compressed(occ_path, **{names_key: names, "block": np.int64(occlusion_block), **occ_all})
                    console.log(f"Occlusion maps of the {what}s (blocks of {occlusion_block}, {len(occ_all['delta'])} (window, block) pairs) "
                                f"written to {occ_path.name}.")
                elif occ_path.exists():             # no occlusion was asked for: the file that said otherwise goes
                    occ_path.unlink()
                if attribution_bin is not None:
                    np.savez_compressed(attr_path, **{names_key: names, "bin": np.int64(attribution_bin), **attr_all})
                    console.log(f"Attention contribution maps of the {what}s (bins of {attribution_bin} pooled positions, "
                                f"{len(attr_all['contrib'])} windows) written to {attr_path.name}.")
                elif attr_path.exists():            # likewise
                    attr_path.unlink()
                if region_penalty is not None:
                    contig_offsets = np.concatenate([[0], np.cumsum(scans_all["contig_len"])]).astype(np.int64)
                    res = eng.call_regions(scans_all["track"], scans_all["bin_offsets"], region_penalty, contig_offsets, scan_stride)
                    np.savez_compressed(regions_path, **{names_key: names, "stride": np.int64(scan_stride), "penalty": np.float64(region_penalty),
                                                         **{k: v for k, v in res.asdict().items() if k not in ("stride", "penalty")}})
                    write_regions_tsv(regions_tsv_path, names, res)
                    console.log(f"Regions of the {what}s (stride {scan_stride}, switch penalty {region_penalty:g}, {len(res.region_contig)} regions) "
                                f"written to {regions_path.name} and {regions_tsv_path.name}.")
                else:                               # likewise, both files
                    for p in (regions_path, regions_tsv_path):
                        if p.exists():
                            p.unlink()
                if region_emb_path is not None:
                    re_ = region_emb_all
                    mine = (re_["contig"], re_["start"], re_["end"], re_["state"])
                    called = (res.region_contig, res.start, res.end, res.region_state)
                    if not all(np.array_equal(a, b) for a, b in zip(mine, called)):
                        raise RuntimeError(f"the regions the pieces embedded ({len(mine[0])}) are not the regions called on the gathered "
                                           f"track ({len(called[0])}, {regions_path.name})")
                    np.savez_compressed(region_emb_path, **{names_key: names, "contig": re_["contig"], "start": re_["start"],
                                                            "end": re_["end"], "state": re_["state"], "embedding": re_["embedding"],
                                                            "count": re_["count"], "coherence": re_["coherence"], "scores": re_["scores"],
                                                            "stride": np.int64(scan_stride), "penalty": np.float64(region_penalty),
                                                            "strand": np.array(strand)})
                    console.log(f"Encoder embeddings of the {len(mine[0])} regions of the {what}s written to {region_emb_path.name}.")
                elif region_emb_file.exists():      # likewise
                    region_emb_file.unlink()
                for a in ANALYSES_RUN:
                    npz, tsv = outputs.files(what, a.name)
                    request = requests[a.name]
                    if request is None:             # likewise, both files
                        for p in (npz, tsv):
                            if p is not None and p.exists():
                                p.unlink()
                        continue
                    ctx = SimpleNamespace(what=what, names=names, ids=ids, request=request, base=bases.get(a.name),
                                          base_path=base_paths.get(a.name))
                    try:
                        res = a.run(eng, embeddings_all, request, ctx)
                    except a.errors as e:           # nothing of this analysis was written; the earlier ones' files are
                        console.error(f"{a.switch}={request[0] if isinstance(request, tuple) else request:g}: {e}. {a.advice}")
                        sys.exit(1)
                    a.write(npz, tsv, names_key, names, res, strand, ctx)
                    title = a.title.format(what=what, base=ctx.base_path.name if ctx.base_path is not None else None)
                    console.log(f"{title} ({a.summary(res, request, what, ctx)}) written to {npz.name}"
                                + (f" and {tsv.name}." if tsv is not None else "."))
        if cleanup and rank0 and enc_dir.is_dir():
            console.log(f"Deleting encoded {what} data.")
            shutil.rmtree(enc_dir)
        if rank0:
            write_tsv(tsv_path, names, predictions)

    def run(fasta, what, names_key, ids_key):
        if device_front_end:
            stage_device(fasta, what, names_key, ids_key)
        else:
            stage(fasta, *outputs.classification_files(what), names_key, ids_key, what)

    try:
        run(input_path, "sequence", "contig_names", "contig_ids")
        if classify_proviruses:                                                      # :248-281, :355-425
            run(outputs.find_proviruses_nucleotide_output, "provirus", "provirus_names", "provirus_ids")
    finally:
        if check_pool is not None:
            check_pool.shutdown(wait=True)
        if state["info_writer"] is not None:
            if os.environ.get("GENOMAD_AMD_DEFER_EXECUTION_INFO") == "1" and sys.exc_info()[0] is None:
                # opt-in: do not wait for the input's md5 (one sequential pass at ~1 GB/s, utils.py:216-223 - with 8 GPUs it is
                # the longest thing main() does).  The scores are on disk; the execution-info JSON appears, with the same
                # content, when the digest is ready (a non-daemon thread: the process does not exit before).  A caller that
                # runs the next geNomad module in the same process right away (end-to-end: aggregated-classification requires
                # the JSON, aggregated_classification.py:101) must call wait_execution_info() first - hence opt-in.
                _DEFERRED.append(state["info_writer"])
            else:
                state["info_writer"].join()
    if comm is not None:
        comm.barrier()               # rank 0 has written everything before any rank returns
    console.log("geNomad nn-classification finished!")


_DEFERRED = []


def wait_execution_info():
    """Block until every execution-info JSON deferred by GENOMAD_AMD_DEFER_EXECUTION_INFO=1 has been written."""
    while _DEFERRED:
        _DEFERRED.pop().join()


def install():
    """Make the reference CLI use this module: ``genomad.nn_classification`` is looked up at call
    time (cli.py:772, :1367), so rebinding the attribute is enough."""
    from . import rccl
    import genomad
    import genomad.modules          # importing the reference module exports CUDA_VISIBLE_DEVICES=-1 (:8) ...
    rccl.prepare_env()              # ... which HIP would honour: undo it before any HIP call
    this = sys.modules[__name__]
    genomad.nn_classification = this
    genomad.modules.nn_classification = this
    sys.modules["genomad.modules.nn_classification"] = this
    return this
