"""Data-parallel sharding of windows / contigs across GPUs (one process per GPU).

Windows are independent (every score depends only on its own 6000 bytes and the replicated weights), so
the path shards with no data-path collective: rank r classifies a contiguous range of windows, and the
per-window scores (12 B each) are collected on rank 0 with ONE gather at the end (the loop
being sharded is nn_classification.py:316-320 of the reference).  Contiguous ranges keep every contig on
at most two ranks and preserve window order, so the per-contig segment mean runs on rank 0 over the
gathered array and the result is bit-identical for any number of ranks (no cross-rank reduction).

This module is transport-agnostic and imports neither torch nor the HIP library.  A transport ("comm") is
any object with

    rank, world                        ints
    barrier()
    allgather_i64(values)              list of ints -> int64 array (world, len(values))
    gather_array(arr, root=0)          same-shape/dtype numpy array from every rank -> (world, *shape) on
                                       ``root``, None elsewhere

The product transport is :class:`genomad_amd.rccl.RcclComm` (RCCL over xGMI through the C ABI's
``gnn_comm_*``); ``LocalComm`` below is the one-process case; the CPU test-suite drives the same functions
with a gloo transport (tests/gloo_comm.py, world size 2 and 3).
"""
import io
import json
from typing import List, Optional, Tuple

import numpy as np


def shard_range(n_windows: int, world_size: int, rank: int) -> Tuple[int, int]:
    """Half-open window range of ``rank``: ceil(n/G) windows per rank, the tail ranks get fewer
    (possibly zero)."""
    if world_size < 1 or not (0 <= rank < world_size) or n_windows < 0:
        raise ValueError("bad shard arguments")
    per = -(-n_windows // world_size)
    a = min(rank * per, n_windows)
    return a, min(a + per, n_windows)


def shard_counts(n_windows: int, world_size: int) -> List[int]:
    return [b - a for a, b in (shard_range(n_windows, world_size, r) for r in range(world_size))]


class LocalComm:
    """The one-process transport (world size 1)."""
    rank, world = 0, 1

    def barrier(self):
        pass

    def allgather_i64(self, values):
        return np.asarray(values, dtype=np.int64).reshape(1, -1)

    def gather_array(self, arr, root=0):
        return np.asarray(arr)[None]


def gather_scores(comm, local_scores: np.ndarray, n_windows: int, root: int = 0) -> Optional[np.ndarray]:
    """Collect the (n_local, 3) float32 score shards of all ranks on ``root`` in window order.  Shards are
    padded to ceil(n/G) rows so that a single fixed-size gather suffices.  Returns (n_windows, 3) on
    ``root`` and None elsewhere."""
    per = -(-n_windows // comm.world)
    a, b = shard_range(n_windows, comm.world, comm.rank)
    local = np.ascontiguousarray(local_scores, dtype=np.float32).reshape(-1, 3)
    if len(local) != b - a:
        raise ValueError(f"rank {comm.rank}: expected shard of {b - a} windows, got {len(local)}")
    send = np.zeros((per, 3), np.float32)
    send[: b - a] = local
    got = comm.gather_array(send, root)
    if got is None:
        return None
    return got.reshape(comm.world * per, 3)[:n_windows]


def classify_sharded(windows, score_fn, comm=None):
    """Score ``windows`` (n, 6000) with ``score_fn`` on this rank's contiguous shard and collect the (n, 3)
    scores on rank 0 (None on the other ranks).  Without a transport this is just ``score_fn(windows)``."""
    if comm is None or comm.world == 1:
        return np.ascontiguousarray(score_fn(windows), dtype=np.float32)
    a, b = shard_range(len(windows), comm.world, comm.rank)
    return gather_scores(comm, score_fn(windows[a:b]), len(windows))


def gather_bytes(comm, payload: bytes, root: int = 0) -> Optional[List[bytes]]:
    """Variable-length byte strings of every rank on ``root`` (None elsewhere): sizes travel in one small
    all-gather, the payloads padded to the longest in one gather."""
    sizes = comm.allgather_i64([len(payload)])[:, 0]
    width = max(int(sizes.max()), 1)
    send = np.zeros(width, np.uint8)
    send[: len(payload)] = np.frombuffer(payload, np.uint8)
    got = comm.gather_array(send, root)
    if got is None:
        return None
    return [got[r, : int(sizes[r])].tobytes() for r in range(comm.world)]


def contig_subset(offsets, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous contig range [a, b) of ``rank`` when every rank holds the WHOLE contig table (compressed
    inputs, which cannot be read by byte range): ranges are balanced by sequence length (windows are
    proportional to it) and never split a contig."""
    off = np.asarray(offsets, dtype=np.int64)
    n = len(off) - 1
    if world < 1 or not (0 <= rank < world):
        raise ValueError("bad shard arguments")
    total = int(off[-1])
    cut = lambda r: int(np.searchsorted(off[:-1], total * r // world, side="left")) if r < world else n  # noqa: E731
    return (0 if rank == 0 else cut(rank)), cut(rank + 1)


def gather_contig_parts(comm, parts, root: int = 0):
    """Contig-sharded results -> ``root``.  ``parts`` = this rank's list of (order_key, names (k,),
    predictions (k, 3) float32, window_ids) — one entry per piece of the input it classified, window ids
    counting contigs from 0 inside the piece.  A contig never straddles pieces, so every per-contig mean is
    local and the assembled table is bit-identical to a single-process run.  The scores travel in ONE
    gather; names, window ids and the piece table are small host objects and go as bytes.  ``root`` puts the
    pieces of all ranks in ``order_key`` order (= file order) and returns (names, predictions, window_ids,
    total_windows); the other ranks get (None, None, None, total_windows) — the window total is known
    everywhere so that all ranks take the same exit."""
    comm = comm or LocalComm()
    parts = list(parts)
    table = np.array([[int(key), len(nm), len(ids)] for key, nm, _, ids in parts], dtype="<i8").reshape(-1, 3)
    k = int(table[:, 1].sum()) if len(table) else 0
    meta = comm.allgather_i64([k, int(table[:, 2].sum()) if len(table) else 0])
    total_windows = int(meta[:, 1].sum())
    per = max(int(meta[:, 0].max()), 1)
    send = np.zeros((per, 3), np.float32)
    if k:
        send[:k] = np.concatenate([np.ascontiguousarray(pr, dtype=np.float32).reshape(-1, 3) for _, _, pr, _ in parts])
    preds = comm.gather_array(send, root)
    names = [str(n) for _, nm, _, _ in parts for n in nm]
    ids = np.concatenate([np.asarray(i, dtype="<i8") for _, _, _, i in parts]) if parts else np.zeros(0, "<i8")
    table_blobs = gather_bytes(comm, table.tobytes(), root)
    name_blobs = gather_bytes(comm, json.dumps(names).encode("utf-8", "surrogateescape"), root)
    id_blobs = gather_bytes(comm, ids.tobytes(), root)
    if comm.rank != root:
        return None, None, None, total_windows
    pieces = []                      # (order_key, rank, contig slice, window slice)
    r_names, r_ids = [], []
    for r in range(comm.world):
        t = np.frombuffer(table_blobs[r], dtype="<i8").reshape(-1, 3)
        r_names.append(json.loads(name_blobs[r].decode("utf-8", "surrogateescape")))
        r_ids.append(np.frombuffer(id_blobs[r], dtype="<i8").astype(np.int64))
        c0 = w0 = 0
        for key, nc, nw in t:
            pieces.append((int(key), r, c0, c0 + int(nc), w0, w0 + int(nw)))
            c0, w0 = c0 + int(nc), w0 + int(nw)
    pieces.sort()
    if len({p[0] for p in pieces}) != len(pieces):
        raise ValueError("duplicate piece keys in gather_contig_parts")
    out_names, out_preds, out_ids, base = [], [], [], 0
    for _, r, c0, c1, w0, w1 in pieces:
        out_names.extend(r_names[r][c0:c1])
        out_preds.append(preds[r][c0:c1])
        out_ids.append(r_ids[r][w0:w1] + base)
        base += c1 - c0
    return (np.array(out_names) if out_names else np.zeros(0, dtype="<U1"),
            np.concatenate(out_preds, axis=0) if out_preds else np.zeros((0, 3), np.float32),
            np.concatenate(out_ids) if out_ids else np.zeros(0, np.int64), total_windows)


def gather_contig_embeddings(comm, parts, width: int = 512, root: int = 0):
    """Per-contig rows of contig-sharded pieces -> ``root``, in the piece order of :func:`gather_contig_parts`.  ``parts`` = this
    rank's list of (order_key, rows (k, width) float32), the same keys and contig counts as the pieces handed to
    gather_contig_parts (the encoder embeddings of main()).  The rows travel in ONE padded gather, the piece table as bytes; the
    rows are only moved, so the table is bit-identical for any number of ranks.  Returns (n_contigs, width) float32 on ``root``,
    None elsewhere."""
    comm = comm or LocalComm()
    parts = list(parts)
    table = np.array([[int(key), len(rows)] for key, rows in parts], dtype="<i8").reshape(-1, 2)
    k = int(table[:, 1].sum()) if len(table) else 0
    per = max(int(comm.allgather_i64([k])[:, 0].max()), 1)
    send = np.zeros((per, width), np.float32)
    if k:
        send[:k] = np.concatenate([np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, width) for _, rows in parts])
    got = comm.gather_array(send, root)
    table_blobs = gather_bytes(comm, table.tobytes(), root)
    if comm.rank != root:
        return None
    pieces = []                      # (order_key, rank, contig slice)
    for r in range(comm.world):
        c0 = 0
        for key, nc in np.frombuffer(table_blobs[r], dtype="<i8").reshape(-1, 2):
            pieces.append((int(key), r, c0, c0 + int(nc)))
            c0 += int(nc)
    pieces.sort()
    if len({p[0] for p in pieces}) != len(pieces):
        raise ValueError("duplicate piece keys in gather_contig_embeddings")
    out = [got[r][c0:c1] for _, r, c0, c1 in pieces]
    return np.concatenate(out, axis=0) if out else np.zeros((0, width), np.float32)


SCAN_WINDOW_FIELDS = ("starts", "lens", "kept", "scores")      # per window; CSR over contigs by win_offsets
SCAN_BIN_FIELDS = ("track", "cover")                           # per bin; CSR over contigs by bin_offsets


def gather_contig_strand_scores(comm, parts, root: int = 0):
    """Each strand's own per-contig scores of contig-sharded pieces -> ``root``, in the piece order of :func:`gather_contig_parts`.
    ``parts`` = this rank's list of (order_key, forward (k, 3) float32, reverse (k, 3) float32), the arrays
    ``NNEngine.classify_contigs_strand`` returns beside the mode's scores.  They travel as one (k, 6) row table through
    :func:`gather_contig_embeddings` - moved, never recomputed, so the same bits for any number of ranks.  Returns (forward, reverse),
    each (n_contigs, 3) float32, on ``root``; None elsewhere."""
    rows = [(key, np.concatenate([np.asarray(f, np.float32).reshape(-1, 3), np.asarray(r, np.float32).reshape(-1, 3)], axis=1))
            for key, f, r in parts]
    got = gather_contig_embeddings(comm, rows, width=6, root=root)
    if got is None:
        return None
    return np.ascontiguousarray(got[:, :3]), np.ascontiguousarray(got[:, 3:])


SCAN_LENGTH_FIELDS = ("contig_len",)                           # per contig: its length in bases (main() adds it for the region table)
SCAN_STRAND_FIELDS = ("scores_fwd", "scores_rev")              # per window, of a scan with a strand mode (StrandScanResult)


def gather_contig_scans(comm, parts, root: int = 0, extra_window_fields=(), extra_contig_fields=()):
    """Score tracks of contig-sharded pieces -> ``root``, in the piece order of :func:`gather_contig_parts`.  ``parts`` = this rank's
    list of (order_key, scan) with the same keys and contig counts as the pieces handed to gather_contig_parts; ``scan`` = the
    arrays of one ``NNEngine.scan_contigs`` call (win_offsets, starts, lens, kept, scores, bin_offsets, track, cover; an object with
    ``asdict()`` or a dict).  Window and bin counts differ from rank to rank, so each rank's pieces travel as one byte string
    (:func:`gather_bytes`).  ``root`` concatenates the pieces and rebases the two CSR offset arrays; the values are only moved, so
    the result is bit-identical for any number of ranks.  Returns a dict of those eight arrays on ``root``, None elsewhere.
    ``extra_window_fields`` (SCAN_STRAND_FIELDS for the scans of ``NNEngine.scan_contigs_strand``): further (n_windows, 3) float32
    arrays of every scan, gathered and returned the same way.  ``extra_contig_fields`` (SCAN_LENGTH_FIELDS: the contig lengths the
    region table needs): further (n_contigs,) int64 arrays of every scan, likewise - they ride in the same byte string."""
    comm = comm or LocalComm()
    window_fields = SCAN_WINDOW_FIELDS + tuple(extra_window_fields) + tuple(extra_contig_fields)
    arrays = {"keys": np.array([int(key) for key, _ in parts], dtype="<i8")}
    for i, (_, scan) in enumerate(parts):
        scan = scan.asdict() if hasattr(scan, "asdict") else scan
        for f in ("win_offsets", "bin_offsets") + window_fields + SCAN_BIN_FIELDS:
            arrays[f"{i}_{f}"] = np.ascontiguousarray(scan[f])
    buf = io.BytesIO()
    np.savez(buf, **arrays)
    blobs = gather_bytes(comm, buf.getvalue(), root)
    if comm.rank != root:
        return None
    pieces = []                      # (order_key, {field: array})
    for blob in blobs:
        z = np.load(io.BytesIO(blob))
        for i, key in enumerate(z["keys"]):
            pieces.append((int(key), {f[len(str(i)) + 1:]: z[f] for f in z.files if f.startswith(f"{i}_")}))
    if len({p[0] for p in pieces}) != len(pieces):
        raise ValueError("duplicate piece keys in gather_contig_scans")
    pieces.sort(key=lambda p: p[0])
    out = {"win_offsets": [np.zeros(1, np.int64)], "bin_offsets": [np.zeros(1, np.int64)]}
    out.update({f: [] for f in window_fields + SCAN_BIN_FIELDS})
    w0 = b0 = 0
    for _, d in pieces:
        out["win_offsets"].append(d["win_offsets"][1:].astype(np.int64) + w0)
        out["bin_offsets"].append(d["bin_offsets"][1:].astype(np.int64) + b0)
        w0, b0 = w0 + int(d["win_offsets"][-1]), b0 + int(d["bin_offsets"][-1])
        for f in window_fields + SCAN_BIN_FIELDS:
            out[f].append(d[f])
    empty = {"starts": np.zeros(0, np.int64), "lens": np.zeros(0, np.int32), "kept": np.zeros(0, bool),
             "scores": np.zeros((0, 3), np.float32), "track": np.zeros((0, 3), np.float32), "cover": np.zeros(0, np.int32)}
    empty.update({f: np.zeros((0, 3), np.float32) for f in extra_window_fields})
    empty.update({f: np.zeros(0, np.int64) for f in extra_contig_fields})
    return {f: np.concatenate(v) if v else empty[f] for f, v in out.items()}


OCCLUSION_WINDOW_FIELDS = ("starts", "lens", "kept", "scores")      # per window; CSR over contigs by win_offsets
OCCLUSION_EMPTY = {"starts": np.zeros(0, np.int64), "lens": np.zeros(0, np.int32), "kept": np.zeros(0, bool),
                   "scores": np.zeros((0, 3), np.float32), "delta": np.zeros((0, 3), np.float32),
                   "contig_scores": np.zeros((0, 3), np.float32)}


def _gather_csr_pieces(comm, parts, csr, fields, empty, what, root):
    """The mechanism of the occlusion and attribution gathers.  ``parts`` = this rank's list of (order_key, result), a result being
    an object with ``asdict()`` or a dict of arrays.  Each rank's pieces travel as one byte string (:func:`gather_bytes`); ``root``
    sorts them by key, concatenates every array of ``fields`` and rebases the CSR arrays: ``csr`` = (name, ...), each continued by
    its own last entry.  The values are only moved.  ``empty``: what a field is when there is no piece at all.  Returns the dict
    on ``root``, None elsewhere."""
    comm = comm or LocalComm()
    arrays = {"keys": np.array([int(key) for key, _ in parts], dtype="<i8")}
    for i, (_, res) in enumerate(parts):
        res = res.asdict() if hasattr(res, "asdict") else res
        for f in csr + fields:
            arrays[f"{i}_{f}"] = np.ascontiguousarray(res[f])
    buf = io.BytesIO()
    np.savez(buf, **arrays)
    blobs = gather_bytes(comm, buf.getvalue(), root)
    if comm.rank != root:
        return None
    pieces = []                      # (order_key, {field: array})
    for blob in blobs:
        z = np.load(io.BytesIO(blob))
        for i, key in enumerate(z["keys"]):
            pieces.append((int(key), {f: z[f"{i}_{f}"] for f in csr + fields}))
    if len({p[0] for p in pieces}) != len(pieces):
        raise ValueError(f"duplicate piece keys in {what}")
    pieces.sort(key=lambda p: p[0])
    out = {f: [np.zeros(1, np.int64)] for f in csr}
    out.update({f: [] for f in fields})
    base = {f: 0 for f in csr}
    for _, d in pieces:
        for f in csr:
            out[f].append(d[f][1:].astype(np.int64) + base[f])
            base[f] += int(d[f][-1])
        for f in fields:
            out[f].append(d[f])
    return {f: np.concatenate(v) if v else empty[f] for f, v in out.items()}


def gather_contig_occlusions(comm, parts, root: int = 0):
    """Occlusion maps of contig-sharded pieces -> ``root``, in the piece order of :func:`gather_contig_parts`: the sibling of
    :func:`gather_contig_scans`.  ``parts`` = this rank's list of (order_key, result) with the keys and contig counts of the pieces
    handed to gather_contig_parts; ``result`` = the arrays of one ``NNEngine.occlude_contigs`` call (win_offsets, starts, lens, kept,
    scores, blk_offsets, delta, contig_scores; an object with ``asdict()`` or a dict).  ``root`` rebases the two CSR arrays -
    win_offsets over contigs, blk_offsets over windows; the values are only moved, so the result is bit-identical for any number of
    ranks.  Returns a dict of those eight arrays on ``root``, None elsewhere."""
    return _gather_csr_pieces(comm, parts, ("win_offsets", "blk_offsets"), OCCLUSION_WINDOW_FIELDS + ("delta", "contig_scores"),
                              OCCLUSION_EMPTY, "gather_contig_occlusions", root)


REGION_EMBEDDING_FIELDS = ("start", "end", "state", "count", "embedding", "coherence", "scores")      # per region


def gather_contig_region_embeddings(comm, parts, width: int = 512, root: int = 0):
    """Interval embeddings of the regions of contig-sharded pieces -> ``root``, by the mechanism of
    :func:`gather_contig_occlusions`: a third CSR family per contig.  ``result`` = a dict of ``region_offsets`` (the CSR of a piece's
    regions over its contigs, n_contigs + 1 entries) and, per region, ``start``, ``end`` (int64 bases), ``state`` (uint8), ``count``
    (int32), ``embedding`` (n, ``width``) float32, ``coherence`` (float32) and ``scores`` (n, 3) float32.  ``root`` rebases the CSR
    and derives every region's contig index from it; the values are only moved, so the result is bit-identical for any number of
    ranks.  Returns a dict of region_offsets, ``contig`` and the per-region arrays on ``root``, None elsewhere."""
    empty = {"start": np.zeros(0, np.int64), "end": np.zeros(0, np.int64), "state": np.zeros(0, np.uint8), "count": np.zeros(0, np.int32),
             "embedding": np.zeros((0, int(width)), np.float32), "coherence": np.zeros(0, np.float32),
             "scores": np.zeros((0, 3), np.float32)}
    out = _gather_csr_pieces(comm, parts, ("region_offsets",), REGION_EMBEDDING_FIELDS, empty, "gather_contig_region_embeddings", root)
    if out is None:
        return None
    per_contig = np.diff(out["region_offsets"])
    out["contig"] = np.repeat(np.arange(len(per_contig), dtype=np.int64), per_contig)
    return out


ATTRIBUTION_WINDOW_FIELDS = ("starts", "lens", "kept", "window_scores", "contrib", "bias", "logits")      # per window


def gather_contig_attributions(comm, parts, nb: int, root: int = 0):
    """Contribution maps of contig-sharded pieces -> ``root``, by the mechanism of :func:`gather_contig_occlusions`.  ``result`` =
    the arrays of one ``NNEngine.attribute_contigs`` call, every map with ``nb`` bins; win_offsets is the one CSR array.  Returns a
    dict of win_offsets, the per-window arrays and contig_scores on ``root``, None elsewhere."""
    row = np.zeros((0, 3), np.float32)
    empty = {"starts": np.zeros(0, np.int64), "lens": np.zeros(0, np.int32), "kept": np.zeros(0, bool), "window_scores": row,
             "contrib": np.zeros((0, 2, int(nb), 3), np.float32), "bias": row, "logits": row, "contig_scores": row}
    return _gather_csr_pieces(comm, parts, ("win_offsets",), ATTRIBUTION_WINDOW_FIELDS + ("contig_scores",), empty,
                              "gather_contig_attributions", root)


def gather_contig_results(comm, names, predictions, window_ids, root: int = 0):
    """One piece per rank, in rank order (see :func:`gather_contig_parts`)."""
    comm = comm or LocalComm()
    return gather_contig_parts(comm, [(comm.rank, names, predictions, window_ids)], root)


def broadcast_flags(comm, flags, root: int = 0):
    """Small ints decided on ``root`` (e.g. "skip this stage") made known to every rank."""
    got = comm.allgather_i64([int(f) for f in flags])
    return [int(v) for v in got[root]]


def accession_digests(accessions) -> np.ndarray:
    """64-bit digests of record accessions, as a uint64 array: what travels instead of the strings (the same function as the
    native one-pass :func:`genomad_amd.sequence.accession_digests_of_text`)."""
    from .sequence import _digest_of_accession
    return np.array([_digest_of_accession(a) for a in accessions], dtype="<u8")


def fasta_verdict(comm, accessions, exact_check, root: int = 0) -> bool:
    """check_fasta (genomad/sequence.py:124-131: False for a file without records or with two records of one accession) when
    every rank has seen only ITS records: ``accessions`` = the accessions of all records of this rank's share of the file (no N
    stripping: records that the classification pass drops count) - or, as the product path passes them, their uint64 digests
    already (``sequence.accession_digests_of_text``).  ONE gather of 64-bit digests to ``root``; equal digests, inside a share or
    across shares, are either a true duplicate or a collision (about 1e-7 for a million records): ``exact_check()`` - the
    sequential whole-file check - decides, on ``root`` only.  Every rank returns the same verdict."""
    comm = comm or LocalComm()
    if isinstance(accessions, np.ndarray) and accessions.dtype.kind == "u":
        mine = np.ascontiguousarray(accessions, dtype="<u8")        # digests already (sequence.accession_digests_of_text: one native pass)
    else:
        mine = accession_digests(list(accessions))
    local_dup = len(np.unique(mine)) != len(mine)                   # equal digests inside a share: a duplicate, or a collision
    meta = comm.allgather_i64([len(mine), int(local_dup)])
    blobs = gather_bytes(comm, mine.tobytes() if not meta[:, 1].any() else b"", root)
    ok = True
    if comm.rank == root:
        if int(meta[:, 0].sum()) == 0:
            ok = False
        elif meta[:, 1].any():
            ok = bool(exact_check())
        else:
            d = np.sort(np.concatenate([np.frombuffer(b, dtype="<u8") for b in blobs]))
            if len(d) > 1 and bool((d[1:] == d[:-1]).any()):
                ok = bool(exact_check())
    return bool(broadcast_flags(comm, [ok], root)[0])
