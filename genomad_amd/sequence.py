"""Host-side FASTA -> padded 6 kbp windows, mirroring the reference's data preparation.

Mirrors (same rules, same order, same error behaviour):
  genomad/sequence.py:96-121   read_fasta(filepath, strip_n=True)
  genomad/sequence.py:124-131  check_fasta
  genomad/sequence.py:150-167  seq_windows(seq, 6000, 2500, max_windows)
  genomad/modules/nn_classification.py:54-82  generate_data (window filter, upper-casing, ljust)
without the per-window Python objects and the TFRecord round trip: a contig is turned into rows of
one (n_windows, 6000) uint8 array with numpy slicing.  Tokenising and everything after it happens
on the GPU (libgenomad_nn_hip.so).
"""
import bz2
from fractions import Fraction
import gzip
import lzma
import sys
from pathlib import Path
from typing import Iterator, List, Tuple

import numpy as np

WINDOW = 6000
MIN_TAIL = 2500
MAX_N = 4000


def compression_of(path) -> str:
    """Magic-byte sniffing, genomad/utils.py:126-149: 'gzip' | 'bzip2' | 'xz' | 'zstd' | 'uncompressed'."""
    with open(path, "rb") as fin:
        sig = fin.read(8)
    if sig[:2] == b"\x1f\x8b":
        return "gzip"
    if sig[:3] == b"\x42\x5a\x68":
        return "bzip2"
    if sig[:7] == b"\xfd\x37\x7a\x58\x5a\x00\x00":
        return "xz"
    if sig[:4] == b"\x28\xb5\x2f\xfd":
        return "zstd"
    return "uncompressed"


def open_text(path):
    """genomad/utils.py:152-168 (zstd only on Python >= 3.14, like the reference)."""
    kind = compression_of(path)
    if kind == "gzip":
        return gzip.open(path, "rt")
    if kind == "bzip2":
        return bz2.open(path, "rt")
    if kind == "xz":
        return lzma.open(path, "rt")
    if kind == "zstd" and sys.version_info >= (3, 14):
        from compression import zstd  # type: ignore
        return zstd.open(path, "rt")
    return open(path, "r")


def read_fasta(path, strip_n: bool = False) -> Iterator[Tuple[str, str]]:
    """Yield (header, sequence).  Text before the first '>' is skipped, only the trailing newline
    of every line is removed, ``strip_n`` strips leading/trailing n/N, empty records are dropped."""
    with open_text(path) as fin:
        header, chunks = None, []

        def flush():
            s = "".join(chunks)
            if strip_n:
                s = s.strip("nN")
            return s

        for line in fin:
            if line[0] == ">":
                if header is not None:
                    s = flush()
                    if len(s):
                        yield header, s
                header, chunks = line.removesuffix("\n")[1:], []
            elif header is not None:
                chunks.append(line.removesuffix("\n"))
        if header is not None:
            s = flush()
            if len(s):
                yield header, s


def accession(header: str) -> str:
    return header.split()[0]   # genomad/sequence.py:24-25


def check_fasta_py(path) -> bool:
    """False if the file has no record or two records share an accession (sequence.py:124-131)."""
    acc = [accession(h) for h, _ in read_fasta(path)]
    return bool(acc) and len(acc) == len(set(acc))


def check_fasta(path, chunk_bytes: int = 256 << 20) -> bool:
    """:func:`check_fasta_py` with the line loop done by the library's packer in index mode, over
    record-aligned chunks of the (decompressed) text: host memory is bounded by one chunk plus the set of
    accessions, like the reference's line-by-line read (sequence.py:124-131)."""
    seen, n = set(), 0
    for chunk in iter_text_chunks(path, chunk_bytes):
        acc, _, _ = _pack(chunk, strip_n=False, copy=False)
        n += len(acc)
        seen.update(acc)
        if len(seen) != n:
            return False
    return n > 0


def _decode_header(raw: bytes) -> str:
    """Header bytes -> str.  The reference reads the file in text mode with the locale's encoding (UTF-8 in
    practice, utils.py:152-168), so non-ASCII header text is legal; ``surrogateescape`` keeps undecodable
    bytes round-trippable instead of raising on one rank of a multi-rank run."""
    return raw.decode("utf-8", "surrogateescape")


def window_spans(length: int, single_window: bool = False) -> List[Tuple[int, int]]:
    """seq_windows(seq, 6000, 2500, max_windows=1 if single_window else None) as (start, end)."""
    spans, win = [], 0
    while win * WINDOW < length:
        a, b = win * WINDOW, min((win + 1) * WINDOW, length)
        if b - a < MIN_TAIL:
            if win == 0:
                spans.append((a, b))
            break
        spans.append((a, b))
        win += 1
        if single_window and win == 1:
            break
    return spans


def contig_windows(seq: str, single_window: bool = False) -> np.ndarray:
    """(n, 6000) uint8: the windows generate_data keeps for one contig, upper-cased, 'N'-padded.

    The skip rule counts literal upper-case 'N' on the RAW sequence (Sequence.count,
    sequence.py:38-39) and never applies to window 0 (nn_classification.py:70-71).
    """
    raw = np.frombuffer(seq.encode("ascii"), dtype=np.uint8)
    spans = window_spans(len(raw), single_window)
    keep = [(a, b) for i, (a, b) in enumerate(spans)
            if i == 0 or int(np.count_nonzero(raw[a:b] == 78)) <= MAX_N]
    out = np.full((len(keep), WINDOW), 78, dtype=np.uint8)
    if keep:
        up = np.frombuffer(seq.upper().encode("ascii"), dtype=np.uint8)
        for i, (a, b) in enumerate(keep):
            out[i, :b - a] = up[a:b]
    return out


def encode_fasta(path, single_window: bool = False):
    """(contig_names, contig_ids, windows) like generate_data (nn_classification.py:54-82): names are
    accessions of the records that survive strip_n, ids index into them, one id per kept window."""
    names, ids, wins = [], [], []
    for cid, (header, seq) in enumerate(read_fasta(path, strip_n=True)):
        names.append(accession(header))
        w = contig_windows(seq, single_window)
        wins.append(w)
        ids.extend([cid] * len(w))
    windows = np.concatenate(wins) if wins else np.zeros((0, WINDOW), dtype=np.uint8)
    return np.array(names), np.array(ids, dtype=np.int64), windows


def _read_text_bytes(path) -> bytes:
    """Whole file as bytes, decompressed (utils.py:126-171 magic-byte sniffing), newlines normalised
    the way the reference's text-mode read does (universal newlines)."""
    kind = compression_of(path)
    opener = {"gzip": gzip.open, "bzip2": bz2.open, "xz": lzma.open}.get(kind)
    if kind == "zstd" and sys.version_info >= (3, 14):
        from compression import zstd  # type: ignore
        opener = zstd.open
    with (opener(path, "rb") if opener else open(path, "rb")) as fin:
        data = fin.read()
    if b"\r" in data:
        data = data.replace(b"\r\n", b"\n").replace(b"\r", b"\n")
    return data


def read_fasta_packed_py(path, strip_n: bool = True):
    """Pure-Python/numpy form of :func:`read_fasta_packed` (the readable specification the native
    packer is tested against; ≈ 0.2 GB/s)."""
    data = _read_text_bytes(path)
    records = (b"\n" + data).split(b"\n>")[1:]            # text before the first header line is dropped
    names, chunks, lengths = [], [], []
    for rec in records:
        header, _, body = rec.partition(b"\n")
        s = body.replace(b"\n", b"")
        if strip_n:
            s = s.strip(b"nN")
        if len(s):
            names.append(accession(_decode_header(header)))
            chunks.append(s)
            lengths.append(len(s))
    offsets = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(np.asarray(lengths, dtype=np.int64), out=offsets[1:])
    seq = np.frombuffer(b"".join(chunks), dtype=np.uint8) if chunks else np.zeros(0, dtype=np.uint8)
    return np.array(names), seq, offsets


def record_aligned_range(path, rank: int, world: int, piece: int = 0, pieces: int = 1) -> Tuple[int, int]:
    """Half-open byte range of ``rank``'s share of an UNCOMPRESSED FASTA file, aligned to record
    starts: both ends are moved forward to the next line that begins with '>' (a record belongs to
    the rank whose nominal range contains its '>').  Ranges of consecutive ranks tile the file, so
    every rank can read and pack only its own part (contigs shard embarrassingly).  Rank 0 starts
    at 0: text before the first header is dropped by the packer anyway.  ``piece``/``pieces`` cut a
    rank's share further the same way (used to pack piece k+1 while the GPU classifies piece k)."""
    if world < 1 or not (0 <= rank < world) or pieces < 1 or not (0 <= piece < pieces):
        raise ValueError("bad shard arguments")
    size = Path(path).stat().st_size
    rank, world = rank * pieces + piece, world * pieces

    def align(a: int) -> int:
        if a <= 0:
            return 0
        if a >= size:
            return size
        with open(path, "rb") as fin:
            pos = a - 1                                   # "\n>" may straddle the nominal boundary
            while pos < size:
                fin.seek(pos)
                block = fin.read(1 << 20)
                if not block:
                    break
                k = block.find(b"\n>")
                if k >= 0:
                    return pos + k + 1
                if len(block) < 2:                        # the last byte cannot start a "\n>" pair
                    break
                pos += len(block) - 1                     # keep one byte of overlap
        return size

    return align(size * rank // world), align(size * (rank + 1) // world)


def _read_text_array(path, byte_range=None) -> np.ndarray:
    """Writable uint8 array with the decompressed file contents (no newline normalisation);
    ``byte_range`` (uncompressed files only) reads just [start, end)."""
    kind = compression_of(path)
    opener = {"gzip": gzip.open, "bzip2": bz2.open, "xz": lzma.open}.get(kind)
    if kind == "zstd" and sys.version_info >= (3, 14):
        from compression import zstd  # type: ignore
        opener = zstd.open
    if opener is None:
        start, end = byte_range if byte_range is not None else (0, Path(path).stat().st_size)
        size = max(end - start, 0)
        buf = bytearray(size)
        with open(path, "rb", buffering=0) as fin:
            fin.seek(start)
            got, view = 0, memoryview(buf)
            while got < size:
                k = fin.readinto(view[got:])
                if not k:
                    break
                got += k
        return np.frombuffer(buf, dtype=np.uint8)[:got]
    if byte_range is not None:
        raise ValueError("byte ranges need an uncompressed file")
    with opener(path, "rb") as fin:
        return np.frombuffer(bytearray(fin.read()), dtype=np.uint8)


def _open_binary(path):
    kind = compression_of(path)
    opener = {"gzip": gzip.open, "bzip2": bz2.open, "xz": lzma.open}.get(kind)
    if kind == "zstd" and sys.version_info >= (3, 14):
        from compression import zstd  # type: ignore
        opener = zstd.open
    return opener(path, "rb") if opener else open(path, "rb")


def iter_text_chunks(path, chunk_bytes: int = 128 << 20):
    """The decompressed file as writable uint8 arrays of about ``chunk_bytes``, each cut at a record start
    (a line beginning with '>'), so that every chunk can be packed on its own and the chunks tile the
    file.  A record longer than a chunk simply makes that chunk longer."""
    with _open_binary(path) as fin:
        carry = []                       # blocks of a record that is longer than one read: joined ONCE, when it ends
        while True:
            block = fin.read(chunk_bytes)
            if not block:
                break
            # the record start may straddle two reads ("\n" ends one block, ">" starts the next)
            cut = block.rfind(b"\n>")
            if cut < 0 and carry and carry[-1].endswith(b"\n") and block.startswith(b">"):
                yield np.frombuffer(bytearray(b"".join(carry)), dtype=np.uint8)
                carry = [block]
                continue
            if cut < 0:
                carry.append(block)
                continue
            carry.append(block[:cut + 1])
            yield np.frombuffer(bytearray(b"".join(carry)), dtype=np.uint8)
            carry = [block[cut + 1:]]
        if carry and any(carry):
            yield np.frombuffer(bytearray(b"".join(carry)), dtype=np.uint8)


def index_accessions(text: np.ndarray):
    """Accessions of ALL records of a text array (no N stripping: what check_fasta counts), without consuming it."""
    acc, _, _ = _pack(text, strip_n=False, copy=False)
    return acc


def _digest_of_accession(acc: str) -> int:
    """Python mirror of gnn_fasta_accession_digests' hash (FNV-1a 64 of the accession's bytes + the splitmix64 mixer)."""
    h, m = 0xcbf29ce484222325, (1 << 64) - 1
    for b in acc.encode("utf-8", "surrogateescape"):
        h = ((h ^ b) * 0x100000001b3) & m
    h ^= h >> 30
    h = (h * 0xbf58476d1ce4e5b9) & m
    h ^= h >> 27
    h = (h * 0x94d049bb133111eb) & m
    return h ^ (h >> 31)


def accession_digests_of_text(text: np.ndarray) -> np.ndarray:
    """uint64 digests of the accessions of ALL records of a text array with a non-empty raw sequence (what check_fasta counts,
    genomad/sequence.py:124-131), without consuming it: one native pass (``gnn_fasta_accession_digests``).  A text with a
    non-ASCII byte inside a first header token (Python's ``split()`` knows non-ASCII white space) takes the Python route -
    the same digests, computed from :func:`index_accessions`."""
    import ctypes as C
    from . import _lib
    lib = _lib.load()
    nh, hb, cr = C.c_int64(), C.c_int64(), C.c_int()
    _lib.check(lib.gnn_fasta_scan(text.ctypes.data, len(text), C.byref(nh), C.byref(hb), C.byref(cr)))
    if not cr.value:
        out = np.empty(max(nh.value, 1), dtype="<u8")
        nrec, odd = C.c_int64(), C.c_int()
        _lib.check(lib.gnn_fasta_accession_digests(text.ctypes.data, len(text), out.ctypes.data, nh.value, C.byref(nrec), C.byref(odd)))
        if not odd.value:
            return out[:nrec.value].copy()
    return np.array([_digest_of_accession(a) for a in index_accessions(text)], dtype="<u8")


def pack_text(text: np.ndarray, strip_n: bool = True):
    """(names, seq, offsets) of the records in a writable text array (consumed: packed in place)."""
    names, seq, offsets = _pack(text, strip_n)
    return (np.array(names) if names else np.zeros(0, dtype="<U1")), seq, offsets


def _pack(text: np.ndarray, strip_n: bool, copy: bool = True):
    """Run gnn_fasta_scan / gnn_fasta_pack over a writable text array.  copy=True packs IN PLACE
    (``text`` is consumed) and returns (names, seq view, offsets); copy=False is the index mode."""
    import ctypes as C
    from . import _lib
    lib = _lib.load()
    nh, hb, cr = C.c_int64(), C.c_int64(), C.c_int()
    _lib.check(lib.gnn_fasta_scan(text.ctypes.data, len(text), C.byref(nh), C.byref(hb), C.byref(cr)))
    if cr.value:        # universal newlines, as the reference's text-mode read (utils.py:152-168); rare
        text = np.frombuffer(bytearray(text.tobytes().replace(b"\r\n", b"\n").replace(b"\r", b"\n")), dtype=np.uint8)
        _lib.check(lib.gnn_fasta_scan(text.ctypes.data, len(text), C.byref(nh), C.byref(hb), C.byref(cr)))
    cap = nh.value
    offsets = np.zeros(cap + 1, dtype=np.int64)
    hoff = np.zeros(cap + 1, dtype=np.int64)
    headers = np.empty(max(hb.value, 1), dtype=np.uint8)
    nrec = C.c_int64()
    _lib.check(lib.gnn_fasta_pack(text.ctypes.data, len(text), int(bool(strip_n)), text.ctypes.data if copy else None,
                                  offsets.ctypes.data, headers.ctypes.data, hoff.ctypes.data, cap, C.byref(nrec)))
    k = nrec.value
    offsets = offsets[:k + 1].copy()
    hraw = headers.tobytes()
    names = [accession(_decode_header(hraw[hoff[i]:hoff[i + 1]])) for i in range(k)]
    return names, (text[:offsets[-1]] if copy else None), offsets


def read_fasta_packed(path, strip_n: bool = True, byte_range=None):
    """(names, seq, offsets): every record that ``read_fasta(path, strip_n)`` yields, packed into ONE
    uint8 buffer of raw (case-preserved) sequence bytes; contig i is seq[offsets[i]:offsets[i+1]].

    Same record rules as :func:`read_fasta` (header = a line starting with '>', only '\\n' is
    removed, leading/trailing n/N stripped, empty records dropped); the line work is done by the
    library's host-side packer (``gnn_fasta_pack``: memchr/memmove, IN PLACE in the buffer the file
    was read into, several GB/s) so that real inputs keep up with the device.  ``byte_range`` (from
    :func:`record_aligned_range`) restricts the read to one rank's share of an uncompressed file.
    """
    names, seq, offsets = _pack(_read_text_array(path, byte_range), strip_n)
    return (np.array(names) if names else np.zeros(0, dtype="<U1")), seq, offsets


def candidate_spans(offsets: np.ndarray, single_window: bool = False):
    """Vectorised seq_windows(seq, 6000, 2500, max_windows) over all contigs (sequence.py:150-167):
    returns (starts int64, lens int32, contig_ids int64, window_n int32) of every candidate window,
    before the N-content rule."""
    lengths = np.diff(offsets)
    nfull, rem = lengths // WINDOW, lengths % WINDOW
    nwin = nfull + (rem >= MIN_TAIL)
    nwin = np.where((lengths > 0) & (nwin == 0), 1, nwin)          # window 0 is always yielded
    if single_window:
        nwin = np.minimum(nwin, 1)
    ids = np.repeat(np.arange(len(lengths), dtype=np.int64), nwin)
    first = np.cumsum(nwin) - nwin
    window_n = (np.arange(int(nwin.sum()), dtype=np.int64) - np.repeat(first, nwin)).astype(np.int32)
    starts = offsets[:-1][ids] + window_n.astype(np.int64) * WINDOW
    lens = np.minimum(WINDOW, offsets[1:][ids] - starts).astype(np.int32)
    return starts, lens, ids, window_n


def scan_spans(offsets: np.ndarray, stride: int, single_window: bool = False):
    """The window rule of a scan (``gnn_scan_plan`` / ``gnn_scan_contigs``), vectorised over all contigs: windows of 6000 bases
    starting every ``stride`` bases (1 <= stride <= 6000).  Window 0 of a non-empty contig always exists; window k > 0 exists
    while no earlier window reached the contig's end and it is at least 2500 long - so with k* = max(0, ceil((L - 6000) / stride))
    a contig of length L has k* + (k* == 0 or L - k* * stride >= 2500) windows, and only the last can be shorter than 6000.  Bins
    are stride wide: ceil(L / stride) per contig.  Returns (starts int64 - positions in the packed buffer, as
    :func:`candidate_spans`; the contig-relative start is window_n * stride -, lens int32, contig_ids int64, window_n int32,
    win_offsets int64 (n_contigs + 1), bin_offsets int64 (n_contigs + 1)).  At stride 6000 the first four are candidate_spans."""
    stride = int(stride)
    if not 1 <= stride <= WINDOW:
        raise ValueError(f"stride {stride} is outside [1, {WINDOW}]")
    offsets = np.asarray(offsets, dtype=np.int64)
    lengths = np.diff(offsets)
    if len(lengths) and int(lengths.min()) < 0:
        raise ValueError("contig offsets are not non-decreasing")
    kstar = np.maximum(0, -(-(lengths - WINDOW) // stride))
    nwin = kstar + ((kstar == 0) | (lengths - kstar * stride >= MIN_TAIL))
    nwin = np.where(lengths > 0, nwin, 0)
    if single_window:
        nwin = np.minimum(nwin, 1)
    win_offsets = np.concatenate([[0], np.cumsum(nwin)]).astype(np.int64)
    bin_offsets = np.concatenate([[0], np.cumsum(-(-lengths // stride))]).astype(np.int64)
    ids = np.repeat(np.arange(len(lengths), dtype=np.int64), nwin)
    window_n = (np.arange(int(win_offsets[-1]), dtype=np.int64) - win_offsets[:-1][ids]).astype(np.int32)
    starts = offsets[:-1][ids] + window_n.astype(np.int64) * stride
    lens = np.minimum(WINDOW, offsets[1:][ids] - starts).astype(np.int32)
    return starts, lens, ids, window_n, win_offsets, bin_offsets


def materialize_spans(seq: np.ndarray, starts, lens) -> np.ndarray:
    """(n, 6000) uint8: the spans seq[start : start + len] upper-cased and right-padded with 'N' - what the device front end
    materialises for every window (nn_classification.py:72: seq_window.seq_ascii.ljust(6000, b"N")), in numpy."""
    out = np.full((len(starts), WINDOW), ord("N"), dtype=np.uint8)
    for i, (a, l) in enumerate(zip(starts, lens)):
        w = np.asarray(seq[int(a):int(a) + int(l)], dtype=np.uint8)
        out[i, :len(w)] = np.where((w >= 97) & (w <= 122), w - 32, w)
    return out


STRANDS = ("forward", "reverse", "both")              # gnn_strand: GNN_STRAND_FORWARD = 0, _REVERSE = 1, _BOTH = 2
_COMPLEMENT = np.arange(256, dtype=np.uint8)
_COMPLEMENT[[ord(c) for c in "ACGT"]] = [ord(c) for c in "TGCA"]


def revcomp_spans(seq: np.ndarray, starts, lens) -> np.ndarray:
    """(n, 6000) uint8: the REVERSE windows of the spans seq[start : start + len] (``gnn_revcomp_spans_dev``, in numpy):
    out[i] = comp(upper(seq[start + len - 1 - i])) for i < len and 'N' for len <= i < 6000 - right-padded like the forward window
    of :func:`materialize_spans`; the pad is not reversed to the front.  comp: A <-> T, C <-> G, every other byte unchanged.  The
    tokenizer maps any non-ACGT byte to token 0 on either strand, so an IUPAC-exact complement table would change no score."""
    fwd = materialize_spans(seq, starts, lens)
    out = np.full_like(fwd, ord("N"))
    for i, l in enumerate(lens):
        out[i, :int(l)] = _COMPLEMENT[fwd[i, :int(l)][::-1]]
    return out


def strand_mean(f, r) -> np.ndarray:
    """The window score under strand mode ``both``: (f + r) * 0.5 per class in float32 - one float32 addition (the only rounding)
    and an exact halving, what the device's split kernel computes."""
    f, r = np.asarray(f, dtype=np.float32), np.asarray(r, dtype=np.float32)
    return (f + r) * np.float32(0.5)


def occlude_spans(seq: np.ndarray, starts, lens, lo, hi) -> np.ndarray:
    """(n, 6000) uint8: the OCCLUDED windows of the spans seq[start : start + len] (``gnn_occlude_spans_dev``, in numpy): the forward
    window of :func:`materialize_spans` with the window-relative interval [lo, hi) set to 'N'.  0 <= lo <= hi <= 6000; an empty
    interval gives the forward window, an interval that reaches into the pad changes nothing there."""
    out = materialize_spans(seq, starts, lens)
    for i, (a, b) in enumerate(zip(lo, hi)):
        a, b = int(a), int(b)
        if not 0 <= a <= b <= WINDOW:
            raise ValueError(f"span {i} has the interval [{a}, {b}): 0 <= lo <= hi <= {WINDOW} is required")
        out[i, a:b] = ord("N")
    return out


def occlusion_blocks(lens, block: int):
    """The (window, block) pairs of an occlusion map (``gnn_occlusion_plan`` / ``gnn_occlude_contigs``): window i of length lens[i]
    has ceil(lens[i] / block) blocks, block j is the window-relative interval [j * block, min((j + 1) * block, lens[i])); the pad is
    never a block.  Pairs run in window order, then block order.  Returns (blk_offsets int64 (n_windows + 1) - the CSR of the pairs
    over the windows -, owner int64 (n_pairs: the pair's window), lo int32, hi int32 (n_pairs))."""
    block = int(block)
    if not 1 <= block <= WINDOW:
        raise ValueError(f"block {block} is outside [1, {WINDOW}]")
    lens = np.asarray(lens, dtype=np.int64)
    nb = -(-lens // block)
    blk_offsets = np.concatenate([[0], np.cumsum(nb)]).astype(np.int64)
    owner = np.repeat(np.arange(len(lens), dtype=np.int64), nb)
    j = np.arange(int(blk_offsets[-1]), dtype=np.int64) - blk_offsets[:-1][owner]
    lo = j * block
    hi = np.minimum(lo + block, lens[owner])
    return blk_offsets, owner, lo.astype(np.int32), hi.astype(np.int32)


def scan_track(scores, kept, lens, win_offsets, bin_offsets, stride: int):
    """The track of a scan, spelled out (the definition ``gnn_scan_contigs`` folds on the device; readable, not fast): bin b of a
    contig is [b * stride, (b + 1) * stride); window k covers it iff k <= b and b * stride < k * stride + lens[k].  track[b] = the
    float32 sum, in increasing k, of the scores of the KEPT windows covering b, divided once by their number cover[b]; NaN where
    cover[b] == 0.  Returns (track (n_bins, 3) float32, cover (n_bins,) int32)."""
    scores = np.asarray(scores, dtype=np.float32).reshape(-1, 3)
    stride = int(stride)
    n_bins = int(bin_offsets[-1])
    track = np.full((n_bins, 3), np.nan, dtype=np.float32)
    cover = np.zeros(n_bins, dtype=np.int32)
    for c in range(len(win_offsets) - 1):
        w0, nw = int(win_offsets[c]), int(win_offsets[c + 1] - win_offsets[c])
        for b in range(int(bin_offsets[c + 1] - bin_offsets[c])):
            s, n = np.zeros(3, dtype=np.float32), 0
            for k in range(max(0, b - (WINDOW - 1) // stride), min(b, nw - 1) + 1):
                if b * stride < k * stride + int(lens[w0 + k]) and kept[w0 + k]:
                    s = s + scores[w0 + k]                       # float32 + float32: the device's sequential sum
                    n += 1
            if n:
                track[int(bin_offsets[c]) + b] = s / np.float32(n)
                cover[int(bin_offsets[c]) + b] = n
    return track, cover


REGION_Q_ONE = 1 << 20                    # the integer a score of 1.0 becomes (gnn_regions.hip)
REGION_PENALTY_MAX = 4096.0
REGION_FIELDS = ("contig", "lo", "hi", "state", "evidence", "qsum")


def region_penalty(penalty) -> int:
    """P = rint(penalty * 2^20) (ties to even), the switch penalty in the integer units of the emissions; 0 <= penalty <= 4096."""
    p = float(penalty)
    if not 0.0 <= p <= REGION_PENALTY_MAX:             # a NaN fails both comparisons
        raise ValueError(f"penalty {penalty!r} is outside [0, {REGION_PENALTY_MAX:g}]")
    return int(np.rint(np.float64(p) * REGION_Q_ONE))


def region_emissions(track):
    """(q int64 (n_bins, 3), evidence bool (n_bins,)) of a track: a bin is an evidence bin iff its three values are finite; its
    q = rint(min(max(v, 0), 1) * 2^20) - the float32 product with a power of two is exact, the rounding is to nearest, ties to
    even; every other bin has q = 0."""
    t = np.asarray(track, dtype=np.float32).reshape(-1, 3)
    evidence = np.isfinite(t).all(axis=1)
    with np.errstate(invalid="ignore"):
        q = np.rint(np.minimum(np.maximum(t, np.float32(0)), np.float32(1)) * np.float32(REGION_Q_ONE))
    return np.where(evidence[:, None], q, 0).astype(np.int64), evidence


def call_regions(track, bin_offsets, penalty):
    """Region calls along contigs, spelled out (the definition ``gnn_call_regions`` computes on the device; readable, not fast):
    one 3-state Viterbi path per contig over the integer emissions of :func:`region_emissions`, with a switch costing
    P = :func:`region_penalty`.  d[0][s] = q[0][s]; d[b][s] = q[b][s] + max(d[b-1][s], max_{s' != s} d[b-1][s'] - P); the back
    pointer stays on a tie and otherwise names the lowest s' attaining the maximum; the last bin takes the lowest s with maximal
    d, and the path follows the back pointers.  Python integers throughout: exact.  A region is a maximal run of equal states
    within one contig.  ``track`` (n_bins, 3) and ``bin_offsets`` (n_contigs + 1) are those of a scan; bins below bin_offsets[0]
    belong to no contig and keep state 0.  Returns (state uint8 (n_bins,), regions): ``regions`` is a dict of ``contig``, ``lo``,
    ``hi`` (int64; contig-relative bins, half-open), ``state`` (uint8), ``evidence`` (int64: evidence bins in the region) and
    ``qsum`` (int64 (n_regions, 3): the sum of q over the region), ordered by contig, then position."""
    P = region_penalty(penalty)
    off = np.asarray(bin_offsets, dtype=np.int64)
    if off.ndim != 1 or len(off) < 1:
        raise ValueError("bin_offsets must hold n_contigs + 1 offsets")
    if int(off[0]) < 0:
        raise ValueError(f"the first bin offset {int(off[0])} is negative")
    if len(off) > 1 and int(np.diff(off).min()) < 0:
        raise ValueError("bin offsets are not non-decreasing")
    q, evidence = region_emissions(track)
    if len(q) != int(off[-1]):
        raise ValueError(f"the track has {len(q)} bins, bin_offsets end at {int(off[-1])}")
    state = np.zeros(len(q), dtype=np.uint8)
    out = {k: [] for k in REGION_FIELDS}
    for c in range(len(off) - 1):
        a, n = int(off[c]), int(off[c + 1] - off[c])
        if n == 0:
            continue
        d = [int(v) for v in q[a]]
        psi = np.zeros((n, 3), dtype=np.uint8)
        for b in range(1, n):
            nxt = []
            for s in range(3):
                o1, o2 = (t for t in range(3) if t != s)
                best = o1 if d[o1] >= d[o2] else o2                  # the lowest s' attaining the maximum
                if d[s] >= d[best] - P:                               # a tie stays
                    psi[b, s] = s
                    nxt.append(int(q[a + b, s]) + d[s])
                else:
                    psi[b, s] = best
                    nxt.append(int(q[a + b, s]) + d[best] - P)
            d = nxt
        s = d.index(max(d))                                           # the lowest s with maximal d
        for b in range(n - 1, -1, -1):
            state[a + b] = s
            s = int(psi[b, s])
        st = state[a:a + n]
        lo = np.concatenate([[0], np.flatnonzero(st[1:] != st[:-1]) + 1])
        hi = np.concatenate([lo[1:], [n]])
        for l, h in zip(lo, hi):
            out["contig"].append(c), out["lo"].append(l), out["hi"].append(h), out["state"].append(st[l])
            out["evidence"].append(int(evidence[a + l:a + h].sum()))
            out["qsum"].append(q[a + l:a + h].sum(axis=0))
    regions = {k: np.asarray(out[k], dtype=np.uint8 if k == "state" else np.int64) for k in REGION_FIELDS}
    regions["qsum"] = regions["qsum"].reshape(-1, 3)
    return state, regions


def region_table(regions, offsets, stride: int):
    """What a reader of regions wants, derived from the exact fields of :func:`call_regions`: ``start`` = lo * stride and ``end`` =
    min(hi * stride, L) (int64: 0-based half-open bases within the contig of length L = diff(offsets)), ``mean`` (n_regions, 3)
    float64 = qsum / (evidence * 2^20), NaN where evidence == 0, and ``margin`` float64 = (qsum[state] - the larger of the other
    two) / 2^20: by how many bins' worth of score the called class leads.  Returns a dict of the four."""
    lengths = np.diff(np.asarray(offsets, dtype=np.int64))
    stride = int(stride)
    contig, qsum = np.asarray(regions["contig"], np.int64), np.asarray(regions["qsum"], np.int64).reshape(-1, 3)
    state, ev = np.asarray(regions["state"], np.int64), np.asarray(regions["evidence"], np.int64)
    start = np.asarray(regions["lo"], np.int64) * stride
    end = np.minimum(np.asarray(regions["hi"], np.int64) * stride, lengths[contig])
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(ev[:, None] > 0, qsum / (ev[:, None] * float(REGION_Q_ONE)), np.nan)
    rows = np.arange(len(state))
    others = qsum.copy()
    others[rows, state] = np.iinfo(np.int64).min
    margin = (qsum[rows, state] - others.max(axis=1)) / float(REGION_Q_ONE) if len(state) else np.zeros(0)
    return {"start": start, "end": end, "mean": mean.reshape(-1, 3), "margin": np.asarray(margin, dtype=np.float64)}


def interval_windows(offsets, stride: int, iv_contig, iv_start, iv_end, single_window: bool = False):
    """The member windows of intervals of contigs (``gnn_interval_plan``, in numpy).  Intervals are triples (contig, start, end),
    0-based half-open bases within the contig, 0 <= start <= end <= L, sorted by (contig, start) and pairwise disjoint within a
    contig; gaps and empty intervals are allowed, anything else is a ValueError naming the first offending interval.  Window k of
    a contig (:func:`scan_spans` at ``stride``) has the centre base m_k = k * stride + len_k // 2 and belongs to the interval of
    its contig with start <= m_k < end, or to none.  m_k is strictly increasing in k, so the members are one range of the global
    window order.  Membership does not depend on the N rule.  Returns (w_lo, w_hi) int64 (n_intervals,): members [w_lo, w_hi)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    _, lens, _, window_n, win_offsets, _ = scan_spans(offsets, stride, single_window)
    centre = window_n.astype(np.int64) * int(stride) + lens.astype(np.int64) // 2
    contig, start, end = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (iv_contig, iv_start, iv_end))
    if not len(contig) == len(start) == len(end):
        raise ValueError("iv_contig, iv_start and iv_end differ in length")
    n_contigs = len(offsets) - 1
    w_lo, w_hi = np.zeros(len(contig), np.int64), np.zeros(len(contig), np.int64)
    for i, (c, s, e) in enumerate(zip(contig.tolist(), start.tolist(), end.tolist())):
        def bad(why):
            return ValueError(f"interval {i} (contig {c}, [{s}, {e})) {why}")
        if not 0 <= c < n_contigs:
            raise bad(f"names a contig outside [0, {n_contigs})")
        length = int(offsets[c + 1] - offsets[c])
        if s < 0:
            raise bad("starts below 0")
        if e < s:
            raise bad("ends before it starts")
        if e > length:
            raise bad(f"ends beyond its contig of {length} bases")
        if i > 0 and (contig[i - 1] > c or (contig[i - 1] == c and start[i - 1] > s)):
            raise bad(f"is not sorted by (contig, start): it follows contig {int(contig[i - 1])}, start {int(start[i - 1])}")
        if i > 0 and contig[i - 1] == c and end[i - 1] > s:
            raise bad(f"overlaps interval {i - 1}, which ends at {int(end[i - 1])}")
        a, b = int(win_offsets[c]), int(win_offsets[c + 1])
        w_lo[i] = a + np.searchsorted(centre[a:b], s, side="left")
        w_hi[i] = a + np.searchsorted(centre[a:b], e, side="left")
    return w_lo, w_hi


def interval_embeddings(rows, scores, kept, w_lo, w_hi, rows_rev=None):
    """Interval embeddings, spelled out (the definition ``gnn_embed_intervals`` folds on the device; readable, not fast).  ``rows``
    (n_windows, 512) float32 are the windows' encoder embeddings, ``scores`` (n_windows, 3) their scores of the strand mode (or
    None), ``kept`` the N rule's mask, [w_lo[i], w_hi[i]) the members of interval i (:func:`interval_windows`).  With e_0, e_1, ...
    the rows of an interval's KEPT members in window order:

    - ``count`` int32: their number;
    - ``embedding``: ((0 + e_0) + e_1) + ... in float32, divided once by float32(count); a zero row when count == 0;
    - ``scores``: the same sequential float32 sum and single divide over the members' scores (zeros when ``scores`` is None);
    - ``coherence`` float64 in [0, 1], the mean resultant length of the unit rows: u_i = e_i / sqrt(sum_j e_i[j]^2), a zero row
      when e_i has a non-finite element or is all zeros (in float64 the sum of squares of a finite float32 row neither overflows
      nor vanishes: every other row has a unit row, whatever its scale); coherence = |u_0 + u_1 + ...| / count, 0 when count == 0 - evaluated in float64.

    ``rows_rev`` (the reverse windows' rows) selects strand mode ``both``: two independent sums, embedding = (S_f + S_r) /
    float32(2 count) and coherence = |U_f + U_r| / (2 count); ``scores`` are then the combined window scores
    (:func:`strand_mean`).  Returns a dict of ``count``, ``embedding``, ``scores`` and ``coherence``."""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, NEIGHBOUR_DIM)
    strands = [rows] if rows_rev is None else [rows, np.asarray(rows_rev, dtype=np.float32).reshape(-1, NEIGHBOUR_DIM)]
    if scores is not None:
        scores = np.asarray(scores, dtype=np.float32).reshape(-1, 3)
    kept = np.asarray(kept).astype(bool)
    n = len(w_lo)
    out = {"count": np.zeros(n, np.int32), "embedding": np.zeros((n, NEIGHBOUR_DIM), np.float32),
           "scores": np.zeros((n, 3), np.float32), "coherence": np.zeros(n, np.float64)}
    for i in range(n):
        members = [k for k in range(int(w_lo[i]), int(w_hi[i])) if kept[k]]
        if not members:
            continue
        S = np.zeros(NEIGHBOUR_DIM, np.float32)
        U = np.zeros(NEIGHBOUR_DIM, np.float64)
        sc = np.zeros(3, np.float32)
        for strand, r in enumerate(strands):
            s = np.zeros(NEIGHBOUR_DIM, np.float32)
            for k in members:
                with np.errstate(over="ignore", invalid="ignore"):
                    s = s + r[k]                                  # float32 + float32: the device's sequential sum
                    n2 = np.square(r[k].astype(np.float64)).sum()
                if n2 > 0 and np.isfinite(n2):
                    U += r[k].astype(np.float64) / np.sqrt(n2)
            S = s if strand == 0 else S + s
        for k in members:
            if scores is not None:
                sc = sc + scores[k]
        count = len(members)
        out["count"][i] = count
        with np.errstate(over="ignore", invalid="ignore"):
            out["embedding"][i] = S / np.float32(len(strands) * count)
        out["scores"][i] = sc / np.float32(count)
        out["coherence"][i] = np.sqrt(np.square(U).sum()) / (len(strands) * count)
    return out


NEIGHBOUR_DIM = 512                       # GNN_EMBED_DIM: the rows are encoder embeddings
NEIGHBOUR_K_MAX = 64
NEIGHBOUR_METRICS = ("cosine", "dot")


def neighbour_rows(rows, what="query") -> np.ndarray:
    """(n, 512) float32, C-contiguous: the rows of a neighbour search as the device takes them."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    if rows.ndim != 2 or rows.shape[1] != NEIGHBOUR_DIM:
        raise ValueError(f"{what} has the shape {rows.shape}: (n, {NEIGHBOUR_DIM}) rows are required")
    return rows


def neighbour_k(k) -> int:
    k = int(k)
    if not 1 <= k <= NEIGHBOUR_K_MAX:
        raise ValueError(f"k {k} is outside [1, {NEIGHBOUR_K_MAX}]")
    return k


def neighbour_metric(metric) -> str:
    if metric not in NEIGHBOUR_METRICS:
        raise ValueError(f"metric {metric!r}: expected one of {NEIGHBOUR_METRICS}")
    return metric


def _row_rule(r32, metric):
    """(r float64 (n, 512), ok bool (n,)): the row rule of every definition below, stated in :func:`nearest_neighbours`.  A row is
    valid iff every element is finite and, under ``cosine``, its norm is > 0; ``r`` holds zeros where the row is not valid, unit
    vectors under ``cosine`` and the rows themselves under ``dot``."""
    ok = np.isfinite(r32).all(axis=1)
    r = np.where(ok[:, None], r32, 0).astype(np.float64)
    if metric == "cosine":
        norm = np.sqrt((r * r).sum(axis=1))
        ok &= norm > 0
        r = r / np.where(ok, norm, 1.0)[:, None]
    return r, ok


def _namer(names):
    """i -> the int i where ``names`` is None, otherwise the str ``names[i]``: how every ``*_table`` names a row or a class"""
    return (lambda i: int(i)) if names is None else (lambda i: str(names[int(i)]))


def nearest_neighbours(query, base=None, k=10, metric="cosine"):
    """Nearest neighbours among encoder embeddings, spelled out (the definition ``gnn_neighbours`` computes on the device; float64
    throughout, readable, not fast).  ``query`` (nq, 512) and ``base`` (nb, 512) are float32 rows; ``base=None`` is the self-search:
    base = query and the pair (i, i) is excluded.  A row is valid iff every element is finite and, under ``cosine``, its norm is
    > 0 (a contig without a kept window has a zero row); an invalid query gets no neighbours, an invalid base row is nobody's.
    ``cosine``: x.y / (|x| |y|); ``dot``: x.y, under which a zero row is valid.  Returns (idx int64 (nq, k), sim float32 (nq, k)),
    each row ordered by (similarity descending, base index ascending) and padded with idx = -1, sim = NaN where fewer than k
    candidates exist.  1 <= k <= 64."""
    k = neighbour_k(k)
    neighbour_metric(metric)
    q32 = neighbour_rows(query)
    self_search = base is None
    b32 = q32 if self_search else neighbour_rows(base, "base")
    q, q_ok = _row_rule(q32, metric)
    b, b_ok = (q, q_ok) if self_search else _row_rule(b32, metric)
    idx = np.full((len(q), k), -1, dtype=np.int64)
    sim = np.full((len(q), k), np.nan, dtype=np.float32)
    cand = np.flatnonzero(b_ok)
    for i in np.flatnonzero(q_ok):
        c = cand[cand != i] if self_search else cand
        s = b[c] @ q[i]
        order = np.lexsort((c, -s))[:k]                  # similarity descending, then base index ascending
        idx[i, :len(order)] = c[order]
        sim[i, :len(order)] = s[order]
    return idx, sim


CLUSTER_FIELDS = ("label", "degree", "size", "rep")


def cluster_threshold(threshold) -> np.float32:
    """The threshold as the device compares it: the float32 it rounds to; it must be finite (before and after the rounding)."""
    try:
        with np.errstate(over="ignore"):
            t = np.float32(threshold)
    except (TypeError, ValueError):
        raise ValueError(f"threshold {threshold!r}: a finite float is required") from None
    if not np.isfinite(t):
        raise ValueError(f"threshold {threshold!r}: a finite float is required")
    return t


def threshold_clusters(rows, threshold, metric="cosine"):
    """Clusters among encoder embeddings, spelled out (the definition ``gnn_cluster`` computes on the device; float64 throughout,
    readable, not fast, n x n).  ``rows`` (n, 512) float32; validity and ``metric`` as in :func:`nearest_neighbours`.  There is an
    edge {i, j}, i != j, iff both rows are valid and sim(i, j) >= the float32 ``threshold`` rounds to; clusters are the connected
    components (single linkage at the threshold), a valid row without an edge a cluster of one.  Returns four int64 arrays of n:
    ``label`` (the smallest index of the row's cluster), ``degree`` (edges at the row), ``size`` (rows of its cluster) and ``rep``
    (the member of its cluster with the largest degree, ties to the smallest index); an invalid row has -1, 0, 0, -1."""
    neighbour_metric(metric)
    r32 = neighbour_rows(rows, "rows")
    thr = float(cluster_threshold(threshold))
    n = len(r32)
    r, ok = _row_rule(r32, metric)
    adj = (r @ r.T >= thr) & ok[:, None] & ok[None, :]
    adj |= adj.T                        # x.y and y.x may differ in the last bit of a float64 sum: an edge either way is an edge
    adj[np.arange(n), np.arange(n)] = False
    label = np.full(n, -1, dtype=np.int64)
    degree = adj.sum(axis=1).astype(np.int64)
    size = np.zeros(n, dtype=np.int64)
    rep = np.full(n, -1, dtype=np.int64)
    for i in np.flatnonzero(ok):        # ascending: the first unlabelled row of a component is its smallest
        if label[i] >= 0:
            continue
        members, stack = [i], [i]
        label[i] = i
        while stack:
            for j in np.flatnonzero(adj[stack.pop()] & (label < 0)):
                label[j] = i
                members.append(j)
                stack.append(j)
        members = np.sort(np.asarray(members, dtype=np.int64))
        size[members] = len(members)
        rep[members] = members[np.argmax(degree[members])]        # argmax: the first = the smallest index among equals
    return label, degree, size, rep


def threshold_graph(rows, threshold, metric="cosine"):
    """The similarity graph among encoder embeddings, spelled out (the definition ``gnn_graph_count`` / ``gnn_graph_fill`` compute on
    the device; float64 throughout, readable, not fast, n x n): the edges :func:`threshold_clusters` joins, kept.  ``rows`` (n, 512)
    float32; validity, ``metric`` and the threshold as there, and the same adjacency - an edge {i, j} iff both rows are valid and
    sim(i, j) or sim(j, i) >= the float32 ``threshold`` rounds to.  Returns the upper triangle in CSR form: ``indptr`` (int64, n + 1),
    ``col`` (int32: row i owns ``col[indptr[i]:indptr[i + 1]]``, its partners j > i in ascending order; an invalid row owns nothing)
    and ``sim`` (float64: r[i] . r[j])."""
    neighbour_metric(metric)
    r32 = neighbour_rows(rows, "rows")
    thr = float(cluster_threshold(threshold))
    r, ok = _row_rule(r32, metric)
    s = r @ r.T
    adj = (s >= thr) & ok[:, None] & ok[None, :]
    adj |= adj.T                        # as threshold_clusters: an edge either way is an edge
    upper = np.triu(adj, 1)
    a, b = np.nonzero(upper)            # row-major: rows in order, a row's columns ascending
    indptr = np.concatenate([[0], np.cumsum(upper.sum(axis=1))]).astype(np.int64)
    return indptr, b.astype(np.int32), s[a, b].astype(np.float64)


def valid_rows(rows, metric="cosine") -> np.ndarray:
    """bool (n,): the rows a search over encoder embeddings takes part with - every element finite and, under ``cosine``, a norm
    > 0 (:func:`nearest_neighbours`)"""
    neighbour_metric(metric)
    return _row_rule(neighbour_rows(rows, "rows"), metric)[1]


def graph_edges(indptr, col):
    """(a, b) int64 of an upper-triangle CSR: edge e joins rows a[e] < b[e], in the CSR's order"""
    indptr = np.asarray(indptr, dtype=np.int64)
    a = np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr))
    return a, np.asarray(col, dtype=np.int64)


def graph_degree(indptr, col) -> np.ndarray:
    """int64 (n,): the edges at every row, both ends counted - the ``degree`` of :func:`threshold_clusters`"""
    a, b = graph_edges(indptr, col)
    n = len(indptr) - 1
    return (np.bincount(a, minlength=n) + np.bincount(b, minlength=n)).astype(np.int64)


def graph_symmetric(indptr, col, sim):
    """The full CSR of an upper-triangle one: (indptr int64, col int32, sim) with every edge at both its rows, a row's partners
    ascending."""
    a, b = graph_edges(indptr, col)
    n = len(indptr) - 1
    sim = np.asarray(sim)
    src, dst = np.concatenate([a, b]), np.concatenate([b, a])
    order = np.lexsort((dst, src))
    full = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))]).astype(np.int64)
    return full, dst[order].astype(np.int32), np.concatenate([sim, sim])[order]


def _find(root, x):
    """The root of x in the union-find ``root`` - a list over the rows 0 .. n - 1 (a dict where the nodes are other keys), every
    entry its own root at the start -, with path halving"""
    while root[x] != x:                 # ends: a link points to a smaller index
        root[x] = root[root[x]]
        x = root[x]
    return x


def _join(root, x, y) -> bool:
    """Joins the components of x and y, the larger root linked to the smaller - a root is its component's smallest member -, and
    says whether they were two."""
    x, y = _find(root, x), _find(root, y)
    root[max(x, y)] = min(x, y)
    return x != y


def _root_labels(root, valid) -> np.ndarray:
    """int64 (n,): the smallest member of every row's component in the union-find ``root``, -1 where ``valid`` is false"""
    label = np.fromiter((_find(root, i) for i in range(len(root))), dtype=np.int64, count=len(root))
    return np.where(np.asarray(valid, dtype=bool), label, -1)


def graph_components(indptr, col, valid) -> np.ndarray:
    """int64 (n,): the smallest index of every row's connected component, -1 where ``valid`` is false - the ``label`` of
    :func:`threshold_clusters`.  A union-find whose links point to the smaller index, edge by edge."""
    a, b = graph_edges(indptr, col)
    root = list(range(len(indptr) - 1))
    for u, v in zip(a.tolist(), b.tolist()):
        _join(root, u, v)
    return _root_labels(root, valid)


def graph_table(indptr, col, sim, names=None):
    """One record per edge of an upper-triangle CSR, in its order: ``a`` < ``b`` (indices; the names where ``names`` is given) and
    ``sim``."""
    a, b = graph_edges(indptr, col)
    name = _namer(names)
    return [{"a": name(i), "b": name(j), "sim": float(s)} for i, j, s in zip(a, b, np.asarray(sim))]


def threshold_matches(query, base, threshold, metric="cosine"):
    """Matches against a reference, spelled out (the definition ``gnn_match_count`` / ``gnn_match_fill`` compute on the device; float64
    throughout, readable, not fast, nq x nb): the bipartite similarity graph between two sets of encoder embeddings.  ``query``
    (nq, 512) and ``base`` (nb, 512) are float32 rows; validity, ``metric`` and the threshold are those of :func:`threshold_graph`.
    The pair (i, j) is a match iff query row i and base row j are valid and sim(i, j) = q[i] . b[j] >= the float32 ``threshold``
    rounds to.  No pair is excluded: where query and base are the same rows, (i, i) and both orientations are there.  Returns the CSR
    by query row: ``indptr`` (int64, nq + 1), ``col`` (int32: query i owns ``col[indptr[i]:indptr[i + 1]]``, its base partners in
    ascending order; an invalid query owns nothing, an invalid base row is nobody's partner) and ``sim`` (float64)."""
    neighbour_metric(metric)
    q32, b32 = neighbour_rows(query), neighbour_rows(base, "base")
    thr = float(cluster_threshold(threshold))
    (q, q_ok), (b, b_ok) = _row_rule(q32, metric), _row_rule(b32, metric)
    s = q @ b.T
    hit = (s >= thr) & q_ok[:, None] & b_ok[None, :]
    i, j = np.nonzero(hit)              # row-major: queries in order, a query's partners ascending
    indptr = np.concatenate([[0], np.cumsum(hit.sum(axis=1))]).astype(np.int64)
    return indptr, j.astype(np.int32), s[i, j].astype(np.float64)


def match_best(indptr, col, sim):
    """(idx int64 (nq,), sim (nq,)) of a match CSR: every query's partner with the largest ``sim``, ties to the smaller index; -1 / NaN
    where it has none - ``nearest_neighbours(query, base, 1)`` wherever that similarity reaches the threshold."""
    a, b = graph_edges(indptr, col)
    sim = np.asarray(sim)
    nq = len(indptr) - 1
    order = np.lexsort((b, -sim, a))    # by query, then similarity descending, then base index ascending: segments stay in place
    idx = np.full(nq, -1, dtype=np.int64)
    best = np.full(nq, np.nan, dtype=sim.dtype if sim.dtype.kind == "f" else np.float64)
    has = np.flatnonzero(np.diff(np.asarray(indptr, dtype=np.int64)) > 0)
    first = order[np.asarray(indptr, dtype=np.int64)[has]]
    idx[has] = b[first]
    best[has] = sim[first]
    return idx, best


def match_transpose(indptr, col, sim, n_base):
    """The CSR by base row of a match CSR: (indptr int64 (n_base + 1,), col int32 - the queries that matched the base row, ascending -,
    sim: the same values, the pair's orientation unchanged)."""
    a, b = graph_edges(indptr, col)
    n_base = int(n_base)
    if len(b) and int(b.max()) >= n_base:
        raise ValueError(f"a partner is base row {int(b.max())}, beyond the {n_base} base rows")
    order = np.lexsort((a, b))
    t_ptr = np.concatenate([[0], np.cumsum(np.bincount(b, minlength=n_base))]).astype(np.int64)
    return t_ptr, a[order].astype(np.int32), np.asarray(sim)[order]


def match_table(indptr, col, sim, query_names=None, base_names=None):
    """One record per match of a match CSR, in its order: ``query`` and ``base`` (indices; the names where given) and ``sim``."""
    a, b = graph_edges(indptr, col)
    qn, bn = _namer(query_names), _namer(base_names)
    return [{"query": qn(i), "base": bn(j), "sim": float(s)} for i, j, s in zip(a, b, np.asarray(sim))]


VOTE_FIELDS = ("count", "weight", "nearest", "nearest_sim")
VOTE_CLASSES_MAX = 1024
VOTE_BASE_MAX = 1 << 30                   # kmeans' N_MAX: |rint(s * 2^32)| <= 2^32 + 2^10, so the int64 sums of 2^30 voters cannot overflow
VOTE_UNIT = float(1 << 32)                # ``weight`` counts similarity in units of 2^-32
VOTE_RULES = ("weight", "count", "nearest")


def vote_classes(n_classes) -> int:
    return _whole(n_classes, "n_classes", 1, VOTE_CLASSES_MAX)


def vote_labels(label, n_rows, n_classes) -> np.ndarray:
    """``label`` as the int64 (n_rows,) the device takes: one integer in [-1, n_classes) per base row"""
    label = np.asarray(label)
    if label.shape != (n_rows,) or label.dtype.kind not in "iu":
        raise ValueError(f"label has the shape {label.shape} and the type {label.dtype}: one integer per base row ({n_rows}) is required")
    label = np.ascontiguousarray(label, dtype=np.int64)
    if len(label) and (label.min() < -1 or label.max() >= n_classes):
        raise ValueError(f"a label is outside [-1, {n_classes})")
    return label


def class_votes(query, base, label, n_classes, threshold, sims=None):
    """Label transfer among encoder embeddings, spelled out (the definition ``gnn_vote`` computes on the device; float64 where it
    matters, readable, not fast, nq x nb).  Cosine only.  ``query`` (nq, 512) and ``base`` (nb, 512) are float32 rows whose validity
    is that of :func:`nearest_neighbours` under cosine; ``label`` is one int64 per base row: a value in [0, ``n_classes``) makes a
    valid row a voter, -1 means unlabelled (the row is ignored), anything else is a ValueError.  ``threshold`` is a finite float,
    compared as the float32 it rounds to with >= (:func:`cluster_threshold`).  ``base=None`` is the self form: the rows vote among
    themselves, ``label`` runs over them and the pair (i, i) is left out - leave-one-out.

    Per valid query i and class c, over the voters j of class c with s_ij >= threshold: ``count[i][c]`` (int64) - how many;
    ``weight[i][c]`` (int64) - the sum of rint(float64(s_ij) * 2^32), the similarity sum in units of 2^-32 (the product by a power
    of two is exact, rint rounds half to even as the device's llrint does, and |s| <= 1 + 2^-22 keeps 2^30 voters from overflowing);
    ``nearest[i][c]`` (int64) and ``nearest_sim[i][c]`` (float32) - the most similar such voter, ties to the smaller index, -1 / NaN
    where the class has none.  An invalid query has 0 / 0 / -1 / NaN in every class.

    ``sims``: a (nq, nb) array to take s_ij from instead of the float64 cosines - the device's own float32 values give the
    device's integers bit for bit.  Returns (count, weight, nearest, nearest_sim), each (nq, n_classes)."""
    n_classes = vote_classes(n_classes)
    thr = float(cluster_threshold(threshold))
    q32 = neighbour_rows(query)
    self_form = base is None
    b32 = q32 if self_form else neighbour_rows(base, "base")
    if len(b32) > VOTE_BASE_MAX:
        raise ValueError(f"{len(b32)} base rows is outside [0, 2^30]")
    label = vote_labels(label, len(b32), n_classes)
    q, q_ok = _row_rule(q32, "cosine")
    b, b_ok = (q, q_ok) if self_form else _row_rule(b32, "cosine")
    s = q @ b.T if sims is None else np.asarray(sims, dtype=np.float64)
    if s.shape != (len(q32), len(b32)):
        raise ValueError(f"sims has the shape {s.shape}: ({len(q32)}, {len(b32)}) is required")
    with np.errstate(invalid="ignore"):
        vote = (s >= thr) & q_ok[:, None] & (b_ok & (label >= 0))[None, :]
    if self_form:
        vote[np.arange(len(q32)), np.arange(len(q32))] = False
    units = np.rint(np.where(vote, s, 0.0) * VOTE_UNIT).astype(np.int64)
    shape = (len(q32), n_classes)
    count, weight = np.zeros(shape, dtype=np.int64), np.zeros(shape, dtype=np.int64)
    nearest, nearest_sim = np.full(shape, -1, dtype=np.int64), np.full(shape, np.nan, dtype=np.float32)
    for c in range(n_classes):
        cols = np.flatnonzero(label == c)
        if not len(cols):
            continue
        v = vote[:, cols]
        count[:, c] = v.sum(axis=1)
        weight[:, c] = units[:, cols].sum(axis=1)
        masked = np.where(v, s[:, cols], -np.inf)
        best = np.argmax(masked, axis=1)                # argmax: the first = the smaller index among equals
        has = v.any(axis=1)
        nearest[has, c] = cols[best[has]]
        nearest_sim[has, c] = masked[has, best[has]]
    return count, weight, nearest, nearest_sim


def vote_predict(count, weight, rule="weight", nearest_sim=None, min_votes=1):
    """One label per query from the arrays of :func:`class_votes` (numpy only).  ``rule``: the statistic whose argmax over the classes
    is the label - ``weight`` (the similarity sum), ``count`` (the voters) or ``nearest`` (the similarity of the most similar voter;
    needs ``nearest_sim``, a class without voters never wins) - ties to the smaller class.  Returns (``label`` int64: -1 where fewer
    than ``min_votes`` (>= 1) voters are within the threshold, all classes together; ``confidence`` float64: the winner's share of
    the statistic's total over the classes, from the integers - NaN under ``nearest``, where the total is not positive, and where
    there is no label; ``margin`` float64: winner minus runner-up, in similarity units for ``weight`` / ``nearest``, in votes for
    ``count``; the winner's own statistic where it is the only class with a voter; NaN where there is no label).  A share of votes
    is no calibrated probability."""
    if rule not in VOTE_RULES:
        raise ValueError(f"rule {rule!r}: expected one of {VOTE_RULES}")
    min_votes = _whole(min_votes, "min_votes", 1, 1 << 62)
    count, weight = np.asarray(count, dtype=np.int64), np.asarray(weight, dtype=np.int64)
    if count.ndim != 2 or weight.shape != count.shape:
        raise ValueError(f"count {count.shape} and weight {weight.shape}: two (n_query, n_classes) arrays are required")
    nq, nc = count.shape
    voted = count > 0
    if rule == "nearest":
        if nearest_sim is None or np.shape(nearest_sim) != count.shape:
            raise ValueError("rule 'nearest' needs nearest_sim of count's shape")
        stat = np.where(voted, np.asarray(nearest_sim, dtype=np.float64), -np.inf)
        unit = 1.0
    else:
        stat = np.where(voted, (weight if rule == "weight" else count).astype(np.float64), -np.inf)
        unit = VOTE_UNIT if rule == "weight" else 1.0
    label = np.full(nq, -1, dtype=np.int64)
    confidence, margin = np.full(nq, np.nan), np.full(nq, np.nan)
    if nc == 0:
        return label, confidence, margin
    # the integers decide the winner under weight / count: a float64 image of an int64 may round
    key = stat if rule == "nearest" else np.where(voted, weight if rule == "weight" else count, np.iinfo(np.int64).min)
    best = np.argmax(key, axis=1)                       # argmax: the first = the smaller class among equals
    ok = count.sum(axis=1) >= min_votes
    label[ok] = best[ok]
    rows = np.flatnonzero(ok)
    top = stat[rows, best[rows]]
    rest = stat[rows].copy()
    rest[np.arange(len(rows)), best[rows]] = -np.inf
    second = rest.max(axis=1) if nc > 1 else np.full(len(rows), -np.inf)
    margin[rows] = np.where(np.isfinite(second), top - second, top) / unit
    if rule != "nearest":
        ints = weight if rule == "weight" else count
        total = ints[rows].sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            share = ints[rows, best[rows]].astype(np.float64) / total.astype(np.float64)
        confidence[rows] = np.where(total > 0, share, np.nan)
    return label, confidence, margin


def vote_table(count, weight, nearest, nearest_sim, names=None, class_names=None, base_names=None, rule="weight", min_votes=1):
    """One record per query of a :func:`class_votes` result: ``query`` (its index; its name where ``names`` is given), ``label`` (the
    class of :func:`vote_predict` under ``rule``; its name where ``class_names`` is given; None where there is none),
    ``confidence``, ``votes`` (the winner's voters), ``total_votes`` (all classes'), ``nearest`` (the winner's most similar voter;
    its name where ``base_names`` is given) and ``similarity`` (to that voter); None where there is no label."""
    label, confidence, _ = vote_predict(count, weight, rule, nearest_sim, min_votes)
    count = np.asarray(count, dtype=np.int64)
    qn, cn, bn = _namer(names), _namer(class_names), _namer(base_names)
    out = []
    for i, c in enumerate(label.tolist()):
        rec = {"query": qn(i), "label": None, "confidence": None, "votes": 0, "total_votes": int(count[i].sum()), "nearest": None,
               "similarity": None}
        if c >= 0:
            rec.update(label=cn(c), confidence=None if np.isnan(confidence[i]) else float(confidence[i]), votes=int(count[i, c]),
                       nearest=bn(nearest[i][c]), similarity=float(nearest_sim[i][c]))
        out.append(rec)
    return out


def graph_extend(old, cross, new):
    """The upper-triangle CSR of the concatenated rows [old rows; new rows] from three pieces, each an (indptr, col, sim): ``old`` =
    the graph of the old rows, ``cross`` = the matches of query = the old rows against base = the new rows, ``new`` = the graph of the
    new rows.  Row i < n_old gets its old partners followed by ``cross``'s columns + n_old; row n_old + i gets ``new``'s columns +
    n_old.  A pair's value depends on its two rows only and the pair i < j is (query i, base row j) in all three pieces: this IS the
    graph of the concatenation - for the device's pieces bit for bit -, and the old x old products are not computed again."""
    (o_ptr, o_col, o_sim), (c_ptr, c_col, c_sim), (n_ptr, n_col, n_sim) = (
        (np.asarray(p, dtype=np.int64), np.asarray(c, dtype=np.int64), np.asarray(s)) for p, c, s in (old, cross, new))
    n_old, n_new = len(o_ptr) - 1, len(n_ptr) - 1
    if len(c_ptr) - 1 != n_old:
        raise ValueError(f"the cross matches have {len(c_ptr) - 1} query rows, the old graph {n_old} rows: query = the old rows is required")
    if len(c_col) and int(c_col.max()) >= n_new:
        raise ValueError(f"the cross matches name base row {int(c_col.max())}, the new graph has {n_new} rows: base = the new rows is required")
    o_deg, c_deg = np.diff(o_ptr), np.diff(c_ptr)
    indptr = np.concatenate([[0], np.cumsum(np.concatenate([o_deg + c_deg, np.diff(n_ptr)]))]).astype(np.int64)
    col = np.empty(indptr[-1], dtype=np.int32)
    sim = np.empty(indptr[-1], dtype=np.result_type(o_sim, c_sim, n_sim))
    at_old =np.repeat(indptr[:n_old] - o_ptr[:-1], o_deg) + np.arange(len(o_col))                # the row's segment, from its start
    at_cross = np.repeat(indptr[:n_old] + o_deg - c_ptr[:-1], c_deg) + np.arange(len(c_col))      # behind the row's old partners
    at_new = indptr[n_old] + np.arange(len(n_col))
    col[at_old], sim[at_old] = o_col, o_sim
    col[at_cross], sim[at_cross] = c_col + n_old, c_sim
    col[at_new], sim[at_new] = n_col + n_old, n_sim
    return indptr, col, sim


def cluster_table(result, names=None):
    """One record per cluster of a :func:`threshold_clusters` result (the four arrays, a dict of them, or anything with them as
    attributes), ordered by label: ``label``, ``size``, ``rep``, ``members`` (their indices in ascending order; the names where
    ``names`` is given, as are then ``label`` and ``rep``) and ``edges``, the number of edges inside the cluster (half the sum of
    its degrees: size * (size - 1) / 2 for a clique, size - 1 at the least - a chain)."""
    if isinstance(result, dict):
        label, degree, size, rep = (result[k] for k in CLUSTER_FIELDS)
    elif isinstance(result, (tuple, list)):
        label, degree, size, rep = result
    else:
        label, degree, size, rep = (getattr(result, k) for k in CLUSTER_FIELDS)
    label, degree, size, rep = (np.asarray(a, dtype=np.int64) for a in (label, degree, size, rep))
    name = _namer(names)
    order = np.argsort(label, kind="stable")
    order = order[label[order] >= 0]
    out = []
    bounds = np.flatnonzero(np.diff(label[order], prepend=-1)) if len(order) else []
    for a, b in zip(bounds, list(bounds[1:]) + [len(order)]):
        members = order[a:b]
        root = int(label[members[0]])
        out.append({"label": name(root), "size": int(size[root]), "rep": name(rep[root]), "members": [name(i) for i in members],
                    "edges": int(degree[members].sum()) // 2})
    return out


DENSITY_FIELDS = ("label", "degree", "size", "anchor", "sim", "kind")
DENSITY_KINDS = ("invalid", "noise", "border", "core")          # the values of ``kind``: 0, 1, 2, 3
DENSITY_MIN_POINTS_END = 1 << 31


def density_min_points(min_points) -> int:
    """``min_points`` as an int: an integer in [1, 2^31) (a bool or a float with a fraction is a ValueError)"""
    ok = not isinstance(min_points, (bool, np.bool_))
    try:
        m = int(min_points) if ok else 0
        ok = ok and m == min_points
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok or not 1 <= m < DENSITY_MIN_POINTS_END:
        raise ValueError(f"min_points {min_points!r}: an integer in [1, 2^31) is required")
    return m


def density_clusters(rows, threshold, min_points=5, metric="cosine"):
    """Density clusters among encoder embeddings, spelled out (the definition ``gnn_density`` computes on the device; float64
    throughout, readable, not fast, n x n): DBSCAN at one (``threshold``, ``min_points``).  Rows, validity, ``metric``, the threshold
    and the adjacency are those of :func:`threshold_clusters`: an edge {i, j}, i != j, iff both rows are valid and sim(i, j) or
    sim(j, i) >= the float32 ``threshold`` rounds to.  ``degree`` is that function's.  A valid row is *core* iff degree + 1 >=
    ``min_points`` (the row counts itself, as scikit-learn's ``min_samples`` does).  Clusters are the connected components of the
    core rows under core-core edges, a cluster's ``label`` its smallest core index.  A valid row that is not core and has a core
    neighbour is a *border* row: ``anchor`` = the core neighbour with the largest similarity, ties to the smaller index; ``label`` =
    the anchor's; ``sim`` = that similarity.  A border row joins nothing.  Any other valid row is *noise*: ``label`` = ``anchor`` =
    -1.  A core row has ``anchor`` = itself and ``sim`` = NaN.  ``size`` = the rows, core and border, that carry the row's label; 0
    for noise.  ``kind``: 0 invalid, 1 noise, 2 border, 3 core.  An invalid row: -1, 0, 0, -1, NaN, 0.  The border rule looks at all
    core neighbours: unlike textbook DBSCAN, the result does not depend on a visiting order.  Returns ``label``, ``degree``, ``size``,
    ``anchor`` (int64), ``sim`` (float64) and ``kind`` (uint8), each of n."""
    neighbour_metric(metric)
    r32 = neighbour_rows(rows, "rows")
    thr = float(cluster_threshold(threshold))
    need = density_min_points(min_points)
    n = len(r32)
    r, ok = _row_rule(r32, metric)
    s = r @ r.T
    adj = (s >= thr) & ok[:, None] & ok[None, :]
    adj |= adj.T                        # as threshold_clusters: an edge either way is an edge
    adj[np.arange(n), np.arange(n)] = False
    s = np.maximum(s, s.T)              # the similarity of an edge: the larger of its two float64 sums
    degree = adj.sum(axis=1).astype(np.int64)
    core = ok & (degree + 1 >= need)
    label = np.full(n, -1, dtype=np.int64)
    size = np.zeros(n, dtype=np.int64)
    anchor = np.full(n, -1, dtype=np.int64)
    sim = np.full(n, np.nan, dtype=np.float64)
    kind = np.where(core, 3, np.where(ok, 1, 0)).astype(np.uint8)
    core_adj = adj & core[:, None] & core[None, :]
    for i in np.flatnonzero(core):      # ascending: the first unlabelled core row of a component is its smallest
        if label[i] >= 0:
            continue
        stack = [i]
        label[i] = i
        while stack:
            for j in np.flatnonzero(core_adj[stack.pop()] & (label < 0)):
                label[j] = i
                stack.append(j)
    anchor[core] = np.flatnonzero(core)
    for i in np.flatnonzero(ok & ~core):
        near = np.flatnonzero(adj[i] & core)
        if len(near):
            a = near[np.argmax(s[i, near])]       # argmax: the first = the smallest index among equals
            anchor[i], label[i], sim[i], kind[i] = a, label[a], s[i, a], 2
    labelled = label >= 0
    size[labelled] = np.bincount(label[labelled], minlength=n)[label[labelled]]
    return label, degree, size, anchor, sim, kind


def density_table(result, names=None):
    """One record per cluster of a :func:`density_clusters` result (the six arrays, a dict of them, or anything with them as
    attributes), ordered by label: ``label``, ``size``, ``cores``, ``borders`` (how many of either) and ``members`` (core and border
    rows, their indices in ascending order; the names where ``names`` is given, as is then ``label``).  Noise and invalid rows are
    in no record."""
    if isinstance(result, dict):
        arrays = [result[k] for k in DENSITY_FIELDS]
    elif isinstance(result, (tuple, list)):
        arrays = list(result)
    else:
        arrays = [getattr(result, k) for k in DENSITY_FIELDS]
    label, kind = np.asarray(arrays[0], dtype=np.int64), np.asarray(arrays[5], dtype=np.uint8)
    name = _namer(names)
    order = np.argsort(label, kind="stable")
    order = order[label[order] >= 0]
    out = []
    bounds = np.flatnonzero(np.diff(label[order], prepend=-1)) if len(order) else []
    for a, b in zip(bounds, list(bounds[1:]) + [len(order)]):
        members = order[a:b]
        out.append({"label": name(label[members[0]]), "size": len(members), "cores": int((kind[members] == 3).sum()),
                    "borders": int((kind[members] == 2).sum()), "members": [name(i) for i in members]})
    return out


REPRESENTATIVE_FIELDS = ("rep", "sim", "size", "rank")


def priority_order(weight, n) -> np.ndarray:
    """The order in which :func:`greedy_representatives` walks n rows: their indices by (``weight`` descending, index ascending);
    ``weight=None`` is the index order.  ``order[k]`` is the row of rank k.  A weight array of another length than n, or one that
    holds a value that is not finite, is a ValueError."""
    n = int(n)
    if weight is None:
        return np.arange(n, dtype=np.int64)
    try:
        w = np.asarray(weight, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"weight {weight!r}: {n} finite numbers are required") from None
    if w.shape != (n,):
        raise ValueError(f"weight has the shape {w.shape}: one value for each of the {n} rows is required")
    if not np.isfinite(w).all():
        raise ValueError(f"weight holds {int((~np.isfinite(w)).sum())} values that are not finite: finite weights are required")
    return np.argsort(-w, kind="stable").astype(np.int64)         # stable: equal weights keep the index order


def representative_rounds(edge, valid):
    """The synchronous rounds ``gnn_representatives`` runs in place of the walk, on rows in priority order: ``edge`` (n, n) bool, read
    for i < j only; ``valid`` (n,) bool.  A round looks at the states of its start: an undecided row with an edge to a smaller-rank
    row that became a representative in the previous round turns member; otherwise an undecided row with no edge to a smaller-rank
    undecided row turns representative; otherwise it stays undecided.  Returns (is_rep bool (n,), rounds): the rounds until no row is
    undecided.  The undecided row of smallest rank is decided in every round, so at most n rounds run."""
    valid = np.asarray(valid, dtype=bool)
    n = len(valid)
    up = np.triu(np.asarray(edge, dtype=bool).reshape(n, n), 1) & valid[:, None] & valid[None, :]
    undecided, fresh, is_rep = valid.copy(), np.zeros(n, bool), np.zeros(n, bool)
    rounds = 0
    while undecided.any():
        hit = up[fresh].any(axis=0)                      # an edge from a representative of the previous round
        wait = up[undecided].any(axis=0)                 # an edge from a smaller-rank undecided row
        member = undecided & hit
        fresh = undecided & ~hit & ~wait
        is_rep |= fresh
        undecided = undecided & ~member & ~fresh
        rounds += 1
    return is_rep, rounds


def greedy_representatives(rows, threshold, weight=None, metric="cosine"):
    """Representatives among encoder embeddings, spelled out (the definition ``gnn_representatives`` computes on the device; float64
    throughout, readable, not fast, n x n): greedy incremental clustering.  ``rows`` (n, 512) float32; validity, ``metric`` and
    ``threshold`` as in :func:`threshold_clusters`.  The valid rows are walked by rank (:func:`priority_order`: ``weight`` descending,
    index ascending).  A row becomes a representative iff no representative of smaller rank has sim >= threshold to it; otherwise
    it is a member of the representative of smaller rank with the largest similarity, ties to the smaller rank.  The similarity of a
    pair is taken once, as (smaller rank) . (larger rank).  Returns (rep, sim, size, rank, rounds): ``rep`` int64 - the row's
    representative in the caller's index space, a representative names itself, an invalid row has -1; ``sim`` float32 - a member's
    similarity to ``rep``, NaN for representatives and invalid rows; ``size`` int64 - the rows of its cluster, 0 for an invalid
    row; ``rank`` int64 - the row's place in the order; ``rounds`` - what :func:`representative_rounds` counts on this graph."""
    neighbour_metric(metric)
    r32 = neighbour_rows(rows, "rows")
    thr = float(cluster_threshold(threshold))
    n = len(r32)
    order = priority_order(weight, n)
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    r, ok = _row_rule(r32[order], metric)                # from here on index = rank
    # one pair at a time and the same sum either way round: identical rows get identical values, so a tie is a tie (a matrix
    # product may round two equal pairs differently); read for i < j only.  The sums as they are, not _pair_values' s + 0.0:
    # ``sim`` returns them, and the float32 of a sum of -0 is -0
    s = _pair_sums(r)
    edge = np.triu(s >= thr, 1) & ok[:, None] & ok[None, :]
    rep_p = np.full(n, -1, dtype=np.int64)
    sim_p = np.full(n, np.nan, dtype=np.float32)
    reps = []
    for j in np.flatnonzero(ok):                         # the walk
        near = [i for i in reps if edge[i, j]]
        if not near:
            reps.append(int(j))
            rep_p[j] = j
        else:
            best = max(near, key=lambda i: (s[i, j], -i))
            rep_p[j], sim_p[j] = best, s[best, j]
    count = np.bincount(rep_p[rep_p >= 0], minlength=n)
    size_p = np.where(rep_p >= 0, count[np.maximum(rep_p, 0)], 0).astype(np.int64)
    _, rounds = representative_rounds(edge, ok)
    rep, sim, size = np.empty(n, np.int64), np.empty(n, np.float32), np.empty(n, np.int64)
    rep[order] = np.where(rep_p >= 0, order[np.maximum(rep_p, 0)], -1)
    sim[order], size[order] = sim_p, size_p
    return rep, sim, size, rank, int(rounds)


def representative_table(result, names=None):
    """One record per cluster of a :func:`greedy_representatives` result (the tuple, a dict of its arrays, or anything with them as
    attributes), ordered by the representative's rank: ``rep``, ``size``, ``members`` (every row of the cluster by rank, so the
    representative comes first; the names where ``names`` is given, as is then ``rep``) and ``min_sim``, the smallest similarity of
    a member to the representative (None for a cluster of one)."""
    if isinstance(result, dict):
        rep, sim, size, rank = (result[k] for k in REPRESENTATIVE_FIELDS)
    elif isinstance(result, (tuple, list)):
        rep, sim, size, rank = result[:4]
    else:
        rep, sim, size, rank = (getattr(result, k) for k in REPRESENTATIVE_FIELDS)
    rep, size, rank = (np.asarray(a, dtype=np.int64) for a in (rep, size, rank))
    sim = np.asarray(sim, dtype=np.float32)
    name = _namer(names)
    by_rank = np.argsort(rank, kind="stable")
    members = {}
    for i in by_rank:
        if rep[i] >= 0:
            members.setdefault(int(rep[i]), []).append(int(i))
    out = []
    for r in by_rank:
        if rep[r] != r:
            continue
        rows_of = members[int(r)]
        sims = [float(sim[i]) for i in rows_of if i != r]
        out.append({"rep": name(r), "size": int(size[r]), "members": [name(i) for i in rows_of], "min_sim": min(sims) if sims else None})
    return out


def single_linkage_tree(rows, metric="cosine"):
    """The single-linkage tree among encoder embeddings, spelled out (the definition ``gnn_linkage`` computes on the device; float64
    throughout, readable, not fast, n x n): the maximum-similarity spanning tree of the complete graph over the valid rows - the
    dendrogram that answers :func:`threshold_clusters` at every threshold at once.  ``rows`` (n, 512) float32; validity and
    ``metric`` as in :func:`nearest_neighbours`.  The value of the pair {i, j} is taken once, for i < j; -0 counts as +0 and a pair
    whose value is NaN is no edge (the result is then a forest).  An edge is better when its value is larger, ties go to the smaller
    lo = min(i, j), then to the smaller hi = max(i, j); Kruskal walks the pairs in that order and takes an edge iff it joins two
    different components.  Returns (a, b, sim, valid): the tree's edges in that order, best first - ``a`` int64 (lo), ``b`` int64
    (hi), ``sim`` float32 (the float64 value, rounded) - and ``valid`` uint8 (n,)."""
    s, ok = _pair_values(rows, metric)                   # a tie is a tie, -0 is +0; read for i < j only
    lo, hi = np.triu_indices(len(ok), 1)
    keep = ok[lo] & ok[hi] & ~np.isnan(s[lo, hi])
    lo, hi = lo[keep], hi[keep]
    v = s[lo, hi]
    order = np.lexsort((hi, lo, -v))                     # value descending, then lo, then hi ascending
    return _kruskal(lo, hi, v, order, ok) + (ok.astype(np.uint8),)


def _kruskal(lo, hi, value, order, ok):
    """(a int64, b int64, sim float32): the pairs (lo[e], hi[e]) that Kruskal takes when it walks them in ``order`` - a pair iff
    it joins two components - with their ``value``, rounded, until the tree spans the rows of ``ok``"""
    root, a, b, sim = list(range(len(ok))), [], [], []
    want = max(int(ok.sum()) - 1, 0)
    for e in order.tolist():
        if len(a) == want:                               # the tree spans the valid rows: nothing later joins anything
            break
        if _join(root, int(lo[e]), int(hi[e])):
            a.append(lo[e])
            b.append(hi[e])
            sim.append(value[e])
    return np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64), np.asarray(sim, dtype=np.float32)


def _linkage_arrays(a, b, sim):
    a, b = np.asarray(a, dtype=np.int64).ravel(), np.asarray(b, dtype=np.int64).ravel()
    sim = np.asarray(sim, dtype=np.float32).ravel()
    if not len(a) == len(b) == len(sim):
        raise ValueError(f"a, b and sim have {len(a)}, {len(b)} and {len(sim)} entries: one of each per edge is required")
    return a, b, sim


def linkage_cut(a, b, sim, valid, threshold) -> np.ndarray:
    """The clusters of a :func:`single_linkage_tree` at ``threshold``: the rows joined by its edges with sim >= the float32 the
    threshold rounds to (a tie is an edge).  Returns int64 ``label`` (n,): the smallest index of the row's cluster, -1 for an
    invalid row - ``threshold_clusters(rows, threshold)[0]`` where the tree is that of the same values."""
    a, b, sim = _linkage_arrays(a, b, sim)
    valid = np.asarray(valid).astype(bool).ravel()
    keep = sim >= cluster_threshold(threshold)
    root = list(range(len(valid)))
    for x, y in zip(a[keep].tolist(), b[keep].tolist()):
        _join(root, x, y)
    return _root_labels(root, valid)


def linkage_cluster_counts(sim, n_valid, thresholds) -> np.ndarray:
    """Clusters (singletons included) that a cut of the tree leaves at each of ``thresholds``: n_valid - #(sim >= t), int64."""
    sim = np.asarray(sim, dtype=np.float32).ravel()
    return np.array([int(n_valid) - int((sim >= cluster_threshold(t)).sum()) for t in np.atleast_1d(thresholds)], dtype=np.int64)


def linkage_matrix(a, b, sim, n) -> np.ndarray:
    """The tree as a linkage matrix in the convention of SciPy's ``scipy.cluster.hierarchy.linkage`` (float64, (n - 1, 4)): per
    merge, best first, the ids of the two clusters merged (the smaller first), the distance 1 - sim and the new cluster's size; a
    row is cluster i, the cluster of step k is n + k.  For cosine similarities, all rows valid and a spanning tree: anything else -
    another number of edges than n - 1, an edge inside one cluster, an index outside [0, n) - is a ValueError."""
    a, b, sim = _linkage_arrays(a, b, sim)
    n = int(n)
    if n < 1 or len(a) != n - 1:
        raise ValueError(f"{len(a)} edges among {n} rows: a linkage matrix needs a spanning tree of n - 1 edges over n >= 1 valid rows")
    if len(a) and (min(a.min(), b.min()) < 0 or max(a.max(), b.max()) >= n):
        raise ValueError(f"an edge names a row outside [0, {n})")
    if np.isnan(sim).any():
        raise ValueError("an edge's similarity is not a number")
    root = list(range(n))

    def merges():
        for k, (i, j, s) in enumerate(zip(a.tolist(), b.tolist(), sim.tolist())):
            x, y = _find(root, i), _find(root, j)
            if x == y:
                raise ValueError(f"edge {k} ({i}, {j}) joins two rows of one cluster: not a tree")
            root[y] = x                                  # the edge's own orientation: x stays its cluster's slot
            yield x, y, s

    return _scipy_matrix(n, merges())


def _scipy_matrix(n, merges) -> np.ndarray:
    """The (n - 1, 4) float64 linkage matrix of SciPy's convention from n - 1 ``merges`` (x, y, sim) in their order: x and y are
    the rows that stand for the two clusters merged, x goes on to stand for the merged one.  Per merge the two clusters' ids (the
    smaller first), the distance 1 - sim and the new size; row i is cluster i, the cluster of merge k is n + k."""
    cluster, size = list(range(n)), [1] * n              # at a row that stands for a cluster: its SciPy id and its size
    z = np.zeros((n - 1, 4), dtype=np.float64)
    for k, (x, y, sim) in enumerate(merges):
        z[k] = (min(cluster[x], cluster[y]), max(cluster[x], cluster[y]), 1.0 - sim, size[x] + size[y])
        cluster[x], size[x] = n + k, size[x] + size[y]
    return z


def linkage_table(a, b, sim, n_valid, names=None):
    """One record per merge of a :func:`single_linkage_tree`, best first: ``rank`` (from 1), ``a``, ``b`` (the names where ``names``
    is given), ``sim`` and ``clusters_left``, the clusters among the valid rows once the merge is made: n_valid - rank."""
    a, b, sim = _linkage_arrays(a, b, sim)
    name = _namer(names)
    return [{"rank": k + 1, "a": name(a[k]), "b": name(b[k]), "sim": float(sim[k]), "clusters_left": int(n_valid) - k - 1}
            for k in range(len(a))]


DENSITY_TREE_MIN_POINTS_MAX = NEIGHBOUR_K_MAX + 1     # the row itself and the neighbour search's 64
HDBSCAN_FIELDS = ("label", "lambda_out", "cluster", "parent", "birth", "stability", "size", "selected")
HDBSCAN_D_MIN = 2.0 ** -24                # the floor of the distance 1 - sim: duplicates (sim = 1) get a finite lambda


def density_tree_min_points(min_points) -> int:
    """``min_points`` of the density tree as an int: an integer in [1, 65]"""
    return _whole(min_points, "min_points", 1, DENSITY_TREE_MIN_POINTS_MAX)


def _pair_values(rows, metric):
    """(s float64 (n, n), ok bool (n,)): the pair values as :func:`single_linkage_tree` forms them - one pair at a time, the same sum
    either way round, so s is symmetric to the bit - and the rows' validity"""
    neighbour_metric(metric)
    r, ok = _row_rule(neighbour_rows(rows, "rows"), metric)
    return _pair_sums(r) + 0.0, ok                       # -0 + 0 = +0


def _pair_sums(r):
    """float64 (n, n): r[i] . r[j] as one sum per pair, the same either way round - the one place these sums are formed"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([(r * r[i]).sum(axis=1) for i in range(len(r))]) if len(r) else np.zeros((0, 0))


def core_similarity(rows, min_points=5, metric="cosine"):
    """The core similarities of the density tree, spelled out (float64): for a valid row i its similarity to its
    (``min_points`` - 1)-th most similar partner among the valid rows j != i whose pair value is a number - the row counts itself,
    as in :func:`density_clusters`.  Fewer partners than that: the least similar partner there is.  ``min_points`` 1: +inf.  An
    invalid row, or a row without such a partner: NaN.  Returns (core float64 (n,), valid uint8 (n,)).  The device takes core from
    ``gnn_neighbours``' lists, whose (i -> j) value may differ in the last bit from the pair value of i < j: this definition has one
    value per pair."""
    m = density_tree_min_points(min_points)
    s, ok = _pair_values(rows, metric)
    core = np.full(len(ok), np.nan, dtype=np.float64)
    for i in np.flatnonzero(ok):
        if m == 1:
            core[i] = np.inf
            continue
        v = s[i][ok & (np.arange(len(ok)) != i)]
        v = np.sort(v[~np.isnan(v)])[::-1]
        if len(v):
            core[i] = v[min(m - 1, len(v)) - 1]
    return core, ok.astype(np.uint8)


def mutual_reachability_tree(rows, min_points=5, metric="cosine"):
    """The density-aware linkage tree among encoder embeddings, spelled out (the definition ``gnn_density_tree`` computes on the
    device; float64 throughout, readable, not fast, n x n): :func:`single_linkage_tree` over the mutual-reachability values w(i, j)
    = min(v(i, j), core_i, core_j), core from :func:`core_similarity`.  The same pairs are edges (both rows valid, v a number), the
    same strict order decides - w descending, lo ascending, hi ascending; mutual reachability makes many pairs tie exactly - and
    Kruskal takes an edge iff it joins two components.  Returns (a int64, b int64, sim float32, core float32 (n,), valid uint8 (n,)):
    the edges best first, sim = w rounded."""
    core, _ = core_similarity(rows, min_points, metric)
    s, ok = _pair_values(rows, metric)
    lo, hi = np.triu_indices(len(ok), 1)
    keep = ok[lo] & ok[hi] & ~np.isnan(s[lo, hi])
    lo, hi = lo[keep], hi[keep]
    w = np.minimum(np.minimum(s[lo, hi], core[lo]), core[hi])
    order = np.lexsort((hi, lo, -w))
    return _kruskal(lo, hi, w, order, ok) + (core.astype(np.float32), ok.astype(np.uint8))


def density_tree_cut(a, b, sim, core, valid, threshold) -> np.ndarray:
    """The clusters of a :func:`mutual_reachability_tree` at ``threshold``: the labels of the core-only form of DBSCAN at
    (threshold, min_points).  A valid row whose core >= the float32 the threshold rounds to gets the smallest index of its
    component under the tree's edges with sim >= it (an edge's sim is at most either end's core: such a component holds core rows
    only); every other row gets -1.  Where at least ``min_points`` rows are valid this is ``density_clusters(...)``'s label at the
    rows of kind 3 (with fewer, core is the least similar partner and the row would never be core there)."""
    core = np.asarray(core, dtype=np.float32).ravel()
    label = linkage_cut(a, b, sim, valid, threshold)
    if len(core) != len(label):
        raise ValueError(f"core has {len(core)} entries for {len(label)} rows")
    with np.errstate(invalid="ignore"):
        label[~(core >= cluster_threshold(threshold))] = -1
    return label


def density_tree_cluster_counts(sim, core, valid, thresholds) -> np.ndarray:
    """Clusters of core rows that :func:`density_tree_cut` leaves at each of ``thresholds``: #(core >= t) - #(sim >= t), int64."""
    sim = np.asarray(sim, dtype=np.float32).ravel()
    core = np.asarray(core, dtype=np.float32).ravel()[np.asarray(valid).astype(bool).ravel()]
    with np.errstate(invalid="ignore"):
        return np.array([int((core >= cluster_threshold(t)).sum()) - int((sim >= cluster_threshold(t)).sum())
                         for t in np.atleast_1d(thresholds)], dtype=np.int64)


def hdbscan_clusters(a, b, sim, valid, min_cluster_size=5, allow_single_cluster=False):
    """HDBSCAN's flat clusters from a :func:`mutual_reachability_tree` over cosine similarities, defined BY LEVELS, not by binary
    merges: mutual reachability makes many edges tie exactly, and nothing here depends on the order of tied edges or on which
    spanning tree was found.  The tree must span the valid rows (n_valid - 1 edges; a forest is a ValueError).
      distance   d = max(1 - float64(sim), 2^-24), lambda = 1 / d.
      levels     the distinct values of ``sim``, from small lambda to large.  At a level a current cluster falls apart into the
                 components of its members under the edges with larger sim.  Two or more components of >= ``min_cluster_size`` rows:
                 each is a new cluster born at that lambda, and the smaller components fall out as points at that lambda.  Exactly
                 one: the cluster continues in it, the rest falls out.  None: the cluster ends, all its points leave at that lambda.
      stability  S(C) = sum over the points ever in C of (lambda_p - lambda_birth(C)); lambda_p is the lambda at which p left C, by
                 falling out or by the split.  The root, all valid rows, is born at lambda = 0.
      selection  excess of mass, bottom-up: a cluster is selected when S(C) >= the summed stability selected beneath it (a tie
                 keeps the parent), which unselects everything beneath.  The root is never selected unless ``allow_single_cluster``.
      label      the smallest member index of the selected cluster from whose subtree the row left; otherwise -1.
    Returns a dict: ``label`` (int64 (n,)), ``lambda_out`` (float64 (n,): the lambda at which the row left the deepest cluster it
    was in; NaN for an invalid row) and per cluster, in the order of creation (the root first, a parent before its children),
    ``cluster`` (its smallest member), ``parent`` (the index of its parent cluster, -1), ``birth``, ``stability``, ``size`` and
    ``selected``.  ``min_cluster_size`` >= 2."""
    a, b, sim = _linkage_arrays(a, b, sim)
    valid = np.asarray(valid).astype(bool).ravel()
    n = len(valid)
    mcs = _whole(min_cluster_size, "min_cluster_size", 2, 1 << 31)
    rows_in = np.flatnonzero(valid)
    if len(a) != max(len(rows_in) - 1, 0):
        raise ValueError(f"{len(a)} edges among {len(rows_in)} valid rows: hdbscan needs a spanning tree, not a forest")
    if np.isnan(sim).any():
        raise ValueError("an edge's similarity is not a number")
    if len(a) and (min(a.min(), b.min()) < 0 or max(a.max(), b.max()) >= n or not (valid[a].all() and valid[b].all())):
        raise ValueError("an edge names a row that is not valid")
    lam_of = lambda s: 1.0 / max(1.0 - float(s), HDBSCAN_D_MIN)
    # The dendrogram by levels, bottom-up: node x < n is row x; walking the distinct values of sim downwards, every component that the
    # level's edges form becomes a node whose children are the components they joined.  kids / level / count / least per node.
    kids, level, count, least = [None] * n, [None] * n, [1] * n, list(range(n))
    root = list(range(n))
    node_at = list(range(n))                             # at a union-find root: the dendrogram node of its component
    order = np.argsort(-sim.astype(np.float64), kind="stable")
    e = 0
    while e < len(order):
        f = e
        while f < len(order) and sim[order[f]] == sim[order[e]]:
            f += 1
        touched = {}                                     # new union-find root -> the nodes joined under it at this level
        for k in order[e:f].tolist():
            x, y = _find(root, int(a[k])), _find(root, int(b[k]))
            if x == y:
                raise ValueError(f"edge {k} ({a[k]}, {b[k]}) joins two rows of one component: not a tree")
            lo, hi = min(x, y), max(x, y)                # the two roots are needed below: the link is made here, as _join makes it
            root[hi] = lo
            touched[lo] = touched.pop(lo, [node_at[lo]]) + touched.pop(hi, [node_at[hi]])
        for r, nodes in touched.items():
            kids.append(nodes)
            level.append(float(sim[order[e]]))
            count.append(sum(count[x] for x in nodes))
            least.append(min(least[x] for x in nodes))
            node_at[r] = len(kids) - 1
        e = f
    label = np.full(n, -1, dtype=np.int64)
    lambda_out = np.full(n, np.nan, dtype=np.float64)
    out = {"label": label, "lambda_out": lambda_out}
    c_least, c_parent, c_birth, c_stab, c_size = [], [], [], [], []
    deepest = np.full(n, -1, dtype=np.int64)             # the row's deepest cluster

    def leaves(x):
        stack, got = [x], []
        while stack:
            y = stack.pop()
            if kids[y] is None:
                got.append(y)
            else:
                stack.extend(kids[y])
        return got

    def new_cluster(x, parent, birth):
        for lst, v in ((c_least, least[x]), (c_parent, parent), (c_birth, birth), (c_stab, 0.0), (c_size, count[x])):
            lst.append(v)
        return len(c_least) - 1

    if len(rows_in):
        top = node_at[_find(root, int(rows_in[0]))]
        new_cluster(top, -1, 0.0)
        work = [(0, top)]                                # (cluster, the dendrogram node it lives in now)
        while work:
            c, x = work.pop()
            while True:
                if kids[x] is None:                      # a single row that is all of the root: it never leaves
                    deepest[x], lambda_out[x] = c, 0.0
                    break
                lam = lam_of(level[x])
                big = [y for y in kids[x] if count[y] >= mcs]
                stays = big[0] if len(big) == 1 else -1  # the component the cluster continues in
                for y in kids[x]:
                    if y == stays:
                        continue
                    c_stab[c] += count[y] * (lam - c_birth[c])
                    if len(big) >= 2 and count[y] >= mcs:
                        work.append((new_cluster(y, c, lam), y))
                    else:
                        for p in leaves(y):
                            deepest[p], lambda_out[p] = c, lam
                if stays < 0:
                    break
                x = stays
    nc = len(c_least)
    selected = np.zeros(nc, dtype=bool)
    beneath = np.zeros(nc, dtype=np.float64)             # the stability selected in the cluster's subtree
    child_sum = np.zeros(nc, dtype=np.float64)
    has_child = np.zeros(nc, dtype=bool)
    for c in range(nc - 1, -1, -1):                      # a child was created after its parent
        if (c > 0 or allow_single_cluster) and (not has_child[c] or c_stab[c] >= child_sum[c]):
            selected[c], beneath[c] = True, c_stab[c]
        else:
            beneath[c] = child_sum[c]
        if c_parent[c] >= 0:
            child_sum[c_parent[c]] += beneath[c]
            has_child[c_parent[c]] = True
    owner = np.full(nc, -1, dtype=np.int64)              # the topmost selected cluster at or above c
    for c in range(nc):
        up = owner[c_parent[c]] if c_parent[c] >= 0 else -1
        owner[c] = up if up >= 0 else (c if selected[c] else -1)
    for c in range(nc):
        selected[c] = owner[c] == c
    for p in rows_in:
        if deepest[p] >= 0 and owner[deepest[p]] >= 0:
            label[p] = c_least[owner[deepest[p]]]
    out.update(cluster=np.asarray(c_least, dtype=np.int64), parent=np.asarray(c_parent, dtype=np.int64),
               birth=np.asarray(c_birth, dtype=np.float64), stability=np.asarray(c_stab, dtype=np.float64),
               size=np.asarray(c_size, dtype=np.int64), selected=selected)
    return out


def hdbscan_table(result, names=None):
    """One record per selected cluster of a :func:`hdbscan_clusters` result, ordered by label: ``label``, ``size`` (the rows that
    carry the label), ``birth``, ``stability`` and ``members`` (indices ascending; the names where ``names`` is given, as is then
    ``label``)."""
    name = _namer(names)
    label = np.asarray(result["label"])
    sel = np.flatnonzero(result["selected"])
    recs = []
    for c in sel[np.argsort(np.asarray(result["cluster"])[sel], kind="stable")]:
        rows_of = np.flatnonzero(label == result["cluster"][c])
        recs.append({"label": name(result["cluster"][c]), "size": len(rows_of), "birth": float(result["birth"][c]),
                     "stability": float(result["stability"][c]), "members": [name(i) for i in rows_of]})
    return recs


KMEANS_FIELDS = ("label", "sim", "centroids", "size", "iterations", "converged", "init_rows")
KMEANS_K_MAX = 65535
KMEANS_MAX_ITER_MAX = 1000
KMEANS_MAX_ITER_DEFAULT = 50


def _whole(value, what, lo, hi) -> int:
    """``value`` as an int in [lo, hi] (a bool or a float with a fraction is a ValueError)"""
    ok = not isinstance(value, (bool, np.bool_))
    try:
        v = int(value) if ok else 0
        ok = ok and v == value
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok or not lo <= v <= hi:
        raise ValueError(f"{what} {value!r}: an integer in [{lo}, {hi}] is required")
    return v


def kmeans_k(k) -> int:
    return _whole(k, "k", 1, KMEANS_K_MAX)


def kmeans_max_iter(max_iter) -> int:
    return _whole(max_iter, "max_iter", 0, KMEANS_MAX_ITER_MAX)


def farthest_first(unit, ok, k) -> np.ndarray:
    """The farthest-first traversal of :func:`spherical_kmeans` over float64 unit rows: int64 (k,) row indices.  The first centre is
    the valid row of smallest index, every next one the valid row, not yet picked, whose largest similarity to the centres so far
    is smallest - ties to the smaller row index."""
    cand = np.flatnonzero(ok)
    picks = [int(cand[0])]
    best = unit[cand] @ unit[picks[0]]                  # per candidate: its largest similarity to a centre so far
    free = np.ones(len(cand), dtype=bool)
    free[0] = False
    while len(picks) < k:
        j = int(np.flatnonzero(free)[np.argmin(best[free])])       # argmin: the first = the smallest index among equals
        picks.append(int(cand[j]))
        free[j] = False
        best = np.maximum(best, unit[cand] @ unit[cand[j]])
    return np.asarray(picks, dtype=np.int64)


def spherical_kmeans(rows, k, init=None, max_iter=KMEANS_MAX_ITER_DEFAULT, trace=None):
    """Spherical k-means among encoder embeddings, spelled out (the definition ``gnn_kmeans`` computes on the device; float64
    throughout, readable, not fast).  ``rows`` (n, 512) float32, cosine only; the valid rows are exactly those of
    :func:`nearest_neighbours` under cosine, and an invalid row has label -1, sim NaN and contributes to nothing.  1 <= ``k`` <=
    min(valid rows, 65535); 0 <= ``max_iter`` <= 1000.

    *Assignment*: a row's label is the centroid with the largest cosine, ties to the smaller centroid index.  *Update*: centroid c
    becomes the unit vector of the sum of its members' unit rows; a centroid without members, or whose sum is exactly zero, keeps
    its previous value.  *Loop*: label = assign(centroids); stop if no label changed against the previous assignment (``converged``)
    or ``iterations`` == ``max_iter``; otherwise centroids = update(label), ``iterations`` += 1, again.  The labels returned are
    therefore always the assignment to the centroids returned; ``max_iter`` = 0 is a pure assignment to ``init``.

    ``init``: a (k, 512) array whose rows are all valid (their unit rows are the first centroids), or None - the farthest-first
    traversal of :func:`farthest_first`; no random number is drawn.  ``trace``: a list that receives, per assignment, a dict of its
    ``label``, its ``objective`` and its ``gap`` (the smallest distance between a valid row's best and second-best similarity; inf
    for k = 1).

    Returns ``label`` (int64 (n,)), ``sim`` (float32 (n,): the similarity to the row's own centroid), ``centroids`` (float32
    (k, 512), unit rows), ``size`` (int64 (k,): the members, 0 for a centroid nobody chose), ``iterations`` (int), ``converged``
    (bool) and ``init_rows`` (int64 (k,): the rows the traversal picked, -1 for a given ``init``)."""
    r32 = neighbour_rows(rows, "rows")
    k, max_iter = kmeans_k(k), kmeans_max_iter(max_iter)
    unit, ok = _row_rule(r32, "cosine")
    n, valid = len(r32), np.flatnonzero(ok)
    if k > len(valid):
        raise ValueError(f"k {k} is more than the {len(valid)} valid rows of {n}")
    if init is None:
        init_rows = farthest_first(unit, ok, k)
        centroids = unit[init_rows].copy()
    else:
        i32 = neighbour_rows(init, "init")
        centroids, i_ok = _row_rule(i32, "cosine")
        if len(i32) != k:
            raise ValueError(f"init has {len(i32)} rows: k = {k} are required")
        if not i_ok.all():
            raise ValueError(f"{int((~i_ok).sum())} of the {k} init rows are not valid (finite, norm > 0)")
        init_rows = np.full(k, -1, dtype=np.int64)
    label = np.full(n, -1, dtype=np.int64)
    sim = np.full(n, np.nan, dtype=np.float64)
    previous, iterations, converged = None, 0, False
    while True:
        s = unit[valid] @ centroids.T
        best = np.argmax(s, axis=1)                     # argmax: the first = the smaller centroid among equals
        label[valid], sim[valid] = best, s[np.arange(len(valid)), best]
        if trace is not None:
            top = np.sort(s, axis=1)[:, -2:]
            trace.append({"label": label.copy(), "objective": float(sim[valid].sum()),
                          "gap": float((top[:, 1] - top[:, 0]).min()) if k > 1 else float("inf")})
        if previous is not None and np.array_equal(label, previous):
            converged = True
            break
        if iterations == max_iter:
            break
        previous = label.copy()
        for c in range(k):
            total = unit[valid[best == c]].sum(axis=0)
            norm = np.sqrt((total * total).sum())
            if (best == c).any() and norm > 0:
                centroids[c] = total / norm
        iterations += 1
    size = np.bincount(label[valid], minlength=k).astype(np.int64)
    return label, sim.astype(np.float32), centroids.astype(np.float32), size, iterations, converged, init_rows


def group_centroids(rows, label, k):
    """One unit row per group of ``label``, spelled out (the definition ``gnn_centroids`` computes on the device; float64): the
    update of :func:`spherical_kmeans` alone, for any int64 labels in [-1, k).  ``rows`` (n, 512) float32; label -1 and invalid
    rows are skipped; centroid c is the unit vector of the sum of its members' unit rows, a zero row for a group without members
    or with a zero sum.  Returns ``centroids`` (float32 (k, 512)) and ``size`` (int64 (k,): the valid members)."""
    r32 = neighbour_rows(rows, "rows")
    k = kmeans_k(k)
    label = np.asarray(label)
    if label.shape != (len(r32),) or label.dtype.kind not in "iu":
        raise ValueError(f"label has the shape {label.shape} and the type {label.dtype}: one integer per row is required")
    label = label.astype(np.int64)
    if len(label) and (label.min() < -1 or label.max() >= k):
        raise ValueError(f"a label is outside [-1, {k})")
    unit, ok = _row_rule(r32, "cosine")
    centroids = np.zeros((k, NEIGHBOUR_DIM), dtype=np.float64)
    size = np.zeros(k, dtype=np.int64)
    for c in range(k):
        members = np.flatnonzero(ok & (label == c))
        total = unit[members].sum(axis=0)
        norm = np.sqrt((total * total).sum())
        size[c] = len(members)
        if len(members) and norm > 0:
            centroids[c] = total / norm
    return centroids.astype(np.float32), size


def kmeans_table(result, names=None):
    """One record per cluster of a :func:`spherical_kmeans` result (its tuple, a dict of its fields, or anything with them as
    attributes), by cluster index: ``cluster``, ``size``, ``mean_sim`` (the members' mean similarity to the centroid) and
    ``nearest`` (the member most similar to it, ties to the smaller index; its name where ``names`` is given); ``mean_sim`` and
    ``nearest`` are None for a cluster without members."""
    if isinstance(result, dict):
        label, sim, size = (result[f] for f in ("label", "sim", "size"))
    elif isinstance(result, (tuple, list)):
        label, sim, size = result[0], result[1], result[3]
    else:
        label, sim, size = (getattr(result, f) for f in ("label", "sim", "size"))
    label, sim = np.asarray(label, dtype=np.int64), np.asarray(sim, dtype=np.float64)
    name = _namer(names)
    out = []
    for c in range(len(size)):
        members = np.flatnonzero(label == c)
        if len(members):
            out.append({"cluster": c, "size": int(size[c]), "mean_sim": float(sim[members].mean()),
                        "nearest": name(members[np.argmax(sim[members])])})
        else:
            out.append({"cluster": c, "size": int(size[c]), "mean_sim": None, "nearest": None})
    return out


PCA_COMPONENTS_MAX = 64
PCA_ROWS_MAX = 1 << 30


def pca_components(n_components) -> int:
    return _whole(n_components, "n_components", 1, PCA_COMPONENTS_MAX)


def pca_moments(rows):
    """The second moments of the unit rows, spelled out (the definition ``gnn_pca_moments`` computes on the device in fixed point;
    float64 here).  ``rows`` (n, 512) float32; the valid rows are exactly those of :func:`nearest_neighbours` under cosine and an
    invalid row contributes nothing.  Returns ``G`` (float64 (512, 512): the sum of u uT over the valid rows' unit vectors u),
    ``S`` (float64 (512,): the sum of u) and ``n_valid`` (int)."""
    unit, ok = _row_rule(neighbour_rows(rows, "rows"), "cosine")
    return unit.T @ unit, unit.sum(axis=0), int(ok.sum())


def pca_from_moments(G, S, n_valid, n_components, center=True):
    """Principal components from the moments of :func:`pca_moments` - the product code of the 512 x 512 step, which the engine calls
    too (there is no device eigen-solver: the matrix is 2 MB whatever n is).  Float64 throughout.  C = G / n_valid - mu muT with
    mu = S / n_valid, or G / n_valid when ``center`` is false (mu is then zero); ``numpy.linalg.eigh``; components ordered by
    eigenvalue descending, each one's sign fixed so that its entry of largest magnitude is positive (ties to the smallest index).
    ``n_valid`` < 2 is a ValueError.

    Returns a dict: ``mean`` (float64 (512,)), ``components`` (float64 (c, 512), unit rows), ``explained_variance`` (float64 (c,):
    the eigenvalues, clipped at 0), ``explained_variance_ratio`` (over trace(C); NaN when that is 0) and ``total_variance``
    (trace(C))."""
    c = pca_components(n_components)
    G, S = np.asarray(G, dtype=np.float64), np.asarray(S, dtype=np.float64)
    if G.shape != (NEIGHBOUR_DIM, NEIGHBOUR_DIM) or S.shape != (NEIGHBOUR_DIM,):
        raise ValueError(f"G {G.shape} and S {S.shape}: ({NEIGHBOUR_DIM}, {NEIGHBOUR_DIM}) and ({NEIGHBOUR_DIM},) are required")
    n_valid = int(n_valid)
    if n_valid < 2:
        raise ValueError(f"{n_valid} valid rows: principal components need two at the least")
    mean = S / n_valid if center else np.zeros(NEIGHBOUR_DIM)
    C = G / n_valid - np.outer(mean, mean)
    C = (C + C.T) / 2
    w, v = np.linalg.eigh(C)
    order = np.argsort(-w, kind="stable")[:c]
    comp = v[:, order].T.copy()
    lead = np.argmax(np.abs(comp), axis=1)                 # argmax: the first = the smallest index among equals
    comp[comp[np.arange(c), lead] < 0] *= -1
    total = float(np.trace(C))
    var = np.clip(w[order], 0, None)
    return {"mean": mean, "components": comp, "explained_variance": var,
            "explained_variance_ratio": var / total if total > 0 else np.full(c, np.nan), "total_variance": total}


def pca_directions(components):
    """``components`` (c, 512) float32, 1 <= c <= 64, every row valid -> (the float32 rows, their float64 renormalisation)"""
    c32 = neighbour_rows(components, "components")
    if not 1 <= len(c32) <= PCA_COMPONENTS_MAX:
        raise ValueError(f"{len(c32)} components: 1 to {PCA_COMPONENTS_MAX} are required")
    unit, ok = _row_rule(c32, "cosine")
    if not ok.all():
        raise ValueError(f"{int((~ok).sum())} of the {len(c32)} components are not valid (finite, norm > 0)")
    return c32, unit


def pca_offsets(components, mean):
    """What :func:`pca_project` subtracts per component: mean . v in float64, v the float64 renormalisation of the float32
    component; ``mean`` None: zeros"""
    _, unit = pca_directions(components)
    if mean is None:
        return np.zeros(len(unit))
    mean = np.asarray(mean, dtype=np.float64)
    if mean.shape != (NEIGHBOUR_DIM,):
        raise ValueError(f"mean has the shape {mean.shape}: ({NEIGHBOUR_DIM},) is required")
    return unit @ mean


def pca_project(rows, components, mean=None):
    """Principal-component scores, spelled out (the definition ``gnn_pca_project`` computes on the device; float64): u_i . v_c -
    mean . v_c for the unit vector u_i of row i and the unit vector v_c of component c; NaN for an invalid row.  Returns float64
    (n, c)."""
    unit, ok = _row_rule(neighbour_rows(rows, "rows"), "cosine")
    _, v = pca_directions(components)
    out = unit @ v.T - pca_offsets(components, mean)[None, :]
    out[~ok] = np.nan
    return out


def pca_table(projection, valid, names=None):
    """One record per row of a projection: ``row`` (its index, or its name where ``names`` is given) and ``pc`` (the list of its
    scores; None for a row without a valid embedding)"""
    name = _namer(names)
    return [{"row": name(i), "pc": [float(x) for x in projection[i]] if valid[i] else None} for i in range(len(projection))]


MCL_ONE = 1 << 30                  # a column's flow sums to (a little under) this
MCL_W = 1 << 24                    # a similarity of 1 as an integer weight
MCL_SIM_END = 64.0                 # similarities are below this: weights stay below 2^30
MCL_SELECT_MAX = 1024
MCL_PRECISION_MAX = 1 << 20
MCL_MAX_ITER_MAX = 10000
MCL_N_MAX = 1 << 24
MCL_FIELDS = ("label", "size", "attractor", "flow", "is_attractor")


def mcl_inflation(inflation) -> int:
    """4 * ``inflation`` as the integer in [5, 32] the integer power is built from; anything else is a ``ValueError``: the power is
    made of floor operations alone (products, square roots, fourth roots), so the inflation is a multiple of 0.25 in [1.25, 8]."""
    try:
        a = float(inflation) * 4.0
        ok = not isinstance(inflation, (bool, np.bool_)) and a == int(a) and 5 <= a <= 32
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"inflation {inflation!r}: a multiple of 0.25 in [1.25, 8] is required")
    return int(a)


def _mcl_isqrt(x):
    """floor(sqrt(x)) of uint64 x <= 2^60: the float64 estimate is off by one at the most, integer comparisons correct it"""
    r = np.sqrt(x.astype(np.float64)).astype(np.uint64)
    r = np.where(r * r > x, r - np.uint64(1), r)
    return np.where((r + np.uint64(1)) * (r + np.uint64(1)) <= x, r + np.uint64(1), r)


def _mcl_pow(u, a):
    """u^(a / 4) in 2^-30 fixed point, u <= 2^30 (uint64): a // 4 products by u, one by its square root where a % 4 >= 2, one by its
    fourth root where a is odd; every product is floored"""
    one, sh = np.uint64(MCL_ONE), np.uint64(30)
    h = _mcl_isqrt(u * one)
    g = _mcl_isqrt(h * one)
    r = np.full(u.shape, MCL_ONE, dtype=np.uint64)
    for _ in range(a // 4):
        r = (r * u) >> sh
    if a % 4 >= 2:
        r = (r * h) >> sh
    if a % 2:
        r = (r * g) >> sh
    return r


def _mcl_segments(cj):
    """(first position of every run of the sorted ``cj``, the run every position belongs to)"""
    first = np.flatnonzero(np.concatenate([[True], cj[1:] != cj[:-1]]))
    return first, np.cumsum(np.concatenate([[0], cj[1:] != cj[:-1]]))


def _mcl_prune(cj, ci, y, select, precision):
    """``prune`` of every column at once: entries (column cj, row ci, y > 0) sorted by (cj, ci) -> (cj, ci, p) in the same order"""
    if not len(cj):
        return cj, ci, y
    first, seg = _mcl_segments(cj)
    keep = y * np.uint64(precision) >= np.add.reduceat(y, first)[seg]
    cj, ci, y = cj[keep], ci[keep], y[keep]
    if not len(cj):                                       # the cutoff kept nothing (precision below a column's equal entries)
        return cj, ci, y
    order = np.lexsort((ci, ~y, cj))                      # column, then y descending, then row ascending
    cj, ci, y = cj[order], ci[order], y[order]
    first, seg = _mcl_segments(cj)
    keep = np.arange(len(cj)) - first[seg] < select
    cj, ci, y = cj[keep], ci[keep], y[keep]
    order = np.lexsort((ci, cj))
    cj, ci, y = cj[order], ci[order], y[order]
    first, seg = _mcl_segments(cj)
    p = y * np.uint64(MCL_ONE) // np.add.reduceat(y, first)[seg]
    keep = p > 0
    return cj[keep], ci[keep], p[keep]


MCL_DENSE_ROWS = 2048              # up to this many rows the definition multiplies dense matrices; no result depends on it


def _mcl_products(n, cj, ci, p):
    """(key, e) of the matrix (cj, ci, p), sorted by (cj, ci): e_ij = sum_k p_ik * p_kj at key = j * n + i, keys ascending, zeros left
    out.  Every sum is exact.  A small matrix is multiplied densely, in float64 on 15-bit halves of p <= 2^30: a product is below
    2^31 and a sum of n <= 2048 of them below 2^53.  A large one entry by entry - (k, j) meets the entries (i, k) of column k -, the
    products added in uint64 behind a sort."""
    if n <= MCL_DENSE_ROWS:
        hi, lo = np.zeros((n, n)), np.zeros((n, n))
        hi[ci, cj], lo[ci, cj] = p >> np.uint64(15), p & np.uint64(0x7fff)
        e = (((hi @ hi).astype(np.uint64) << np.uint64(30)) + ((hi @ lo + lo @ hi).astype(np.uint64) << np.uint64(15))
             + (lo @ lo).astype(np.uint64)).T.ravel()              # [j][i]
        key = np.flatnonzero(e)
        return key, e[key]
    length = np.bincount(cj, minlength=n)
    ptr = np.concatenate([[0], np.cumsum(length)])
    cnt = length[ci]
    src = np.repeat(np.arange(len(ci)), cnt)
    pos = ptr[ci[src]] + np.arange(len(src)) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    key = cj[src] * np.int64(n) + ci[pos]
    prod = p[pos] * p[src]
    order = np.argsort(key, kind="stable")
    key, prod = key[order], prod[order]
    first = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
    return key[first], np.add.reduceat(prod, first)


def _mcl_expand(n, cj, ci, p, a, select, precision):
    """One iteration on the matrix (cj, ci, p), sorted by (cj, ci): expansion, inflation, prune."""
    if not len(cj):
        return cj, ci, p
    key, e = _mcl_products(n, cj, ci, p)
    t = e >> np.uint64(30)
    key, t = key[t > 0], t[t > 0]
    if not len(key):
        return key, key, t
    cj, ci = key // n, key % n
    first, seg = _mcl_segments(cj)
    y = _mcl_pow(t * np.uint64(MCL_ONE) // np.maximum.reduceat(t, first)[seg], a)
    return _mcl_prune(cj[y > 0], ci[y > 0], y[y > 0], select, precision)


def _mcl_changed(n, old, new) -> int:
    """the columns of the matrix ``new`` that differ from ``old``'s"""
    lo, ln = np.bincount(old[0], minlength=n), np.bincount(new[0], minlength=n)
    same = lo == ln
    a, b = same[old[0]], same[new[0]]
    diff = (old[1][a] != new[1][b]) | (old[2][a] != new[2][b])
    return int(np.count_nonzero(~same)) + len(np.unique(new[0][b][diff]))


def mcl_weights(indptr, col, sim, valid=None):
    """The integer graph Markov clustering starts from: (n, a, b, q, valid) - the edges a < b that exist, with their weights q =
    rint(float32(sim) * 2^24) > 0, and the rows' validity.  ``ValueError`` for a CSR that is none (indptr not rising from 0 to
    len(col)), a column outside (row, n), a similarity that is not finite or >= 64, more than 2^24 rows, a ``valid`` of another length."""
    indptr = np.asarray(indptr)
    col = np.asarray(col)
    if indptr.ndim != 1 or len(indptr) < 1 or indptr.dtype.kind not in "iu" or col.ndim != 1 or col.dtype.kind not in "iu":
        raise ValueError("indptr (n + 1,) and col (nnz,) must be integer arrays")
    indptr, col = indptr.astype(np.int64), col.astype(np.int64)
    n = len(indptr) - 1
    if n > MCL_N_MAX:
        raise ValueError(f"{n} rows: at most 2^24 are supported")
    s32 = np.asarray(sim)
    if s32.ndim != 1 or s32.dtype.kind != "f" or len(s32) != len(col):
        raise ValueError("sim must be a float array with one value per entry of col")
    with np.errstate(over="ignore"):
        s32 = s32.astype(np.float32)
    if indptr[0] != 0 or indptr[-1] != len(col) or (np.diff(indptr) < 0).any():
        raise ValueError("indptr does not rise from 0 to len(col)")
    a = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    if ((col <= a) | (col >= n)).any():
        raise ValueError("col: a row's entries must lie in (row, n) - the upper triangle")
    if not (np.isfinite(s32) & (s32 < MCL_SIM_END)).all():
        raise ValueError("sim: every value must be finite and below 64")
    ok = np.ones(n, dtype=bool) if valid is None else np.asarray(valid)
    if ok.shape != (n,) or ok.dtype.kind != "b":
        raise ValueError(f"valid must be a bool array of {n}")
    q = np.rint(s32.astype(np.float64) * MCL_W).astype(np.int64)
    keep = (q > 0) & ok[a] & ok[col]
    return n, a[keep], col[keep], q[keep].astype(np.uint64), ok


def mcl_initial(n, a, b, q, valid, select, precision):
    """The initial matrix (cj, ci, p): node j's column is ``prune`` of its edges' weights - parallel edges count once, with the largest
    of their weights - and its loop, the largest of them (2^24 for a node without an edge); an invalid node's column is empty."""
    key = np.concatenate([a * np.int64(n) + b, b * np.int64(n) + a])
    w = np.concatenate([q, q])
    order = np.argsort(key, kind="stable")
    key, w = key[order], w[order]
    if len(key):
        first = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
        key, w = key[first], np.maximum.reduceat(w, first)
    loop = np.full(n, MCL_W, dtype=np.uint64)
    if len(key):
        first, _ = _mcl_segments(key // n)
        loop[(key // n)[first]] = np.maximum.reduceat(w, first)
    nodes = np.flatnonzero(valid).astype(np.int64)
    key = np.concatenate([key, nodes * np.int64(n) + nodes])
    w = np.concatenate([w, loop[nodes]])
    order = np.argsort(key, kind="stable")
    key, w = key[order], w[order]
    return _mcl_prune(key // n, key % n, w, select, precision)


def mcl_interpret(n, cj, ci, p, valid):
    """(label, size, attractor, flow, is_attractor) of the matrix (cj, ci, p), sorted by (cj, ci)"""
    label = np.arange(n, dtype=np.int64)
    while True:                                           # ends: labels only fall, and stop at the component's smallest index
        low = np.minimum(label[ci], label[cj])
        nxt = label.copy()
        np.minimum.at(nxt, ci, low)
        np.minimum.at(nxt, cj, low)
        nxt = nxt[nxt]
        if np.array_equal(nxt, label):
            break
        label = nxt
    label = np.where(valid, label, -1)
    size = np.where(valid, np.bincount(label[valid], minlength=n)[np.maximum(label, 0)], 0).astype(np.int64)
    attractor = np.full(n, -1, dtype=np.int64)
    flow = np.zeros(n, dtype=np.uint32)
    is_attractor = np.zeros(n, dtype=bool)
    if len(cj):
        order = np.lexsort((ci, ~p, cj))                  # a column's largest entry first, among equals the smallest row
        first, _ = _mcl_segments(cj)
        top = order[first]
        attractor[cj[top]] = ci[top]
        flow[cj[top]] = p[top].astype(np.uint32)
        is_attractor[cj[ci == cj]] = True
    return label, size, attractor, flow, is_attractor


def markov_clusters(indptr, col, sim, valid=None, inflation=2.0, select=256, precision=10000, max_iter=100):
    """Markov clustering (van Dongen's MCL) of a similarity graph, in integers throughout (the definition ``gnn_mcl`` computes on the
    device).  The graph is an upper-triangle CSR as :func:`threshold_graph` returns it: row i owns
    ``col[indptr[i]:indptr[i + 1]]``, its partners j > i in any order, with ``sim`` (cast to float32 first); ``valid`` is a bool per
    row (None: all).  ONE = 2^30, W = 2^24; every quantity is a non-negative integer below 2^63.

    Weights: q = rint(float32(sim) * W); an edge with q <= 0 or an invalid end does not exist; an edge sits at both its ends; parallel
    edges count once, with the largest q; node j's loop is the largest q at j, W without an edge.
    prune(entries (i, y > 0)): S = sum y; keep y * precision >= S; of more than ``select`` keep the first ``select`` under (y
    descending, i ascending); S' = sum of the kept; p_i = y_i * ONE // S'; drop p = 0; ascending by i.
    Initial column of a valid node: prune(its edges' q and its loop); an invalid node's column is empty.
    One iteration, per column j from the previous matrix: e_i = sum_k p_ik * p_kj (exact); t_i = e_i >> 30, zeros dropped; u_i =
    t_i * ONE // max t; y_i = pow(u_i), zeros dropped; prune.  pow for inflation = a / 4 (:func:`mcl_inflation`): mul(x, y) = x * y
    >> 30, h = isqrt(u * ONE), g = isqrt(h * ONE); from ONE, a // 4 times mul by u, then by h if a % 4 >= 2, then by g if a is odd.
    It stops behind the first iteration that changes no column (``converged``) or behind ``max_iter`` iterations.

    Returns a dict: ``label`` (int64: the smallest index of the node's connected component in the graph {i, j : p_ij > 0} of the final
    matrix; -1 for an invalid row), ``size`` (int64: nodes of its cluster), ``attractor`` (int64: the i with the largest p_ij in column
    j, ties to the smaller i; -1 for an invalid row), ``flow`` (uint32: that p), ``is_attractor`` (bool: p_jj > 0), ``iterations``,
    ``converged``, ``changed`` (int64: the columns every iteration changed) and the final matrix as ``length`` (int64 (n,)), ``idx``
    (int32) and ``val`` (uint32): column j owns the next ``length[j]`` entries, rows ascending."""
    a4 = mcl_inflation(inflation)
    select = _whole(select, "select", 1, MCL_SELECT_MAX)
    precision = _whole(precision, "precision", 1, MCL_PRECISION_MAX)
    max_iter = _whole(max_iter, "max_iter", 0, MCL_MAX_ITER_MAX)
    n, a, b, q, ok = mcl_weights(indptr, col, sim, valid)
    m = mcl_initial(n, a, b, q, ok, select, precision)
    changed, converged = [], False
    while len(changed) < max_iter and not converged:
        nxt = _mcl_expand(n, *m, a4, select, precision)
        changed.append(_mcl_changed(n, m, nxt))
        converged = changed[-1] == 0
        m = nxt
    out = dict(zip(MCL_FIELDS, mcl_interpret(n, *m, ok)))
    out.update(iterations=len(changed), converged=converged, changed=np.asarray(changed, dtype=np.int64),
               length=np.bincount(m[0], minlength=n).astype(np.int64), idx=m[1].astype(np.int32), val=m[2].astype(np.uint32))
    return out


def mcl_table(label, size, is_attractor, names=None):
    """One record per cluster, ordered by label: ``label``, ``size``, ``members`` and ``attractors`` (the members with flow to
    themselves), as indices in ascending order or - where ``names`` is given - as names"""
    label = np.asarray(label, dtype=np.int64)
    name = _namer(names)
    order = np.argsort(label, kind="stable")
    order = order[label[order] >= 0]
    bounds = np.flatnonzero(np.diff(label[order], prepend=-1)) if len(order) else []
    out = []
    for a, b in zip(bounds, list(bounds[1:]) + [len(order)]):
        members = order[a:b]
        out.append({"label": name(label[members[0]]), "size": int(size[members[0]]), "members": [name(i) for i in members],
                    "attractors": [name(i) for i in members if is_attractor[i]]})
    return out


SPREAD_ONE = 1 << 30              # a score of 1
SPREAD_P = 1 << 31                # a row's transition mass
SPREAD_MAX_ITER_MAX = 10000
SPREAD_FIELDS = ("score", "best", "best_score", "second_score", "total", "first")


def spread_alpha(alpha) -> int:
    """64 * ``alpha`` as the integer in [1, 63] the iteration multiplies by; anything else is a ``ValueError``: the damping is a
    shift by 6 bits, so alpha is a multiple of 1/64 in (0, 1)."""
    try:
        a = float(alpha) * 64.0
        ok = not isinstance(alpha, (bool, np.bool_)) and a == int(a) and 1 <= a <= 63
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"alpha {alpha!r}: a multiple of 1/64 in (0, 1) is required")
    return int(a)


def spread_transitions(indptr, col, sim, valid=None):
    """The integer random-walk rows label spreading runs on: (n, i, j, p, valid) - every existing entry of :func:`mcl_weights` at both
    its ends (row i, partner j), sorted by i, with p_ij = (q_ij << 31) // d_i for d_i = the sum of q over the entries at row i;
    parallel entries stay apart (their p add up in every sum)."""
    n, a, b, q, ok = mcl_weights(indptr, col, sim, valid)
    i, j, q = np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([q, q])
    order = np.argsort(i, kind="stable")
    i, j, q = i[order], j[order], q[order]
    d = np.zeros(n, dtype=np.uint64)
    np.add.at(d, i, q)
    return n, i, j, (q << np.uint64(31)) // d[i] if len(i) else q, ok


def spread_step(n, i, j, p, F, base, fixed, a):
    """One synchronous iteration: F (uint64 (n, c)) -> the next F.  ``base`` = (64 - a) * ONE * y, ``fixed`` = the rows that keep
    ``fixed_value`` = their row of ONE * y (clamped seeds) or 0 (invalid rows) - given as (mask, values)."""
    g = np.zeros_like(F)
    if len(i):
        first = np.flatnonzero(np.concatenate([[True], i[1:] != i[:-1]]))
        g[i[first]] = np.add.reduceat(p[:, None] * F[j], first, axis=0)      # every sum is below 2^61
    nxt = (np.uint64(a) * (g >> np.uint64(31)) + base) >> np.uint64(6)
    nxt[fixed[0]] = fixed[1][fixed[0]]
    return nxt


def label_spread(indptr, col, sim, label, n_classes, valid=None, alpha=0.5, clamp=True, max_iter=200, trace=None):
    """Label spreading over a similarity graph, in integers throughout (the definition ``gnn_spread`` computes on the device; DESIGN.md
    section 5t): the labels of seed rows spread along the edges until nothing changes - multi-hop label transfer, where
    :func:`class_votes` crosses one edge.  The graph is the upper-triangle CSR of :func:`threshold_graph`, with ``valid`` (bool per
    row, None: all), read as :func:`markov_clusters` reads it; ``label`` is one int64 per row in [-1, ``n_classes``), -1 = unlabelled;
    1 <= ``n_classes`` <= 1024; ``alpha`` = a / 64 (:func:`spread_alpha`); ``max_iter`` in [1, 10000].  ONE = 2^30 is a score of 1.

    Weights: q = rint(float32(sim) * 2^24); an entry with q <= 0 or an invalid end does not exist; an entry sits at both its ends;
    parallel entries are added.  d_i = the sum of q at row i, p_ij = (q_ij << 31) // d_i: a row's p sum to 2^31 at the most, and with
    scores <= 2^30 a row's sum stays below 2^61 at any degree.
    Seeds: the valid rows with label >= 0; y_i[c] = 1 where label_i == c, else 0.
    Iteration (synchronous, F^0 = 0): g_i[c] = (sum_j p_ij * F_j[c]) >> 31; F'_i[c] = ONE * y_i[c] for a seed under ``clamp``, otherwise
    (a * g_i[c] + (64 - a) * ONE * y_i[c]) >> 6; an invalid row stays 0.  It stops behind the first iteration that changes no row
    (``converged``) or behind ``max_iter`` iterations.

    Why it ends: the map F -> F' is monotone - every term is a floor of a sum of products with non-negative constants, so F <= G
    entry by entry gives F' <= G' - and F^1 >= F^0 = 0, hence F^(t+1) >= F^t for every t by induction; every score is an integer in
    [0, ONE] (g <= ONE because the p of a row sum to <= 2^31, and a * ONE + (64 - a) * ONE = 64 * ONE).  A sequence of integer matrices
    that never falls and is bounded stops changing.  Nothing bounds the number of iterations short of n * n_classes * 2^30, so
    ``iterations`` and ``converged`` are outputs.  ``trace``: a list that receives every F^t (uint64 copies), t = 1, 2, ...

    Returns a dict: ``score`` (uint32 (n, n_classes), units of 2^-30), ``best`` (int32: the class of the largest score, ties to the
    smaller class; -1 where every score is 0, so for an invalid row), ``best_score`` and ``second_score`` (uint32: the largest score
    among the other classes; 0 with one class), ``total`` (uint64: the sum over the classes), ``first`` (int32: the first iteration,
    counted from 1, behind which the row's total was not 0; -1: never.  A score is floored, so mass that has become smaller than
    2^-30 on its way is 0: ``first`` can be larger than the row's hop distance from a seed, and a row far enough away stays -1),
    ``seed`` (bool: the row is a seed), ``iterations``, ``converged`` and ``changed`` (int64: the rows every iteration changed)."""
    a = spread_alpha(alpha)
    nc = vote_classes(n_classes)
    max_iter = _whole(max_iter, "max_iter", 1, SPREAD_MAX_ITER_MAX)
    n, i, j, p, ok = spread_transitions(indptr, col, sim, valid)
    label = vote_labels(label, n, nc)
    seed = ok & (label >= 0)
    y = np.zeros((n, nc), dtype=np.uint64)
    y[np.flatnonzero(seed), label[seed]] = 1
    base = np.uint64((64 - a) * SPREAD_ONE) * y
    hold = seed if clamp else np.zeros(n, dtype=bool)
    fixed = (hold | ~ok, np.uint64(SPREAD_ONE) * y)           # an invalid row is no seed: its row of y is 0
    F = np.zeros((n, nc), dtype=np.uint64)
    first = np.full(n, -1, dtype=np.int32)
    changed, converged = [], False
    while len(changed) < max_iter and not converged:
        nxt = spread_step(n, i, j, p, F, base, fixed, a)
        changed.append(int(np.count_nonzero((nxt != F).any(axis=1))))
        converged = changed[-1] == 0
        F = nxt
        first[(first < 0) & (F.sum(axis=1) > 0)] = len(changed)
        if trace is not None:
            trace.append(F.copy())
    out = spread_summary(F)
    out.update(seed=seed, iterations=len(changed), converged=converged, changed=np.asarray(changed, dtype=np.int64), first=first)
    return out


def spread_summary(score):
    """``score``, ``best``, ``best_score``, ``second_score`` and ``total`` of a score matrix, as :func:`label_spread` returns them"""
    F = np.asarray(score).astype(np.uint64)
    n, nc = F.shape
    top = np.argmax(F, axis=1) if n else np.zeros(0, dtype=np.int64)          # argmax: the first = the smallest class among equals
    best_score = F[np.arange(n), top]
    rest = F.copy()
    rest[np.arange(n), top] = 0
    return {"score": F.astype(np.uint32), "best": np.where(best_score > 0, top, -1).astype(np.int32), "best_score": best_score.astype(np.uint32),
            "second_score": (rest.max(axis=1) if nc > 1 else np.zeros(n, dtype=np.uint64)).astype(np.uint32), "total": F.sum(axis=1)}


def spread_predict(best, best_score, second_score, total, min_score=0.0):
    """One label per row from the arrays of :func:`label_spread`: (``label`` int64: ``best``, -1 where there is none or where
    ``best_score`` / 2^30 is below ``min_score``; ``confidence`` float64: ``best_score`` / ``total``; ``margin`` float64:
    (``best_score`` - ``second_score``) / ``total``; NaN where there is no label).  A share of the seed mass that reached the row, no
    calibrated probability."""
    min_score = float(min_score)
    if not 0.0 <= min_score <= 1.0:
        raise ValueError(f"min_score {min_score!r}: a float in [0, 1] is required")
    best = np.asarray(best, dtype=np.int64)
    bs, ss, tot = (np.asarray(x).astype(np.float64) for x in (best_score, second_score, total))
    has = (best >= 0) & (bs / SPREAD_ONE >= min_score)
    with np.errstate(divide="ignore", invalid="ignore"):
        confidence = np.where(has, bs / tot, np.nan)
        margin = np.where(has, (bs - ss) / tot, np.nan)
    return np.where(has, best, -1), confidence, margin


def spread_table(best, best_score, second_score, total, first, names=None, class_names=None, min_score=0.0):
    """One record per row: ``row`` (its index, or its name), ``label`` (the class, or its name; None without one), ``confidence``,
    ``score`` (``best_score`` / 2^30), ``total_score`` (``total`` / 2^30) and ``first``"""
    label, confidence, _ = spread_predict(best, best_score, second_score, total, min_score)
    name = _namer(names)
    cname = _namer(class_names)
    return [{"row": name(i), "label": cname(label[i]) if label[i] >= 0 else None, "confidence": float(confidence[i]) if label[i] >= 0 else None,
             "score": int(best_score[i]) / SPREAD_ONE, "total_score": int(total[i]) / SPREAD_ONE, "first": int(first[i])}
            for i in range(len(label))]


AVGLINK_STOP_DEFAULT = 2.0 ** -24  # stop_q = 1: every merge with a positive average
AVGLINK_MAX_ROUNDS_MAX = 1 << 20
AVGLINK_FIELDS = ("a", "b", "weight", "size_a", "size_b", "round")


def average_linkage_stop(stop) -> int:
    """``stop_q`` = rint(``stop`` * 2^24), the smallest average (in units of 2^-24) at which a pair still merges, for a float in
    (0, 64) that rounds to 1 at the least; anything else is a ``ValueError``."""
    try:
        s = float(stop)
        ok = not isinstance(stop, (bool, np.bool_)) and 0.0 < s < MCL_SIM_END
    except (TypeError, ValueError, OverflowError):
        ok = False
    q = int(np.rint(s * MCL_W)) if ok else 0
    if not 1 <= q < (1 << 30):
        raise ValueError(f"stop {stop!r}: a similarity in (0, 64) that is at least 2^-25 is required")
    return q


def _avglink_better(s1, d1, id1, s2, d2, id2) -> bool:
    """(s1 / d1, id1) comes before (s2 / d2, id2): the larger ratio, among equals the smaller id - in Python integers"""
    l, r = s1 * d2, s2 * d1
    return l > r or (l == r and id1 < id2)


def average_linkage_order(a, b, weight, size_a, size_b, round):
    """The merges of an average-linkage tree in its output order - the average ``weight / (size_a * size_b)`` descending as an exact
    rational, then ``round`` ascending, then ``a`` ascending - as the arrays of :data:`AVGLINK_FIELDS` (``a``, ``b``, ``size_a``,
    ``size_b``, ``round`` int64, ``weight`` uint64) and ``sim`` (float64: ``weight / (size_a * size_b) / 2^24``, rounded once)."""
    import functools
    m = [tuple(int(v) for v in t) for t in zip(a, b, weight, size_a, size_b, round)]

    def cmp(x, y):
        l, r = x[2] * y[3] * y[4], y[2] * x[3] * x[4]
        if l != r:
            return -1 if l > r else 1
        return -1 if (x[5], x[0]) < (y[5], y[0]) else (1 if (x[5], x[0]) > (y[5], y[0]) else 0)

    m.sort(key=functools.cmp_to_key(cmp))
    cols = list(zip(*m)) if m else [()] * 6
    out = {k: np.asarray(cols[i], dtype=np.uint64 if k == "weight" else np.int64) for i, k in enumerate(AVGLINK_FIELDS)}
    from fractions import Fraction
    out["sim"] = np.asarray([float(Fraction(w, sa * sb * MCL_W)) for _, _, w, sa, sb, _ in m], dtype=np.float64)
    return out


def average_linkage(indptr, col, sim, valid=None, stop=AVGLINK_STOP_DEFAULT, max_rounds=AVGLINK_MAX_ROUNDS_MAX):
    """Average linkage (UPGMA) over a similarity graph by rounds of reciprocal best pairs, in integers throughout (the definition
    ``gnn_avglink`` computes on the device).  The graph is the upper-triangle CSR of :func:`threshold_graph`,
    with ``valid`` (bool per row, None: all), read as :func:`markov_clusters` reads it.

    Weights: q = rint(float32(sim) * 2^24); an entry with q <= 0 or an invalid end does not exist; parallel entries are added.
    Clusters: a cluster's id is its smallest member; S(A, B) = the sum of q over the entries between A and B; the average is
    S / (|A| * |B|) - a pair of rows without an entry counts as similarity 0, so on a graph cut at a threshold the average is a lower
    bound of the true mean, and on a complete graph it is the true mean.
    A round: every live cluster A with a neighbour names best[A], the neighbour B with the largest S(A, B) / |B| (ties to the smaller
    id; S1 * |B2| against S2 * |B1| as exact integers), if S(A, B) >= stop_q * |A| * |B| (:func:`average_linkage_stop`); every pair
    with best[A] = B, best[B] = A and A < B merges - B is absorbed into A -; the rows are contracted: columns relabelled, self entries
    dropped, duplicates summed.  It stops behind the first round that merges nothing (``complete``) or behind ``max_rounds`` rounds.
    A round in which a cluster names a best merges a pair (the largest pair under average, smaller id, larger id names itself).

    Returns a dict: per merge, ordered by :func:`average_linkage_order` (children before parents), ``a`` < ``b`` (int64: the absorbing
    and the absorbed cluster), ``weight`` (uint64: S), ``size_a``, ``size_b``, ``round`` (int64, from 0) and ``sim`` (float64);
    ``valid``, ``rounds``, ``merged_per_round`` (int64), ``complete`` and ``stop`` (stop_q / 2^24)."""
    stop_q = average_linkage_stop(stop)
    max_rounds = _whole(max_rounds, "max_rounds", 1, AVGLINK_MAX_ROUNDS_MAX)
    n, ea, eb, eq, ok = mcl_weights(indptr, col, sim, valid)
    rows = {}
    for x, y, w in zip(ea.tolist(), eb.tolist(), eq.tolist()):
        rx, ry = rows.setdefault(x, {}), rows.setdefault(y, {})
        rx[y] = rx.get(y, 0) + w
        ry[x] = ry.get(x, 0) + w
    size = {i: 1 for i in rows}
    merges, merged, complete = [], [], False
    while len(merged) < max_rounds and not complete:
        best = {}
        for A, row in rows.items():
            top = None
            for B, S in row.items():
                if top is None or _avglink_better(S, size[B], B, top[1], size[top[0]], top[0]):
                    top = (B, S)
            if top is not None and top[1] >= stop_q * size[A] * size[top[0]]:
                best[A] = top
        pairs = [(A, B, S) for A, (B, S) in best.items() if A < B and B in best and best[B][0] == A]
        merged.append(len(pairs))
        complete = not pairs
        if complete:
            break
        into = {}
        for A, B, S in pairs:
            merges.append((A, B, S, size[A], size[B], len(merged) - 1))
            into[B] = A
        for A, B, _ in pairs:
            size[A] += size.pop(B)
        contracted = {}
        for A, row in rows.items():
            R = into.get(A, A)
            new = contracted.setdefault(R, {})
            for c, S in row.items():
                m = into.get(c, c)
                if m != R:
                    new[m] = new.get(m, 0) + S
        rows = contracted
    out = average_linkage_order(*zip(*merges)) if merges else average_linkage_order(*[()] * 6)
    out.update(valid=ok, rounds=len(merged), merged_per_round=np.asarray(merged, dtype=np.int64), complete=complete, stop=stop_q / MCL_W)
    return out


def average_linkage_cut(result, t) -> np.ndarray:
    """The clusters of an average-linkage tree (the dict of :func:`average_linkage`, or anything with its keys) at the similarity
    ``t``: the merges with ``weight >= t_q * size_a * size_b`` applied, in Python integers (t_q = :func:`average_linkage_stop`).
    Returns int64 ``label`` (n,): the smallest member of the row's cluster, -1 for an invalid row.  ``t`` below the tree's ``stop``
    cuts where the tree stopped."""
    t_q = average_linkage_stop(t)
    valid = np.asarray(result["valid"]).astype(bool).ravel()
    root = list(range(len(valid)))
    for a, b, w, sa, sb in zip(*(np.asarray(result[k]).tolist() for k in AVGLINK_FIELDS[:5])):
        if w >= t_q * sa * sb:
            _join(root, a, b)
    return _root_labels(root, valid)


def average_linkage_cluster_counts(result, thresholds) -> np.ndarray:
    """Clusters (singletons included) among the valid rows that :func:`average_linkage_cut` leaves at each of ``thresholds``: the
    valid rows minus the merges at or above it, int64."""
    n_valid = int(np.count_nonzero(np.asarray(result["valid"])))
    m = list(zip(*(np.asarray(result[k]).tolist() for k in ("weight", "size_a", "size_b"))))
    return np.array([n_valid - sum(1 for w, sa, sb in m if w >= average_linkage_stop(t) * sa * sb) for t in np.atleast_1d(thresholds)],
                    dtype=np.int64)


def average_linkage_matrix(result) -> np.ndarray:
    """The tree as a linkage matrix in the convention of SciPy's ``scipy.cluster.hierarchy.linkage`` (float64, (n - 1, 4)), as
    :func:`linkage_matrix` builds it: per merge, in the tree's order, the ids of the two clusters merged (the smaller first), the
    distance 1 - sim and the new cluster's size; a row is cluster i, the cluster of step k is n + k.  For all rows valid and a whole
    tree of n - 1 merges (a complete graph, or a connected one with ``stop`` at its lowest): anything else is a ValueError."""
    valid = np.asarray(result["valid"]).astype(bool).ravel()
    n = len(valid)
    a, b, sim = np.asarray(result["a"]).tolist(), np.asarray(result["b"]).tolist(), np.asarray(result["sim"], dtype=np.float64)
    if n < 1 or not valid.all() or len(a) != n - 1:
        raise ValueError(f"{len(a)} merges among {n} rows, {int(valid.sum())} of them valid: a linkage matrix needs n - 1 merges over n >= 1 "
                         "valid rows")
    return _scipy_matrix(n, zip(a, b, sim.tolist()))     # a absorbs b: a cluster's id, its smallest member, stands for it


def average_linkage_table(result, names=None):
    """One record per merge of an average-linkage tree, best first: ``rank`` (from 1), ``a``, ``b`` (the names where ``names`` is
    given), ``sim``, ``size`` (of the merged cluster), ``round`` and ``clusters_left`` among the valid rows once the merge is made."""
    n_valid = int(np.count_nonzero(np.asarray(result["valid"])))
    name = _namer(names)
    cols = [np.asarray(result[k]).tolist() for k in ("a", "b", "sim", "size_a", "size_b", "round")]
    return [{"rank": k + 1, "a": name(a), "b": name(b), "sim": float(s), "size": int(sa + sb), "round": int(r), "clusters_left": n_valid - k - 1}
            for k, (a, b, s, sa, sb, r) in enumerate(zip(*cols))]


COMM_R_ONE = 64                    # a resolution of 1
COMM_R_MAX = 256                   # resolution 4
COMM_LEVELS_MAX = 32
COMM_SWEEPS_MAX = 1 << 20
COMM_M2_END = 1 << 58              # the graph's doubled weight stays below this: every quantity then fits 128 bits with its sign
COMM_LEVEL_FIELDS = ("nodes", "communities", "sweeps", "accepted", "moved", "rejected", "split")


def communities_resolution(resolution) -> int:
    """64 * ``resolution`` as the integer r in [1, 256] the gains are built from; anything else is a ``ValueError``: the resolution
    is a multiple of 1/64 in [1/64, 4]."""
    try:
        a = float(resolution) * COMM_R_ONE
        ok = not isinstance(resolution, (bool, np.bool_)) and a == int(a) and 1 <= a <= COMM_R_MAX
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"resolution {resolution!r}: a multiple of 1/64 in [1/64, 4] is required")
    return int(a)


def communities_hash(i, s) -> int:
    """h of node ``i`` in sweep ``s``: the middle part of a mover's priority (D, h, -i)"""
    return ((i + 1) * 2654435761 + s * 40503) & 0xffffffff


def communities_qnum(rows, comm, m2, r) -> int:
    """Qnum = 64 * M2 * sum_c in_c - r * sum_c tot_c^2 of the assignment ``comm`` (node -> community) over the rows ``rows`` (node ->
    {neighbour: weight}, self entries included): the modularity is Qnum / (64 * M2^2)"""
    inner, tot = 0, {}
    for i, row in rows.items():
        tot[comm[i]] = tot.get(comm[i], 0) + sum(row.values())
        inner += sum(w for j, w in row.items() if comm[j] == comm[i])
    return 64 * m2 * inner - r * sum(t * t for t in tot.values())


def _comm_sweep(rows, k, comm, m2, r, s):
    """One synchronous sweep ``s`` over the assignment ``comm``: (want {node: (D, target)}, the new assignment, the movers)"""
    tot = {}
    for i, c in comm.items():
        tot[c] = tot.get(c, 0) + k[i]
    want = {}
    for i, row in rows.items():
        a, w = comm[i], {}
        for j, x in row.items():
            if j != i:
                w[comm[j]] = w.get(comm[j], 0) + x
        wa, top = w.get(a, 0), None
        for c, wc in w.items():
            if c == a:
                continue
            d = 64 * m2 * (wc - wa) - r * k[i] * (tot[c] + k[i] - tot[a])
            if d > 0 and (top is None or d > top[0] or (d == top[0] and c < top[1])):
                top = (d, c)
        if top is not None:
            want[i] = top
    prio = {i: (d, communities_hash(i, s), -i) for i, (d, _) in want.items()}
    new, moved = dict(comm), 0
    for i, (_, c) in want.items():
        if all(prio[j] < prio[i] for j in rows[i] if j != i and j in want and comm[j] in (comm[i], c)):
            new[i] = c
            moved += 1
    return want, new, moved


def _comm_roots(nodes, pairs):
    """node -> the smallest node of its connected component under ``pairs``"""
    root = {i: i for i in nodes}                          # a dict: a level's nodes are the keys of its rows
    for x, y in pairs:
        _join(root, x, y)
    return {i: _find(root, i) for i in nodes}


def modularity_communities(indptr, col, sim, valid=None, resolution=1.0, max_levels=COMM_LEVELS_MAX, max_sweeps=COMM_SWEEPS_MAX,
                           trace=None):
    """Modularity communities (Louvain's levels, a synchronous move rule) of a similarity graph, in integers throughout (the
    definition ``gnn_communities`` computes on the device).  The graph is the upper-triangle CSR of
    :func:`threshold_graph`, with ``valid`` (bool per row, None: all), read as :func:`markov_clusters` reads it.

    Graph: q = rint(float32(sim) * 2^24); an entry with q <= 0 or an invalid end does not exist; the graph is symmetric, parallel
    entries are added.  A level works on *nodes*: at level 0 the valid rows, under their row indices; later the components of the
    level before, numbered from 0 in the order of their smallest member.  A node's row may hold a self entry A_ii (none at level 0;
    later the node's inner weight, both directions counted).  k_i = sum_j A_ij, M2 = sum_i k_i (the same at every level, < 2^58),
    r = 64 * ``resolution`` (:func:`communities_resolution`).
    A level starts with comm[i] = i; a community is named by its founding node; tot_c = the sum of k over c's members.  Sweep s = 0,
    1, ... is synchronous.  *Want*: for node i of community a and every community c != a that holds a neighbour j != i, with w_ic =
    the sum of A_ij over j in c, j != i: D(i, c) = 64 * M2 * (w_ic - w_ia) - r * k_i * (tot_c + k_i - tot_a), which is 32 * M2^2 times
    the modularity change of the move alone; i wants the c of the largest D > 0, ties to the smaller c.  *Pick*: a wanting node has
    the priority (D, h, -i), h = :func:`communities_hash`; i moves iff every neighbour j != i that wants to move and sits in comm[i]
    or in i's target has a strictly smaller priority.  *Score*: Qnum (:func:`communities_qnum`) of the new assignment; strictly
    larger than before: the sweep is accepted; otherwise it is discarded and ends the level (``rejected``).  A sweep that moves
    nobody - nobody wanted: the largest priority always moves - ends the level too, and so do ``max_sweeps`` sweeps.
    End of a level with an accepted sweep: every community is split into the connected components of its induced subgraph, the
    components are numbered by their smallest member and the graph is contracted - a node per component, entries summed, the inner
    weight as the self entry.  A level without an accepted sweep is the last; ``max_levels`` caps them.  M2 = 0: no level.

    ``trace``: a list that receives, per sweep that moved somebody, a dict ``level``, ``sweep``, ``comm`` (before), ``want`` (node
    -> (D, target)), ``new``, ``qnum`` (of ``new``), ``accepted`` and ``node_of`` (row -> its node at this level).

    Returns a dict: per row ``label`` (int64: the smallest row of its final community; -1 for an invalid row) and ``size``;
    ``level_label`` (int64 (levels, n)): the labelling behind each level; per level (int64) ``nodes``, ``communities``, ``sweeps``
    (the level's last one included, whatever ended it), ``accepted``, ``moved`` (in accepted sweeps), ``rejected`` (0 or 1), ``split``
    (components minus communities) and ``qnum`` (a list of Python ints: Qnum of the level's labelling); ``levels``, ``complete`` (the
    last level had no accepted sweep and ``max_sweeps`` ended none), ``m2``, ``resolution`` (r / 64), ``modularity`` (float64 of the
    last qnum / (64 * m2^2); 0.0 without a level) and ``valid``."""
    r = communities_resolution(resolution)
    max_levels = _whole(max_levels, "max_levels", 1, COMM_LEVELS_MAX)
    max_sweeps = _whole(max_sweeps, "max_sweeps", 1, COMM_SWEEPS_MAX)
    n, ea, eb, eq, ok = mcl_weights(indptr, col, sim, valid)
    rows = {int(i): {} for i in np.flatnonzero(ok)}
    for x, y, w in zip(ea.tolist(), eb.tolist(), eq.tolist()):
        rows[x][y] = rows[x].get(y, 0) + w
        rows[y][x] = rows[y].get(x, 0) + w
    m2 = sum(sum(row.values()) for row in rows.values())
    if m2 >= COMM_M2_END:
        raise ValueError(f"the graph's doubled weight {m2} is not below 2^58")
    node_of = {i: i for i in rows}                            # row -> its node
    first_row = {i: i for i in rows}                          # node -> its smallest row
    stats = {f: [] for f in COMM_LEVEL_FIELDS}
    qnums, level_label = [], []
    complete, capped = m2 == 0, False
    while m2 > 0 and len(qnums) < max_levels and not complete:
        k = {i: sum(row.values()) for i, row in rows.items()}
        comm = {i: i for i in rows}
        qn = communities_qnum(rows, comm, m2, r)
        sweeps = accepted = moved = rejected = 0
        while sweeps < max_sweeps:
            want, new, mv = _comm_sweep(rows, k, comm, m2, r, sweeps)
            sweeps += 1
            if mv == 0:
                break
            qnew = communities_qnum(rows, new, m2, r)
            if trace is not None:
                trace.append({"level": len(qnums), "sweep": sweeps - 1, "comm": dict(comm), "want": want, "new": dict(new), "qnum": qnew,
                              "accepted": qnew > qn, "node_of": dict(node_of)})
            if qnew <= qn:
                rejected = 1
                break
            comm, qn, accepted, moved = new, qnew, accepted + 1, moved + mv
        else:
            capped = True                                     # max_sweeps sweeps, the last one accepted
        comp = comm
        if accepted:
            comp = _comm_roots(rows, ((i, j) for i, row in rows.items() for j in row if comm[i] == comm[j]))
            number = {c: v for v, c in enumerate(sorted(set(comp.values())))}
            contracted = {v: {} for v in number.values()}
            for i, row in rows.items():
                new_row = contracted[number[comp[i]]]
                for j, w in row.items():
                    new_row[number[comp[j]]] = new_row.get(number[comp[j]], 0) + w
            first_row = {number[c]: first_row[c] for c in number}      # a component's smallest node holds its smallest row
            node_of = {row: number[comp[i]] for row, i in node_of.items()}
            n_comp = len(number)
        else:
            contracted, n_comp = rows, len(rows)
            complete = not capped
        for f, v in zip(COMM_LEVEL_FIELDS, (len(rows), len(set(comm.values())), sweeps, accepted, moved, rejected,
                                            n_comp - len(set(comm.values())))):
            stats[f].append(v)
        rows = contracted
        qnums.append(communities_qnum(rows, {i: i for i in rows}, m2, r) if accepted else qn)
        lab = np.full(n, -1, dtype=np.int64)
        for row, i in node_of.items():
            lab[row] = first_row[i]
        level_label.append(lab)
        if not accepted:
            break
    label = level_label[-1] if level_label else np.where(ok, np.arange(n, dtype=np.int64), -1)
    size = np.where(ok, np.bincount(label[ok], minlength=n)[np.maximum(label, 0)], 0).astype(np.int64)
    out = {"label": label.copy(), "size": size, "level_label": np.asarray(level_label, dtype=np.int64).reshape(len(level_label), n),
           "qnum": qnums, "levels": len(qnums), "complete": bool(complete), "m2": m2, "resolution": r / COMM_R_ONE,
           "modularity": float(Fraction(qnums[-1], 64 * m2 * m2)) if qnums else 0.0, "valid": ok}
    out.update({f: np.asarray(v, dtype=np.int64) for f, v in stats.items()})
    return out


def label_components(indptr, col, sim, label, valid=None) -> np.ndarray:
    """The connected components of every label's induced subgraph over the existing entries of a similarity graph (read as
    :func:`modularity_communities` reads it; the definition ``gnn_label_components`` computes on the device): int64 per row - the
    smallest row of its component among the rows of its own ``label`` (int64 per row, -1: none); -1 for label -1 and for an invalid
    row."""
    n, ea, eb, _, ok = mcl_weights(indptr, col, sim, valid)
    label = np.asarray(label)
    if label.shape != (n,) or label.dtype.kind not in "iu" or (label < -1).any():
        raise ValueError(f"label must be an integer array of {n} with values >= -1")
    label = label.astype(np.int64)
    same = (label[ea] == label[eb]) & (label[ea] >= 0)
    root = list(range(n))
    for x, y in zip(ea[same].tolist(), eb[same].tolist()):
        _join(root, x, y)
    return _root_labels(root, ok & (label >= 0))


def communities_table(result, names=None):
    """One record per community of a result of :func:`modularity_communities` (or anything with its ``label`` and ``size``), ordered
    by label: ``label``, ``size`` and ``members``, as indices in ascending order or - where ``names`` is given - as names"""
    label = np.asarray(result["label"], dtype=np.int64)
    size = np.asarray(result["size"])
    name = _namer(names)
    order = np.argsort(label, kind="stable")
    order = order[label[order] >= 0]
    bounds = np.flatnonzero(np.diff(label[order], prepend=-1)) if len(order) else []
    return [{"label": name(label[order[a]]), "size": int(size[order[a]]), "members": [name(i) for i in order[a:b]]}
            for a, b in zip(bounds, list(bounds[1:]) + [len(order)])]


KNN_GRAPH_MODES = ("union", "mutual")                  # gnn_knn_graph_mode: GNN_KNN_GRAPH_UNION = 0, _MUTUAL = 1
KNN_GRAPH_WEIGHTS = ("similarity", "jaccard")          # gnn_knn_graph_weight: GNN_KNN_GRAPH_SIMILARITY = 0, _JACCARD = 1
KNN_GRAPH_FIELDS = ("indptr", "col", "sim", "mutual", "valid")


def knn_graph_mode(mode) -> str:
    if mode not in KNN_GRAPH_MODES:
        raise ValueError(f"mode {mode!r} is outside {KNN_GRAPH_MODES}")
    return mode


def knn_graph_weight(weight) -> str:
    if weight not in KNN_GRAPH_WEIGHTS:
        raise ValueError(f"weight {weight!r} is outside {KNN_GRAPH_WEIGHTS}")
    return weight


def knn_graph(rows, k, mode="union", weight="similarity", metric="cosine", neighbours=None):
    """The k-nearest-neighbour graph among encoder embeddings, spelled out (the definition ``gnn_knn_graph_count`` /
    ``gnn_knn_graph_fill`` compute on the device; readable, not fast).  ``rows`` (n, 512) float32; validity, ``metric`` and ``k``
    (1..64) as in :func:`nearest_neighbours`, whose self-search gives the lists - or ``neighbours`` = (idx, sim), lists computed
    elsewhere (the device's own).  N(i) is row i's entries other than -1, N+(i) = N(i) + {i}; an invalid row has an empty list and is
    in nobody's.  The edges are the unordered pairs i < j of valid rows with j in N(i) or i in N(j) (``union``), or both (``mutual``);
    a pair stands once, at its smaller row.  ``weight`` "similarity": where j is in N(i), the float32 that stands in row i's list for
    j - what :func:`threshold_graph` computes for the pair; otherwise the float32 in row j's list for i, the other orientation, which
    on the device may differ from the graph's value in the last bit.  Negative similarities are kept: the consumers (:func:`mcl_weights`,
    :func:`spread_transitions`, :func:`average_linkage`, :func:`modularity_communities`) drop weights <= 0.  "jaccard": s = |N+(i) &
    N+(j)|, u = |N+(i)| + |N+(j)| - s, and the weight is float32(s) / float32(u), one correctly rounded division - every edge has
    s >= 1, so it lies in (0, 1].  Returns a dict: ``indptr`` (int64, n + 1), ``col`` (int32: row i owns ``col[indptr[i]:indptr[i + 1]]``,
    its partners j > i strictly ascending), ``sim`` (float32), ``mutual`` (uint8: 1 when both ends list each other - everywhere under
    ``mutual``) and ``valid`` (bool, n).  There are at most n_valid * k edges."""
    k = neighbour_k(k)
    knn_graph_mode(mode)
    knn_graph_weight(weight)
    r32 = neighbour_rows(rows, "rows")
    valid = valid_rows(r32, metric)
    n = len(r32)
    idx, sim = nearest_neighbours(r32, None, k, metric) if neighbours is None else neighbours
    idx, sim = np.asarray(idx, dtype=np.int64), np.asarray(sim, dtype=np.float32)
    src, slot = np.nonzero(idx >= 0)                     # the arcs src -> dst
    dst, s = idx[src, slot], sim[src, slot]
    back = np.isin(dst * n + src, src * n + dst)         # the arc dst -> src is there too
    own = src < dst                                      # the arc of the pair's smaller row: its value is the pair's
    keep = own & back if mode == "mutual" else own | ~back
    a, b = np.minimum(src, dst)[keep], np.maximum(src, dst)[keep]
    order = np.lexsort((b, a))
    a, b, s, both = a[order], b[order], s[keep][order], back[keep][order]
    if weight == "jaccard":
        plus = [set(idx[i][idx[i] >= 0].tolist()) | {i} for i in range(n)]
        shared = np.array([len(plus[i] & plus[j]) for i, j in zip(a.tolist(), b.tolist())], dtype=np.int64).reshape(len(a))
        size = np.array([len(p) for p in plus], dtype=np.int64).reshape(n)
        s = shared.astype(np.float32) / (size[a] + size[b] - shared).astype(np.float32)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=n))]).astype(np.int64)
    return {"indptr": indptr, "col": b.astype(np.int32), "sim": s.astype(np.float32), "mutual": both.astype(np.uint8), "valid": valid}


def knn_graph_table(indptr, col, sim, mutual, names=None):
    """One record per edge of a k-nearest-neighbour graph, in its order: ``a`` < ``b`` (indices; the names where ``names`` is given),
    ``weight`` and ``mutual`` (both ends list each other)."""
    a, b = graph_edges(indptr, col)
    name = _namer(names)
    return [{"a": name(i), "b": name(j), "weight": float(s), "mutual": bool(m)}
            for i, j, s, m in zip(a, b, np.asarray(sim), np.asarray(mutual))]


TSNE_N_MAX = 1 << 21               # Z < 2^63: DESIGN.md section 5x
TSNE_ITER_MAX = 100000
TSNE_GRANULE = 256                 # columns of one float32 chain, aligned to the column index
TSNE_Z_UNIT = float(1 << 20)       # a granule's sum of q in units of 2^-20
TSNE_F_UNIT = float(1 << 32)       # forces in units of 2^-32
TSNE_EXAGGERATION_MAX = 1024.0
TSNE_LEARNING_RATE_MAX = float(1 << 20)
TSNE_FIELDS = ("layout", "z_trace", "iterations", "valid")
_TSNE_BLOCK_CELLS = 1 << 22        # cells of the definition's row blocks; no result depends on it


def tsne_init(n, offset=0) -> np.ndarray:
    """The layout t-SNE starts from when none is given: float32 (n, 2), coordinate k = 2 i + c the (k + offset)-th output of splitmix64
    from seed 0 - z = (k + offset + 1) * 0x9E3779B97F4A7C15, z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9, z = (z ^ z >> 27) *
    0x94D049BB133111EB, z ^= z >> 31, all mod 2^64 - whose top 24 bits u map to float32((u / 2^23 - 1) * 1e-4), in [-1e-4, 1e-4).  No
    random state: the same n gives the same bits everywhere."""
    n = _whole(n, "n", 0, TSNE_N_MAX)
    z = (np.arange(2 * n, dtype=np.uint64) + np.uint64(_whole(offset, "offset", 0, 1 << 62) + 1)) * np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    u = (z >> np.uint64(40)).astype(np.float64)
    return ((u / float(1 << 23) - 1.0) * 1e-4).astype(np.float32).reshape(n, 2)


def tsne_params(n_iter=750, exaggeration_iter=250, exaggeration=12.0, learning_rate=None, n_valid=0):
    """(n_iter, exaggeration_iter, exaggeration as a float, learning_rate as a float32) as the library takes them; a ``ValueError`` for
    one out of range.  ``learning_rate`` None: max(n_valid / exaggeration / 4, 50), scikit-learn's "auto"."""
    n_iter = _whole(n_iter, "n_iter", 0, TSNE_ITER_MAX)
    exaggeration_iter = _whole(exaggeration_iter, "exaggeration_iter", 0, TSNE_ITER_MAX)
    try:
        e = float(exaggeration)
        lr = np.float32(max(n_valid / e / 4.0, 50.0) if learning_rate is None else learning_rate)
    except (TypeError, ValueError, ZeroDivisionError):
        raise ValueError(f"exaggeration {exaggeration!r} and learning_rate {learning_rate!r}: floats are required") from None
    if not 1.0 <= e <= TSNE_EXAGGERATION_MAX:
        raise ValueError(f"exaggeration {exaggeration!r} is outside [1, 1024]")
    if not 0.0 < lr <= TSNE_LEARNING_RATE_MAX:
        raise ValueError(f"learning_rate {learning_rate!r} is outside (0, 2^20]")
    return n_iter, exaggeration_iter, e, lr


def tsne_affinities(indptr, col, sim, valid=None):
    """The affinities t-SNE attracts by, from the upper-triangle CSR :func:`threshold_graph` / :func:`knn_graph` return: (n, i, j, p, q,
    m2, valid).  The weights are :func:`mcl_weights`': q = rint(float64(float32(sim)) * 2^24), an entry with q <= 0 or an invalid end
    does not exist.  Every entry stands in both orientations (i, j) and (j, i), parallel entries stay separate entries; ``m2`` is the
    integer sum of q over all of them and p = float32(float64(q) / float64(m2)).  ``ValueError`` as there, and for more than 2^21 rows."""
    n, a, b, q, ok = mcl_weights(indptr, col, sim, valid)
    if n > TSNE_N_MAX:
        raise ValueError(f"{n} rows: at most 2^21 are supported")
    i, j, q = np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([q, q]).astype(np.int64)
    m2 = int(q.sum())
    p = (q.astype(np.float64) / np.float64(m2)).astype(np.float32) if m2 else np.zeros(0, dtype=np.float32)
    return n, i, j, p, q, m2, ok


def _tsne_q(dx, dy, m):
    """m / (1 + (dx dx + dy dy)) in float32, one rounding per operation"""
    return m / (np.float32(1.0) + (dx * dx + dy * dy))


def _tsne_image(chain, unit):
    return np.rint(chain.astype(np.float64) * unit).astype(np.int64)


def tsne_forces(y, i, j, p, valid, attract=True):
    """One evaluation of t-SNE's forces at the layout ``y`` (float32 (n, 2), finite at every valid row) for the entries (i, j, p) of
    :func:`tsne_affinities`: int64 (zi, rx, ry, ax, ay), each (n,) and 0 at an invalid row.  Every float32 operation is a single IEEE
    operation.  Repulsion, row r against column c: dx = x_r - x_c, dy = y_r - y_c, q = 1 / (1 + (dx dx + dy dy)), and q = 0 where
    c == r, c is invalid or c is padding behind n; for every granule of 256 columns, aligned to the column index, three float32 chains
    in ascending column order - cz += q, cx += (q q) dx, cy += (q q) dy - and at its end zi += rint(float64(cz) * 2^20), rx +=
    rint(float64(cx) * 2^32), ry likewise.  Attraction, per entry: ax_i += rint(float64((p q) dx) * 2^32), ay likewise - integer adds,
    in any order."""
    y = np.ascontiguousarray(y, dtype=np.float32)
    ok = np.asarray(valid, dtype=bool)
    n = len(ok)
    if y.shape != (n, 2):
        raise ValueError(f"the layout must be ({n}, 2)")
    granules = -(-n // TSNE_GRANULE)
    pad = granules * TSNE_GRANULE
    cx_, cy_, m = (np.zeros(pad, dtype=np.float32) for _ in range(3))
    cx_[:n], cy_[:n], m[:n] = np.where(ok, y[:, 0], 0), np.where(ok, y[:, 1], 0), ok
    zi, rx, ry, ax, ay = (np.zeros(n, dtype=np.int64) for _ in range(5))
    rows = np.flatnonzero(ok)
    block = max(1, _TSNE_BLOCK_CELLS // max(pad, 1))
    for s in range(0, len(rows), block):
        r = rows[s:s + block]
        dx, dy = y[r, 0][:, None] - cx_[None, :], y[r, 1][:, None] - cy_[None, :]
        q = _tsne_q(dx, dy, m[None, :])
        q[np.arange(len(r)), r] = 0
        q2 = q * q
        for out, term, unit in ((zi, q, TSNE_Z_UNIT), (rx, q2 * dx, TSNE_F_UNIT), (ry, q2 * dy, TSNE_F_UNIT)):
            # np.add.accumulate adds one element at a time, in the array's own type: the chain
            chain = np.add.accumulate(term.reshape(len(r), granules, TSNE_GRANULE), axis=2, dtype=np.float32)[:, :, -1]
            out[r] = _tsne_image(chain, unit).sum(axis=1)
    if attract and len(i):
        dx, dy = y[i, 0] - y[j, 0], y[i, 1] - y[j, 1]
        pq = np.asarray(p, dtype=np.float32) * _tsne_q(dx, dy, np.float32(1.0))
        np.add.at(ax, i, _tsne_image(pq * dx, TSNE_F_UNIT))
        np.add.at(ay, i, _tsne_image(pq * dy, TSNE_F_UNIT))
    return zi, rx, ry, ax, ay


def tsne_layout(indptr, col, sim, init, valid=None, n_iter=750, exaggeration_iter=250, exaggeration=12.0, learning_rate=None):
    """The exact t-SNE layout of a similarity graph, spelled out (the definition ``gnn_tsne`` computes on the device, bit for bit;
    DESIGN.md section 5x).  The graph is an upper-triangle CSR as :func:`threshold_graph` / :func:`knn_graph` return it, ``valid`` a
    bool per row (None: all), ``init`` the float32 (n, 2) layout it starts from (finite at every valid row: ``ValueError`` otherwise).
    The affinities are :func:`tsne_affinities`' - the graph's own weights, not perplexity-calibrated ones.

    Iteration ``it`` = 0 .. n_iter - 1, with Y in float32: the forces of :func:`tsne_forces`; Z = sum zi, an integer; in float64,
    rounded to float32 once, g = 4 (e A / 2^32 - (R / 2^32) / (Z / 2^20)) with e = ``exaggeration`` while it < ``exaggeration_iter``
    and 1 from there on, the second term 0 where Z == 0.  Then elementwise in float32: gain += 0.2 where g and the previous update have
    strictly opposite signs (g > 0 and upd < 0, or g < 0 and upd > 0), otherwise gain *= 0.8, and gain is at least 0.01 (it starts at
    1, upd at 0); upd = mom upd - lr (gain g) with mom = 0.5 while it < ``exaggeration_iter`` and 0.8 from there on; Y += upd.  There is
    no recentring and no early end.  ``learning_rate`` None: max(n_valid / exaggeration / 4, 50).

    Returns a dict: ``layout`` (float32 (n, 2), NaN at an invalid row), ``z_trace`` (uint64 (n_iter + 1,): the Z of every iterate, the
    final one included), ``iterations`` and ``valid``."""
    n, i, j, p, _, _, ok = tsne_affinities(indptr, col, sim, valid)
    n_iter, exaggeration_iter, e_early, lr = tsne_params(n_iter, exaggeration_iter, exaggeration, learning_rate, int(ok.sum()))
    with np.errstate(over="ignore"):
        y = np.array(init, dtype=np.float32)
    if y.shape != (n, 2):
        raise ValueError(f"init must be ({n}, 2)")
    if not np.isfinite(y[ok]).all():
        raise ValueError("init: every valid row must be finite")
    y[~ok] = np.nan
    gain, upd = np.ones((n, 2), dtype=np.float32), np.zeros((n, 2), dtype=np.float32)
    z_trace = np.zeros(n_iter + 1, dtype=np.uint64)
    for it in range(n_iter + 1):
        zi, rx, ry, ax, ay = tsne_forces(y, i, j, p, ok, attract=it < n_iter)
        z = int(zi.sum())
        z_trace[it] = z
        if it == n_iter:
            break
        early = it < exaggeration_iter
        att = (e_early if early else 1.0) * (np.stack([ax, ay], axis=1).astype(np.float64) / TSNE_F_UNIT)
        rep = (np.stack([rx, ry], axis=1).astype(np.float64) / TSNE_F_UNIT) / (float(z) / TSNE_Z_UNIT) if z else 0.0
        g = (4.0 * (att - rep)).astype(np.float32)
        opposite = ((g > 0) & (upd < 0)) | ((g < 0) & (upd > 0))
        gain = np.maximum(np.where(opposite, gain + np.float32(0.2), gain * np.float32(0.8)), np.float32(0.01))
        upd = np.float32(0.5 if early else 0.8) * upd - lr * (gain * g)
        y = y + upd
    return {"layout": y, "z_trace": z_trace, "iterations": n_iter, "valid": ok}


def tsne_kl(indptr, col, sim, layout, z, valid=None) -> float:
    """The Kullback-Leibler divergence of a layout from the graph's affinities, in float64 and O(entries): sum over the entries of
    p (log p - log q) + log(z / 2^20), with q = 1 / (1 + |y_i - y_j|^2) as :func:`tsne_forces` computes it in float32 and ``z`` the
    layout's integer Z (``z_trace[-1]``).  A graph without an entry has 0."""
    _, i, j, p, _, m2, ok = tsne_affinities(indptr, col, sim, valid)
    if not m2 or int(z) <= 0:
        return 0.0
    y = np.ascontiguousarray(layout, dtype=np.float32)
    q = _tsne_q(y[i, 0] - y[j, 0], y[i, 1] - y[j, 1], np.float32(1.0)).astype(np.float64)
    p = p.astype(np.float64)
    keep = p > 0
    return float((p[keep] * (np.log(p[keep]) - np.log(q[keep]))).sum() + np.log(float(int(z)) / TSNE_Z_UNIT))


def tsne_table(layout, valid, names=None):
    """One record per row: ``name`` (the index without ``names``), ``x`` and ``y`` (None at an invalid row)"""
    name = _namer(names)
    return [{"name": name(i), "x": float(xy[0]) if ok else None, "y": float(xy[1]) if ok else None}
            for i, (xy, ok) in enumerate(zip(np.asarray(layout), np.asarray(valid, dtype=bool)))]


def prefix_of(input_path: Path) -> str:
    """nn_classification.py:106-108: stem, minus one more extension if the file is compressed."""
    prefix = Path(input_path).stem
    if compression_of(input_path) != "uncompressed":
        prefix = prefix.rsplit(".", 1)[0]
    return prefix
