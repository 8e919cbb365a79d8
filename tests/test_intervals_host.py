"""Interval embeddings without a GPU: the member ranges against a brute-force loop, every validation error,
partitions, the numpy definition of the outputs, gnn_interval_plan (host only) against the numpy mirror, main()'s
GENOMAD_AMD_REGION_EMBEDDINGS switch and the gather of the regions' rows over two gloo ranks."""
import socket

import numpy as np
import pytest

from genomad_amd import nn_classification as nnc
from genomad_amd import sequence, sharding
from tests.test_embeddings_gpu import _contigs
from tests.test_regions_host import FakeRegionEngine, _write_fasta

INTERVALS = [(1, 0, 9000), (1, 9000, 9000), (1, 9000, 20000), (1, 26000, 33000), (2, 0, 19000), (3, 0, 100), (5, 0, 9000),
             (5, 9000, 18000), (6, 0, 1000), (6, 1000, 31000), (6, 31000, 31500), (6, 31500, 70000), (9, 0, 13000)]


def _iv(intervals=INTERVALS):
    return tuple(np.array(x, dtype=np.int64) for x in zip(*intervals)) if intervals else (np.zeros(0, np.int64),) * 3


def _kept(seq, starts, lens, window_n):
    n_count = np.array([np.count_nonzero(seq[a:a + l] == ord("N")) for a, l in zip(starts, lens)])
    return (window_n == 0) | (n_count <= sequence.MAX_N)


def _brute_force(offsets, stride, single_window, contig, start, end):
    """the definition, window by window: the interval of window k is the one of its contig that holds its centre base"""
    _, lens, ids, window_n, _, _ = sequence.scan_spans(offsets, stride, single_window)
    centre = window_n.astype(np.int64) * stride + lens // 2
    owner = np.full(len(lens), -1, np.int64)
    for i, (c, s, e) in enumerate(zip(contig, start, end)):
        hit = (ids == c) & (centre >= s) & (centre < e)
        assert (owner[hit] == -1).all()                            # a window has at most one interval
        owner[hit] = i
    return owner


@pytest.mark.parametrize("stride,single_window", [(6000, False), (2000, False), (1000, False), (1, False), (2000, True), (1, True)])
def test_member_ranges_against_a_brute_force_loop(stride, single_window):
    seq, offsets = _contigs()
    contig, start, end = _iv()
    w_lo, w_hi = sequence.interval_windows(offsets, stride, contig, start, end, single_window)
    owner = _brute_force(offsets, stride, single_window, contig, start, end)
    assert w_lo.dtype == np.int64 and w_hi.dtype == np.int64
    for i in range(len(contig)):
        members = np.flatnonzero(owner == i)
        assert w_hi[i] - w_lo[i] == len(members)
        if len(members):
            assert (members == np.arange(w_lo[i], w_hi[i])).all()  # one contiguous range of the global window order
    assert (w_lo[1:] >= w_hi[:-1]).all() and (w_lo <= w_hi).all()   # disjoint and ordered: what the device's bisection relies on


def test_centres_increase_strictly_at_every_stride_around_a_short_last_window():
    """what makes the members one range: only the last window is shorter than 6000, by less than twice its advance"""
    for stride in (1, 2, 3, 7, 2999, 3000, 3001, 5999, 6000):
        for length in (6001, 6002, 8499, 8500, 8501, 12000 + stride, 6000 + 3 * stride + 1):
            _, lens, _, window_n, _, _ = sequence.scan_spans(np.array([0, length]), stride)
            centre = window_n.astype(np.int64) * stride + lens // 2
            assert (np.diff(centre) > 0).all(), (stride, length)


def test_the_fixture_counts():
    seq, offsets = _contigs()
    starts, lens, _, window_n, _, _ = sequence.scan_spans(offsets, 2000)
    kept = _kept(seq, starts, lens, window_n)
    w_lo, w_hi = sequence.interval_windows(offsets, 2000, *_iv())
    assert len(starts) == 75 and kept.sum() == 72
    assert list(w_hi - w_lo) == [3, 0, 6, 3, 8, 1, 3, 4, 0, 14, 1, 18, 5]
    assert [int(kept[a:b].sum()) for a, b in zip(w_lo, w_hi)] == [3, 0, 6, 3, 7, 1, 3, 3, 0, 14, 1, 18, 4]
    assert (w_lo[11], w_hi[11]) == (47, 65)


BAD = [("unsorted by contig", [(2, 0, 10), (1, 0, 10)], r"interval 1 .*not sorted by \(contig, start\)"),
       ("unsorted by start", [(1, 500, 600), (1, 100, 200)], r"interval 1 .*not sorted by \(contig, start\)"),
       ("overlapping", [(1, 0, 1000), (1, 999, 2000)], r"interval 1 .*overlaps interval 0, which ends at 1000"),
       ("beyond the contig", [(0, 0, 2001)], r"interval 0 .*ends beyond its contig of 2000 bases"),
       ("negative", [(0, -1, 5)], r"interval 0 .*starts below 0"),
       ("reversed", [(0, 10, 5)], r"interval 0 .*ends before it starts"),
       ("bad contig index", [(0, 0, 5), (10, 0, 5)], r"interval 1 .*names a contig outside \[0, 10\)"),
       ("negative contig index", [(-1, 0, 5)], r"interval 0 .*names a contig outside \[0, 10\)")]


def _lib_plan(offsets, stride, single_window, contig, start, end):
    from genomad_amd import _lib
    lib = _lib.load()
    w_lo, w_hi = np.full(len(contig), -7, np.int64), np.full(len(contig), -7, np.int64)
    rc = lib.gnn_interval_plan(offsets.ctypes.data, len(offsets) - 1, int(stride), int(single_window), contig.ctypes.data, start.ctypes.data,
                               end.ctypes.data, len(contig), w_lo.ctypes.data, w_hi.ctypes.data)
    return rc, w_lo, w_hi, (lib.gnn_last_error() or b"").decode()


@pytest.mark.parametrize("what,intervals,pattern", BAD, ids=[b[0] for b in BAD])
def test_every_validation_error_names_the_interval_in_numpy_and_in_the_library(what, intervals, pattern):
    import re
    from genomad_amd import _lib
    _, offsets = _contigs()
    with pytest.raises(ValueError, match=pattern):
        sequence.interval_windows(offsets, 2000, *_iv(intervals))
    rc, _, _, msg = _lib_plan(offsets, 2000, False, *_iv(intervals))
    assert rc == _lib.ERR_ARG and re.search(r"gnn_interval_plan: " + pattern, msg), msg


def test_touching_and_empty_intervals_are_valid():
    _, offsets = _contigs()
    ok = [(1, 0, 0), (1, 0, 3000), (1, 3000, 3000), (1, 3000, 3000), (1, 3000, 33000), (1, 33000, 33000), (4, 0, 0)]
    w_lo, w_hi = sequence.interval_windows(offsets, 2000, *_iv(ok))
    assert list(w_hi - w_lo) == [0, 0, 0, 0, 15, 0, 0]               # window 0 of contig 1 has its centre at 3000


@pytest.mark.parametrize("stride", [6000, 2000, 700])
def test_a_partition_gives_every_window_one_interval(stride):
    seq, offsets = _contigs()
    rng = np.random.default_rng(stride)
    intervals = []
    for c, length in enumerate(np.diff(offsets)):
        cuts = np.unique(np.concatenate([[0, length], rng.integers(0, length + 1, size=4)])) if length else np.array([0, 0])
        intervals += [(c, int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:])]
    contig, start, end = _iv(intervals)
    w_lo, w_hi = sequence.interval_windows(offsets, stride, contig, start, end)
    starts, lens, _, window_n, _, _ = sequence.scan_spans(offsets, stride)
    assert (_brute_force(offsets, stride, False, contig, start, end) >= 0).all()
    assert w_lo[0] == 0 and w_hi[-1] == len(starts) and (w_lo[1:] == w_hi[:-1]).all()
    kept = _kept(seq, starts, lens, window_n)
    rows = rng.standard_normal((len(starts), 512)).astype(np.float32)
    out = sequence.interval_embeddings(rows, None, kept, w_lo, w_hi)
    assert int(out["count"].sum()) == int(kept.sum())


def test_the_numpy_definition_of_the_outputs():
    rng = np.random.default_rng(8)
    rows = rng.standard_normal((12, 512)).astype(np.float32)
    scores = rng.random((12, 3), dtype=np.float32)
    rows[2] = 0.0                                                    # a zero row
    rows[6, 3] = np.inf                                              # a non-finite row
    rows[9] = rows[8] * np.float32(4)                                # the same direction: coherence 1 with row 8
    rows[10] = -rows[8]
    kept = np.ones(12, bool)
    kept[4] = False
    w_lo, w_hi = np.array([0, 3, 3, 5, 7, 8, 8]), np.array([3, 3, 5, 7, 8, 10, 11])
    out = sequence.interval_embeddings(rows, scores, kept, w_lo, w_hi)
    assert list(out["count"]) == [3, 0, 1, 2, 1, 2, 3]
    assert out["embedding"].dtype == np.float32 and out["scores"].dtype == np.float32 and out["coherence"].dtype == np.float64
    # interval 0: sequential float32 sums, one divide; the zero row counts but adds nothing to U
    s = ((np.zeros(512, np.float32) + rows[0]) + rows[1]) + rows[2]
    assert np.array_equal(out["embedding"][0], s / np.float32(3))
    assert np.array_equal(out["scores"][0], (((np.zeros(3, np.float32) + scores[0]) + scores[1]) + scores[2]) / np.float32(3))
    u = rows[0].astype(np.float64) / np.linalg.norm(rows[0].astype(np.float64)) + rows[1].astype(np.float64) / np.linalg.norm(
        rows[1].astype(np.float64))
    assert abs(out["coherence"][0] - np.linalg.norm(u) / 3) < 1e-15
    # interval 1: count == 0 - zero rows, coherence 0;  interval 2: its second member is masked
    assert not out["embedding"][1].any() and not out["scores"][1].any() and out["coherence"][1] == 0.0
    assert np.array_equal(out["embedding"][2], rows[3]) and abs(out["coherence"][2] - 1.0) < 1e-15
    # interval 3: the non-finite row enters the embedding (as the contig fold has it) and adds nothing to U
    assert np.isinf(out["embedding"][3][3]) and abs(out["coherence"][3] - 0.5) < 1e-15
    # intervals 5 and 6: identical directions give 1; the opposite row cancels one of them
    assert abs(out["coherence"][5] - 1.0) < 1e-12 and abs(out["coherence"][6] - 1.0 / 3) < 1e-12
    assert ((out["coherence"] >= 0) & (out["coherence"] <= 1 + 1e-12)).all()
    # both strands: two independent sums
    rev = rng.standard_normal((12, 512)).astype(np.float32)
    both = sequence.interval_embeddings(rows, scores, kept, w_lo, w_hi, rows_rev=rev)
    sr = ((np.zeros(512, np.float32) + rev[0]) + rev[1]) + rev[2]
    assert np.array_equal(both["embedding"][0], (s + sr) / np.float32(6)) and np.array_equal(both["count"], out["count"])
    assert np.array_equal(both["scores"], out["scores"])


@pytest.mark.parametrize("stride,single_window", [(6000, False), (2000, False), (1000, True), (1, False)])
def test_the_library_plan_equals_the_numpy_mirror(stride, single_window):
    _, offsets = _contigs()
    contig, start, end = _iv()
    rc, w_lo, w_hi, msg = _lib_plan(offsets, stride, single_window, contig, start, end)
    assert rc == 0, msg
    want = sequence.interval_windows(offsets, stride, contig, start, end, single_window)
    assert np.array_equal(w_lo, want[0]) and np.array_equal(w_hi, want[1])
    rc, _, _, msg = _lib_plan(offsets, 6001, False, contig, start, end)
    assert rc == -1 and "stride 6001" in msg
    rc, w_lo, _, _ = _lib_plan(offsets, stride, single_window, *_iv([]))
    assert rc == 0 and len(w_lo) == 0


# ---- main() -------------------------------------------------------------------------------------------------------------------
SWITCHES = ("GENOMAD_AMD_FRONT_END", "GENOMAD_AMD_STRAND", "GENOMAD_AMD_EMBEDDINGS", "GENOMAD_AMD_SCAN_STRIDE", "GENOMAD_AMD_PRECISION",
            "GENOMAD_AMD_OCCLUSION_BLOCK", "GENOMAD_AMD_ATTRIBUTION_BIN", "GENOMAD_AMD_REGION_PENALTY", "GENOMAD_AMD_REGION_EMBEDDINGS",
            "GENOMAD_AMD_NEIGHBOURS", "GENOMAD_AMD_CLUSTERS", "GENOMAD_AMD_REPRESENTATIVES")


class FakeIntervalEngine(FakeRegionEngine):
    """the fake engine of the region tests plus embed_intervals: rows made from the interval itself, so that a test can tell whose
    they are"""

    def embed_intervals(self, seq, offsets, stride, contig, start, end, strand="forward", single_window=False, precision=None):
        from genomad_amd.engine import IntervalResult
        type(self).calls.append(("intervals", int(stride), strand, len(contig)))
        contig, start, end = (np.asarray(a, np.int64) for a in (contig, start, end))
        w_lo, w_hi = sequence.interval_windows(offsets, stride, contig, start, end, single_window)
        n = len(contig)
        emb = (start[:, None] + np.arange(512)[None, :]).astype(np.float32) if n else np.zeros((0, 512), np.float32)
        return IntervalResult(stride=int(stride), strand=strand, contig=contig, start=start, end=end, w_lo=w_lo, w_hi=w_hi,
                              count=(w_hi - w_lo).astype(np.int32), embedding=emb, coherence=np.full(n, 0.5, np.float32),
                              scores=np.tile(np.float32([0.2, 0.3, 0.5]), (n, 1)))


@pytest.fixture
def fake_main(monkeypatch):
    monkeypatch.setattr(nnc, "_engine", lambda: FakeIntervalEngine())
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    del FakeRegionEngine.calls[:]
    return lambda fa, out, **kw: nnc.main(fa, out, False, 128, False, 1, False, False, **kw)


def test_switch_values(monkeypatch):
    monkeypatch.delenv("GENOMAD_AMD_REGION_EMBEDDINGS", raising=False)
    assert nnc.region_embeddings_requested() is False
    for v, want in (("", False), ("0", False), (" 1 ", True)):
        monkeypatch.setenv("GENOMAD_AMD_REGION_EMBEDDINGS", v)
        assert nnc.region_embeddings_requested() is want
    monkeypatch.setenv("GENOMAD_AMD_REGION_EMBEDDINGS", "yes")
    with pytest.raises(ValueError, match="GENOMAD_AMD_REGION_EMBEDDINGS='yes': expected 1"):
        nnc.region_embeddings_requested()


def test_main_refuses_the_switch_without_a_penalty_before_any_work(tmp_path, monkeypatch, fake_main, capsys):
    fa = tmp_path / "s.fna"
    _write_fasta(fa, n=3)
    monkeypatch.setenv("GENOMAD_AMD_REGION_EMBEDDINGS", "2")
    with pytest.raises(ValueError, match="GENOMAD_AMD_REGION_EMBEDDINGS"):
        fake_main(fa, tmp_path / "bad")
    assert not (tmp_path / "bad").exists()
    monkeypatch.setenv("GENOMAD_AMD_REGION_EMBEDDINGS", "1")
    monkeypatch.setenv("GENOMAD_AMD_SCAN_STRIDE", "2000")             # a stride alone is not enough
    with pytest.raises(SystemExit) as exc:
        fake_main(fa, tmp_path / "refused")
    assert exc.value.code == 1
    err = capsys.readouterr().err
    assert "GENOMAD_AMD_REGION_EMBEDDINGS=1 needs GENOMAD_AMD_REGION_PENALTY" in err and len(err.strip().splitlines()) == 1
    assert not list((tmp_path / "refused").rglob("*.npz")) and not list((tmp_path / "refused").rglob("*.tsv"))
    monkeypatch.delenv("GENOMAD_AMD_SCAN_STRIDE")
    monkeypatch.setenv("GENOMAD_AMD_REGION_PENALTY", "1")             # and the penalty needs the stride
    with pytest.raises(SystemExit):
        fake_main(fa, tmp_path / "nostride")
    assert "GENOMAD_AMD_REGION_PENALTY needs GENOMAD_AMD_SCAN_STRIDE" in capsys.readouterr().err
    assert FakeRegionEngine.calls == []


def _tree(d):
    return sorted(str(p.relative_to(d)) for p in d.rglob("*") if p.is_file() and p.suffix in (".npz", ".tsv"))


def test_main_writes_the_file_changes_nothing_else_and_resumes(tmp_path, monkeypatch, fake_main):
    fa = tmp_path / "m.fna"
    _write_fasta(fa, n=7)
    monkeypatch.setenv("GENOMAD_AMD_SCAN_STRIDE", "1500")
    monkeypatch.setenv("GENOMAD_AMD_REGION_PENALTY", "0.05")
    fake_main(fa, tmp_path / "unset")
    assert not any(c[0] == "intervals" for c in FakeRegionEngine.calls)
    monkeypatch.setenv("GENOMAD_AMD_REGION_EMBEDDINGS", "1")
    out = tmp_path / "on"
    fake_main(fa, out)
    d0, d1 = tmp_path / "unset" / "m_nn_classification", out / "m_nn_classification"
    assert _tree(d1) == sorted(_tree(d0) + ["m_nn_region_embeddings.npz"])
    for rel in _tree(d0):
        if rel.endswith(".tsv"):
            assert (d0 / rel).read_bytes() == (d1 / rel).read_bytes(), rel
        else:
            a, b = np.load(d0 / rel), np.load(d1 / rel)
            assert sorted(a.files) == sorted(b.files) and all(np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f") for k in a.files)
    z, reg = np.load(d1 / "m_nn_region_embeddings.npz"), np.load(d1 / "m_nn_regions.npz")
    assert sorted(z.files) == sorted(["contig_names", "contig", "start", "end", "state", "embedding", "count", "coherence", "scores",
                                      "stride", "penalty", "strand"])
    for mine, theirs in (("contig", "region_contig"), ("start", "start"), ("end", "end"), ("state", "region_state")):
        assert np.array_equal(z[mine], reg[theirs]) and z[mine].dtype == reg[theirs].dtype
    assert int(z["stride"]) == 1500 and float(z["penalty"]) == 0.05 and str(z["strand"]) == "forward"
    assert z["embedding"].shape == (len(z["start"]), 512) and np.array_equal(z["embedding"][:, 0], z["start"].astype(np.float32))
    runs = lambda: sum(1 for c in FakeRegionEngine.calls if c[0] == "scan")     # noqa: E731  (one piece: one scan per run of the stage)
    n = runs()
    fake_main(fa, out)
    assert runs() == n                                               # same request, everything there: nothing runs
    for env, value in (("GENOMAD_AMD_STRAND", "both"), ("GENOMAD_AMD_REGION_PENALTY", "3"), ("GENOMAD_AMD_SCAN_STRIDE", "2000")):
        monkeypatch.setenv(env, value)
        fake_main(fa, out)
        n += 1
        assert runs() == n, env
        z = np.load(d1 / "m_nn_region_embeddings.npz")
        assert (int(z["stride"]), float(z["penalty"]), str(z["strand"])) == (
            int(nnc.scan_stride_requested()), float(nnc.region_penalty_requested()), nnc.strand_requested())
        fake_main(fa, out)
        assert runs() == n
    monkeypatch.delenv("GENOMAD_AMD_REGION_EMBEDDINGS")
    fake_main(fa, out)                                               # no request: the file goes
    assert runs() == n + 1 and not (d1 / "m_nn_region_embeddings.npz").exists() and (d1 / "m_nn_regions.npz").exists()


# ---- the gather over two ranks ------------------------------------------------------------------------------------------------
def _piece(key, n_contigs):
    rng = np.random.default_rng(key)
    per = rng.integers(0, 4, size=n_contigs)
    n = int(per.sum())
    return {"region_offsets": np.concatenate([[0], np.cumsum(per)]).astype(np.int64), "start": rng.integers(0, 9, n).astype(np.int64),
            "end": rng.integers(9, 99, n).astype(np.int64), "state": rng.integers(0, 3, n).astype(np.uint8),
            "count": rng.integers(0, 7, n).astype(np.int32), "embedding": rng.standard_normal((n, 512)).astype(np.float32),
            "coherence": rng.random(n, dtype=np.float32), "scores": rng.random((n, 3), dtype=np.float32)}


PIECES = {0: [(0, 3), (1, 0), (2, 5)], 1: [(64, 4), (65, 2)]}            # rank -> (piece key, contigs)


def _gloo_gather_worker(rank, world, port, q):
    from tests.gloo_comm import GlooComm
    comm = GlooComm(rank, world, port)
    out = sharding.gather_contig_region_embeddings(comm, [(k, _piece(k, n)) for k, n in PIECES[rank]])
    q.put((rank, out))
    comm.close()


def test_the_gather_over_two_gloo_ranks_is_the_gather_of_one():
    mp = pytest.importorskip("torch.multiprocessing")
    one = sharding.gather_contig_region_embeddings(None, [(k, _piece(k, n)) for r in (1, 0) for k, n in PIECES[r]])
    assert len(one["region_offsets"]) == 1 + 14 and one["region_offsets"][-1] == len(one["contig"]) == len(one["embedding"])
    assert (np.diff(one["contig"]) >= 0).all() and np.array_equal(np.bincount(one["contig"], minlength=14), np.diff(one["region_offsets"]))
    first = _piece(0, 3)
    assert np.array_equal(one["embedding"][:len(first["embedding"])], first["embedding"])
    none = sharding.gather_contig_region_embeddings(None, [])
    assert none["embedding"].shape == (0, 512) and len(none["contig"]) == 0 and list(none["region_offsets"]) == [0]
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_gather_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=180)
        assert p.exitcode == 0
    assert got[1] is None
    assert sorted(got[0]) == sorted(one)
    for k, v in one.items():
        assert got[0][k].dtype == v.dtype and np.array_equal(got[0][k], v), k
