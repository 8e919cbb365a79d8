"""CPU checks of the region calls (Viterbi over score tracks): sequence.call_regions against brute force over all paths, the stated
consequences of the definition, the region arrays, region_table, the quantisation, the argument checks of the C ABI (made before
the ctx is looked at: no GPU needed), and main()'s GENOMAD_AMD_REGION_PENALTY switch over a fake engine that serves call_regions
from sequence.call_regions."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

from genomad_amd import _lib, sequence
from genomad_amd import nn_classification as nnc
from genomad_amd.engine import RegionResult, ScanResult, StrandScanResult
from tests.test_strand_host import FakeStrandEngine, _npz, _same_npz, _tree, _window_scores, _write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q1 = 1 << 20
NAN = np.float32(np.nan)
REGION_KEYS = ("contig", "lo", "hi", "state", "evidence", "qsum")


def _objective(q, path, P):
    return sum(int(q[b, s]) for b, s in enumerate(path)) - P * sum(a != b for a, b in zip(path, path[1:]))


def _tracks():
    rng = np.random.default_rng(17)
    values = np.array([0, 0.25, 0.5, 1, np.nan], np.float32)
    out = []
    for n in range(1, 8):
        for _ in range(6):
            out.append(values[rng.integers(0, 5, (n, 3))])                   # tie-heavy, a NaN makes the bin non-evidence
            out.append(rng.random((n, 3), dtype=np.float32))
    return out


@pytest.mark.parametrize("P", [0, 1 << 18, 1 << 20, 1 << 32])
def test_call_regions_reaches_the_brute_force_maximum(P):
    penalty = P / Q1
    assert sequence.region_penalty(penalty) == P
    for track in _tracks():
        n = len(track)
        q, _ = sequence.region_emissions(track)
        best = max(_objective(q, path, P) for path in itertools.product(range(3), repeat=n))
        state, regions = sequence.call_regions(track, [0, n], penalty)
        assert _objective(q, [int(s) for s in state], P) == best, (track, P)
        assert len(regions["lo"]) == 1 + int((state[1:] != state[:-1]).sum())


def _mixed_track(seed=5, sizes=(0, 9, 0, 1, 40, 300, 0)):
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    track = rng.random((int(off[-1]), 3), dtype=np.float32)
    track[rng.random(len(track)) < 0.1] = NAN
    track[60:75] = NAN                                  # an interior uncovered run
    track[100:110] = (0.5, 0.5, 0)                      # exact ties
    return track, off


def test_zero_penalty_is_the_argmax_of_every_evidence_bin():
    track, off = _mixed_track()
    state, _ = sequence.call_regions(track, off, 0)
    q, ev = sequence.region_emissions(track)
    assert ev.sum() > 200 and (~ev).sum() > 20
    assert np.array_equal(state[ev], q[ev].argmax(axis=1))          # numpy's argmax is the lowest index
    assert (state[100:110] == 0).all()


def test_the_largest_penalty_gives_one_region_per_contig():
    track, off = _mixed_track()
    state, r = sequence.call_regions(track, off, 4096)
    nonempty = np.flatnonzero(np.diff(off) > 0)
    assert np.array_equal(r["contig"], nonempty) and (r["lo"] == 0).all() and np.array_equal(r["hi"], np.diff(off)[nonempty])
    assert np.array_equal(r["state"], r["qsum"].argmax(axis=1))      # the lowest argmax of qsum
    for c, s in zip(r["contig"], r["state"]):
        assert (state[off[c]:off[c + 1]] == s).all()


def test_a_contig_without_evidence_is_one_region_of_state_0():
    track = np.full((12, 3), NAN)
    track[3] = (np.inf, 0.2, 0.1)                       # an infinity is no evidence either
    for penalty in (0, 0.5, 4096):
        state, r = sequence.call_regions(track, [0, 5, 5, 12], penalty)
        assert (state == 0).all()
        assert r["contig"].tolist() == [0, 2] and r["lo"].tolist() == [0, 0] and r["hi"].tolist() == [5, 7]
        assert r["state"].tolist() == [0, 0] and r["evidence"].tolist() == [0, 0] and (r["qsum"] == 0).all()


@pytest.mark.parametrize("penalty", [0, 0.01, 0.25, 1, 30])
def test_an_interior_uncovered_run_never_makes_a_region_of_its_own(penalty):
    rng = np.random.default_rng(3)
    for _ in range(20):
        track = rng.random((60, 3), dtype=np.float32)
        a, b = sorted(rng.integers(1, 59, 2))
        track[a:b + 1] = NAN
        state, r = sequence.call_regions(track, [0, 60], penalty)
        assert (r["evidence"] > 0).all()                               # every region rests on some evidence
        inside = state[a:b + 1]
        switches = int((state[a:b + 2] != state[a - 1:b + 1]).sum())   # between bin a - 1 and bin b + 1
        assert switches <= 1                                           # the run takes its neighbours' states; it forces no switch
        assert set(inside.tolist()) <= {int(state[a - 1]), int(state[b + 1])}


def test_region_arrays_are_maximal_runs_with_exact_sums():
    track, off = _mixed_track(seed=8)
    q, ev = sequence.region_emissions(track)
    for penalty in (0, 0.25, 1, 7.5):
        state, r = sequence.call_regions(track, off, penalty)
        assert state.dtype == np.uint8 and r["state"].dtype == np.uint8 and r["qsum"].shape == (len(r["lo"]), 3)
        assert all(r[k].dtype == np.int64 for k in ("contig", "lo", "hi", "evidence", "qsum"))
        assert set(r["contig"].tolist()) == set(np.flatnonzero(np.diff(off) > 0).tolist())      # empty contigs have no region
        order = list(zip(r["contig"].tolist(), r["lo"].tolist()))
        assert order == sorted(order)
        for i in range(len(r["lo"])):
            c, lo, hi, s = int(r["contig"][i]), int(r["lo"][i]), int(r["hi"][i]), int(r["state"][i])
            a = int(off[c])
            assert 0 <= lo < hi <= off[c + 1] - a and (state[a + lo:a + hi] == s).all()
            assert lo == 0 or state[a + lo - 1] != s                   # maximal to the left ...
            assert hi == off[c + 1] - a or state[a + hi] != s          # ... and to the right, and never across a contig
            assert r["evidence"][i] == ev[a + lo:a + hi].sum() and np.array_equal(r["qsum"][i], q[a + lo:a + hi].sum(axis=0))
        covered = sum(int(h - l) for l, h in zip(r["lo"], r["hi"]))
        assert covered == len(track)


def test_bins_below_the_first_offset_belong_to_no_contig():
    track, off = _mixed_track()
    shifted = np.concatenate([np.full((7, 3), 0.9, np.float32), track])
    s0, r0 = sequence.call_regions(track, off, 0.25)
    s1, r1 = sequence.call_regions(shifted, off + 7, 0.25)
    assert (s1[:7] == 0).all() and np.array_equal(s1[7:], s0) and all(np.array_equal(r0[k], r1[k]) for k in REGION_KEYS)


def test_call_regions_refuses_bad_arguments():
    track = np.zeros((4, 3), np.float32)
    for penalty in (-1, 4097, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"\[0, 4096\]"):
            sequence.call_regions(track, [0, 4], penalty)
    with pytest.raises(ValueError, match="non-decreasing"):
        sequence.call_regions(track, [0, 3, 2, 4], 1)
    with pytest.raises(ValueError, match="negative"):
        sequence.call_regions(track, [-1, 4], 1)
    with pytest.raises(ValueError, match="4 bins"):
        sequence.call_regions(track, [0, 5], 1)


def test_region_table_clips_at_the_contig_length_and_derives_means_and_margins():
    regions = {"contig": np.array([0, 0, 2]), "lo": np.array([0, 3, 0]), "hi": np.array([3, 5, 2]), "state": np.array([2, 0, 0], np.uint8),
               "evidence": np.array([2, 0, 2]), "qsum": np.array([[Q1 // 2, Q1, 2 * Q1], [0, 0, 0], [Q1, Q1, 3]])}
    t = sequence.region_table(regions, [0, 4100, 4100, 5101], 1000)
    assert t["start"].tolist() == [0, 3000, 0] and t["end"].tolist() == [3000, 4100, 1001]       # min(hi * stride, L)
    assert np.array_equal(t["mean"][0], [0.25, 0.5, 1.0]) and np.isnan(t["mean"][1]).all()
    assert t["margin"].tolist() == [1.0, 0.0, 0.0]
    assert t["mean"].dtype == np.float64 and t["margin"].dtype == np.float64 and t["end"].dtype == np.int64
    empty = sequence.region_table({k: np.zeros((0, 3) if k == "qsum" else 0, np.int64) for k in REGION_KEYS}, [0, 10], 5)
    assert empty["mean"].shape == (0, 3) and len(empty["margin"]) == 0


def test_the_quantisation_clamps_drops_non_finite_bins_and_rounds_ties_to_even():
    f = np.float32
    half = f(2.0 ** -21)                               # half a step of 2^-20
    track = np.array([[-0.5, 1.5, 0.25], [np.inf, 0.5, 0.5], [0.5, -np.inf, 0.5], [0.5, 0.5, np.nan],
                      [half, 3 * half, 5 * half], [7 * half, 1 - half, 1], [-0.0, 2.0 ** -22, 3 * 2.0 ** -22]], f)
    q, ev = sequence.region_emissions(track)
    assert ev.tolist() == [True, False, False, False, True, True, True]
    assert q[0].tolist() == [0, Q1, Q1 // 4]
    assert (q[1:4] == 0).all()
    assert q[4].tolist() == [0, 2, 2] and q[5].tolist() == [4, Q1, Q1]        # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4: ties to even
    assert q[6].tolist() == [0, 0, 1]                                          # 0.25 -> 0, 0.75 -> 1: nearest
    assert q.dtype == np.int64
    for penalty, want in ((0, 0), (2.0 ** -21, 0), (3 * 2.0 ** -21, 2), (0.25, 1 << 18), (4096, 1 << 32)):
        assert sequence.region_penalty(penalty) == want


def test_abi_declares_the_region_entry_points_and_checks_arguments_before_the_ctx():
    text = open(os.path.join(ROOT, "include", "genomad_nn.h")).read()
    lib = _lib.load()
    for name in ("gnn_call_regions", "gnn_region_states_dev", "gnn_debug_set_region_tile"):
        assert f"int {name}(" in text and name in _lib.SIGNATURES and hasattr(lib, name)
    from genomad_amd.engine import NNEngine
    for m in ("call_regions", "region_states_dev", "scan_regions"):
        assert hasattr(NNEngine, m)
    off, n = np.array([0, 3, 5], np.int64), C.c_int64(-7)
    tail = (None, None, None, None, None, None, None, 0, C.byref(n))
    for penalty in (-1.0, 4097.0, float("nan")):
        assert lib.gnn_call_regions(None, None, off.ctypes.data, 2, penalty, *tail) == _lib.ERR_ARG
        assert b"[0, 4096]" in lib.gnn_last_error()
        assert lib.gnn_region_states_dev(None, None, off.ctypes.data, 2, penalty, None) == _lib.ERR_ARG
        assert b"[0, 4096]" in lib.gnn_last_error()
    bad = np.array([0, 3, 2], np.int64)
    assert lib.gnn_call_regions(None, None, bad.ctypes.data, 2, 1.0, *tail) == _lib.ERR_ARG
    assert b"non-decreasing" in lib.gnn_last_error() and b"[previous, 2^63)" in lib.gnn_last_error()
    neg = np.array([-1, 3, 5], np.int64)
    assert lib.gnn_call_regions(None, None, neg.ctypes.data, 2, 1.0, *tail) == _lib.ERR_ARG
    assert b"first bin offset -1" in lib.gnn_last_error() and b"[0, 2^63)" in lib.gnn_last_error()
    assert n.value == -7                                 # nothing was written


# ---- main() over a fake engine ---------------------------------------------------------------------------------------------------
class FakeRegionEngine(FakeStrandEngine):
    """The suite's stand-in for the contig entry points main() calls (tests/test_strand_host.py) plus scan_contigs, scan_contigs_strand -
    computed in numpy from the definitions of sequence.py - and call_regions, served from sequence.call_regions."""
    calls = []

    def _scan(self, seq, offsets, stride, single_window, strand):
        offsets = np.asarray(offsets, np.int64)
        starts, lens, ids, window_n, win_off, bin_off = sequence.scan_spans(offsets, stride, single_window)
        nn = np.array([np.count_nonzero(seq[a:a + l] == ord("N")) for a, l in zip(starts, lens)], dtype=np.int64)
        kept = (window_n == 0) | (nn <= sequence.MAX_N)
        f = _window_scores(sequence.materialize_spans(seq, starts, lens))
        r = _window_scores(sequence.revcomp_spans(seq, starts, lens))
        mode = {"forward": f, "reverse": r, "both": sequence.strand_mean(f, r)}[strand]
        track, cover = sequence.scan_track(mode, kept, lens, win_off, bin_off, stride)
        fields = dict(stride=int(stride), win_offsets=win_off, starts=window_n.astype(np.int64) * stride, lens=lens, kept=kept, scores=mode,
                      bin_offsets=bin_off, track=track, cover=cover, contig_scores=self._mean(len(offsets) - 1, ids, kept, mode))
        return fields, f, r

    def scan_contigs(self, seq, offsets, stride, single_window=False, precision=None):
        type(self).calls.append(("scan", int(stride)))
        return ScanResult(**self._scan(seq, offsets, stride, single_window, "forward")[0])

    def scan_contigs_strand(self, seq, offsets, stride, strand="both", single_window=False, precision=None):
        type(self).calls.append(("scan", int(stride), strand))
        fields, f, r = self._scan(seq, offsets, stride, single_window, strand)
        return StrandScanResult(**fields, strand=strand, scores_fwd=f, scores_rev=r)

    def call_regions(self, track, bin_offsets, penalty, offsets=None, stride=None):
        type(self).calls.append(("regions", float(penalty)))
        state, regions = sequence.call_regions(track, bin_offsets, penalty)
        return RegionResult.build(penalty, np.asarray(bin_offsets, np.int64), state, regions, offsets, stride)


SWITCHES = ("GENOMAD_AMD_FRONT_END", "GENOMAD_AMD_STRAND", "GENOMAD_AMD_EMBEDDINGS", "GENOMAD_AMD_SCAN_STRIDE", "GENOMAD_AMD_PRECISION",
            "GENOMAD_AMD_OCCLUSION_BLOCK", "GENOMAD_AMD_ATTRIBUTION_BIN", "GENOMAD_AMD_REGION_PENALTY")
NPZ_KEYS = ("contig_names", "stride", "penalty", "state", "bin_offsets", "region_contig", "region_lo", "region_hi", "region_state",
            "region_evidence", "region_qsum", "start", "end", "mean", "margin")
TSV_COLUMNS = ["seq_name", "start", "end", "class", "n_bins", "evidence_bins", "mean_chromosome", "mean_plasmid", "mean_virus", "margin"]


@pytest.fixture
def fake_main(monkeypatch):
    monkeypatch.setattr(nnc, "_engine", lambda: FakeRegionEngine())
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    del FakeRegionEngine.calls[:]
    return lambda fa, out, **kw: nnc.main(fa, out, False, 128, False, 1, False, False, **kw)


def test_region_switch_values(monkeypatch):
    monkeypatch.delenv("GENOMAD_AMD_REGION_PENALTY", raising=False)
    assert nnc.region_penalty_requested() is None
    for v, want in (("", None), (" 0 ", 0.0), ("0.25", 0.25), ("7.5", 7.5), ("4096", 4096.0), ("1e1", 10.0)):
        monkeypatch.setenv("GENOMAD_AMD_REGION_PENALTY", v)
        assert nnc.region_penalty_requested() == want
    for v in ("-1", "4096.5", "nan", "inf", "much"):
        monkeypatch.setenv("GENOMAD_AMD_REGION_PENALTY", v)
        with pytest.raises(ValueError, match=r"GENOMAD_AMD_REGION_PENALTY.*\[0, 4096\]"):
            nnc.region_penalty_requested()


def test_main_refuses_the_switch_without_a_scan_stride(tmp_path, monkeypatch, fake_main, capsys):
    fa = tmp_path / "s.fna"
    _write_fasta(fa, n=3)
    monkeypatch.setenv("GENOMAD_AMD_REGION_PENALTY", "4097")
    with pytest.raises(ValueError, match="GENOMAD_AMD_REGION_PENALTY"):
        fake_main(fa, tmp_path / "bad")
    assert not (tmp_path / "bad").exists()                  # before anything is written
    monkeypatch.setenv("GENOMAD_AMD_REGION_PENALTY", "1")
    with pytest.raises(SystemExit) as exc:
        fake_main(fa, tmp_path / "refused")
    assert exc.value.code == 1
    err = capsys.readouterr().err
    assert "GENOMAD_AMD_REGION_PENALTY needs GENOMAD_AMD_SCAN_STRIDE" in err and len(err.strip().splitlines()) == 1
    assert not list((tmp_path / "refused").rglob("*.npz")) and not list((tmp_path / "refused").rglob("*.tsv"))
    monkeypatch.setenv("GENOMAD_AMD_SCAN_STRIDE", "2000")
    monkeypatch.setenv("GENOMAD_AMD_FRONT_END", "host")     # and with it, the device front end
    with pytest.raises(SystemExit):
        fake_main(fa, tmp_path / "host")
    assert "needs the device front end" in capsys.readouterr().err
    assert FakeRegionEngine.calls == []


@pytest.mark.parametrize("strand", ["forward", "both"])
def test_main_writes_both_files_and_changes_nothing_else(tmp_path, monkeypatch, fake_main, strand):
    fa = tmp_path / "m.fna"
    _write_fasta(fa, n=7)
    monkeypatch.setenv("GENOMAD_AMD_SCAN_STRIDE", "1500")
    if strand != "forward":
        monkeypatch.setenv("GENOMAD_AMD_STRAND", strand)
    fake_main(fa, tmp_path / "unset")
    assert not any(c[0] == "regions" for c in FakeRegionEngine.calls)
    monkeypatch.setenv("GENOMAD_AMD_REGION_PENALTY", "0.05")
    fake_main(fa, tmp_path / "on")
    assert FakeRegionEngine.calls.count(("regions", 0.05)) == 1
    d0, d1 = tmp_path / "unset" / "m_nn_classification", tmp_path / "on" / "m_nn_classification"
    assert _tree(d1) == sorted(_tree(d0) + ["m_nn_regions.npz", "m_nn_regions.tsv"])
    for rel in _tree(d0):                                   # every other output: the same arrays, the same bytes
        if rel.endswith(".npz"):
            assert _same_npz(d0 / rel, d1 / rel), rel
        elif rel.endswith(".tsv"):
            assert (d0 / rel).read_bytes() == (d1 / rel).read_bytes(), rel
    names, seq, off = sequence.read_fasta_packed(fa)
    scan = _npz(d1 / "m_nn_scan.npz")
    state, regions = sequence.call_regions(scan["track"], scan["bin_offsets"], 0.05)
    table = sequence.region_table(regions, off, 1500)
    z = _npz(d1 / "m_nn_regions.npz")
    assert sorted(z) == sorted(NPZ_KEYS) and list(z["contig_names"]) == list(names)
    assert int(z["stride"]) == 1500 and z["stride"].dtype == np.int64 and float(z["penalty"]) == 0.05 and z["penalty"].dtype == np.float64
    assert np.array_equal(z["state"], state) and z["state"].dtype == np.uint8 and np.array_equal(z["bin_offsets"], scan["bin_offsets"])
    for k in REGION_KEYS:
        assert z["region_" + k].dtype == regions[k].dtype and np.array_equal(z["region_" + k], regions[k]), k
    for k in ("start", "end", "mean", "margin"):
        assert z[k].dtype == table[k].dtype and np.array_equal(z[k], table[k], equal_nan=True), k
    assert len(z["start"]) > len(names) and (z["end"] <= np.diff(off)[z["region_contig"]]).all()
    # the TSV parses back to the npz
    lines = (d1 / "m_nn_regions.tsv").read_text().splitlines()
    assert lines[0].split("\t") == TSV_COLUMNS and len(lines) == 1 + len(z["start"])
    classes = [c[:-len("_score")] for c in nnc.TSV_HEADER.split()[1:]]
    assert classes == ["chromosome", "plasmid", "virus"]
    for i, line in enumerate(lines[1:]):
        f = line.split("\t")
        assert f[0] == names[z["region_contig"][i]] and int(f[1]) == z["start"][i] and int(f[2]) == z["end"][i]
        assert f[3] == classes[z["region_state"][i]] and int(f[4]) == z["region_hi"][i] - z["region_lo"][i]
        assert int(f[5]) == z["region_evidence"][i] and f[6:9] == [f"{x:.4f}" for x in z["mean"][i]] and f[9] == f"{z['margin'][i]:.4f}"


def test_main_resume_follows_stride_and_penalty_and_removes_stale_files(tmp_path, monkeypatch, fake_main):
    fa = tmp_path / "r.fna"
    _write_fasta(fa, seed=4, n=5)
    out = tmp_path / "out"
    d = out / "r_nn_classification"
    runs = lambda: sum(1 for c in FakeRegionEngine.calls if c == "plain")       # noqa: E731
    monkeypatch.setenv("GENOMAD_AMD_SCAN_STRIDE", "3000")
    fake_main(fa, out)
    before = {rel: (d / rel).read_bytes() for rel in _tree(d) if rel.endswith(".tsv")}
    monkeypatch.setenv("GENOMAD_AMD_REGION_PENALTY", "2")
    fake_main(fa, out)                                       # scores on disk, no regions: the stage runs again
    assert runs() == 2 and float(_npz(d / "r_nn_regions.npz")["penalty"]) == 2.0
    first = _npz(d / "r_nn_regions.npz")
    fake_main(fa, out)
    assert runs() == 2                                       # same request, everything there: nothing runs
    monkeypatch.setenv("GENOMAD_AMD_REGION_PENALTY", "0")
    fake_main(fa, out)                                       # another penalty: recomputed
    assert runs() == 3 and float(_npz(d / "r_nn_regions.npz")["penalty"]) == 0.0
    assert len(_npz(d / "r_nn_regions.npz")["start"]) > len(first["start"])
    monkeypatch.setenv("GENOMAD_AMD_SCAN_STRIDE", "2000")
    fake_main(fa, out)                                       # another stride
    assert runs() == 4 and int(_npz(d / "r_nn_regions.npz")["stride"]) == 2000
    (d / "r_nn_regions.tsv").unlink()
    fake_main(fa, out)                                       # half of the pair is gone
    assert runs() == 5 and (d / "r_nn_regions.tsv").exists()
    monkeypatch.delenv("GENOMAD_AMD_REGION_PENALTY")
    monkeypatch.setenv("GENOMAD_AMD_SCAN_STRIDE", "3000")
    fake_main(fa, out)                                       # no request: both files go, every other output is the first run's
    assert runs() == 6 and not (d / "r_nn_regions.npz").exists() and not (d / "r_nn_regions.tsv").exists()
    assert {rel: (d / rel).read_bytes() for rel in _tree(d) if rel.endswith(".tsv")} == before
    fake_main(fa, out)
    assert runs() == 6
