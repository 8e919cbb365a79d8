"""What tests/test_regions_limits_gpu.py leans on, without a GPU: every input of tests/regions_limits_data.py has the property it is made
for under sequence.call_regions, and the two references that share no code with it - exact emissions over fractions, a Viterbi pass
that counts the ties it decides - agree with it, so a pass on the device means what it says.

Counted here (seed 3 of tie_track; `cells` are (bin, state) decisions anywhere, `path` those the path went through):

  penalty   stay on equality   switch, others tied   last bin shared
            cells     path     cells     path        contigs
  0.25      15598     3982     494       97          5
  0.5       12791     2365     423       56          5
  1          8094      945     112        8          6
  2          4535      337      20        0          3

On the first bin of a tile, on the path, over the four penalties: tile 4: 1805 stays, 42 switches; tile 7: 1061 and 26; tile 256: 31
and 2."""
import numpy as np
import pytest

from genomad_amd import sequence
from tests import regions_limits_data as rd

Q1 = rd.Q1


def same_regions(got, want):
    return all(got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]) for k in rd.KEYS)


# ---- emissions ---------------------------------------------------------------------------------------------------------------------

def test_every_edge_value_has_the_q_of_exact_arithmetic():
    e = rd.edge_values()
    assert e.dtype == np.float32 and len(e) == 20 and len(set(e.view(np.uint32).tolist())) == 20
    assert np.signbit(e[0]) and e[0] == 0 and 0 < e[2] < e[4] < np.finfo(np.float32).tiny and e[3] == -e[2]      # -0.0 and subnormals
    assert e[7] > e[6] and float(e[10]) * Q1 == 524288.5 and float(e[11]) * Q1 == Q1 - 0.0625 and e[13] > 1
    assert np.isinf(e[17:19]).all() and np.isnan(e[19]) and np.isfinite(e[:17]).all()
    assert [rd.exact_q(v) for v in e] == list(rd.EDGE_Q)                      # the fractions against the list written by hand
    for i, v in enumerate(e):                                                 # each value alone, in every column
        for col in range(3):
            row = np.full((1, 3), 0.25, np.float32)
            row[0, col] = v
            q, ev = sequence.region_emissions(row)
            want = [Q1 // 4] * 3
            want[col] = rd.EDGE_Q[i]
            assert ev[0] == (rd.EDGE_Q[i] is not None) and q[0].tolist() == (want if ev[0] else [0, 0, 0]), (i, col)


def test_the_edge_track_makes_every_emission_a_region_of_its_own():
    track, off = rd.edge_track()
    e = rd.edge_values()
    assert track.shape == (8000, 3) and len(off) == 8003 and (np.diff(off)[:8000] == 1).all() and off[-1] == off[-2] == off[-3] == 8000
    assert len({tuple(r) for r in track.view(np.uint32).tolist()}) == 8000    # every ordered triple once
    q, ev = sequence.region_emissions(track)
    xq, xev = rd.exact_emissions(track)
    assert q.dtype == xq.dtype and np.array_equal(q, xq) and np.array_equal(ev, xev)
    finite = np.isfinite(e)
    assert int(ev.sum()) == int(finite.sum()) ** 3 == 17 ** 3                 # evidence iff all three values are finite
    assert np.array_equal(ev, np.isfinite(track).all(axis=1))
    assert (q[~ev] == 0).all() and set(np.unique(q).tolist()) == {0, 1, 2, 524288, Q1}
    state, r = sequence.call_regions(track, off, 0)
    assert np.array_equal(r["contig"], np.arange(8000)) and (r["lo"] == 0).all() and (r["hi"] == 1).all()
    assert np.array_equal(r["qsum"], xq) and np.array_equal(r["evidence"], xev.astype(np.int64))
    assert np.array_equal(state, xq.argmax(axis=1)) and len(set(state.tolist())) == 3


# ---- ties --------------------------------------------------------------------------------------------------------------------------

def _on_seam(cells, tile):
    return sum(1 for _, b in cells if b % tile == 0)


def test_the_tie_track_decides_states_by_every_tie_rule_also_on_tile_seams():
    track, off = rd.tie_track()
    assert tuple(np.diff(off)) == rd.TIE_SIZES and rd.TIE_SIZES[:21] == rd.SIZES and rd.TIE_SIZES[21:] == (4095, 4096, 4097, 0)
    q, ev = sequence.region_emissions(track)
    assert set(np.unique(q).tolist()) == {0, Q1 // 4, Q1 // 2, Q1} and 0.4 < ev.mean() < 0.6
    seams = {t: [0, 0] for t in rd.TIE_TILES}
    for penalty in (0,) + rd.TIE_PENALTIES:
        P = sequence.region_penalty(penalty)
        state, counts = rd.counting_viterbi(q, off, P)
        want_state, want = rd.tie_reference(penalty)
        assert state.dtype == want_state.dtype and np.array_equal(state, want_state), penalty
        assert same_regions(rd.regions_of(state, q, ev, off), want), penalty
        cells = counts["cells"]
        print(f"\npenalty {penalty}: stay on equality {len(cells['stay_tie'])} cells, {len(counts['stay_tie'])} on the path; switch with "
              f"the others tied {len(cells['switch_tie'])} cells, {len(counts['switch_tie'])} on the path; last bin shared in "
              f"{len(counts['last_tie'])} contigs; {len(want['lo'])} regions")
        if penalty == 0:
            continue
        assert len(cells["stay_tie"]) >= 20 and len(cells["switch_tie"]) >= 20 and len(counts["last_tie"]) >= 3, penalty
        # a decision off the path changes no output: the path itself stays on equality at every penalty, and switches between tied
        # states where switches are frequent
        assert len(counts["stay_tie"]) >= 20, penalty
        assert len(counts["switch_tie"]) >= 20 or penalty >= 1, penalty
        for t in rd.TIE_TILES:
            seams[t][0] += _on_seam(counts["stay_tie"], t)
            seams[t][1] += _on_seam(counts["switch_tie"], t)
    print(f"\non the first bin of a tile, on the path: {seams}")
    assert all(a >= 1 and b >= 1 for a, b in seams.values()), seams


def test_the_sizes_part_of_the_tie_track_is_dense_in_regions_at_every_penalty():
    track, off = rd.tie_track()
    n = len(rd.SIZES)
    counts = [len(sequence.call_regions(track[:off[n]], off[:n + 1], p)[1]["lo"]) for p in (0, 0.25, 0.5, 1, 2)]
    assert counts == [334, 190, 109, 47, 25]


@pytest.mark.parametrize("T", (4, 7, 256))
@pytest.mark.parametrize("p", (1, 3))
def test_planted_ties_give_the_regions_written_by_hand(T, p):
    track, off, state, regions = rd.planted_ties(T, p)
    got_state, got = sequence.call_regions(track, off, p)
    assert got_state.dtype == state.dtype and np.array_equal(got_state, state)
    assert same_regions(got, regions)
    assert np.bincount(regions["contig"]).tolist() == [1, 2, 1, 3]
    q, ev = sequence.region_emissions(track)
    _, counts = rd.counting_viterbi(q, off, p * Q1)
    assert 0 in counts["last_tie"] and any(c == 2 for c, _ in counts["stay_tie"])        # the ties that were planted, on the path
    for c in range(4):                                                                   # the run lies on a multiple of T
        run = np.flatnonzero(track[off[c]:off[c + 1], 1] == 1)
        seam = T * -(-(3 * p + 3) // T)
        assert len(run) == (p, p + 1, 2 * p, 2 * p + 1)[c] and run[0] <= seam <= run[-1] and (len(run) == 1 or run[0] < seam)


def test_the_fine_track_shows_how_the_penalty_is_rounded():
    track, off = rd.fine_track()
    q, _ = sequence.region_emissions(track)
    assert set(np.unique(q).tolist()) == {0, 1, 2, 3, 4}
    by_P = {P: sequence.call_regions(track, off, P * 2.0 ** -20)[0] for P in (0, 1, 2)}
    assert not np.array_equal(by_P[0], by_P[1]) and not np.array_equal(by_P[1], by_P[2])
    # cutting the fraction off gives P = 1 at 3 * 2^-21 and at 1.5e-6, rounding a half up gives P = 1 at 2^-21: both show
    assert [int(p * Q1) for p, _ in rd.FINE_PENALTIES] == [0, 1, 2, 1, 1] and [P for _, P in rd.FINE_PENALTIES] == [0, 2, 2, 1, 2]
    for penalty, P in rd.FINE_PENALTIES:
        assert sequence.region_penalty(penalty) == P
        assert np.array_equal(sequence.call_regions(track, off, penalty)[0], by_P[P])
        assert np.array_equal(rd.counting_viterbi(q, off, P)[0], by_P[P])


# ---- the long track ----------------------------------------------------------------------------------------------------------------

def test_the_long_track_passes_1024_blocks_1024_tiles_and_2_to_the_32():
    track, off = rd.long_track()
    n_bins = int(off[-1])
    assert tuple(np.diff(off)) == rd.LONG_SIZES and n_bins == 262845 and -(-n_bins // 256) == 1027 > 1024
    assert -(-rd.LONG_SIZES[rd.LONG_CONTIG] // 256) == 1024
    assert 0.09 < np.isnan(track[:, 0]).mean() < 0.11
    q, ev = sequence.region_emissions(track)
    a, b = int(off[rd.LONG_CONTIG]), int(off[rd.LONG_CONTIG + 1])
    # penalty 4096: more than any path gains by a switch in this contig, so it is ONE region, and its sums need the high word
    state, r = rd.long_reference(4096)
    assert r["contig"].tolist() == [1, 2, 3, 5] and r["lo"].tolist() == [0] * 4 and r["hi"].tolist() == [5, 262139, 1, 700]
    assert np.array_equal(r["qsum"][1], q[a:b].sum(axis=0)) and (r["qsum"][1] > 1 << 32).all() and r["evidence"][1] == ev[a:b].sum()
    assert (r["qsum"][1] & 0xFFFFFFFF != r["qsum"][1]).all()
    # penalty 4: a region that begins and ends inside blocks of 256 bins and lies in four of them or more
    state, r = rd.long_reference(4)
    g0, g1 = off[r["contig"]] + r["lo"], off[r["contig"]] + r["hi"]
    inside = (g0 % 256 != 0) & (g1 % 256 != 0) & ((g1 - 1) // 256 - g0 // 256 + 1 >= 4)
    print(f"\nlong track, penalty 4: {len(g0)} regions, the longest {int((g1 - g0).max())} bins, {int(inside.sum())} across four blocks or more")
    flag = np.concatenate([[True], state[1:] != state[:-1]])
    flag[off[:-1][np.diff(off) > 0]] = True
    assert inside.any() and len(g0) == int(flag.sum()) > 500
