"""Representatives among encoder embeddings without a GPU: the numpy definition (sequence.greedy_representatives) against a sequential
brute-force walk on the planted rows under three priority orders, the round rule against the walk, the invariants of a greedy
clustering in fp64, what it does to a path single linkage chains, invalid rows, the edges of n, ties at the threshold on integer rows,
priority_order's errors, representative_table, the ABI's argument checks (before the ctx is looked at: no GPU needed), and main()'s
GENOMAD_AMD_REPRESENTATIVES switch over a fake engine served from the definition."""
import os

import numpy as np
import pytest

from genomad_amd import _lib, nn_classification as nnc, sequence
from genomad_amd.engine import NNEngine, RepresentativeResult
from tests.fake_engine import FakeEngine
from tests.neighbours_data import rows
from tests.representatives_data import PATH, THRESHOLD, conditioned, planted_path, sims64, walk, weightings
from tests.test_neighbours_host import SWITCHES, FakeNeighbourEngine
from tests.test_strand_host import _npz, _same_npz, _tree, _write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = ("index", "random", "reversed")


def same(got, want):
    """rep, size, rank exactly; sim bit for bit, NaN where the other has NaN"""
    return (all(np.asarray(a).dtype == np.int64 and np.array_equal(a, b) for a, b in ((got[0], want[0]), (got[2], want[2]), (got[3], want[3])))
            and got[1].dtype == np.float32 and np.array_equal(got[1], want[1], equal_nan=True))


@pytest.fixture(scope="module")
def plant():
    r, groups = planted_path()
    s64 = sims64(r, r)
    w = weightings(groups, len(r))
    return {"rows": r, "groups": groups, "s64": s64, "weights": w,
            "got": {k: sequence.greedy_representatives(r, THRESHOLD, w[k]) for k in ORDERS}}


@pytest.mark.parametrize("order", ORDERS)
def test_definition_equals_the_brute_force_walk_on_planted_rows(plant, order):
    w = plant["weights"][order]
    if order == "random":
        assert len(set(w)) < len(w) / 10                       # many ties: the index decides among them
    want = walk(plant["s64"].tolist(), float(np.float32(THRESHOLD)), None, w)
    got = plant["got"][order]
    assert conditioned(plant["s64"], float(np.float32(THRESHOLD)), want[0], want[3])      # what the exact comparisons on the GPU rest on
    assert same(got[:4], want)
    assert np.array_equal(got[3], np.argsort(np.argsort(-w, kind="stable"), kind="stable") if w is not None else np.arange(len(want[0])))


@pytest.mark.parametrize("order", ORDERS)
def test_the_round_rule_finds_the_representatives_of_the_walk(plant, order):
    w, s, n = plant["weights"][order], plant["s64"], len(plant["rows"])
    by_rank = sequence.priority_order(w, n)
    edge = s[np.ix_(by_rank, by_rank)] >= float(np.float32(THRESHOLD))
    is_rep, rounds = sequence.representative_rounds(edge, np.ones(n, bool))
    rep = walk(s.tolist(), float(np.float32(THRESHOLD)), None, w)[0]
    assert np.array_equal(by_rank[is_rep], np.flatnonzero(rep == np.arange(n))[np.argsort(plant["got"][order][3][rep == np.arange(n)])])
    assert rounds == plant["got"][order][4]
    print(f"\n{order}: {int(is_rep.sum())} representatives in {rounds} rounds")
    if order != "random":
        assert rounds == PATH                                  # a path walked end to end: as many rounds as it has rows


@pytest.mark.parametrize("order", ORDERS)
def test_invariants_of_a_greedy_clustering(plant, order):
    rep, sim, size, rank, _ = plant["got"][order]
    s, thr, n = plant["s64"], float(np.float32(THRESHOLD)), len(plant["rows"])
    reps = np.flatnonzero(rep == np.arange(n))
    between = s[np.ix_(reps, reps)][np.triu_indices(len(reps), 1)]
    assert (between < thr).all()                               # no two representatives within the threshold of each other
    for j in np.flatnonzero(rep != np.arange(n)):
        r = rep[j]
        assert rep[r] == r and rank[r] < rank[j] and s[r, j] >= thr and abs(float(sim[j]) - s[r, j]) <= 1e-7
        earlier = reps[(rank[reps] < rank[j]) & (s[reps, j] >= thr)]
        assert s[r, j] == s[earlier, j].max() and rank[r] == rank[earlier[s[earlier, j] == s[r, j]]].min()
    for j in reps:
        assert not ((rank[reps] < rank[j]) & (s[reps, j] >= thr)).any() and np.isnan(sim[j])
    assert np.array_equal(size, np.bincount(rep, minlength=n)[rep])


def test_a_path_is_cut_into_stars_where_single_linkage_chains(plant):
    r, path = plant["rows"], plant["groups"]["path"]
    label, _, csize, _ = sequence.threshold_clusters(r, THRESHOLD)
    assert len(set(label[path])) == 1 and (csize[path] == PATH).all()           # one cluster of 40
    rep, sim, size, rank, rounds = plant["got"]["index"]
    assert rounds == PATH
    assert list(rep[path]) == [p for p in path[0::2] for _ in range(2)]         # 20 stars of 2: every other row founds one
    assert (size[path] == 2).all() and np.isnan(sim[path[0::2]]).all() and np.allclose(sim[path[1::2]], 0.9375, atol=1e-6)
    rep, _, size, _, _ = plant["got"]["reversed"]                                # walked from the other end: the other rows found them
    assert list(rep[path]) == [p for p in path[1::2] for _ in range(2)] and (size[path] == 2).all()


@pytest.mark.parametrize("order", ORDERS)
def test_planted_families_and_the_chain_are_one_cluster_around_their_first_member(plant, order):
    rep, _, size, rank, _ = plant["got"][order]
    for name, members in plant["groups"].items():
        if name == "path":
            continue
        first = members[np.argmin(rank[members])]
        assert (rep[members] == first).all() and (size[members] == len(members)).all(), name


def test_invalid_rows_belong_to_nobody():
    r = np.tile(rows(1, 4), (7, 1))
    r[1] = 0
    r[3, 100] = np.nan
    r[5, 511] = np.inf
    rep, sim, size, rank, rounds = sequence.greedy_representatives(r, 0.5)
    assert list(rep) == [0, -1, 0, -1, 0, -1, 0] and list(size) == [4, 0, 4, 0, 4, 0, 4] and list(rank) == list(range(7)) and rounds == 2
    assert np.isnan(sim[[0, 1, 3, 5]]).all() and np.allclose(sim[[2, 4, 6]], 1.0, atol=1e-6) and sim.dtype == np.float32
    rep, sim, size, rank, rounds = sequence.greedy_representatives(r, 0.5, weight=[0, 9, 0, 9, 0, 9, 5])
    assert list(rep) == [6, -1, 6, -1, 6, -1, 6] and list(rank) == [4, 0, 5, 1, 6, 2, 3] and rounds == 2   # invalid rows have a rank too
    rep, _, size, _, _ = sequence.greedy_representatives(r, 0.0, metric="dot")     # a zero row is valid under dot: 0 >= 0
    assert list(rep) == [0, 0, 0, -1, 0, -1, 0] and list(size) == [5, 5, 5, 0, 5, 0, 5]
    rep, sim, size, rank, rounds = sequence.greedy_representatives(np.zeros((3, 512), np.float32), 0.5)
    assert list(rep) == [-1] * 3 and list(size) == [0] * 3 and np.isnan(sim).all() and rounds == 0


def test_edges_of_n_and_of_the_arguments():
    r = rows(9, 2)
    for n in (0, 1):
        rep, sim, size, rank, rounds = sequence.greedy_representatives(r[:n], 0.5)
        assert all(a.dtype == np.int64 and a.shape == (n,) for a in (rep, size, rank)) and sim.dtype == np.float32 and sim.shape == (n,)
        assert rounds == n and list(rep) == list(range(n)) and list(size) == [1] * n
    rep, sim, size, _, rounds = sequence.greedy_representatives(r, 1.0)             # above every similarity: everybody founds a cluster
    assert list(rep) == list(range(9)) and (size == 1).all() and np.isnan(sim).all() and rounds == 1
    rep, _, size, _, rounds = sequence.greedy_representatives(r, -1.0, weight=np.arange(9))
    assert (rep == 8).all() and (size == 9).all() and rounds == 2                   # the heaviest row stands for all
    for bad in (np.nan, np.inf, 1e39, "x"):
        with pytest.raises(ValueError, match="threshold"):
            sequence.greedy_representatives(r, bad)
    with pytest.raises(ValueError, match="metric"):
        sequence.greedy_representatives(r, 0.5, metric="euclid")
    with pytest.raises(ValueError, match="512"):
        sequence.greedy_representatives(r[:, :100], 0.5)


def integer_rows():
    rng = np.random.default_rng(11)
    base = rng.integers(0, 8, (200, 512)).astype(np.float32)          # every dot is an integer below 512 * 49 < 2^24
    base[40:60] = base[10]
    base[150] = base[3]
    base[199] = base[3]
    return base


def test_integer_dots_with_ties_at_the_threshold():
    r = integer_rows()
    dots = sims64(r, r, "dot")
    upper = dots[np.triu_indices(200, 1)]
    w = np.random.default_rng(3).integers(0, 4, 200)
    for threshold in (float(np.median(upper)), float(dots[0, 1])):
        assert (upper == threshold).sum() > 10                         # ties exactly at the threshold: edges
        for weight in (None, w):
            got = sequence.greedy_representatives(r, threshold, weight, "dot")
            assert same(got[:4], walk(dots.tolist(), threshold, None, weight))
    rep, sim, _, _, _ = sequence.greedy_representatives(r, float(dots[0, 1]), None, "dot")
    assert rep[1] == 0 and sim[1] == dots[0, 1]                        # row 1 holds on to row 0 by the tie alone


def test_a_tie_between_representatives_goes_to_the_smaller_rank():
    r = np.zeros((4, 512), np.float32)
    r[0, 0], r[1, 1], r[2, :2], r[3, :3] = 2, 2, (1, 1), (1, 1, 7)     # 0.1 = 0; 0.2 = 1.2 = 2; 0.3 = 1.3 = 2; 2.3 = 2
    rep, sim, size, _, rounds = sequence.greedy_representatives(r, 2.0, None, "dot")
    assert list(rep) == [0, 1, 0, 0] and list(size) == [3, 1, 3, 3] and list(sim[2:]) == [2.0, 2.0] and rounds == 2
    rep, _, _, rank, _ = sequence.greedy_representatives(r, 2.0, [0, 1, 0, 0], "dot")      # row 1 first: the tie goes to it now
    assert list(rep) == [0, 1, 1, 1] and list(rank) == [1, 0, 2, 3]


def test_priority_order():
    assert list(sequence.priority_order(None, 4)) == [0, 1, 2, 3] and sequence.priority_order(None, 0).dtype == np.int64
    assert list(sequence.priority_order([1, 3, 3, 0.5, 3], 5)) == [1, 2, 4, 0, 3]        # descending, ties by index
    assert list(sequence.priority_order(np.array([2, 2, 2], np.int32), 3)) == [0, 1, 2]
    for bad, word in (([1, 2], "shape"), (np.ones((3, 1)), "shape"), ([1, np.nan, 2], "finite"), ([np.inf, 0, 0], "finite"),
                      ([0, -np.inf, 0], "finite"), (["a", "b", "c"], "finite")):
        with pytest.raises(ValueError, match=word):
            sequence.priority_order(bad, 3)


def star_rows():
    """dots: 0 - 2, 0 - 3 (row 0 the hub), 1 - 4, 5 alone, 6 invalid"""
    r = np.zeros((7, 512), np.float32)
    for e, (a, b) in enumerate([(0, 2), (0, 3), (1, 4)]):
        r[a, e] = r[b, e] = 1
    r[3, 1] = 2                                                        # 0.3 = 2
    r[5, 9] = 1
    r[6, 0] = np.nan
    return r


def test_representative_table():
    out = sequence.greedy_representatives(star_rows(), 1.0, None, "dot")
    want = [{"rep": 0, "size": 3, "members": [0, 2, 3], "min_sim": 1.0}, {"rep": 1, "size": 2, "members": [1, 4], "min_sim": 1.0},
            {"rep": 5, "size": 1, "members": [5], "min_sim": None}]
    assert sequence.representative_table(out) == want
    assert sequence.representative_table(dict(zip(sequence.REPRESENTATIVE_FIELDS, out))) == want
    res = RepresentativeResult.build(out, 1.0, "dot")
    assert res.table() == want and res.n_clusters == 3 and list(res.is_rep) == [True, True, False, False, False, True, False]
    assert res.rounds == 2 and res.threshold == 1.0 and res.metric == "dot" and sorted(res.asdict()) == sorted(RepresentativeResult.FIELDS)
    assert res.table(list("abcdefg"))[0] == {"rep": "a", "size": 3, "members": ["a", "c", "d"], "min_sim": 1.0}
    by_weight = sequence.greedy_representatives(star_rows(), 1.0, [0, 0, 0, 5, 7, 0, 9], "dot")          # 4, then 3, then the rest
    assert sequence.representative_table(by_weight) == [
        {"rep": 4, "size": 2, "members": [4, 1], "min_sim": 1.0}, {"rep": 3, "size": 2, "members": [3, 0], "min_sim": 2.0},
        {"rep": 2, "size": 1, "members": [2], "min_sim": None}, {"rep": 5, "size": 1, "members": [5], "min_sim": None}]
    assert sequence.representative_table(sequence.greedy_representatives(star_rows()[:0], 1.0)) == []


def test_abi_declares_the_entry_points_and_checks_arguments_before_the_ctx():
    text = open(os.path.join(ROOT, "include", "genomad_nn.h")).read()
    lib = _lib.load()
    for name in ("gnn_representatives", "gnn_representatives_dev"):
        assert f"int {name}(" in text and name in _lib.SIGNATURES and hasattr(lib, name)
    assert "#define GNN_K_COUNT 8" in text
    for m in ("representatives", "representatives_dev"):
        assert hasattr(NNEngine, m)
    q = rows(2, 1)
    out = [np.full(2, 7, np.int64), np.full(2, 7, np.float32), np.full(2, 7, np.int64), np.full(1, 7, np.int64)]
    ptrs = [a.ctypes.data for a in out]
    for fn in (lib.gnn_representatives, lib.gnn_representatives_dev):
        name = b"gnn_representatives_dev" if fn is lib.gnn_representatives_dev else b"gnn_representatives:"
        for n in (-1, 1 << 31):
            assert fn(None, q.ctypes.data, n, 0.5, 0, *ptrs) == _lib.ERR_ARG
            assert f"{n} rows is outside [0, 2^31)".encode() in lib.gnn_last_error() and name in lib.gnn_last_error()
        for t, word in ((float("nan"), b"nan"), (float("inf"), b"inf"), (float("-inf"), b"-inf"), (1e39, b"inf")):
            assert fn(None, q.ctypes.data, 2, t, 0, *ptrs) == _lib.ERR_ARG
            assert b"threshold " + word in lib.gnn_last_error() and b"finite" in lib.gnn_last_error()
        for metric in (2, -1, 9):
            assert fn(None, q.ctypes.data, 2, 0.5, metric, *ptrs) == _lib.ERR_ARG
            assert f"metric {metric} is outside [0, 1]".encode() in lib.gnn_last_error()
        for hole in range(5):
            args = [q.ctypes.data] + ptrs
            args[hole] = None
            assert fn(None, args[0], 2, 0.5, 0, *args[1:]) == _lib.ERR_ARG
            assert b"the rows, the three outputs and rounds are required" in lib.gnn_last_error()
        assert fn(None, q.ctypes.data, 2, 0.5, 1, *ptrs) == _lib.ERR_ARG           # valid, but no ctx
        assert b"ctx is NULL" in lib.gnn_last_error()
        assert fn(None, None, 0, 0.5, 0, None, None, None, None) == _lib.ERR_ARG    # n = 0 needs no pointer, but a ctx
        assert b"ctx is NULL" in lib.gnn_last_error()
    assert all((a == 7).all() for a in out)                       # nothing was written


# ---- main() over a fake engine ---------------------------------------------------------------------------------------------------
class FakeRepresentativeEngine(FakeNeighbourEngine, FakeEngine):
    """the contig entry points main() calls from the stand-in of tests/test_neighbours_host.py, the rest of an engine from
    tests/fake_engine.py's, plus representatives, served from sequence.greedy_representatives"""
    calls = []

    def representatives(self, rows, threshold, weight=None, metric="cosine"):
        type(self).calls.append(("representatives", len(rows), float(threshold), None if weight is None else tuple(int(w) for w in weight), metric))
        return RepresentativeResult.build(sequence.greedy_representatives(rows, threshold, weight, metric), threshold, metric)


@pytest.fixture
def fake_main(monkeypatch):
    monkeypatch.setattr(nnc, "_engine", lambda: FakeRepresentativeEngine())
    for k in SWITCHES + ("GENOMAD_AMD_CLUSTERS", "GENOMAD_AMD_REPRESENTATIVES"):
        monkeypatch.delenv(k, raising=False)
    del FakeRepresentativeEngine.calls[:]
    return lambda fa, out, **kw: nnc.main(fa, out, False, 128, False, 1, False, False, **kw)


def test_representative_switch_values(monkeypatch):
    monkeypatch.delenv("GENOMAD_AMD_REPRESENTATIVES", raising=False)
    assert nnc.representatives_requested() is None
    for v, want in (("", None), (" 0.9 ", float(np.float32(0.9))), ("1", 1.0), ("-1", -1.0), ("0", 0.0), ("5e-1", 0.5)):
        monkeypatch.setenv("GENOMAD_AMD_REPRESENTATIVES", v)
        assert nnc.representatives_requested() == want
    for v in ("1.01", "-1.5", "nan", "inf", "high", "0,9"):
        monkeypatch.setenv("GENOMAD_AMD_REPRESENTATIVES", v)
        with pytest.raises(ValueError, match=r"GENOMAD_AMD_REPRESENTATIVES.*\[-1, 1\]"):
            nnc.representatives_requested()


def test_main_refuses_the_switch_without_embeddings(tmp_path, monkeypatch, fake_main, capsys):
    fa = tmp_path / "s.fna"
    _write_fasta(fa, n=3)
    monkeypatch.setenv("GENOMAD_AMD_REPRESENTATIVES", "1.5")
    with pytest.raises(ValueError, match="GENOMAD_AMD_REPRESENTATIVES"):
        fake_main(fa, tmp_path / "bad")
    assert not (tmp_path / "bad").exists()                  # before anything is written
    monkeypatch.setenv("GENOMAD_AMD_REPRESENTATIVES", "0.9")
    with pytest.raises(SystemExit) as exc:
        fake_main(fa, tmp_path / "refused")
    assert exc.value.code == 1
    err = capsys.readouterr().err
    assert "GENOMAD_AMD_REPRESENTATIVES needs GENOMAD_AMD_EMBEDDINGS=1" in err and len(err.strip().splitlines()) == 1
    assert not list((tmp_path / "refused").rglob("*.npz")) and not list((tmp_path / "refused").rglob("*.tsv"))
    assert FakeRepresentativeEngine.calls == []


def test_main_writes_both_files_weighs_by_kept_windows_and_removes_stale_ones(tmp_path, monkeypatch, fake_main):
    fa = tmp_path / "m.fna"
    recs = _write_fasta(fa, n=6)
    with open(fa, "a") as f:
        f.write(f">twin of c2\n{dict(recs)['c2']}\n")        # the same bytes as c2: the same embedding
    monkeypatch.setenv("GENOMAD_AMD_EMBEDDINGS", "1")
    fake_main(fa, tmp_path / "unset")
    assert not any(c[0] == "representatives" for c in FakeRepresentativeEngine.calls)
    monkeypatch.setenv("GENOMAD_AMD_REPRESENTATIVES", "0.999")
    out = tmp_path / "on"
    fake_main(fa, out)
    d0, d1 = tmp_path / "unset" / "m_nn_classification", out / "m_nn_classification"
    assert _tree(d1) == sorted(_tree(d0) + ["m_nn_representatives.npz", "m_nn_representatives.tsv"])
    for rel in _tree(d0):                                   # every other output: the same arrays, the same bytes
        if rel.endswith(".npz"):
            assert _same_npz(d0 / rel, d1 / rel), rel
        elif rel.endswith(".tsv"):
            assert (d0 / rel).read_bytes() == (d1 / rel).read_bytes(), rel
    z, emb, wid = _npz(d1 / "m_nn_representatives.npz"), _npz(d1 / "m_nn_embeddings.npz"), _npz(d1 / "m_encoded_sequences" / "m_seq_window_id.npz")
    names = list(z["contig_names"])
    n = len(names)
    t32 = float(np.float32(0.999))
    assert sorted(z) == ["contig_names", "metric", "rank", "rep", "rounds", "sim", "size", "threshold", "weight"]
    assert names == list(emb["contig_names"])
    assert float(z["threshold"]) == t32 and z["threshold"].dtype == np.float64 and str(z["metric"]) == "cosine"
    weight = np.bincount(wid["contig_ids"], minlength=n)                                    # the contig's kept windows
    assert z["weight"].dtype == np.int64 and np.array_equal(z["weight"], weight) and len(set(weight)) > 1
    assert FakeRepresentativeEngine.calls.count(("representatives", n, t32, tuple(int(w) for w in weight), "cosine")) == 1
    want = sequence.greedy_representatives(emb["embeddings"], 0.999, weight)
    assert same([z[k] for k in sequence.REPRESENTATIVE_FIELDS], want[:4]) and int(z["rounds"]) == want[4] == 2
    assert np.array_equal(z["rank"], np.argsort(np.argsort(-weight, kind="stable"), kind="stable"))       # ties in FASTA order
    a, b = sorted((names.index("c2"), names.index("twin")))
    assert list(z["rep"][[a, b]]) == [a, a] and list(z["size"][[a, b]]) == [2, 2] and np.isnan(z["sim"][a]) and abs(z["sim"][b] - 1) < 1e-6
    lines = (d1 / "m_nn_representatives.tsv").read_text().splitlines()
    assert lines[0] == "seq_name\trepresentative\tsimilarity\tcluster_size\tis_representative" and len(lines) == n + 1
    for i, line in enumerate(lines[1:]):
        own = z["rep"][i] == i
        assert line == f"{names[i]}\t{names[z['rep'][i]]}\t{'NA' if own else format(z['sim'][i], '.6f')}\t{z['size'][i]}\t{own}"
    assert lines[1 + b] == f"{names[b]}\t{names[a]}\t1.000000\t2\tFalse" and lines[1 + a] == f"{names[a]}\t{names[a]}\tNA\t2\tTrue"
    runs = lambda: sum(1 for c in FakeRepresentativeEngine.calls if c == "plain")       # noqa: E731
    before = runs()
    fake_main(fa, out)
    assert runs() == before                                  # same request, everything there: nothing runs
    monkeypatch.setenv("GENOMAD_AMD_REPRESENTATIVES", "-1")
    fake_main(fa, out)                                       # another threshold: recomputed
    z = _npz(d1 / "m_nn_representatives.npz")
    assert runs() == before + 1 and float(z["threshold"]) == -1.0 and (z["size"] == n).all()
    assert (z["rep"] == np.flatnonzero(z["rank"] == 0)[0]).all() and z["weight"][z["rep"][0]] == weight.max()
    (d1 / "m_nn_representatives.tsv").unlink()
    fake_main(fa, out)                                       # one of the pair is gone: recomputed
    assert runs() == before + 2 and (d1 / "m_nn_representatives.tsv").exists()
    monkeypatch.delenv("GENOMAD_AMD_REPRESENTATIVES")
    fake_main(fa, out)                                       # no request: both files go
    assert runs() == before + 3 and not (d1 / "m_nn_representatives.npz").exists() and not (d1 / "m_nn_representatives.tsv").exists()
    assert _tree(d1) == _tree(d0)
    monkeypatch.setenv("GENOMAD_AMD_REPRESENTATIVES", "0.5")
    monkeypatch.setenv("GENOMAD_AMD_CLUSTERS", "0.5")        # both clusterings in one run
    monkeypatch.setenv("GENOMAD_AMD_STRAND", "both")
    from tests.test_clusters_host import FakeClusterEngine
    from tests.test_strand_host import FakeStrandEngine
    FakeRepresentativeEngine.cluster = FakeClusterEngine.cluster
    FakeRepresentativeEngine.classify_contigs_strand = lambda self, seq, offsets, strand="both", single_window=False, precision=None, embed=False: (
        lambda r: (r[0], r[1], FakeRepresentativeEngine.embed_contigs(self, seq, offsets)[1], r[3], r[4]))(
            FakeStrandEngine.classify_contigs_strand(self, seq, offsets, strand, single_window, precision, embed))
    try:
        fake_main(fa, out)
    finally:
        del FakeRepresentativeEngine.classify_contigs_strand, FakeRepresentativeEngine.cluster
    assert str(_npz(d1 / "m_nn_representatives.npz")["strand"]) == "both" and str(_npz(d1 / "m_nn_clusters.npz")["strand"]) == "both"


def test_a_contig_without_a_valid_embedding_is_na_in_the_table(tmp_path):
    r = np.concatenate([rows(2, 3), np.zeros((1, 512), np.float32)])
    res = RepresentativeResult.build(sequence.greedy_representatives(r, -1.0, [1, 2, 3]), -1.0, "cosine")
    nnc.write_representatives_tsv(tmp_path / "t.tsv", ["a", "b", "c"], res)
    sim = format(res.sim[0], ".6f")
    assert (tmp_path / "t.tsv").read_text() == ("seq_name\trepresentative\tsimilarity\tcluster_size\tis_representative\n"
                                                f"a\tb\t{sim}\t2\tFalse\nb\tb\tNA\t2\tTrue\nc\tNA\tNA\t0\tFalse\n")
