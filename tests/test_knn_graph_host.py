"""The k-nearest-neighbour graph, host side (no GPU): ``sequence.knn_graph`` against a brute force over Python sets, its invariants,
the consumers' contract, the plant that a single threshold cannot serve, the argument errors and ``main()`` over a fake engine."""
import itertools
import shutil

import numpy as np
import pytest

from genomad_amd import nn_classification as nnc, sequence
from genomad_amd.engine import GraphResult, KNNGraphResult
from tests.test_analyses_host import ENV as OTHER_ENV, FakeAnalysisEngine, fake_main, same_file
from tests.test_strand_host import _npz, _same_npz, _tree, _write_fasta

MODES, WEIGHTS, KS = sequence.KNN_GRAPH_MODES, sequence.KNN_GRAPH_WEIGHTS, (1, 2, 7, 64)


def mixed_rows(n=40, seed=5):
    """mixed-sign rows with a zero row, a NaN row, an Inf row and duplicates (ties go to the smaller index)"""
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, 512)).astype(np.float32)
    rows[3] = 0
    rows[11, 7] = np.nan
    rows[20, 500] = np.inf
    rows[17] = rows[5]
    rows[30] = rows[5]
    rows[31] = 2 * rows[8]
    return rows


def integer_rows(n=33, seed=9):
    """small integers, few of them non-zero: exact dot products with many ties, and a zero row, which is valid under dot"""
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 512), dtype=np.float32)
    for i in range(n):
        rows[i, rng.choice(12, size=4, replace=False)] = rng.integers(-2, 3, size=4)
    rows[4] = 0
    return rows


def brute(rows, k, mode, weight, metric):
    """the issue's wording, over Python sets: (indptr, col, sim, mutual) as lists"""
    idx, sim = sequence.nearest_neighbours(rows, None, k, metric)
    n = len(rows)
    N = [set(int(j) for j in idx[i] if j >= 0) for i in range(n)]
    value = {(i, int(j)): sim[i, s] for i in range(n) for s, j in enumerate(idx[i]) if j >= 0}
    edges = []
    for i, j in itertools.combinations(range(n), 2):
        fwd, back = j in N[i], i in N[j]
        if (fwd and back) if mode == "mutual" else (fwd or back):
            if weight == "similarity":
                w = value[(i, j)] if fwd else value[(j, i)]
            else:
                s = len((N[i] | {i}) & (N[j] | {j}))
                w = np.float32(s) / np.float32(len(N[i]) + 1 + len(N[j]) + 1 - s)
            edges.append((i, j, np.float32(w), int(fwd and back)))
    indptr = np.zeros(n + 1, dtype=np.int64)
    for i, _, _, _ in edges:
        indptr[i + 1] += 1
    return np.cumsum(indptr), [e[1] for e in edges], [e[2] for e in edges], [e[3] for e in edges]


def assert_is_brute(rows, k, mode, weight, metric):
    g = sequence.knn_graph(rows, k, mode, weight, metric)
    indptr, col, sim, mutual = brute(rows, k, mode, weight, metric)
    assert g["indptr"].dtype == np.int64 and g["col"].dtype == np.int32 and g["sim"].dtype == np.float32
    assert g["mutual"].dtype == np.uint8 and g["valid"].dtype == bool
    assert np.array_equal(g["indptr"], indptr) and g["col"].tolist() == col and g["mutual"].tolist() == mutual
    assert g["sim"].view(np.uint32).tolist() == np.array(sim, dtype=np.float32).view(np.uint32).tolist()
    assert np.array_equal(g["valid"], sequence.valid_rows(rows, metric))
    return g


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("weight", WEIGHTS)
def test_the_definition_equals_the_brute_force_over_sets(mode, weight):
    rows = mixed_rows()
    for k in KS:
        g = assert_is_brute(rows, k, mode, weight, "cosine")
        assert not g["valid"][[3, 11, 20]].any() and g["valid"].sum() == 37
        assert_is_brute(rows[:5], k, mode, weight, "cosine")              # n <= k: the lists are padded
        assert_is_brute(integer_rows(), k, mode, weight, "dot")
    assert_is_brute(rows[:1], 3, mode, weight, "cosine")
    g = sequence.knn_graph(rows[:0], 3, mode, weight)
    assert g["indptr"].tolist() == [0] and len(g["col"]) == len(g["sim"]) == len(g["mutual"]) == len(g["valid"]) == 0


def test_duplicate_rows_tie_to_the_smaller_index():
    rows = mixed_rows()
    g = sequence.knn_graph(rows, 1, "union")
    a, b = sequence.graph_edges(g["indptr"], g["col"])
    pairs = set(zip(a.tolist(), b.tolist()))
    # rows 5, 17 and 30 are one row: 5 lists 17, 17 lists 5, 30 lists 5 (not 17)
    assert {(5, 17), (5, 30)} <= pairs and (17, 30) not in pairs


@pytest.mark.parametrize("rows,metric", [(mixed_rows(), "cosine"), (integer_rows(), "dot")])
def test_the_invariants(rows, metric):
    ok = sequence.valid_rows(rows, metric)
    for k in KS:
        union = sequence.knn_graph(rows, k, "union", "similarity", metric)
        mutual = sequence.knn_graph(rows, k, "mutual", "similarity", metric)
        for g in (union, mutual):
            a, b = sequence.graph_edges(g["indptr"], g["col"])
            assert (b > a).all() and ok[a].all() and ok[b].all()
            assert all((np.diff(g["col"][p:q]) > 0).all() for p, q in zip(g["indptr"][:-1], g["indptr"][1:]))
            assert len(g["col"]) <= ok.sum() * k
        # the mutual graph is the union graph filtered by its flag
        keep = union["mutual"] == 1
        ua, ub = sequence.graph_edges(union["indptr"], union["col"])
        ma, mb = sequence.graph_edges(mutual["indptr"], mutual["col"])
        assert np.array_equal(ua[keep], ma) and np.array_equal(ub[keep], mb) and (mutual["mutual"] == 1).all()
        assert np.array_equal(union["sim"][keep].view(np.uint32), mutual["sim"].view(np.uint32))
        deg_u = sequence.graph_degree(union["indptr"], union["col"])
        deg_m = sequence.graph_degree(mutual["indptr"], mutual["col"])
        if ok.sum() - 1 >= k:
            assert (deg_u[ok] >= k).all()
        assert (deg_m <= k).all() and (deg_u[~ok] == 0).all()
        for mode in MODES:
            j = sequence.knn_graph(rows, k, mode, "jaccard", metric)
            assert ((j["sim"] > 0) & (j["sim"] <= 1)).all()
            assert np.array_equal(j["col"], (union if mode == "union" else mutual)["col"])


def test_jaccard_on_a_hand_worked_case():
    """N+(0) = N+(1) = {0, 1, 2}, N+(2) = {1, 2, 3}, N+(3) = {2, 3}"""
    rows = np.random.default_rng(1).standard_normal((4, 512)).astype(np.float32)
    idx = np.array([[1, 2], [2, 0], [3, 1], [2, -1]], dtype=np.int64)
    sim = np.array([[.5, .25], [.75, .5], [.125, .75], [.25, np.nan]], dtype=np.float32)
    g = sequence.knn_graph(rows, 2, "union", "jaccard", neighbours=(idx, sim))
    assert g["indptr"].tolist() == [0, 2, 3, 4, 4] and g["col"].tolist() == [1, 2, 2, 3] and g["mutual"].tolist() == [1, 0, 1, 1]
    assert g["sim"].tolist() == [1.0, 0.5, 0.5, float(np.float32(2) / np.float32(3))]
    s = sequence.knn_graph(rows, 2, "union", "similarity", neighbours=(idx, sim))
    # (2, 3): 3 is in N(2), so row 2's value .125 stands, not row 3's .25; (0, 2): only row 0 lists the other
    assert s["sim"].tolist() == [.5, .25, .75, .125]
    m = sequence.knn_graph(rows, 2, "mutual", "jaccard", neighbours=(idx, sim))
    assert m["col"].tolist() == [1, 2, 3] and m["sim"].tolist() == [1.0, 0.5, float(np.float32(2) / np.float32(3))]
    assert sequence.knn_graph_table(s["indptr"], s["col"], s["sim"], s["mutual"], names=list("abcd"))[1] == \
        {"a": "a", "b": "c", "weight": .25, "mutual": False}


def exact_rows(n=24, seed=3):
    """sixteen entries of +-1 per row: the norm is 4 and every cosine a multiple of 1/16 - exact in every arithmetic"""
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 512), dtype=np.float32)
    for i in range(n):
        rows[i, rng.choice(40, size=16, replace=False)] = rng.choice([-1.0, 1.0], size=16)
    return rows


@pytest.mark.parametrize("rows", [exact_rows(), mixed_rows()])
def test_where_j_is_in_the_list_of_i_the_weight_has_the_bits_of_the_threshold_graphs_value(rows):
    indptr, col, sim = sequence.threshold_graph(rows, -1.0)
    a, b = sequence.graph_edges(indptr, col)
    graph = {(i, j): np.float32(s) for i, j, s in zip(a.tolist(), b.tolist(), sim)}
    for k in (2, 7):
        idx, _ = sequence.nearest_neighbours(rows, None, k)
        g = sequence.knn_graph(rows, k)
        ga, gb = sequence.graph_edges(g["indptr"], g["col"])
        listed = [(i, j, s) for i, j, s in zip(ga.tolist(), gb.tolist(), g["sim"]) if j in idx[i]]
        assert len(listed) > len(ga) // 4
        assert all(s.view(np.uint32) == graph[(i, j)].view(np.uint32) for i, j, s in listed)


def test_the_consumers_take_the_csr():
    """k = 64 on 14 rows lists every pair, the negative similarities among them: they are kept, and the consumers drop them"""
    for (k, rows), mode, weight in itertools.product(((7, mixed_rows()), (64, mixed_rows()[:14])), MODES, WEIGHTS):
        g = sequence.knn_graph(rows, k, mode, weight)
        csr = (g["indptr"], g["col"], g["sim"], g["valid"])
        if weight == "similarity" and k == 64:
            assert (g["sim"] < 0).any() and (g["sim"] > 0).any()
        assert len(sequence.mcl_weights(*csr)) > 0 and len(sequence.spread_transitions(*csr)) > 0
        tree = sequence.average_linkage(*csr)
        comm = sequence.modularity_communities(*csr)
        assert len(tree["a"]) > 0 and len(comm["label"]) == len(rows)
        assert ((comm["label"] >= 0) == g["valid"]).all()
        res = KNNGraphResult.build((g["indptr"], g["col"], g["sim"], g["mutual"]), g["valid"], k, mode, weight, "cosine")
        assert isinstance(res, GraphResult) and res.n_edges == len(g["col"]) and res.k == k and res.mode == mode and res.weight == weight
        assert np.array_equal(res.degree(), sequence.graph_degree(g["indptr"], g["col"])) and len(res.edges()[0]) == res.n_edges
        assert len(res.symmetric()[1]) == 2 * res.n_edges and len(res.components()) == len(rows) and len(res.table()) == res.n_edges


# ---- the plant that one threshold cannot serve ------------------------------------------------------------------------------------------
# A tight family of 10 (each row sqrt(.9) of its centre) inside a halo of 30 rows that carry sqrt(.45) of the same centre, a loose
# family of 12 (sqrt(.2) of another centre) and 20 rows of background noise; unit noise in 512 dimensions has a cosine of 0 +- .044.
# Inside the tight family the cosine is about .9, between it and the halo .64, inside the halo .45, inside the loose family .2.
# Where the loose family has its edges (t <= .2) the tight family and its halo are one weighted clique that modularity does not
# split; where the halo has let go of the tight family (t >= .7) the loose family has no edge left.  With k = 9 the tight family's
# lists hold exactly its 9 other members and the loose family's 9 of its 11 others: the mutual graph cuts both free.
PLANT = dict(seed=7, tight=10, halo=30, loose=12, noise=20, a_tight=.9, a_halo=.45, a_loose=.2, k=9)
THRESHOLD_GRID = tuple(round(0.05 * i, 2) for i in range(1, 20))


def plant(seed, tight, halo, loose, noise, a_tight, a_halo, a_loose, k):
    rng = np.random.default_rng(seed)

    def unit(m):
        x = rng.standard_normal((m, 512))
        return x / np.linalg.norm(x, axis=1, keepdims=True)

    c1, c2 = unit(1)[0], unit(1)[0]
    parts = [np.sqrt(a_tight) * c1 + np.sqrt(1 - a_tight) * unit(tight), np.sqrt(a_halo) * c1 + np.sqrt(1 - a_halo) * unit(halo),
             np.sqrt(a_loose) * c2 + np.sqrt(1 - a_loose) * unit(loose), unit(noise)]
    rows = np.concatenate(parts).astype(np.float32)
    order = rng.permutation(len(rows))
    family = np.repeat(np.arange(4), [tight, halo, loose, noise])
    return rows[order], family[order]


def whole(label, members) -> bool:
    """the members are one community, and nobody else is in it"""
    label = np.asarray(label)
    return len(set(label[members].tolist())) == 1 and (label == label[members][0]).sum() == len(members)


def test_no_threshold_returns_both_families_whole_and_the_mutual_jaccard_graph_does():
    rows, family = plant(**PLANT)
    tight, loose = np.flatnonzero(family == 0), np.flatnonzero(family == 2)
    verdicts = []
    for t in THRESHOLD_GRID:
        indptr, col, sim = sequence.threshold_graph(rows, t)
        label = sequence.modularity_communities(indptr, col, sim.astype(np.float32))["label"]
        verdicts.append((whole(label, tight), whole(label, loose)))
    assert not any(a and b for a, b in verdicts)
    assert any(a for a, _ in verdicts) and any(b for _, b in verdicts)      # each family has its threshold; they have none in common
    g = sequence.knn_graph(rows, PLANT["k"], "mutual", "jaccard")
    label = sequence.modularity_communities(g["indptr"], g["col"], g["sim"], g["valid"])["label"]
    assert whole(label, tight) and whole(label, loose)


# ---- arguments ------------------------------------------------------------------------------------------------------------------------

def test_argument_errors_carry_the_value_and_the_range():
    rows = mixed_rows()[:8]
    for k in (0, 65, -3):
        with pytest.raises(ValueError, match=rf"k {k} is outside \[1, 64\]"):
            sequence.knn_graph(rows, k)
    with pytest.raises(ValueError, match=r"mode 'both' is outside \('union', 'mutual'\)"):
        sequence.knn_graph(rows, 3, mode="both")
    with pytest.raises(ValueError, match=r"weight 'snn' is outside \('similarity', 'jaccard'\)"):
        sequence.knn_graph(rows, 3, weight="snn")
    with pytest.raises(ValueError, match="metric 'l2'"):
        sequence.knn_graph(rows, 3, metric="l2")
    with pytest.raises(ValueError, match=r"\(n, 512\) rows are required"):
        sequence.knn_graph(rows[:, :100], 3)
    assert sequence.knn_graph_mode("mutual") == "mutual" and sequence.knn_graph_weight("jaccard") == "jaccard"


# ---- main() over a fake engine ------------------------------------------------------------------------------------------------------------

KNN_ENV = ("GENOMAD_AMD_KNN_GRAPH", "GENOMAD_AMD_KNN_GRAPH_MODE", "GENOMAD_AMD_KNN_GRAPH_WEIGHT")
BASE = {"GENOMAD_AMD_EMBEDDINGS": "1"}
FILES = ["m_nn_knn_graph.npz", "m_nn_knn_graph.tsv"]


class FakeKnnEngine(FakeAnalysisEngine):
    """the stand-in of tests/test_analyses_host.py plus the k-nearest-neighbour graph from sequence.knn_graph"""

    def knn_graph(self, rows, k=15, mode="union", weight="similarity", metric="cosine"):
        type(self).calls.append(("knn_graph", len(rows), int(k), mode, weight, metric))
        g = sequence.knn_graph(rows, k, mode, weight, metric)
        return KNNGraphResult.build((g["indptr"], g["col"], g["sim"], g["mutual"]), g["valid"], k, mode, weight, metric)


def set_env(mp, env):
    """exactly the switches of ``env``, none of the others"""
    mp.setattr(nnc, "_engine", lambda: FakeKnnEngine())
    for k in OTHER_ENV + KNN_ENV + ("GENOMAD_AMD_COMMUNITIES", "GENOMAD_AMD_COMMUNITIES_MAX_LEVELS"):
        mp.delenv(k, raising=False)
    for k, v in env.items():
        mp.setenv(k, v)


def names_of_calls():
    return [c[0] if isinstance(c, tuple) else c for c in FakeKnnEngine.calls]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """one run with the embeddings but without GENOMAD_AMD_KNN_GRAPH and one with it, shared and left unchanged.  The contigs: c0 ..
    c5, one run of N and two twins of c2."""
    root = tmp_path_factory.mktemp("knn_graph")
    fa = root / "m.fna"
    recs = _write_fasta(fa, n=6)
    with open(fa, "a") as f:
        for k in range(2):
            f.write(f">twin{k} of c2\n{dict(recs)['c2']}\n")
    with pytest.MonkeyPatch.context() as mp:
        set_env(mp, BASE)
        fake_main(fa, root / "unset")
        on = dict(BASE, GENOMAD_AMD_KNN_GRAPH="2")
        set_env(mp, on)
        del FakeKnnEngine.calls[:]
        fake_main(fa, root / "on")
        found = list(FakeKnnEngine.calls)
    return {"fa": fa, "env": on, "unset": root / "unset" / "m_nn_classification", "on": root / "on", "calls": found}


def copy_of(world, tmp_path):
    out = tmp_path / "on"
    shutil.copytree(world["on"], out)
    return out, out / "m_nn_classification"


def test_the_switch_adds_its_two_files_and_changes_nothing_else(world):
    d0, d1 = world["unset"], world["on"] / "m_nn_classification"
    assert _tree(d1) == sorted(_tree(d0) + FILES)
    for rel in _tree(d0):                                       # every other output: the same arrays, the same bytes
        if rel.endswith(".npz"):
            assert _same_npz(d0 / rel, d1 / rel), rel
        elif rel.endswith(".tsv"):
            assert (d0 / rel).read_bytes() == (d1 / rel).read_bytes(), rel
    calls = [c for c in world["calls"] if isinstance(c, tuple)]
    assert calls == [("knn_graph", 9, 2, "union", "similarity", "cosine")]
    log = [line for line in (world["on"] / "m_nn_classification.log").read_text().splitlines() if " written to " in line]
    assert log[-1].endswith("written to m_nn_knn_graph.npz and m_nn_knn_graph.tsv.")
    assert "k-nearest-neighbour graph of the sequences (2 neighbours per sequence, cosine similarity of the encoder embeddings, union, " \
           "weighted by similarity: " in log[-1]


def test_the_files_hold_the_definition(world):
    d = world["on"] / "m_nn_classification"
    z, emb = _npz(d / FILES[0]), _npz(d / "m_nn_embeddings.npz")
    want = sequence.knn_graph(emb["embeddings"], 2)
    for k in sequence.KNN_GRAPH_FIELDS:
        assert z[k].dtype == want[k].dtype and np.array_equal(z[k], want[k]), k
    assert z["k"] == 2 and str(z["mode"]) == "union" and str(z["weight"]) == "similarity" and str(z["metric"]) == "cosine" and "strand" not in z
    names = [str(x) for x in z["contig_names"]]
    lines = (d / FILES[1]).read_bytes().decode().split("\n")
    assert lines[0] == "contig_a\tcontig_b\tweight" and lines[-1] == "" and len(lines) == len(want["col"]) + 2
    a, b = sequence.graph_edges(want["indptr"], want["col"])
    assert lines[1:-1] == [f"{names[i]}\t{names[j]}\t{float(s):.6f}" for i, j, s in zip(a, b, want["sim"])]
    # c2 and its twins are one row: with k = 2 they list each other and nobody else
    c2, t0, t1 = (names.index(x) for x in ("c2", "twin0", "twin1"))
    pairs = dict(zip(zip(a.tolist(), b.tolist()), want["mutual"].tolist()))
    assert pairs[(c2, t0)] == pairs[(c2, t1)] == pairs[(t0, t1)] == 1


def test_the_same_command_again_calls_nothing_and_another_request_runs_again(world, tmp_path, monkeypatch):
    out, d = copy_of(world, tmp_path)
    everything = _tree(d)
    on = world["env"]
    set_env(monkeypatch, on)
    del FakeKnnEngine.calls[:]
    fake_main(world["fa"], out)
    assert FakeKnnEngine.calls == []
    runs = 0
    for env, entry in ((dict(on, GENOMAD_AMD_KNN_GRAPH="3"), ("k", 3)), (dict(on, GENOMAD_AMD_KNN_GRAPH_MODE="mutual"), ("mode", "mutual")),
                       (dict(on, GENOMAD_AMD_KNN_GRAPH_WEIGHT="jaccard"), ("weight", "jaccard")), (on, ("k", 2))):
        set_env(monkeypatch, env)
        fake_main(world["fa"], out)                             # another k, mode or weight: the stage runs again
        runs += 1
        assert names_of_calls().count("plain") == runs and _npz(d / FILES[0])[entry[0]] == entry[1] and _tree(d) == everything
        fake_main(world["fa"], out)                             # and is resumed from
        assert names_of_calls().count("plain") == runs
    assert same_file(d / FILES[0], world["on"] / "m_nn_classification" / FILES[0])
    assert (d / FILES[1]).read_bytes() == (world["on"] / "m_nn_classification" / FILES[1]).read_bytes()
    (d / FILES[1]).unlink()
    fake_main(world["fa"], out)                                 # one of the pair is gone: again
    assert names_of_calls().count("plain") == runs + 1 and _tree(d) == everything
    set_env(monkeypatch, BASE)                                  # unset again: its files go, every other output is what it was
    fake_main(world["fa"], out)
    assert _tree(d) == _tree(world["unset"])
    for rel in _tree(d):
        if rel.endswith(".npz"):
            assert _same_npz(world["unset"] / rel, d / rel), rel
        elif rel.endswith(".tsv"):
            assert (world["unset"] / rel).read_bytes() == (d / rel).read_bytes(), rel


def test_the_switch_without_the_embeddings_is_refused(world, tmp_path, monkeypatch, capsys):
    set_env(monkeypatch, {"GENOMAD_AMD_KNN_GRAPH": "2"})
    del FakeKnnEngine.calls[:]
    capsys.readouterr()
    with pytest.raises(SystemExit) as exc:
        fake_main(world["fa"], tmp_path / "refused")
    err = capsys.readouterr().err.strip().splitlines()
    assert exc.value.code == 1 and len(err) == 1 and "GENOMAD_AMD_KNN_GRAPH needs GENOMAD_AMD_EMBEDDINGS=1: the neighbour lists are" in err[0]
    assert not list((tmp_path / "refused").rglob("*.npz")) and FakeKnnEngine.calls == []


def test_the_env_parsing_and_the_tables(world, tmp_path, monkeypatch):
    on = world["env"]
    for v in ("0", "65", "x", "1.5", "-2"):
        set_env(monkeypatch, dict(on, GENOMAD_AMD_KNN_GRAPH=v))
        with pytest.raises(ValueError, match=f"GENOMAD_AMD_KNN_GRAPH='{v}': expected an integer in \\[1, 64\\]"):
            fake_main(world["fa"], tmp_path / "bad")
    set_env(monkeypatch, dict(on, GENOMAD_AMD_KNN_GRAPH_MODE="both"))
    with pytest.raises(ValueError, match="GENOMAD_AMD_KNN_GRAPH_MODE='both': expected one of union, mutual"):
        nnc.knn_graph_requested()
    set_env(monkeypatch, dict(on, GENOMAD_AMD_KNN_GRAPH_WEIGHT="snn"))
    with pytest.raises(ValueError, match="GENOMAD_AMD_KNN_GRAPH_WEIGHT='snn': expected one of similarity, jaccard"):
        nnc.knn_graph_requested()
    for companion, v in (("GENOMAD_AMD_KNN_GRAPH_MODE", "mutual"), ("GENOMAD_AMD_KNN_GRAPH_WEIGHT", "jaccard")):
        set_env(monkeypatch, dict(BASE, **{companion: v}))          # a companion without the main switch
        with pytest.raises(ValueError, match=f"{companion}='{v}' needs GENOMAD_AMD_KNN_GRAPH"):
            fake_main(world["fa"], tmp_path / "bad")
    set_env(monkeypatch, dict(on, GENOMAD_AMD_KNN_GRAPH=" 64 ", GENOMAD_AMD_KNN_GRAPH_MODE="mutual", GENOMAD_AMD_KNN_GRAPH_WEIGHT="jaccard"))
    assert nnc.knn_graph_requested() == (64, "mutual", "jaccard")
    set_env(monkeypatch, on)
    assert nnc.knn_graph_requested() == (2, "union", "similarity")
    set_env(monkeypatch, BASE)
    assert nnc.knn_graph_requested() is None
    # the sixteenth record, in a third table: the fifteen that the earlier analyses' tests count are untouched
    assert nnc.ALL_ANALYSES == nnc.ANALYSES + nnc.MORE_ANALYSES and len(nnc.ALL_ANALYSES) == 15
    assert nnc.EVERY_ANALYSIS == nnc.ALL_ANALYSES + nnc.KNN_ANALYSES and [a.name for a in nnc.KNN_ANALYSES] == ["knn_graph"]
    assert len(nnc.EVERY_ANALYSIS) == 16 and len({a.name for a in nnc.EVERY_ANALYSIS}) == 16
    assert not (tmp_path / "bad").exists() or not list((tmp_path / "bad").rglob("*.npz"))
