"""sequence.average_linkage, the definition gnn_avglink computes on the device, on the host alone: against sequential greedy UPGMA on
Fractions (untied graphs, and tied ones, where the equality is observed, not proven), against SciPy's ``average`` on a complete graph,
the ``stop`` rule, no inversions, the progress property, ``cut`` against a brute-force relabel, ``matrix`` in SciPy's hands, the round
limit and bad arguments; and GENOMAD_AMD_AVERAGE_LINKAGE in main(), over a fake engine that serves the graph and the tree from their
definitions: the two files, the resume rule, the refusals, and that nothing else changes."""
import shutil
from fractions import Fraction

import numpy as np
import pytest

from genomad_amd import nn_classification as nnc, sequence
from genomad_amd.engine import AverageLinkageResult
from tests import avglink_data as D
from tests.mcl_data import partition
from tests.test_analyses_host import ENV as OTHER_ENV, FakeAnalysisEngine, fake_main, same_file
from tests.test_strand_host import _npz, _same_npz, _tree, _write_fasta

W = D.W
TIED = [D.tied(k) for k in range(200)]
SPARSE = [D.sparse(k) for k in range(20)]
MIXED = SPARSE[:10] + TIED[:90]                       # the 100 graphs of the stop and inversion tests, tied and untied


def averages(res):
    return [Fraction(w, sa * sb) for w, sa, sb in zip(*(res[k].tolist() for k in ("weight", "size_a", "size_b")))]


def test_untied_graphs_equal_sequential_greedy_upgma():
    for k, g in enumerate(SPARSE):
        res = sequence.average_linkage(*g)
        assert res["complete"] and D.merge_set(res) == D.greedy(g), k
        assert len(set(averages(res))) == len(res["a"]), k        # no two merges share an average: nothing was tied


def test_heavily_tied_graphs_equal_sequential_greedy_too():
    """observed, not proven: the definition is the rounds; on these inputs the merge set is the sequential walk's"""
    tied = 0
    for k, g in enumerate(TIED):
        res = sequence.average_linkage(*g)
        assert D.merge_set(res) == D.greedy(g), k
        tied += len(set(averages(res))) < len(res["a"])
    assert tied > 150


def test_the_output_order_is_average_then_round_then_a_and_children_come_first():
    for g in MIXED:
        res = sequence.average_linkage(*g)
        keys = [(-avg, r, a) for avg, r, a in zip(averages(res), res["round"].tolist(), res["a"].tolist())]
        assert keys == sorted(keys)
        gone = set()
        for a, b in zip(res["a"].tolist(), res["b"].tolist()):      # a cluster merges while it is alive; b is absorbed once
            assert a < b and a not in gone and b not in gone
            gone.add(b)
        assert np.array_equal(res["sim"], np.array([float(x / W) for x in averages(res)]))


def test_the_complete_graph_against_scipys_average_linkage():
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.spatial.distance import squareform
    csr = D.cases()["complete"][0]
    res = D.reference("complete")
    n = D.COMPLETE_N
    assert len(res["a"]) == n - 1 and res["complete"]
    q = np.rint(csr[2].astype(np.float64) * W)
    d = np.zeros((n, n))
    d[np.repeat(np.arange(n), np.diff(csr[0])), csr[1]] = 1.0 - q / W
    z = linkage(squareform(d + d.T, checks=False), "average")
    ours = sequence.average_linkage_matrix(res)
    assert np.abs(np.sort(z[:, 2]) - np.sort(ours[:, 2])).max() <= 1e-12
    assert np.array_equal(np.sort(z[:, 3]), np.sort(ours[:, 3]))
    heights = np.sort(z[:, 2])
    for t in heights[[20, 80, 140, 180, 195]] + 1e-9:          # five cuts, each between two merges
        assert partition(fcluster(z, t, "distance")) == partition(fcluster(ours, t, "distance")) == partition(
            sequence.average_linkage_cut(res, 1.0 - t))
    print(f"\ncomplete graph of {n}: {res['rounds']} rounds, merges per round {res['merged_per_round'].tolist()}")


def test_stop_gives_the_merges_of_the_full_tree_at_or_above_it():
    for k, g in enumerate(MIXED):
        full = sequence.average_linkage(*g)
        for s in (0.125, 0.25, 0.3, 0.5):
            part = sequence.average_linkage(*g, stop=s)
            s_q = sequence.average_linkage_stop(s)
            assert D.merge_set(part) == {m for m in D.merge_set(full) if m[2] >= s_q * m[3] * m[4]}, (k, s)
            assert part["complete"] and part["stop"] == s_q / W


def test_no_merge_has_a_larger_average_than_one_that_built_a_side():
    for k, g in enumerate(MIXED):
        res = sequence.average_linkage(*g)
        last = {}                                             # cluster id -> the average of the merge that last built it
        for a, b, avg in zip(res["a"].tolist(), res["b"].tolist(), averages(res)):
            assert avg <= min(last.get(a, avg), last.get(b, avg)), k
            last[a] = avg


def test_a_round_in_which_a_cluster_names_a_best_merges_a_pair():
    """every round but the last merges; the last merges nothing because nobody names anybody: the rows that are left have no entries"""
    for g in TIED[:50]:
        res = sequence.average_linkage(*g)
        m = res["merged_per_round"]
        assert res["rounds"] == len(m) and (m[:-1] > 0).all() and m[-1] == 0 and m.sum() == len(res["a"])
        comp = sequence.graph_components(g[0], g[1], np.ones(D.n_of(g), bool))
        assert np.array_equal(sequence.average_linkage_cut(res, 2.0 ** -24), comp)       # a whole tree per component


def test_cut_and_cluster_counts_against_a_brute_force_relabel():
    for g in MIXED[::5]:
        res = sequence.average_linkage(*g)
        n = D.n_of(g)
        ts = (0.1, 0.2, 0.3, 0.45, 0.9)
        for t in ts:
            t_q = sequence.average_linkage_stop(t)
            label = list(range(n))
            for a, b, w, sa, sb in zip(*(res[k].tolist() for k in sequence.AVGLINK_FIELDS[:5])):
                if w >= t_q * sa * sb:
                    label = [a if x == b else x for x in label]      # in the tree's order b is a cluster's id when it is absorbed
            assert sequence.average_linkage_cut(res, t).tolist() == label
            assert sequence.average_linkage_cluster_counts(res, [t]).tolist() == [len(set(label))]
        assert (np.diff(sequence.average_linkage_cluster_counts(res, ts)) >= 0).all()


def test_masked_rows_parallel_entries_and_graphs_without_entries():
    csr, valid = D.cases()["masked"]
    res = D.reference("masked")
    label = sequence.average_linkage_cut(res, 0.3)
    assert (label[~valid] == -1).all() and (label[valid] >= 0).all() and not np.isin(np.concatenate([res["a"], res["b"]]), np.flatnonzero(~valid)).any()
    par = D.reference("parallel")                             # rows 0 and 1 list a partner twice: the weights add up
    q = np.rint(np.float64(np.float32([0.5, 0.25])) * W).astype(np.int64)
    assert (0, 1, int(q.sum()), 1, 1) in D.merge_set(par)
    for name, n in (("empty", 5), ("none", 0), ("one", 1)):
        res = D.reference(name)
        assert res["rounds"] == 1 and res["complete"] and res["merged_per_round"].tolist() == [0] and len(res["a"]) == 0
        assert res["weight"].dtype == np.uint64 and res["sim"].dtype == np.float64 and len(sequence.average_linkage_cut(res, 0.5)) == n
    table = sequence.average_linkage_table(par, names=list("abcdefg"))
    assert table[0]["rank"] == 1 and table[0]["clusters_left"] == 6 and {table[0]["a"], table[0]["b"]} <= set("abcdefg")


def test_the_round_limit_cuts_short():
    g = D.cases()["path"][0]
    full = D.reference("path")
    assert full["rounds"] > 30                                # a chain is the worst case, and rounds shows it
    for k in (1, 2, 7):
        part = sequence.average_linkage(*g, max_rounds=k)
        assert part["rounds"] == k and not part["complete"] and np.array_equal(part["merged_per_round"], full["merged_per_round"][:k])
        assert D.merge_set(part) == {m for m, r in zip(zip(*(full[f].tolist() for f in sequence.AVGLINK_FIELDS[:5])), full["round"]) if r < k}
    whole = sequence.average_linkage(*g, max_rounds=full["rounds"])
    assert whole["complete"] and D.merge_set(whole) == D.merge_set(full)


def test_matrix_needs_a_whole_tree():
    with pytest.raises(ValueError, match="n - 1 merges"):
        sequence.average_linkage_matrix(D.reference("masked"))
    with pytest.raises(ValueError, match="n - 1 merges"):
        sequence.average_linkage_matrix(sequence.average_linkage(*D.cases()["complete"][0], stop=0.9))


def test_bad_arguments():
    g = D.cases()["sparse0"][0]
    for kw in (dict(stop=0), dict(stop=0.0), dict(stop=-0.5), dict(stop=64.0), dict(stop=float("nan")), dict(stop="x"), dict(stop=True),
               dict(stop=2.0 ** -26), dict(max_rounds=0), dict(max_rounds=1.5), dict(max_rounds=(1 << 20) + 1), dict(valid=np.ones(3, bool))):
        with pytest.raises(ValueError):
            sequence.average_linkage(*g, **kw)
    with pytest.raises(ValueError, match="upper triangle"):
        sequence.average_linkage(g[0], g[1][::-1].copy(), g[2])
    assert sequence.average_linkage_stop(2.0 ** -24) == 1 and sequence.average_linkage_stop(1.0) == W
    with pytest.raises(ValueError):
        sequence.average_linkage_cut(D.reference("sparse0"), 0.0)


# ---- GENOMAD_AMD_AVERAGE_LINKAGE in main() ---------------------------------------------------------------------------------------------
AVGLINK_ENV = ("GENOMAD_AMD_AVERAGE_LINKAGE", "GENOMAD_AMD_MCL", "GENOMAD_AMD_MCL_SELECT", "GENOMAD_AMD_SPREAD", "GENOMAD_AMD_SPREAD_BASE",
               "GENOMAD_AMD_SPREAD_MAX_ITER")
BASE = {"GENOMAD_AMD_EMBEDDINGS": "1", "GENOMAD_AMD_GRAPH": "0.999"}
FILES = ["m_nn_average_linkage.npz", "m_nn_average_linkage.tsv"]


class FakeAvglinkEngine(FakeAnalysisEngine):
    """the stand-in of tests/test_analyses_host.py plus average linkage from sequence.average_linkage"""

    def average_linkage(self, indptr, col, sim, valid=None, stop=2.0 ** -24, max_rounds=1 << 20):
        type(self).calls.append(("average_linkage", len(indptr) - 1, float(stop), int(max_rounds)))
        return AverageLinkageResult(**sequence.average_linkage(indptr, col, sim, valid, stop, max_rounds), n=len(indptr) - 1)


def set_env(mp, env):
    """exactly the switches of ``env``, none of the others"""
    mp.setattr(nnc, "_engine", lambda: FakeAvglinkEngine())
    for k in OTHER_ENV + AVGLINK_ENV:
        mp.delenv(k, raising=False)
    for k, v in env.items():
        mp.setenv(k, v)


def names_of_calls():
    return [c[0] if isinstance(c, tuple) else c for c in FakeAvglinkEngine.calls]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """One run with the graph but without GENOMAD_AMD_AVERAGE_LINKAGE and one with it, shared and left unchanged.  The contigs: c0 ..
    c5, one run of N and two twins of c2: at 0.999 the graph holds the three pairs among c2 and its twins and nothing else."""
    root = tmp_path_factory.mktemp("avglink")
    fa = root / "m.fna"
    recs = _write_fasta(fa, n=6)
    with open(fa, "a") as f:
        for k in range(2):
            f.write(f">twin{k} of c2\n{dict(recs)['c2']}\n")
    with pytest.MonkeyPatch.context() as mp:
        set_env(mp, BASE)
        fake_main(fa, root / "unset")
        on = dict(BASE, GENOMAD_AMD_AVERAGE_LINKAGE="0.9")
        set_env(mp, on)
        del FakeAvglinkEngine.calls[:]
        fake_main(fa, root / "on")
        found = list(FakeAvglinkEngine.calls)
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
    cut = sequence.average_linkage_stop(0.9) / W
    assert [c[0] for c in calls] == ["graph", "graph", "average_linkage"] and calls[2] == ("average_linkage", 9, cut, 1 << 20)
    log = [line for line in (world["on"] / "m_nn_classification.log").read_text().splitlines() if " written to " in line]
    assert log[-1].endswith("written to m_nn_average_linkage.npz and m_nn_average_linkage.tsv.")
    assert "Average-linkage clusters of the sequences (cosine similarity of the encoder embeddings >= 0.999, 3 edges, " in log[-1]
    assert "a pair without an edge counting as 0: 7 clusters, 2 merges in 3 rounds" in log[-1]


def test_the_files_hold_the_definition_on_a_worked_example(world):
    d = world["on"] / "m_nn_classification"
    z, emb = _npz(d / FILES[0]), _npz(d / "m_nn_embeddings.npz")
    rows = emb["embeddings"]
    g = sequence.threshold_graph(rows, 0.999, "cosine")
    cut = sequence.average_linkage_stop(0.9) / W
    want = sequence.average_linkage(g[0], g[1], g[2].astype(np.float32), sequence.valid_rows(rows), cut)
    for k in sequence.AVGLINK_FIELDS + ("sim", "valid", "merged_per_round"):
        assert z[k].dtype == want[k].dtype and np.array_equal(z[k], want[k]), k
    assert z["cut"] == cut and z["threshold"] == float(np.float32(0.999)) and str(z["metric"]) == "cosine" and "strand" not in z
    assert z["rounds"] == 3 and z["complete"] and np.array_equal(z["label"], sequence.average_linkage_cut(want, cut))
    names = [str(x) for x in z["contig_names"]]
    c2 = names.index("c2")
    got = dict(zip(names, z["label"].tolist()))
    assert got["c2"] == got["twin0"] == got["twin1"] == c2 and z["valid"].all() and got["c0"] == names.index("c0")
    # identical rows: cosine 1, q = 2^24 each.  c2 takes twin0 at S = 2^24; {c2, twin0} takes twin1 at S = 2^25 over 2 * 1 pairs
    assert z["weight"].tolist() == [W, 2 * W] and z["sim"].tolist() == [1.0, 1.0] and z["size_a"].tolist() == [1, 2] and z["round"].tolist() == [0, 1]
    lines = (d / FILES[1]).read_bytes().decode().split("\n")
    assert lines[0] == "seq_name\tcluster\tcluster_size" and lines[-1] == "" and len(lines) == 11
    rows = {x.split("\t")[0]: x.split("\t")[1:] for x in lines[1:-1]}
    assert list(rows) == names and rows["c2"] == rows["twin0"] == rows["twin1"] == ["c2", "3"]
    assert rows["c0"] == ["c0", "1"] and rows["nrun"] == ["nrun", "1"]


def test_the_same_command_again_calls_nothing_and_another_request_runs_again(world, tmp_path, monkeypatch):
    out, d = copy_of(world, tmp_path)
    everything = _tree(d)
    on = world["env"]
    set_env(monkeypatch, on)
    del FakeAvglinkEngine.calls[:]
    fake_main(world["fa"], out)
    assert FakeAvglinkEngine.calls == []
    runs = 0
    for env, entry in ((dict(on, GENOMAD_AMD_AVERAGE_LINKAGE="0.5"), ("cut", 0.5)), (dict(on, GENOMAD_AMD_GRAPH="0.5"), ("threshold", 0.5)),
                       (on, ("cut", sequence.average_linkage_stop(0.9) / W))):
        set_env(monkeypatch, env)
        fake_main(world["fa"], out)                             # another cut or threshold: the stage runs again
        runs += 1
        assert names_of_calls().count("plain") == runs and _npz(d / FILES[0])[entry[0]] == entry[1] and _tree(d) == everything
        fake_main(world["fa"], out)                             # and is resumed from
        assert names_of_calls().count("plain") == runs
    assert same_file(d / FILES[0], world["on"] / "m_nn_classification" / FILES[0])
    assert (d / FILES[1]).read_bytes() == (world["on"] / "m_nn_classification" / FILES[1]).read_bytes()
    (d / FILES[1]).unlink()
    fake_main(world["fa"], out)                                 # one of the pair is gone: again
    assert names_of_calls().count("plain") == runs + 1 and _tree(d) == everything


def test_unset_again_its_files_go_and_every_output_is_what_it_was(world, tmp_path, monkeypatch):
    out, d = copy_of(world, tmp_path)
    set_env(monkeypatch, BASE)
    del FakeAvglinkEngine.calls[:]
    fake_main(world["fa"], out)
    assert "average_linkage" not in names_of_calls() and _tree(d) == _tree(world["unset"])
    for rel in _tree(d):
        if rel.endswith(".npz"):
            assert _same_npz(world["unset"] / rel, d / rel), rel
        elif rel.endswith(".tsv"):
            assert (world["unset"] / rel).read_bytes() == (d / rel).read_bytes(), rel


@pytest.mark.parametrize("missing,said", [("GENOMAD_AMD_GRAPH", "GENOMAD_AMD_AVERAGE_LINKAGE needs GENOMAD_AMD_GRAPH: "),
                                          ("GENOMAD_AMD_EMBEDDINGS", "GENOMAD_AMD_GRAPH needs GENOMAD_AMD_EMBEDDINGS=1: ")])
def test_the_switch_without_its_partners_is_refused(world, tmp_path, monkeypatch, capsys, missing, said):
    """without the embeddings it is the graph, which comes first in the table, that says so"""
    set_env(monkeypatch, {k: v for k, v in world["env"].items() if k != missing})
    del FakeAvglinkEngine.calls[:]
    capsys.readouterr()
    with pytest.raises(SystemExit) as exc:
        fake_main(world["fa"], tmp_path / "refused")
    err = capsys.readouterr().err.strip().splitlines()
    assert exc.value.code == 1 and len(err) == 1 and said in err[0]
    if missing == "GENOMAD_AMD_GRAPH":
        assert "the groups merge by their mean similarity over the similarity graph" in err[0]
    assert not list((tmp_path / "refused").rglob("*.npz")) and FakeAvglinkEngine.calls == []


def test_bad_values_and_the_advice(world, tmp_path, monkeypatch, capsys):
    on = world["env"]
    for v in ("0", "1.5", "-0.2", "x", "nan", "1e-9"):
        set_env(monkeypatch, dict(on, GENOMAD_AMD_AVERAGE_LINKAGE=v))
        with pytest.raises(ValueError, match=f"GENOMAD_AMD_AVERAGE_LINKAGE='{v}': expected a float in"):
            fake_main(world["fa"], tmp_path / "bad")
    set_env(monkeypatch, dict(on, GENOMAD_AMD_AVERAGE_LINKAGE="1"))
    assert nnc.average_linkage_requested() == (1.0, float(np.float32(0.999)))
    set_env(monkeypatch, BASE)
    assert nnc.average_linkage_requested() is None
    a = next(a for a in nnc.ANALYSES if a.name == "average_linkage")
    assert a.advice == "Raise GENOMAD_AMD_GRAPH or unset GENOMAD_AMD_AVERAGE_LINKAGE." and a.after == "graph"
    assert [x.name for x in nnc.ANALYSES].index("average_linkage") == [x.name for x in nnc.ANALYSES].index("mcl") + 1
    assert len(nnc.ANALYSES) == 14
