"""sequence.modularity_communities, the definition gnn_communities computes on the device, on the host alone: against a brute force
on dense matrices of Python integers whose modularity is recomputed from scratch from the labels; Qnum rises strictly over accepted
sweeps and never falls over levels; the levels nest; every community is connected; the consequences of the blocking rule (no two
neighbours swap, no neighbouring member leaves under a mover, the largest priority moves, a clique collapses in a few sweeps); the
float modularity against networkx's; the named graphs against networkx's Louvain; the planted families; label_components; every
limit; and GENOMAD_AMD_COMMUNITIES in main(), over a fake engine that serves the graph and the communities from their definitions:
the two files, the resume rule, the refusals, and that nothing else changes."""
import shutil

import networkx as nx
import numpy as np
import pytest

from genomad_amd import nn_classification as nnc, sequence
from genomad_amd.engine import CommunityResult
from tests import communities_data as D
from tests.mcl_data import csr_of_edges, partition
from tests.test_analyses_host import ENV as OTHER_ENV, FakeAnalysisEngine, fake_main, same_file
from tests.test_strand_host import _npz, _same_npz, _tree, _write_fasta

R = {res: sequence.communities_resolution(res) for res in D.RESOLUTIONS}
SMALL = [(kind, seed, n, p) for kind in D.KINDS for seed, (n, p) in enumerate(((6, 0.6), (17, 0.3), (33, 0.12), (48, 0.08), (59, 0.2)))]


def dense(csr, valid=None):
    """(A, ok): the symmetric integer matrix of the graph as nested lists, parallel entries added, and the rows' validity"""
    n, a, b, q, ok = sequence.mcl_weights(*csr, valid)
    A = [[0] * n for _ in range(n)]
    for x, y, w in zip(a.tolist(), b.tolist(), q.tolist()):
        A[x][y] += w
        A[y][x] += w
    return A, ok


def qnum_of_labels(A, label, r):
    """Qnum of a labelling of the ROWS from scratch: 64 M2 (weight inside the labels) - r (sum of the labels' squared totals)"""
    n = len(A)
    k = [sum(row) for row in A]
    m2 = sum(k)
    inner = sum(A[i][j] for i in range(n) for j in range(n) if label[i] >= 0 and label[i] == label[j])
    tot = {}
    for i in range(n):
        if label[i] >= 0:
            tot[label[i]] = tot.get(label[i], 0) + k[i]
    return 64 * m2 * inner - r * sum(t * t for t in tot.values())


def brute(csr, valid, r, max_levels=32, max_sweeps=1 << 20):
    """The procedure again, written from the issue's text on dense matrices: nodes are lists of rows, every score is taken from the
    row labelling by :func:`qnum_of_labels`.  Returns (level_label, per-level stats, qnums, complete)."""
    A0, ok = dense(csr, valid)
    n = len(A0)
    m2 = sum(sum(row) for row in A0)
    members = {i: [i] for i in range(n) if ok[i]}             # node -> its rows
    levels, stats, qnums, complete, capped = [], [], [], m2 == 0, False

    def labels_of(groups):
        lab = [-1] * n
        for rows in groups:
            for x in rows:
                lab[x] = min(rows)
        return lab

    while m2 > 0 and len(levels) < max_levels and not complete:
        nodes = sorted(members)
        A = {i: {j: sum(A0[x][y] for x in members[i] for y in members[j]) for j in nodes} for i in nodes}
        k = {i: sum(A[i].values()) for i in nodes}
        comm = {i: i for i in nodes}

        def groups_of(assign):
            g = {}
            for i in nodes:
                g.setdefault(assign[i], []).extend(members[i])
            return list(g.values())

        q_now = qnum_of_labels(A0, labels_of(groups_of(comm)), r)
        sweeps = accepted = moved = rejected = 0
        while sweeps < max_sweeps:
            tot = {c: sum(k[i] for i in nodes if comm[i] == c) for c in set(comm.values())}
            want = {}
            for i in nodes:
                best = None
                w_own = sum(A[i][j] for j in nodes if j != i and comm[j] == comm[i])
                for c in sorted({comm[j] for j in nodes if j != i and A[i][j] > 0} - {comm[i]}):
                    w_c = sum(A[i][j] for j in nodes if j != i and comm[j] == c)
                    gain = 64 * m2 * (w_c - w_own) - r * k[i] * (tot[c] + k[i] - tot[comm[i]])
                    if gain > 0 and (best is None or gain > best[0]):      # ascending c: the first of equals stays
                        best = (gain, c)
                if best:
                    want[i] = best
            key = lambda i: (want[i][0], ((i + 1) * 2654435761 + sweeps * 40503) % 2 ** 32, -i)
            new = dict(comm)
            for i in want:
                rivals = [j for j in want if j != i and A[i][j] > 0 and comm[j] in (comm[i], want[i][1])]
                if all(key(j) < key(i) for j in rivals):
                    new[i] = want[i][1]
            sweeps += 1
            movers = sum(new[i] != comm[i] for i in nodes)
            if not movers:
                break
            q_new = qnum_of_labels(A0, labels_of(groups_of(new)), r)
            if q_new <= q_now:
                rejected = 1
                break
            comm, q_now, accepted, moved = new, q_new, accepted + 1, moved + movers
        else:
            capped = True
        n_comm = len(set(comm.values()))
        if accepted:
            comps = []
            for c in sorted(set(comm.values())):
                g = nx.Graph()
                g.add_nodes_from(i for i in nodes if comm[i] == c)
                g.add_edges_from((i, j) for i in g for j in g if i < j and A[i][j] > 0)
                comps += [sorted(x) for x in nx.connected_components(g)]
            comps.sort(key=min)
            members = {v: sorted(x for i in comp for x in members[i]) for v, comp in enumerate(comps)}
        else:
            complete = not capped
        lab = labels_of(members.values())
        levels.append(lab)
        stats.append((len(nodes), n_comm, sweeps, accepted, moved, rejected, len(members) - n_comm))
        qnums.append(qnum_of_labels(A0, lab, r))
        if not accepted:
            break
    return levels, stats, qnums, complete


def assert_is_brute(csr, valid, resolution, max_levels=32, max_sweeps=1 << 20):
    res = sequence.modularity_communities(*csr, valid, resolution, max_levels, max_sweeps)
    levels, stats, qnums, complete = brute(csr, valid, sequence.communities_resolution(resolution), max_levels, max_sweeps)
    assert res["level_label"].tolist() == levels and res["qnum"] == qnums and res["complete"] == complete and res["levels"] == len(levels)
    assert [tuple(int(res[f][l]) for f in sequence.COMM_LEVEL_FIELDS) for l in range(len(levels))] == stats
    n = D.n_of(csr)
    ok = np.ones(n, bool) if valid is None else np.asarray(valid)
    last = np.array(levels[-1]) if levels else np.where(ok, np.arange(n), -1)
    assert np.array_equal(res["label"], last)
    assert np.array_equal(res["size"], [0 if l < 0 else int((last == l).sum()) for l in last])
    return res


@pytest.mark.parametrize("resolution", D.RESOLUTIONS)
def test_random_graphs_of_three_weight_kinds_equal_the_brute_force(resolution):
    for kind, seed, n, p in SMALL:
        assert_is_brute(D.random_graph(seed, n, p, kind), None, resolution)


def test_the_fixtures_equal_the_brute_force_the_searched_ones_reach_the_rare_paths():
    for name in ("rejected", "split", "path", "ring", "parallel", "empty", "none", "one", "grid"):
        csr, valid = D.cases()[name]
        assert_is_brute(csr, valid, 2.5)
    masked = D.random_graph(3, 50, 0.15, "quarter")
    res = assert_is_brute(masked, np.arange(50) % 7 != 3, 1.0)
    assert (res["label"][3::7] == -1).all() and (res["size"][3::7] == 0).all() and (res["label"][np.arange(50) % 7 != 3] >= 0).all()
    assert D.reference("rejected", D.REJECTED["resolution"])["rejected"].any()
    assert D.reference("split", D.SPLIT["resolution"])["split"].any()
    # the fixed seeds are the search's first hits (the split's search takes a second: its hit is checked, and the seeds before it
    # that a quick run can afford)
    assert D.search("rejected", D.REJECTED["n"], D.REJECTED["p"], D.REJECTED["resolution"]) == D.REJECTED["seed"]
    assert D.search("split", D.SPLIT["n"], D.SPLIT["p"], D.SPLIT["resolution"], range(D.SPLIT["seed"] - 40, D.SPLIT["seed"] + 1)) == D.SPLIT["seed"]
    for limits in ((1, 1 << 20), (32, 1), (2, 2), (3, 1)):
        for name in ("rejected", "split"):
            assert_is_brute(*D.cases()[name], 2.5, *limits)


def traces():
    """(name, csr, valid, resolution, result, trace) over the fixtures and small random graphs"""
    for name in ("unit1", "quarter0", "random1", "rejected", "split", "grid", "masked", "ring", "planted"):
        csr, valid = D.cases()[name]
        for resolution in (1.0, 2.5):
            trace = []
            yield name, csr, valid, resolution, sequence.modularity_communities(*csr, valid, resolution, trace=trace), trace


def test_qnum_rises_strictly_over_accepted_sweeps_and_never_falls_over_levels_and_is_the_labels_own():
    seen = 0
    for name, csr, valid, resolution, res, trace in traces():
        r = sequence.communities_resolution(resolution)
        A, _ = dense(csr, valid)
        n = len(A)
        assert all(a <= b for a, b in zip(res["qnum"], res["qnum"][1:])), name
        for l in range(res["levels"]):
            assert qnum_of_labels(A, res["level_label"][l].tolist(), r) == res["qnum"][l], (name, l)
            steps = [t for t in trace if t["level"] == l]
            assert [t["accepted"] for t in steps] == [True] * int(res["accepted"][l]) + [False] * int(res["rejected"][l])
            start = res["qnum"][l - 1] if l else qnum_of_labels(A, [i if res["valid"][i] else -1 for i in range(n)], r)
            for t in steps:
                if n <= 150:                                  # from scratch, from the row labels
                    assert qnum_of_labels(A, [t["new"][t["node_of"][i]] + n if i in t["node_of"] else -1 for i in range(n)], r) == t["qnum"]
                assert (t["qnum"] > start) == t["accepted"], (name, l)
                start = t["qnum"] if t["accepted"] else start
                seen += 1
            if res["split"][l] > 0:
                assert res["qnum"][l] > start, name           # a split raises Qnum strictly
            elif res["accepted"][l]:
                assert res["qnum"][l] == start, name
    assert seen > 150


def test_the_levels_nest_and_every_community_is_connected():
    for name, csr, valid, resolution, res, _ in traces():
        g = D.to_networkx(csr, valid)
        for l in range(res["levels"]):
            lab = res["level_label"][l]
            for members in partition(lab):
                assert nx.is_connected(g.subgraph(members)) and min(members) == lab[min(members)], (name, l)
            if l:                                             # a community of the level before lies in one of this level
                below = res["level_label"][l - 1]
                assert all(len({lab[i] for i in members}) == 1 for members in partition(below)), (name, l)
            assert len(partition(lab)) == res["nodes"][l] - (res["nodes"][l] - res["communities"][l] - res["split"][l]), (name, l)
        assert np.array_equal(res["label"], res["level_label"][-1]) and res["complete"]
        assert (res["nodes"][1:] < res["nodes"][:-1]).all() and res["accepted"][-1] == 0      # strictly fewer nodes behind an accepted sweep


def test_the_consequences_of_the_blocking_rule():
    sweeps = 0
    for name, csr, valid, resolution, res, trace in traces():
        for t in trace:
            comm, new, want = t["comm"], t["new"], t["want"]
            prio = {i: (d, sequence.communities_hash(i, t["sweep"]), -i) for i, (d, _) in want.items()}
            movers = {i for i in comm if new[i] != comm[i]}
            assert movers and movers <= set(want) and all(new[i] == want[i][1] for i in movers)
            assert max(prio, key=prio.get) in movers          # the largest priority always moves
            node_graph = {}
            n, a, b, _, _ = sequence.mcl_weights(*csr, valid)
            for x, y in zip(a.tolist(), b.tolist()):
                i, j = t["node_of"][x], t["node_of"][y]
                if i != j:
                    node_graph.setdefault(i, set()).add(j)
                    node_graph.setdefault(j, set()).add(i)
            for i in movers:
                for j in node_graph.get(i, ()) & movers:
                    # Of two NEIGHBOURS that both move: they do not swap, they do not leave one community together, and where one
                    # leaves the other's target the one that enters has the larger priority - each would have had to have a strictly
                    # smaller priority than the other.  What the rule does not give: two nodes WITHOUT an entry between them can
                    # trade places (rows 37 and 48 in the 12 x 12 grid's first sweep at resolution 1), and a member of a target can
                    # leave for a third community under a mover of larger priority (nodes 12 and 18 of `unit1`); the score step
                    # judges the sweep as a whole.
                    assert not (comm[j] == new[i] and new[j] == comm[i]), (name, i, j)
                    assert comm[j] != comm[i], (name, i, j)
                    assert comm[j] != new[i] or prio[j] < prio[i], (name, i, j)
            sweeps += 1
    assert sweeps > 150
    # a clique of 40 singletons collapses in a few sweeps, not one node per sweep
    clique = csr_of_edges(40, [(x, y, 1.0) for x in range(40) for y in range(x + 1, 40)])
    res = sequence.modularity_communities(*clique)
    assert len(partition(res["label"])) == 1 and res["sweeps"].sum() <= 12, res["sweeps"]


def nx_modularity(csr, valid, label, resolution):
    g = D.to_networkx(csr, valid)
    return nx.community.modularity(g, [set(m) for m in partition(label)], weight="weight", resolution=resolution)


def test_the_float_modularity_is_networkxs_of_the_labels():
    for name, csr, valid, resolution, res, _ in traces():
        assert abs(res["modularity"] - nx_modularity(csr, valid, res["label"], resolution)) <= 1e-12, name
    assert sequence.modularity_communities(*D.EMPTY)["modularity"] == 0.0


def named_graphs():
    relabel = nx.convert_node_labels_to_integers
    yield "karate", D.of_networkx(nx.karate_club_graph())
    yield "les miserables", D.of_networkx(relabel(nx.les_miserables_graph()))
    yield "ring of cliques", D.ring_of_cliques()
    yield "path", D.path()
    yield "grid", D.grid()
    yield "planted", D.cases()["planted"][0]


# Measured here at resolution 1, the definition's modularity against networkx's Louvain (seeds 0, 1, 2: lowest / highest); karate and
# Les Miserables carry networkx's edge weights:
#   karate           0.4449 against 0.4439 / 0.4449
#   les miserables   0.5658 against 0.5654 / 0.5663
#   ring of cliques  0.8258 against 0.8258 / 0.8258
#   path             0.7567 against 0.7514 / 0.7577
#   grid             0.6754 against 0.6690 / 0.6824
#   planted          0.0687 against 0.0661 / 0.0722
# It is nowhere below the lowest seed, and at most 0.0070 (grid) below the best.  The margin is not taken from these figures: it is
# the worst the issue's prototype saw on these graphs against the BEST seed, and it is granted against the lowest one.
NAMED_MARGIN = 0.007


def test_the_named_graphs_against_networkxs_louvain():
    for name, csr in named_graphs():
        valid = D.cases()["planted"][1] if name == "planted" else None
        res = sequence.modularity_communities(*csr, valid)
        g = D.to_networkx(csr, valid)
        theirs = [nx.community.modularity(g, nx.community.louvain_communities(g, weight="weight", seed=seed), weight="weight") for seed in range(3)]
        print(f"{name}: {res['modularity']:.4f} against {min(theirs):.4f} / {max(theirs):.4f}")
        assert res["modularity"] >= min(theirs) - NAMED_MARGIN, (name, res["modularity"], theirs)


def test_planted_families_are_recovered_exactly():
    """the five families of 12 and the pair of tests/clusters_data.py, at a threshold (0.6) that leaves the background rows (pairwise
    cosine about 0.3) without entries - at 0.3 the background is one dense random graph and swallows them, at 0.5 it still reaches
    three of the five; the chain of 24 is no family: modularity cuts a path into stretches - and the twelve five-cliques of the ring"""
    rows, groups = D.planted(D.PLANTED_ROWS)[:2]
    indptr, col, sim = sequence.threshold_graph(rows, 0.6)
    res = sequence.modularity_communities(indptr, col, sim.astype(np.float32), sequence.valid_rows(rows))
    found = partition(res["label"])
    for name, members in groups.items():
        if name != "chain":
            assert frozenset(int(x) for x in members) in found, name
    assert res["complete"] and res["modularity"] > 0.6
    res = D.reference("ring")
    assert partition(res["label"]) == {frozenset(range(5 * c, 5 * c + 5)) for c in range(12)}
    table = sequence.communities_table(res, [f"n{i}" for i in range(60)])
    assert [t["size"] for t in table] == [len(t["members"]) for t in table] == [5] * 12 and table[1]["label"] == "n5"
    assert CommunityResult.build(res).n_communities == 12 and CommunityResult.build(res).table()[0]["members"] == [0, 1, 2, 3, 4]
    assert np.array_equal(CommunityResult.build(res).at_level(-1), res["label"])


def test_label_components_on_hand_made_labellings():
    path = D.path(12)
    label = np.array([0, 0, 1, 1, 0, 0, 0, 2, -1, 0, 0, 5])
    assert sequence.label_components(*path, label).tolist() == [0, 0, 2, 2, 4, 4, 4, 7, -1, 9, 9, 11]      # label 0: three components
    assert sequence.label_components(*path, label, np.arange(12) != 5).tolist() == [0, 0, 2, 2, 4, -1, 6, 7, -1, 9, 9, 11]
    assert sequence.label_components(*path, np.zeros(12, np.int64)).tolist() == [0] * 12
    assert sequence.label_components(*path, np.arange(12)).tolist() == list(range(12))
    # an entry that does not exist (q = 0) joins nothing; parallel entries join once
    assert sequence.label_components(*D.PARALLEL, np.zeros(7, np.int64)).tolist() == [0, 0, 0, 0, 0, 5, 6]
    for name in ("grid", "masked", "split"):                  # a result's own communities are connected: they are their components
        csr, valid = D.cases()[name]
        res = D.reference(name)
        assert np.array_equal(sequence.label_components(*csr, res["label"], valid), res["label"])
    for bad in (np.zeros(11, np.int64), np.zeros(12), np.full(12, -2)):
        with pytest.raises(ValueError):
            sequence.label_components(*path, bad)


def test_every_limit(monkeypatch):
    good = D.cases()["unit0"][0]
    for r in (1 / 64, 1.0, 4.0, 0.25, 63 / 64):
        assert sequence.communities_resolution(r) == r * 64
    for bad in (0, 0.0, 4.0 + 1 / 64, 1 / 128, -1.0, float("nan"), float("inf"), True, "x", None, 1.001):
        with pytest.raises(ValueError, match="resolution"):
            sequence.communities_resolution(bad)
        with pytest.raises(ValueError):
            sequence.modularity_communities(*good, resolution=bad)
    for kw in (dict(max_levels=0), dict(max_levels=33), dict(max_levels=1.5), dict(max_sweeps=0), dict(max_sweeps=(1 << 20) + 1), dict(max_sweeps=True)):
        with pytest.raises(ValueError):
            sequence.modularity_communities(*good, **kw)
    with pytest.raises(ValueError, match="2\\^24"):
        sequence.modularity_communities(np.zeros((1 << 24) + 2, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))
    full = sequence.modularity_communities(*good)
    monkeypatch.setattr(sequence, "COMM_M2_END", full["m2"])      # the doubled weight AT the limit is refused, one below is not
    with pytest.raises(ValueError, match="2\\^58"):
        sequence.modularity_communities(*good)
    monkeypatch.setattr(sequence, "COMM_M2_END", full["m2"] + 1)
    assert sequence.modularity_communities(*good)["qnum"] == full["qnum"]
    assert sequence.COMM_M2_END == full["m2"] + 1
    monkeypatch.undo()
    assert sequence.COMM_M2_END == 1 << 58
    # the largest quantities the bounds allow fit 128 bits with their sign
    m2, r = (1 << 58) - 1, 256
    assert 64 * m2 * m2 + r * m2 * (2 * m2) < 1 << 127 and 64 * m2 * m2 + r * m2 * m2 < 1 << 127
    one = sequence.modularity_communities(*good, max_levels=1)
    assert one["levels"] == 1 and not one["complete"] and full["levels"] > 1 and full["complete"]
    assert np.array_equal(one["level_label"][0], full["level_label"][0])
    short = sequence.modularity_communities(*good, max_sweeps=1)
    assert not short["complete"] and (short["sweeps"] == 1).all() and short["levels"] > full["levels"]
    capped = sequence.modularity_communities(*good, max_sweeps=int(full["sweeps"][0]) - 1)
    assert not capped["complete"] and capped["accepted"][0] == capped["sweeps"][0]
    none = sequence.modularity_communities(*D.EMPTY, np.array([True, False, True, True, True]))
    assert none["levels"] == 0 and none["complete"] and none["m2"] == 0 and none["label"].tolist() == [0, -1, 2, 3, 4]
    assert none["size"].tolist() == [1, 0, 1, 1, 1] and none["level_label"].shape == (0, 5) and none["qnum"] == []


# ---- GENOMAD_AMD_COMMUNITIES in main() -------------------------------------------------------------------------------------------------
COMM_ENV = ("GENOMAD_AMD_COMMUNITIES", "GENOMAD_AMD_COMMUNITIES_MAX_LEVELS", "GENOMAD_AMD_AVERAGE_LINKAGE", "GENOMAD_AMD_MCL",
            "GENOMAD_AMD_MCL_SELECT", "GENOMAD_AMD_SPREAD", "GENOMAD_AMD_SPREAD_BASE", "GENOMAD_AMD_SPREAD_MAX_ITER")
BASE = {"GENOMAD_AMD_EMBEDDINGS": "1", "GENOMAD_AMD_GRAPH": "0.999"}
FILES = ["m_nn_communities.npz", "m_nn_communities.tsv"]


class FakeCommunityEngine(FakeAnalysisEngine):
    """the stand-in of tests/test_analyses_host.py plus the communities from sequence.modularity_communities"""

    def communities(self, indptr, col, sim, valid=None, resolution=1.0, max_levels=32, max_sweeps=1 << 20):
        type(self).calls.append(("communities", len(indptr) - 1, float(resolution), int(max_levels)))
        return CommunityResult.build(sequence.modularity_communities(indptr, col, sim, valid, resolution, max_levels, max_sweeps))


def set_env(mp, env):
    """exactly the switches of ``env``, none of the others"""
    mp.setattr(nnc, "_engine", lambda: FakeCommunityEngine())
    for k in OTHER_ENV + COMM_ENV:
        mp.delenv(k, raising=False)
    for k, v in env.items():
        mp.setenv(k, v)


def names_of_calls():
    return [c[0] if isinstance(c, tuple) else c for c in FakeCommunityEngine.calls]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """One run with the graph but without GENOMAD_AMD_COMMUNITIES and one with it, shared and left unchanged.  The contigs: c0 .. c5,
    one run of N and two twins of c2: at 0.999 the graph holds the three pairs among c2 and its twins and nothing else."""
    root = tmp_path_factory.mktemp("communities")
    fa = root / "m.fna"
    recs = _write_fasta(fa, n=6)
    with open(fa, "a") as f:
        for k in range(2):
            f.write(f">twin{k} of c2\n{dict(recs)['c2']}\n")
    with pytest.MonkeyPatch.context() as mp:
        set_env(mp, BASE)
        fake_main(fa, root / "unset")
        on = dict(BASE, GENOMAD_AMD_COMMUNITIES="1")
        set_env(mp, on)
        del FakeCommunityEngine.calls[:]
        fake_main(fa, root / "on")
        found = list(FakeCommunityEngine.calls)
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
    assert [c[0] for c in calls] == ["graph", "graph", "communities"] and calls[2] == ("communities", 9, 1.0, 32)
    log = [line for line in (world["on"] / "m_nn_classification.log").read_text().splitlines() if " written to " in line]
    assert log[-1].endswith("written to m_nn_communities.npz and m_nn_communities.tsv.")
    assert "Modularity communities of the sequences (cosine similarity of the encoder embeddings >= 0.999, 3 edges, resolution 1: " in log[-1]
    assert "7 communities, modularity 0.0000, 2 levels, complete" in log[-1]


def test_the_files_hold_the_definition_on_a_worked_example(world):
    d = world["on"] / "m_nn_classification"
    z, emb = _npz(d / FILES[0]), _npz(d / "m_nn_embeddings.npz")
    rows = emb["embeddings"]
    g = sequence.threshold_graph(rows, 0.999, "cosine")
    want = sequence.modularity_communities(g[0], g[1], g[2].astype(np.float32), sequence.valid_rows(rows))
    for k in ("label", "size", "level_label", "valid") + sequence.COMM_LEVEL_FIELDS:
        assert z[k].dtype == want[k].dtype and np.array_equal(z[k], want[k]), k
    assert z["resolution"] == 1.0 and z["threshold"] == float(np.float32(0.999)) and z["max_levels"] == 32 and str(z["metric"]) == "cosine"
    assert "strand" not in z and z["levels"] == 2 == want["levels"] and z["complete"] and z["m2"] == want["m2"] == 6 << 24
    assert z["modularity"] == want["modularity"] and z["qnum_words"].dtype == np.uint64 and z["qnum_words"].shape == (2, 2)
    assert [int(lo) | (int(hi) << 64) for lo, hi in z["qnum_words"]] == [q % (1 << 128) for q in want["qnum"]]
    names = [str(x) for x in z["contig_names"]]
    c2 = names.index("c2")
    got = dict(zip(names, z["label"].tolist()))
    # identical rows: a triangle of weight 2^24 each, everything else alone.  One community holds it: in = M2, tot = M2, Qnum = 0
    assert got["c2"] == got["twin0"] == got["twin1"] == c2 and z["valid"].all() and got["c0"] == names.index("c0") and want["qnum"][-1] == 0
    lines = (d / FILES[1]).read_bytes().decode().split("\n")
    assert lines[0] == "seq_name\tcommunity\tcommunity_size" and lines[-1] == "" and len(lines) == 11
    rows = {x.split("\t")[0]: x.split("\t")[1:] for x in lines[1:-1]}
    assert list(rows) == names and rows["c2"] == rows["twin0"] == rows["twin1"] == ["c2", "3"]
    assert rows["c0"] == ["c0", "1"] and rows["nrun"] == ["nrun", "1"]
    # a contig without a valid embedding: NA and 0
    res = CommunityResult.build(sequence.modularity_communities(g[0], g[1], g[2].astype(np.float32), np.arange(len(rows)) != 1))
    nnc.write_communities(d.parent / "x.npz", d.parent / "x.tsv", "contig_names", np.array(names), res, (1.0, 0.999, 32))
    assert (d.parent / "x.tsv").read_text().split("\n")[2] == f"{names[1]}\tNA\t0"


def test_the_same_command_again_calls_nothing_and_another_request_runs_again(world, tmp_path, monkeypatch):
    out, d = copy_of(world, tmp_path)
    everything = _tree(d)
    on = world["env"]
    set_env(monkeypatch, on)
    del FakeCommunityEngine.calls[:]
    fake_main(world["fa"], out)
    assert FakeCommunityEngine.calls == []
    runs = 0
    for env, entry in ((dict(on, GENOMAD_AMD_COMMUNITIES="0.5"), ("resolution", 0.5)), (dict(on, GENOMAD_AMD_GRAPH="0.5"), ("threshold", 0.5)),
                       (dict(on, GENOMAD_AMD_COMMUNITIES_MAX_LEVELS="3"), ("max_levels", 3)), (on, ("resolution", 1.0))):
        set_env(monkeypatch, env)
        fake_main(world["fa"], out)                             # another resolution, threshold or level cap: the stage runs again
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
    del FakeCommunityEngine.calls[:]
    fake_main(world["fa"], out)
    assert "communities" not in names_of_calls() and _tree(d) == _tree(world["unset"])
    for rel in _tree(d):
        if rel.endswith(".npz"):
            assert _same_npz(world["unset"] / rel, d / rel), rel
        elif rel.endswith(".tsv"):
            assert (world["unset"] / rel).read_bytes() == (d / rel).read_bytes(), rel


@pytest.mark.parametrize("missing,said", [("GENOMAD_AMD_GRAPH", "GENOMAD_AMD_COMMUNITIES needs GENOMAD_AMD_GRAPH: "),
                                          ("GENOMAD_AMD_EMBEDDINGS", "GENOMAD_AMD_GRAPH needs GENOMAD_AMD_EMBEDDINGS=1: ")])
def test_the_switch_without_its_partners_is_refused(world, tmp_path, monkeypatch, capsys, missing, said):
    """without the embeddings it is the graph, which comes first in the table, that says so"""
    set_env(monkeypatch, {k: v for k, v in world["env"].items() if k != missing})
    del FakeCommunityEngine.calls[:]
    capsys.readouterr()
    with pytest.raises(SystemExit) as exc:
        fake_main(world["fa"], tmp_path / "refused")
    err = capsys.readouterr().err.strip().splitlines()
    assert exc.value.code == 1 and len(err) == 1 and said in err[0]
    if missing == "GENOMAD_AMD_GRAPH":
        assert "modularity is optimised over the similarity graph" in err[0]
    assert not list((tmp_path / "refused").rglob("*.npz")) and FakeCommunityEngine.calls == []


def test_the_env_parsing(world, tmp_path, monkeypatch):
    on = world["env"]
    for v in ("0", "4.5", "-1", "x", "nan", "0.01", "1.001"):
        set_env(monkeypatch, dict(on, GENOMAD_AMD_COMMUNITIES=v))
        with pytest.raises(ValueError, match=f"GENOMAD_AMD_COMMUNITIES='{v}': expected a multiple of 1/64 in"):
            fake_main(world["fa"], tmp_path / "bad")
    for v in ("0", "33", "x", "1.5"):
        set_env(monkeypatch, dict(on, GENOMAD_AMD_COMMUNITIES_MAX_LEVELS=v))
        with pytest.raises(ValueError, match=f"GENOMAD_AMD_COMMUNITIES_MAX_LEVELS='{v}': expected an integer in \\[1, 32\\]"):
            nnc.communities_requested()
    set_env(monkeypatch, dict(BASE, GENOMAD_AMD_COMMUNITIES_MAX_LEVELS="3"))
    with pytest.raises(ValueError, match="GENOMAD_AMD_COMMUNITIES_MAX_LEVELS='3' needs GENOMAD_AMD_COMMUNITIES"):
        nnc.communities_requested()
    set_env(monkeypatch, dict(on, GENOMAD_AMD_COMMUNITIES="0.25", GENOMAD_AMD_COMMUNITIES_MAX_LEVELS="3"))
    assert nnc.communities_requested() == (0.25, float(np.float32(0.999)), 3)
    set_env(monkeypatch, dict(on, GENOMAD_AMD_COMMUNITIES=" 4 "))
    assert nnc.communities_requested() == (4.0, float(np.float32(0.999)), 32)
    set_env(monkeypatch, BASE)
    assert nnc.communities_requested() is None
    a = next(a for a in nnc.ALL_ANALYSES if a.name == "communities")
    assert a.advice == "Raise GENOMAD_AMD_GRAPH or unset GENOMAD_AMD_COMMUNITIES." and a.after == "graph"
    # the fifteenth record, in a table of its own behind the fourteen that the earlier analyses' tests count
    assert nnc.ALL_ANALYSES == nnc.ANALYSES + nnc.MORE_ANALYSES and [x.name for x in nnc.MORE_ANALYSES] == ["communities"]
    assert len(nnc.ALL_ANALYSES) == 15 and len({x.name for x in nnc.ALL_ANALYSES}) == 15
