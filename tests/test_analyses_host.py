"""The ten analyses of the per-contig encoder embeddings that main() offers - neighbours, clusters, representatives, linkage, graph,
density, kmeans, pca, matches, votes - run TOGETHER over a fake engine: what a run with every switch writes, that a second run
resumes from all of it, that each analysis follows its own request and touches only its own files, the strand mode, and the refusal
without GENOMAD_AMD_EMBEDDINGS=1.  Every analysis's own test checks what its files hold; this one checks the rules they share."""
import shutil

import numpy as np
import pytest

from genomad_amd import nn_classification as nnc, sequence
from genomad_amd.engine import (ClusterResult, DensityResult, GraphResult, KMeansResult, LinkageResult, MatchResult, RepresentativeResult,
                                VoteResult)
from tests.test_match_host import MATCH_SWITCHES
from tests.test_neighbours_host import SWITCHES, FakeNeighbourEngine
from tests.test_pca_host import host_pca
from tests.test_strand_host import FakeStrandEngine, _npz, _same_npz, _tree, _write_fasta
from tests.test_votes_host import VOTE_SWITCHES

# the stem of an analysis's files in main()'s run order, the switches of a first request ({match}: the run's own embeddings file,
# {vote}: the same with labels), the switch that a second request changes, and the npz entry that then spells it (linkage has one
# request only: its file's existence)
ANALYSES = (
    ("neighbours", {"GENOMAD_AMD_NEIGHBOURS": "3"}, ("GENOMAD_AMD_NEIGHBOURS", "2"), ("k", 2)),
    ("clusters", {"GENOMAD_AMD_CLUSTERS": "0.999"}, ("GENOMAD_AMD_CLUSTERS", "0.5"), ("threshold", 0.5)),
    ("representatives", {"GENOMAD_AMD_REPRESENTATIVES": "0.999"}, ("GENOMAD_AMD_REPRESENTATIVES", "0.5"), ("threshold", 0.5)),
    ("linkage", {"GENOMAD_AMD_LINKAGE": "1"}, None, None),
    ("graph", {"GENOMAD_AMD_GRAPH": "0.999"}, ("GENOMAD_AMD_GRAPH", "0.5"), ("threshold", 0.5)),
    ("density", {"GENOMAD_AMD_DENSITY": "0.999", "GENOMAD_AMD_DENSITY_MIN_POINTS": "3"}, ("GENOMAD_AMD_DENSITY_MIN_POINTS", "2"),
     ("min_points", 2)),
    ("kmeans", {"GENOMAD_AMD_KMEANS": "3"}, ("GENOMAD_AMD_KMEANS_MAX_ITER", "7"), ("max_iter", 7)),
    ("pca", {"GENOMAD_AMD_PCA": "2"}, ("GENOMAD_AMD_PCA", "3"), ("n_components", 3)),
    ("matches", {"GENOMAD_AMD_MATCH": "0.999", "GENOMAD_AMD_MATCH_BASE": "{match}"}, ("GENOMAD_AMD_MATCH", "0.5"), ("threshold", 0.5)),
    ("votes", {"GENOMAD_AMD_VOTE": "0.999", "GENOMAD_AMD_VOTE_BASE": "{vote}"}, ("GENOMAD_AMD_VOTE_MIN_VOTES", "2"), ("min_votes", 2)),
)
NAMES = [a[0] for a in ANALYSES]
WITHOUT_TSV = ("neighbours",)
ENV = tuple(dict.fromkeys(SWITCHES + MATCH_SWITCHES + VOTE_SWITCHES + ("GENOMAD_AMD_KMEANS_MAX_ITER",)
                          + tuple(k for a in ANALYSES for k in a[1])))


def files_of(name, prefix="m"):
    return [f"{prefix}_nn_{name}.npz"] + ([] if name in WITHOUT_TSV else [f"{prefix}_nn_{name}.tsv"])


class FakeAnalysisEngine(FakeNeighbourEngine):
    """the stand-in of tests/test_neighbours_host.py plus the nine other analyses, each served from its definition in sequence.py
    through its Result class; under a strand mode the embeddings are the forward ones (a fixed function of the contig's bytes)"""
    calls = []

    def classify_contigs_strand(self, seq, offsets, strand="both", single_window=False, precision=None, embed=False):
        r = FakeStrandEngine.classify_contigs_strand(self, seq, offsets, strand, single_window, precision, embed)
        return r[0], r[1], self.embed_contigs(seq, offsets)[1], r[3], r[4]

    def cluster(self, rows, threshold, metric="cosine"):
        type(self).calls.append(("cluster", len(rows), float(threshold), metric))
        return ClusterResult.build(sequence.threshold_clusters(rows, threshold, metric), threshold, metric)

    def representatives(self, rows, threshold, weight=None, metric="cosine"):
        type(self).calls.append(("representatives", len(rows), float(threshold), metric))
        return RepresentativeResult.build(sequence.greedy_representatives(rows, threshold, weight, metric), threshold, metric)

    def linkage(self, rows, metric="cosine"):
        type(self).calls.append(("linkage", len(rows), metric))
        return LinkageResult.build(sequence.single_linkage_tree(rows, metric), metric)

    def graph(self, rows, threshold, metric="cosine", max_edges=1 << 28):
        type(self).calls.append(("graph", len(rows), float(threshold), metric))
        indptr, col, sim = sequence.threshold_graph(rows, threshold, metric)
        return GraphResult.build((indptr, col, sim.astype(np.float32)), sequence.valid_rows(rows, metric), threshold, metric)

    def density(self, rows, threshold, min_points=5, metric="cosine"):
        type(self).calls.append(("density", len(rows), float(threshold), int(min_points), metric))
        label, degree, size, anchor, sim, kind = sequence.density_clusters(rows, threshold, min_points, metric)
        return DensityResult.build((label, degree, size, anchor, sim.astype(np.float32), kind), threshold, min_points, metric)

    def kmeans(self, rows, k, init=None, max_iter=50):
        type(self).calls.append(("kmeans", len(rows), int(k), init is None, int(max_iter)))
        return KMeansResult.build(sequence.spherical_kmeans(rows, k, init, max_iter))

    def pca(self, rows, n_components=2, center=True):
        type(self).calls.append(("pca", len(rows), int(n_components), bool(center)))
        return host_pca(rows, n_components, center)

    def match(self, query, base, threshold, metric="cosine", max_edges=1 << 28):
        type(self).calls.append(("match", len(query), len(base), float(threshold), metric))
        indptr, col, sim = sequence.threshold_matches(query, base, threshold, metric)
        return MatchResult.build((indptr, col, sim.astype(np.float32)), sequence.valid_rows(query, metric), sequence.valid_rows(base, metric),
                                 threshold, metric)

    def vote(self, query, base, label, n_classes, threshold):
        type(self).calls.append(("vote", len(query), len(base), int(n_classes), float(threshold)))
        return VoteResult.build(sequence.class_votes(query, base, label, n_classes, threshold), sequence.valid_rows(query), n_classes, threshold)


def fake_main(fa, out):
    return nnc.main(fa, out, False, 128, False, 1, False, False)


def set_env(mp, env):
    """exactly the switches of ``env``, none of the others"""
    mp.setattr(nnc, "_engine", lambda: FakeAnalysisEngine())
    for k in ENV:
        mp.delenv(k, raising=False)
    for k, v in env.items():
        mp.setenv(k, v)


def plain_runs():
    """how often the stage ran: one plain pass per run (under a strand mode it is the pass embed_contigs makes for the embeddings)"""
    return FakeAnalysisEngine.calls.count("plain")


def same_file(a, b):
    """_same_npz for the analyses' own files, whose float arrays hold NaN where there is nothing to say"""
    a, b = _npz(a), _npz(b)
    return sorted(a) == sorted(b) and all(a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f") for k in a)


def references(emb_file, stem):
    """the run's own embeddings file as the match's reference, and the same with labels as the vote's"""
    z = _npz(emb_file)
    n = len(z["contig_names"])
    vote = emb_file.parent.parent.parent / f"{stem}_labelled.npz"
    np.savez_compressed(vote, **z, labels=np.array((["virus", "plasmid", "", "virus", "host"] * n)[:n]))
    return {"match": str(emb_file), "vote": str(vote)}


def request_env(refs, only=None):
    env = {"GENOMAD_AMD_EMBEDDINGS": "1"}
    for name, switches, _, _ in ANALYSES:
        if only is None or name == only:
            env.update({k: v.format(**refs) for k, v in switches.items()})
    return env


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """one run without any of the ten switches and one with all of them, shared and left unchanged: a test works on a copy"""
    root = tmp_path_factory.mktemp("analyses")
    fa = root / "m.fna"
    recs = _write_fasta(fa, n=6)
    with open(fa, "a") as f:
        for k in range(2):
            f.write(f">twin{k} of c2\n{dict(recs)['c2']}\n")   # the same bytes as c2: the same embedding
    with pytest.MonkeyPatch.context() as mp:
        set_env(mp, {"GENOMAD_AMD_EMBEDDINGS": "1"})
        fake_main(fa, root / "unset")
        refs = references(root / "unset" / "m_nn_classification" / "m_nn_embeddings.npz", "forward")
        set_env(mp, request_env(refs))
        del FakeAnalysisEngine.calls[:]
        fake_main(fa, root / "on")
        calls = list(FakeAnalysisEngine.calls)
    return {"fa": fa, "root": root, "refs": refs, "unset": root / "unset", "on": root / "on", "calls": calls}


def copy_of(world, tmp_path):
    out = tmp_path / "on"
    shutil.copytree(world["on"], out)
    return out, out / "m_nn_classification"


def written(log):
    """the ten analyses' files in the order of the log's "... written to ..." lines"""
    firsts = {files_of(name)[0]: name for name in NAMES}
    out = []
    for line in log.read_text().splitlines():
        if " written to " in line:
            out += [firsts[w] for w in line.split(" written to ")[1].rstrip(".").split() if w in firsts]
    return out


def test_all_ten_switches_add_their_19_files_and_change_nothing_else(world):
    d0, d1 = world["unset"] / "m_nn_classification", world["on"] / "m_nn_classification"
    ours = [f for name in NAMES for f in files_of(name)]
    assert len(ours) == 19 and all((d1 / f).is_file() for f in ours)
    assert _tree(d1) == sorted(_tree(d0) + ours)
    for rel in _tree(d0):                                       # every other output: the same arrays, the same bytes
        if rel.endswith(".npz"):
            assert _same_npz(d0 / rel, d1 / rel), rel
        elif rel.endswith(".tsv"):
            assert (d0 / rel).read_bytes() == (d1 / rel).read_bytes(), rel
    assert written(world["on"] / "m_nn_classification.log") == NAMES
    assert [c[0] for c in world["calls"] if c != "plain"] == ["neighbours", "cluster", "representatives", "linkage", "graph", "density",
                                                              "kmeans", "pca", "match", "vote"]
    for name in NAMES:
        assert "strand" not in _npz(d1 / files_of(name)[0]), name


def test_the_same_command_again_calls_nothing(world, tmp_path, monkeypatch):
    out, _ = copy_of(world, tmp_path)
    set_env(monkeypatch, request_env(world["refs"]))
    del FakeAnalysisEngine.calls[:]
    before = {rel: (out / rel).read_bytes() for rel in _tree(out) if (out / rel).is_file() and not rel.endswith((".log", ".json", ".tsv"))}
    fake_main(world["fa"], out)
    assert FakeAnalysisEngine.calls == []
    log = (out / "m_nn_classification.log").read_text()
    assert "m_nn_classification.npz was found. Skipping sequence classification." in log and written(out / "m_nn_classification.log") == []
    assert before == {rel: (out / rel).read_bytes() for rel in before}


@pytest.mark.parametrize("name,switches,changed,entry", ANALYSES, ids=NAMES)
def test_each_analysis_follows_its_request_and_touches_only_its_files(world, tmp_path, monkeypatch, name, switches, changed, entry):
    out, d = copy_of(world, tmp_path)
    everything = _tree(d)
    npz = d / files_of(name)[0]
    env = request_env(world["refs"])
    del FakeAnalysisEngine.calls[:]
    runs = 0
    if changed is not None:                                     # another request: the stage runs again and the file spells the new one
        set_env(monkeypatch, dict(env, **{changed[0]: changed[1]}))
        fake_main(world["fa"], out)
        runs += 1
        z = _npz(npz)
        assert plain_runs() == runs and z[entry[0]] == entry[1] and _tree(d) == everything
        assert written(out / "m_nn_classification.log") == NAMES
    set_env(monkeypatch, {k: v for k, v in env.items() if k not in switches})
    fake_main(world["fa"], out)                                 # no request: its files go, and only they
    runs += 1
    assert plain_runs() == runs and _tree(d) == sorted(set(everything) - set(files_of(name)))
    assert written(out / "m_nn_classification.log") == [x for x in NAMES if x != name]
    set_env(monkeypatch, env)
    fake_main(world["fa"], out)                                 # the first request again: they are back
    runs += 1
    assert plain_runs() == runs and _tree(d) == everything
    if name not in WITHOUT_TSV:
        (d / files_of(name)[1]).unlink()
        fake_main(world["fa"], out)                             # one of the pair is gone: the stage runs again
        runs += 1
        assert plain_runs() == runs and _tree(d) == everything
    npz.write_bytes(b"")
    fake_main(world["fa"], out)                                 # an unreadable npz: the stage runs again
    runs += 1
    assert plain_runs() == runs and _tree(d) == everything and same_file(npz, world["on"] / "m_nn_classification" / npz.name)
    fake_main(world["fa"], out)                                 # and everything is in place again: nothing runs
    assert plain_runs() == runs


def test_every_file_carries_the_strand_mode_it_was_computed_under(world, tmp_path, monkeypatch):
    out, d = copy_of(world, tmp_path)
    set_env(monkeypatch, {"GENOMAD_AMD_EMBEDDINGS": "1", "GENOMAD_AMD_STRAND": "both"})
    fake_main(world["fa"], tmp_path / "both")                   # the references of a run under both: that run's embeddings
    refs = references(tmp_path / "both" / "m_nn_classification" / "m_nn_embeddings.npz", "both")
    del FakeAnalysisEngine.calls[:]
    set_env(monkeypatch, dict(request_env(refs), GENOMAD_AMD_STRAND="both"))
    fake_main(world["fa"], out)                                 # files of the forward mode are there: the stage runs again
    assert plain_runs() == 1 and FakeAnalysisEngine.calls[0] == "both"
    for name in NAMES:
        assert str(_npz(d / files_of(name)[0])["strand"]) == "both", name
    assert written(out / "m_nn_classification.log") == NAMES
    fake_main(world["fa"], out)
    assert plain_runs() == 1                                    # resumed under both
    set_env(monkeypatch, request_env(world["refs"]))
    fake_main(world["fa"], out)                                 # back under forward: again
    assert plain_runs() == 2 and FakeAnalysisEngine.calls.count("both") == 1
    for name in NAMES:
        assert "strand" not in _npz(d / files_of(name)[0]), name
        assert same_file(d / files_of(name)[0], world["on"] / "m_nn_classification" / files_of(name)[0]), name


@pytest.mark.parametrize("name,switches,changed,entry", ANALYSES, ids=NAMES)
def test_each_switch_alone_is_refused_without_the_embeddings(world, tmp_path, monkeypatch, capsys, name, switches, changed, entry):
    env = request_env(world["refs"], only=name)
    del env["GENOMAD_AMD_EMBEDDINGS"]
    set_env(monkeypatch, env)
    del FakeAnalysisEngine.calls[:]
    capsys.readouterr()
    with pytest.raises(SystemExit) as exc:
        fake_main(world["fa"], tmp_path / "refused")
    err = capsys.readouterr().err.strip().splitlines()
    assert exc.value.code == 1 and len(err) == 1 and f"{next(iter(switches))} " in err[0] and "GENOMAD_AMD_EMBEDDINGS=1" in err[0]
    assert not list((tmp_path / "refused").rglob("*.npz")) and not list((tmp_path / "refused").rglob("*.tsv"))
    assert FakeAnalysisEngine.calls == []
