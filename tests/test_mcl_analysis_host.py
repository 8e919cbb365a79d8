"""GENOMAD_AMD_MCL in main(), over a fake engine that serves the graph and its Markov clusters from their definitions: the two files and
what they hold, the log line, the refusals (no graph, no embeddings, a select without an inflation, a bad inflation), the resume rule on
(inflation, threshold, select), and that nothing else changes - with the switch unset every output is what it was."""
import shutil

import numpy as np
import pytest

from genomad_amd import nn_classification as nnc, sequence
from genomad_amd.engine import MCLResult
from tests.test_analyses_host import ENV as OTHER_ENV, FakeAnalysisEngine, fake_main, same_file
from tests.test_strand_host import _npz, _same_npz, _tree, _write_fasta

MCL_ENV = ("GENOMAD_AMD_MCL", "GENOMAD_AMD_MCL_SELECT")
BASE = {"GENOMAD_AMD_EMBEDDINGS": "1", "GENOMAD_AMD_GRAPH": "0.999", "GENOMAD_AMD_CLUSTERS": "0.999"}
ON = dict(BASE, GENOMAD_AMD_MCL="2")
FILES = ["m_nn_mcl.npz", "m_nn_mcl.tsv"]


class FakeMclEngine(FakeAnalysisEngine):
    """the stand-in of tests/test_analyses_host.py plus Markov clusters from sequence.markov_clusters"""

    def mcl(self, indptr, col, sim, valid=None, inflation=2.0, select=256, precision=10000, max_iter=100):
        type(self).calls.append(("mcl", len(indptr) - 1, float(inflation), int(select)))
        r = sequence.markov_clusters(indptr, col, sim, valid, inflation, select, precision, max_iter)
        return MCLResult(**{k: r[k] for k in sequence.MCL_FIELDS + ("iterations", "converged", "changed")}, n=len(indptr) - 1,
                         inflation=float(inflation), select=int(select), precision=int(precision))


def set_env(mp, env):
    """exactly the switches of ``env``, none of the others"""
    mp.setattr(nnc, "_engine", lambda: FakeMclEngine())
    for k in OTHER_ENV + MCL_ENV:
        mp.delenv(k, raising=False)
    for k, v in env.items():
        mp.setenv(k, v)


def calls():
    return [c[0] if isinstance(c, tuple) else c for c in FakeMclEngine.calls]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """one run with the graph and the clusters but without GENOMAD_AMD_MCL and one with it, shared and left unchanged"""
    root = tmp_path_factory.mktemp("mcl")
    fa = root / "m.fna"
    recs = _write_fasta(fa, n=6)
    with open(fa, "a") as f:
        for k in range(2):
            f.write(f">twin{k} of c2\n{dict(recs)['c2']}\n")   # the same bytes as c2: the same embedding
    with pytest.MonkeyPatch.context() as mp:
        set_env(mp, BASE)
        fake_main(fa, root / "unset")
        set_env(mp, ON)
        del FakeMclEngine.calls[:]
        fake_main(fa, root / "on")
        found = list(FakeMclEngine.calls)
    return {"fa": fa, "unset": root / "unset" / "m_nn_classification", "on": root / "on", "calls": found}


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
    names = [c[0] for c in world["calls"] if isinstance(c, tuple)]
    assert names == ["cluster", "graph", "graph", "mcl"]        # directly behind the graph, which it computes again
    assert world["calls"][-1] == ("mcl", 9, 2.0, 256)
    log = [line for line in (world["on"] / "m_nn_classification.log").read_text().splitlines() if " written to " in line]
    order = [line.split(" written to ")[1] for line in log]
    assert order.index("m_nn_mcl.npz and m_nn_mcl.tsv.") == order.index("m_nn_graph.npz and m_nn_graph.tsv.") + 1
    line = next(x for x in log if "m_nn_mcl.npz" in x)
    assert "Markov clusters of the sequences (cosine similarity of the encoder embeddings >= 0.999, " in line
    assert "inflation 2, at most 256 entries per column: 7 clusters in " in line and ", converged) written to" in line


def test_the_files_hold_the_definition_of_the_graph_file(world):
    d = world["on"] / "m_nn_classification"
    z, g = _npz(d / "m_nn_mcl.npz"), _npz(d / "m_nn_graph.npz")
    emb = _npz(d / "m_nn_embeddings.npz")
    want = sequence.markov_clusters(g["indptr"], g["col"], g["sim"], sequence.valid_rows(emb["embeddings"]), 2.0, 256)
    for k in sequence.MCL_FIELDS + ("changed",):
        assert z[k].dtype == want[k].dtype and np.array_equal(z[k], want[k]), k
    assert z["inflation"] == 2.0 and z["threshold"] == float(np.float32(0.999)) and z["select"] == 256 and z["precision"] == 10000
    assert z["iterations"] == want["iterations"] and z["converged"] == want["converged"] and str(z["metric"]) == "cosine" and "strand" not in z
    names = [str(x) for x in z["contig_names"]]
    lines = (d / "m_nn_mcl.tsv").read_text().splitlines()
    assert lines[0] == "seq_name\tcluster\tcluster_size\tattractor\tflow" and [x.split("\t")[0] for x in lines[1:]] == names
    rows = {x.split("\t")[0]: x.split("\t")[1:] for x in lines[1:]}
    assert rows["twin0"][:2] == rows["twin1"][:2] == rows["c2"][:2] == ["c2", "3"]             # the three identical contigs: one family
    assert sorted(r[1] for r in rows.values()) == ["1"] * 6 + ["3"] * 3
    for name, r in rows.items():
        i = names.index(name)
        assert r[2] == names[want["attractor"][i]] and abs(float(r[3]) - want["flow"][i] / 2 ** 30) < 1e-6


def test_the_same_command_again_calls_nothing_and_another_request_runs_again(world, tmp_path, monkeypatch):
    out, d = copy_of(world, tmp_path)
    everything = _tree(d)
    set_env(monkeypatch, ON)
    del FakeMclEngine.calls[:]
    fake_main(world["fa"], out)
    assert FakeMclEngine.calls == []
    assert "m_nn_classification.npz was found. Skipping sequence classification." in (out / "m_nn_classification.log").read_text()
    runs = 0
    for env, entry in ((dict(ON, GENOMAD_AMD_MCL="1.5"), ("inflation", 1.5)), (dict(ON, GENOMAD_AMD_MCL="1.5", GENOMAD_AMD_MCL_SELECT="2"), ("select", 2)),
                       (dict(ON, GENOMAD_AMD_GRAPH="0.5"), ("threshold", 0.5)), (ON, ("inflation", 2.0))):
        set_env(monkeypatch, env)
        fake_main(world["fa"], out)                             # another inflation, select or threshold: the stage runs again
        runs += 1
        assert calls().count("plain") == runs and _npz(d / FILES[0])[entry[0]] == entry[1] and _tree(d) == everything
        fake_main(world["fa"], out)                             # and is resumed from
        assert calls().count("plain") == runs
    assert same_file(d / FILES[0], world["on"] / "m_nn_classification" / FILES[0])
    assert (d / FILES[1]).read_bytes() == (world["on"] / "m_nn_classification" / FILES[1]).read_bytes()
    (d / FILES[1]).unlink()
    fake_main(world["fa"], out)                                 # one of the pair is gone: again
    assert calls().count("plain") == runs + 1 and _tree(d) == everything
    (d / FILES[0]).write_bytes(b"")
    fake_main(world["fa"], out)                                 # an unreadable npz: again
    assert calls().count("plain") == runs + 2 and same_file(d / FILES[0], world["on"] / "m_nn_classification" / FILES[0])


def test_unset_again_its_files_go_and_every_output_is_what_it_was(world, tmp_path, monkeypatch):
    out, d = copy_of(world, tmp_path)
    set_env(monkeypatch, BASE)
    del FakeMclEngine.calls[:]
    fake_main(world["fa"], out)
    assert "mcl" not in calls() and _tree(d) == _tree(world["unset"])
    for rel in _tree(d):
        if rel.endswith(".npz"):
            assert _same_npz(world["unset"] / rel, d / rel), rel
        elif rel.endswith(".tsv"):
            assert (world["unset"] / rel).read_bytes() == (d / rel).read_bytes(), rel


@pytest.mark.parametrize("missing,needed", [("GENOMAD_AMD_GRAPH", "GENOMAD_AMD_GRAPH"), ("GENOMAD_AMD_EMBEDDINGS", "GENOMAD_AMD_EMBEDDINGS=1")])
def test_it_is_refused_without_the_graph_or_the_embeddings(world, tmp_path, monkeypatch, capsys, missing, needed):
    env = {k: v for k, v in ON.items() if k not in (missing, "GENOMAD_AMD_CLUSTERS")}
    if missing == "GENOMAD_AMD_EMBEDDINGS":
        del env["GENOMAD_AMD_GRAPH"]                            # the graph's own refusal would come first
    set_env(monkeypatch, env)
    del FakeMclEngine.calls[:]
    capsys.readouterr()
    with pytest.raises(SystemExit) as exc:
        fake_main(world["fa"], tmp_path / "refused")
    err = capsys.readouterr().err.strip().splitlines()
    assert exc.value.code == 1 and len(err) == 1 and f"GENOMAD_AMD_MCL needs {needed}: " in err[0] and "or unset GENOMAD_AMD_MCL." in err[0]
    assert "the flow runs on the similarity graph of the per-contig encoder embeddings" in err[0]
    assert not list((tmp_path / "refused").rglob("*.npz")) and FakeMclEngine.calls == []


def test_bad_values_are_value_errors(world, tmp_path, monkeypatch):
    for env, match in ((dict(ON, GENOMAD_AMD_MCL="1.3"), "GENOMAD_AMD_MCL='1.3'"), (dict(ON, GENOMAD_AMD_MCL="9"), "multiple of 0.25"),
                       (dict(ON, GENOMAD_AMD_MCL="x"), "GENOMAD_AMD_MCL='x'"), (dict(ON, GENOMAD_AMD_MCL_SELECT="0"), "GENOMAD_AMD_MCL_SELECT"),
                       (dict(ON, GENOMAD_AMD_MCL_SELECT="1025"), "GENOMAD_AMD_MCL_SELECT"),
                       (dict(BASE, GENOMAD_AMD_MCL_SELECT="64"), "GENOMAD_AMD_MCL_SELECT='64' needs GENOMAD_AMD_MCL")):
        set_env(monkeypatch, env)
        with pytest.raises(ValueError, match=match):
            fake_main(world["fa"], tmp_path / "bad")
    set_env(monkeypatch, dict(ON, GENOMAD_AMD_MCL="8", GENOMAD_AMD_MCL_SELECT="1024"))
    assert nnc.mcl_requested() == (8.0, float(np.float32(0.999)), 1024)
    set_env(monkeypatch, BASE)
    assert nnc.mcl_requested() is None
