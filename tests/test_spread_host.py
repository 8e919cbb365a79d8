"""sequence.label_spread, the definition gnn_spread computes on the device, on the host alone: against a brute force on Python integers,
its monotone rise, the planted families, the real fixed point it stays under, ``first`` against the hop count, the stopping rule and
``predict``; and GENOMAD_AMD_SPREAD in main(), over a fake engine that serves the graph and the spreading from their definitions: the
two files and their bytes on a worked example, the resume rule, the refusals, and that nothing else changes."""
import shutil

import numpy as np
import pytest

from genomad_amd import nn_classification as nnc, sequence
from genomad_amd.engine import SpreadResult
from tests import spread_data as D
from tests.test_analyses_host import ENV as OTHER_ENV, FakeAnalysisEngine, fake_main, same_file
from tests.test_strand_host import _npz, _same_npz, _tree, _write_fasta

ONE = sequence.SPREAD_ONE


def brute(csr, valid, label, n_classes, a, clamp, max_iter):
    """the definition, entry by entry, on Python integers: (F as a list of lists, changed)"""
    indptr, col, sim = csr
    n = len(indptr) - 1
    ok = [True] * n if valid is None else [bool(v) for v in valid]
    rows = [[] for _ in range(n)]
    for i in range(n):
        for x in range(int(indptr[i]), int(indptr[i + 1])):
            j, q = int(col[x]), int(np.rint(np.float64(np.float32(sim[x])) * 2.0 ** 24))
            if q > 0 and ok[i] and ok[j]:
                rows[i].append((j, q))
                rows[j].append((i, q))
    p = [[(j, (q << 31) // sum(q2 for _, q2 in r)) for j, q in r] for r in rows]
    seed = [ok[i] and label[i] >= 0 for i in range(n)]
    y = [[int(seed[i] and label[i] == c) for c in range(n_classes)] for i in range(n)]
    F = [[0] * n_classes for _ in range(n)]
    changed = []
    while len(changed) < max_iter and (not changed or changed[-1]):
        G = []
        for i in range(n):
            if not ok[i]:
                G.append([0] * n_classes)
            elif clamp and seed[i]:
                G.append([ONE * v for v in y[i]])
            else:
                G.append([(a * (sum(pij * F[j][c] for j, pij in p[i]) >> 31) + (64 - a) * ONE * y[i][c]) >> 6 for c in range(n_classes)])
        changed.append(sum(G[i] != F[i] for i in range(n)))
        F = G
    return F, changed


@pytest.mark.parametrize("name", ["planted", "random_masked", "path", "fan", "parallel", "star_at"])
@pytest.mark.parametrize("clamp,alpha", [(True, 0.5), (False, 63 / 64), (False, 1 / 64)])
def test_the_definition_equals_a_brute_force_on_python_integers(name, clamp, alpha):
    csr, valid, label = D.cases(3)[name]
    got = sequence.label_spread(*csr, label, 3, valid, alpha, clamp, max_iter=12)
    F, changed = brute(csr, valid, label, 3, int(alpha * 64), clamp, 12)
    assert got["score"].dtype == np.uint32 and got["score"].tolist() == F
    assert got["changed"].tolist() == changed and got["iterations"] == len(changed) and got["converged"] == (changed[-1] == 0)
    tot = [sum(r) for r in F]
    assert got["total"].dtype == np.uint64 and got["total"].tolist() == tot
    assert got["best"].tolist() == [r.index(max(r)) if max(r) else -1 for r in F] and got["best"].dtype == np.int32
    assert got["best_score"].tolist() == [max(r) for r in F]
    assert got["second_score"].tolist() == [sorted(r)[-2] for r in F]
    ok = np.ones(len(F), dtype=bool) if valid is None else valid
    assert np.array_equal(got["seed"], ok & (label >= 0))


@pytest.mark.parametrize("n_classes", [1, 3, 5])
@pytest.mark.parametrize("clamp,alpha", [(True, 0.5), (False, 0.75), (True, 63 / 64)])
def test_the_scores_never_fall_and_stay_within_one_on_every_iteration_of_every_fixture(n_classes, clamp, alpha):
    fixtures = dict(D.cases(n_classes))
    if n_classes == 1:
        fixtures["star"] = (D.STAR, None, D.star_labels(D.STAR_LEAVES))
    for name, (csr, valid, label) in fixtures.items():
        trace = []
        r = sequence.label_spread(*csr, label, n_classes, valid, alpha, clamp, max_iter=300 if alpha < 0.9 else 40, trace=trace)
        assert len(trace) == r["iterations"] == len(r["changed"]), name
        before = np.zeros_like(trace[0])
        for t, F in enumerate(trace):
            assert (F >= before).all() and F.max(initial=0) <= ONE, (name, t)
            assert r["changed"][t] == np.count_nonzero((F != before).any(axis=1)), (name, t)
            before = F
        assert r["converged"] == (r["changed"][-1] == 0) and (r["changed"][:-1] > 0).all(), name         # it stops at the first 0
        if valid is not None:
            assert not r["score"][~valid].any() and (r["best"][~valid] == -1).all() and (r["first"][~valid] == -1).all()


def test_the_star_fills_the_64_bit_headroom_and_the_hub_gets_the_leaves_class():
    r = sequence.label_spread(*D.STAR, D.star_labels(D.STAR_LEAVES), 1, alpha=63 / 64, clamp=True, max_iter=5)
    p = (1 << 31) // D.STAR_LEAVES
    assert D.STAR_LEAVES * p * ONE > 1 << 60                   # the hub's sum
    assert r["score"][0, 0] == (63 * ((D.STAR_LEAVES * p * ONE) >> 31)) >> 6 and r["first"][0] == 2 and r["converged"] and r["iterations"] == 3
    assert (r["score"][1:, 0] == ONE).all() and (r["first"][1:] == 1).all()


def test_planted_families_take_their_seeds_class_and_the_unseeded_one_follows_its_bridges():
    label = D.planted_labels(5)
    r = sequence.label_spread(*D.PLANTED, label, 5, alpha=0.5, max_iter=500)
    assert r["converged"]
    pred, conf, margin = sequence.spread_predict(r["best"], r["best_score"], r["second_score"], r["total"])
    for k, g in enumerate(D.PLANTED_SEEDED):
        rows = slice(D.PLANTED_START[g], D.PLANTED_START[g + 1])
        assert (pred[rows] == k).all(), g
        assert (conf[rows] > 0.5).all() and (margin[rows] > 0).all()
    rows = slice(D.PLANTED_START[2], D.PLANTED_START[3])       # bridged to group 1 (class 1) and group 3 (class 2), no seed of its own
    assert set(pred[rows].tolist()) <= {1, 2} and (r["first"][rows] > 1).all()
    assert (pred[D.PLANTED_START[6]:] == -1).all() and (r["total"][D.PLANTED_START[6]:] == 0).all()      # the two singletons
    assert np.isnan(conf[D.PLANTED_START[6]:]).all()


@pytest.mark.parametrize("name,alpha", [("planted", 0.5), ("random", 0.75), ("parallel", 0.5), ("fan", 0.25)])
def test_a_converged_unclamped_run_stands_just_under_the_real_fixed_point(name, alpha):
    """F* = (1 - alpha) (I - alpha P)^-1 Y in float64, P the real random-walk matrix q_ij / d_i.  In units of 2^-30, with f = F and
    T(f) = alpha P f + (1 - alpha) ONE y the real map, one integer step loses, per entry:
      p's floor    p_ij / 2^31 > P_ij - 2^-31, and F_j <= 2^30: sum_j p_ij F_j / 2^31 > (P F)_i - deg_i / 2      (deg_i: entries at row i)
      >> 31        less than 1
      >> 6         less than 1, after the product by alpha = a / 64: alpha * (deg_i / 2 + 1) + 1 in all.
    So T(F) - delta <= T_int(F) <= T(F) with delta = alpha * (deg_max / 2 + 1) + 1.  The integer iterates stay under the real ones
    (both maps are monotone, T_int <= T, both start at 0), which rise to F*: F <= F*.  At the integer fixed point e = F* - F obeys
    e = alpha P e + (T(F) - T_int(F)) <= alpha max(e) + delta, so max(e) <= delta / (1 - alpha): the issue's bound, as derived.  The
    float64 solve of a system whose condition is at most (1 + alpha) / (1 - alpha) <= 7 here is good to about 1e-14, far below the
    2^-40 allowed for it on either side."""
    csr, valid, label = D.cases(4)[name]
    r = sequence.label_spread(*csr, label, 4, valid, alpha, clamp=False, max_iter=2000)
    assert r["converged"]
    n, a, b, q, ok = sequence.mcl_weights(*csr, valid)
    W = np.zeros((n, n))
    np.add.at(W, (a, b), q.astype(np.float64))
    W = W + W.T
    d = W.sum(axis=1)
    P = np.divide(W, d[:, None], out=np.zeros_like(W), where=d[:, None] > 0)
    Y = np.zeros((n, 4))
    Y[np.flatnonzero(r["seed"]), label[r["seed"]]] = 1.0
    star = (1 - alpha) * np.linalg.solve(np.eye(n) - alpha * P, Y)
    deg_max = int(np.bincount(np.concatenate([a, b]), minlength=n).max())
    gap = star - r["score"].astype(np.float64) / ONE
    slack = 2.0 ** -40
    assert gap.min() >= -slack
    assert gap.max() <= (alpha * (deg_max / 2 + 1) + 1) / (1 - alpha) * 2.0 ** -30 + slack


def test_first_is_the_hop_count_until_the_score_floors_to_zero():
    """PATH, one clamped seed at row 0, alpha = 1/2: the mass that arrives at hop k for the first time is 2^(30 - 2k) - a quarter per
    hop (half of the neighbour's row, half of alpha) - so it is 1 at hop 15 and floors to 0 at hop 16: up to hop 15 ``first`` is the
    hop count + 1 (iteration 1 sets the seed), from hop 16 on a row waits for more mass than the first wave, or for ever."""
    n = D.n_of(D.PATH)
    label = np.concatenate([[0], np.full(n - 1, -1)]).astype(np.int64)
    trace = []
    r = sequence.label_spread(*D.PATH, label, 1, alpha=0.5, max_iter=2000, trace=trace)
    assert r["converged"]
    hop = np.arange(n)
    assert np.array_equal(r["first"][:16], hop[:16] + 1)
    for k in range(1, 16):
        assert trace[k][k, 0] == 1 << (30 - 2 * k) and trace[k - 1][k, 0] == 0
    assert trace[16][16, 0] == 0 and ((r["first"][16:] == -1) | (r["first"][16:] > hop[16:] + 1)).all()
    assert (r["first"] == -1).any()                            # the far end is never reached: 40 hops would need 2^-80


def test_max_iter_cuts_it_short_and_changed_ends_in_zero_exactly_when_converged():
    csr, valid, label = D.cases(3)["random"]
    full = sequence.label_spread(*csr, label, 3, valid, 0.5, max_iter=1000)
    assert full["converged"] and full["changed"][-1] == 0 and (full["changed"][:-1] > 0).all() and full["iterations"] > 5
    cut = sequence.label_spread(*csr, label, 3, valid, 0.5, max_iter=5)
    assert not cut["converged"] and cut["iterations"] == 5 and np.array_equal(cut["changed"], full["changed"][:5]) and cut["changed"][-1] > 0
    exact = sequence.label_spread(*csr, label, 3, valid, 0.5, max_iter=full["iterations"])
    assert exact["converged"] and np.array_equal(exact["score"], full["score"])
    none = sequence.label_spread(*csr, np.full(len(label), -1), 3, valid, 0.5)
    assert none["converged"] and none["iterations"] == 1 and none["changed"].tolist() == [0] and not none["score"].any()
    assert (none["best"] == -1).all() and (none["first"] == -1).all()
    empty = sequence.label_spread(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0, np.int64), 2)
    assert empty["score"].shape == (0, 2) and empty["iterations"] == 1 and empty["converged"]


def test_predict_ties_min_score_and_table():
    best = np.array([0, 1, -1, 2], dtype=np.int32)
    bs = np.array([ONE // 2, ONE // 4, 0, ONE // 8], dtype=np.uint32)
    ss = np.array([ONE // 2, 0, 0, ONE // 16], dtype=np.uint32)
    tot = np.array([ONE, ONE // 4, 0, ONE // 4], dtype=np.uint64)
    label, conf, margin = sequence.spread_predict(best, bs, ss, tot)
    assert label.tolist() == [0, 1, -1, 2] and conf[:2].tolist() == [0.5, 1.0] and margin[:2].tolist() == [0.0, 1.0]
    assert np.isnan(conf[2]) and np.isnan(margin[2]) and conf[3] == 0.5 and margin[3] == 0.25
    label, conf, _ = sequence.spread_predict(best, bs, ss, tot, min_score=0.25)
    assert label.tolist() == [0, 1, -1, -1] and np.isnan(conf[3])
    tied = sequence.spread_summary(np.array([[5, 9, 9], [0, 0, 0], [7, 0, 0]], dtype=np.uint32))
    assert tied["best"].tolist() == [1, -1, 0] and tied["second_score"].tolist() == [9, 0, 0] and tied["total"].tolist() == [23, 0, 7]
    t = sequence.spread_table(best, bs, ss, tot, np.array([1, 2, -1, 3]), names=list("abcd"), class_names=["x", "y", "z"])
    assert t[0] == {"row": "a", "label": "x", "confidence": 0.5, "score": 0.5, "total_score": 1.0, "first": 1}
    assert t[2]["label"] is None and t[2]["confidence"] is None and t[2]["first"] == -1
    with pytest.raises(ValueError, match="min_score"):
        sequence.spread_predict(best, bs, ss, tot, min_score=2)


def test_bad_arguments_are_value_errors():
    csr, valid, label = D.cases(3)["path"]
    for alpha in (0, 1, 0.3, 1 / 128, True, "x"):
        with pytest.raises(ValueError, match="alpha"):
            sequence.label_spread(*csr, label, 3, alpha=alpha)
    assert [sequence.spread_alpha(x) for x in (1 / 64, 0.5, 63 / 64)] == [1, 32, 63]
    for kw, match in ((dict(n_classes=0), "n_classes"), (dict(n_classes=1025), "n_classes"), (dict(max_iter=0), "max_iter")):
        with pytest.raises(ValueError, match=match):
            sequence.label_spread(*csr, label, **{"n_classes": 3, **kw})
    with pytest.raises(ValueError, match="label is outside"):
        sequence.label_spread(*csr, np.where(label >= 0, 3, label), 3)
    with pytest.raises(ValueError, match="upper triangle"):
        sequence.label_spread(csr[0], csr[1][::-1].copy(), csr[2], label, 3)


# ---- GENOMAD_AMD_SPREAD in main() --------------------------------------------------------------------------------------------------------------
SPREAD_ENV = ("GENOMAD_AMD_SPREAD", "GENOMAD_AMD_SPREAD_BASE", "GENOMAD_AMD_SPREAD_MAX_ITER", "GENOMAD_AMD_MCL", "GENOMAD_AMD_MCL_SELECT")
BASE = {"GENOMAD_AMD_EMBEDDINGS": "1", "GENOMAD_AMD_GRAPH": "0.999"}
FILES = ["m_nn_spread.npz", "m_nn_spread.tsv"]


class FakeSpreadEngine(FakeAnalysisEngine):
    """the stand-in of tests/test_analyses_host.py plus label spreading from sequence.label_spread"""

    def spread(self, indptr, col, sim, label, n_classes, valid=None, alpha=0.5, clamp=True, max_iter=200, scores=True):
        type(self).calls.append(("spread", len(indptr) - 1, int(n_classes), float(alpha), bool(clamp), int(max_iter), bool(scores)))
        r = sequence.label_spread(indptr, col, sim, label, n_classes, valid, alpha, clamp, max_iter)
        if not scores:
            r["score"] = None
        return SpreadResult(**r, n=len(indptr) - 1, n_classes=int(n_classes), alpha=float(alpha), clamp=bool(clamp))


def set_env(mp, env):
    """exactly the switches of ``env``, none of the others"""
    mp.setattr(nnc, "_engine", lambda: FakeSpreadEngine())
    for k in OTHER_ENV + SPREAD_ENV:
        mp.delenv(k, raising=False)
    for k, v in env.items():
        mp.setenv(k, v)


def names_of_calls():
    return [c[0] if isinstance(c, tuple) else c for c in FakeSpreadEngine.calls]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """One run with the graph but without GENOMAD_AMD_SPREAD and one with it, shared and left unchanged.  The contigs: c0 .. c5, one run of N and
    two twins of c2.  The reference: the run's own c0, c2 and c4 - c0 a virus, c2 a plasmid, c4 without a label - so at 0.999 the twins reach
    the plasmid label through c2's row of the reference, c0 its own, and nobody else anything."""
    root = tmp_path_factory.mktemp("spread")
    fa = root / "m.fna"
    recs = _write_fasta(fa, n=6)
    with open(fa, "a") as f:
        for k in range(2):
            f.write(f">twin{k} of c2\n{dict(recs)['c2']}\n")
    with pytest.MonkeyPatch.context() as mp:
        set_env(mp, BASE)
        fake_main(fa, root / "unset")
        z = _npz(root / "unset" / "m_nn_classification" / "m_nn_embeddings.npz")
        pick = [list(z["contig_names"]).index(c) for c in ("c0", "c2", "c4")]
        ref = root / "reference.npz"
        np.savez_compressed(ref, embeddings=z["embeddings"][pick], contig_names=np.array(["r0", "r2", "r4"]), labels=np.array(["virus", "plasmid", ""]))
        on = dict(BASE, GENOMAD_AMD_SPREAD="0.5", GENOMAD_AMD_SPREAD_BASE=str(ref))
        set_env(mp, on)
        del FakeSpreadEngine.calls[:]
        fake_main(fa, root / "on")
        found = list(FakeSpreadEngine.calls)
    return {"fa": fa, "ref": ref, "env": on, "unset": root / "unset" / "m_nn_classification", "on": root / "on", "calls": found}


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
    assert [c[0] for c in calls] == ["graph", "graph", "spread"]          # the last of the analyses, over a graph of its own
    assert calls[1][1] == 3 + 9 and calls[2] == ("spread", 12, 2, 0.5, True, 200, True)
    log = [line for line in (world["on"] / "m_nn_classification.log").read_text().splitlines() if " written to " in line]
    assert log[-1].endswith("written to m_nn_spread.npz and m_nn_spread.tsv.")
    assert "Labels of reference.npz spread to the sequences (cosine similarity of the encoder embeddings >= 0.999, " in log[-1]
    assert "8 edges among 3 reference rows and 9 sequences, alpha 0.5, 2 classes: 4 of 9 sequences got a label in " in log[-1]
    assert log[-1].split(" iterations, ")[1].startswith("converged)")


def test_the_files_hold_the_definition_on_a_worked_example(world):
    d = world["on"] / "m_nn_classification"
    z, emb, ref = _npz(d / FILES[0]), _npz(d / "m_nn_embeddings.npz"), _npz(world["ref"])
    rows = np.concatenate([ref["embeddings"], emb["embeddings"]])
    g = sequence.threshold_graph(rows, 0.999, "cosine")
    label = np.array([1, 0, -1] + [-1] * 9)                      # classes sorted: plasmid 0, virus 1
    want = sequence.label_spread(g[0], g[1], g[2].astype(np.float32), label, 2, sequence.valid_rows(rows), 0.5, True, 200)
    for k in sequence.SPREAD_FIELDS:
        assert z[k].dtype == want[k].dtype and np.array_equal(z[k], want[k][3:]), k
    assert z["classes"].tolist() == ["plasmid", "virus"] and z["base_names"].tolist() == ["r0", "r2", "r4"] and z["base_label"].tolist() == [1, 0, -1]
    assert z["alpha"] == 0.5 and z["threshold"] == float(np.float32(0.999)) and z["max_iter"] == 200 and str(z["metric"]) == "cosine"
    assert z["iterations"] == want["iterations"] and z["converged"] and np.array_equal(z["changed"], want["changed"]) and "strand" not in z
    assert z["n_edges"] == len(g[1]) == 8                        # r0-c0, r4-c4, and the six pairs among r2, c2 and the twins
    names = [str(x) for x in z["contig_names"]]
    got = dict(zip(names, z["label"].tolist()))
    assert got == {"c0": 1, "c1": -1, "c2": 0, "nrun": -1, "c3": -1, "c4": -1, "c5": -1, "twin0": 0, "twin1": 0}
    # identical rows: cosine 1, q = 2^24 each.  c0 has the one neighbour r0: p = 2^31, g = ONE, score = (32 * ONE) >> 6 = ONE / 2
    # behind iteration 2.  c2 has three: p = floor(2^31 / 3) each; the seed r2 gives ONE, the twins what they have
    c0, c2 = names.index("c0"), names.index("c2")
    assert z["best_score"][c0] == ONE // 2 and z["first"][c0] == 2 and z["total"][c0] == ONE // 2 and z["confidence"][c0] == 1.0
    assert z["first"][c2] == 2 and z["score"][c2].tolist() == [z["best_score"][c2], 0] and ONE // 6 <= z["best_score"][c2] < ONE // 4 + 1
    lines = (d / FILES[1]).read_bytes().decode().split("\n")
    assert lines[0] == "seq_name\tlabel\tconfidence\tscore\ttotal_score\tfirst" and lines[-1] == "" and len(lines) == 11
    rows = {x.split("\t")[0]: x.split("\t")[1:] for x in lines[1:-1]}
    assert list(rows) == names
    assert rows["c0"] == ["virus", "1.000000", "0.500000", "0.500000", "2"]
    assert rows["c1"] == rows["c4"] == ["NA", "NA", "NA", "0.000000", "NA"]
    assert rows["c2"] == rows["twin0"] == rows["twin1"] == ["plasmid", "1.000000", f"{z['best_score'][c2] / ONE:.6f}", f"{z['best_score'][c2] / ONE:.6f}", "2"]


def test_the_same_command_again_calls_nothing_and_another_request_runs_again(world, tmp_path, monkeypatch):
    out, d = copy_of(world, tmp_path)
    everything = _tree(d)
    on = world["env"]
    set_env(monkeypatch, on)
    del FakeSpreadEngine.calls[:]
    fake_main(world["fa"], out)
    assert FakeSpreadEngine.calls == []
    runs = 0
    for env, entry in ((dict(on, GENOMAD_AMD_SPREAD="0.75"), ("alpha", 0.75)), (dict(on, GENOMAD_AMD_SPREAD_MAX_ITER="2"), ("max_iter", 2)),
                       (dict(on, GENOMAD_AMD_GRAPH="0.5"), ("threshold", 0.5)), (on, ("alpha", 0.5))):
        set_env(monkeypatch, env)
        fake_main(world["fa"], out)                             # another alpha, max_iter or threshold: the stage runs again
        runs += 1
        assert names_of_calls().count("plain") == runs and _npz(d / FILES[0])[entry[0]] == entry[1] and _tree(d) == everything
        fake_main(world["fa"], out)                             # and is resumed from
        assert names_of_calls().count("plain") == runs
    assert same_file(d / FILES[0], world["on"] / "m_nn_classification" / FILES[0])
    assert (d / FILES[1]).read_bytes() == (world["on"] / "m_nn_classification" / FILES[1]).read_bytes()
    (d / FILES[1]).unlink()
    fake_main(world["fa"], out)                                 # one of the pair is gone: again
    assert names_of_calls().count("plain") == runs + 1 and _tree(d) == everything
    z = dict(_npz(world["ref"]))
    z["labels"] = np.array(["virus", "virus", ""])
    other = tmp_path / "reference.npz"
    np.savez_compressed(other, **z)
    set_env(monkeypatch, dict(on, GENOMAD_AMD_SPREAD_BASE=str(other)))
    fake_main(world["fa"], out)                                 # the same names under other labels: again
    assert names_of_calls().count("plain") == runs + 2 and _npz(d / FILES[0])["classes"].tolist() == ["virus"]


def test_unset_again_its_files_go_and_every_output_is_what_it_was(world, tmp_path, monkeypatch):
    out, d = copy_of(world, tmp_path)
    set_env(monkeypatch, BASE)
    del FakeSpreadEngine.calls[:]
    fake_main(world["fa"], out)
    assert "spread" not in names_of_calls() and _tree(d) == _tree(world["unset"])
    for rel in _tree(d):
        if rel.endswith(".npz"):
            assert _same_npz(world["unset"] / rel, d / rel), rel
        elif rel.endswith(".tsv"):
            assert (world["unset"] / rel).read_bytes() == (d / rel).read_bytes(), rel


@pytest.mark.parametrize("missing,said", [("GENOMAD_AMD_GRAPH", "GENOMAD_AMD_SPREAD needs GENOMAD_AMD_GRAPH: "),
                                          ("GENOMAD_AMD_SPREAD_BASE", "GENOMAD_AMD_SPREAD and GENOMAD_AMD_SPREAD_BASE need each other and GENOMAD_AMD_EMBEDDINGS=1: "),
                                          ("GENOMAD_AMD_SPREAD", "GENOMAD_AMD_SPREAD and GENOMAD_AMD_SPREAD_BASE need each other and GENOMAD_AMD_EMBEDDINGS=1: "),
                                          ("GENOMAD_AMD_EMBEDDINGS", "GENOMAD_AMD_GRAPH needs GENOMAD_AMD_EMBEDDINGS=1: ")])
def test_each_switch_without_its_partners_is_refused(world, tmp_path, monkeypatch, capsys, missing, said):
    """without the embeddings it is the graph, which the spread needs and which comes first in the table, that says so"""
    set_env(monkeypatch, {k: v for k, v in world["env"].items() if k != missing})
    del FakeSpreadEngine.calls[:]
    capsys.readouterr()
    with pytest.raises(SystemExit) as exc:
        fake_main(world["fa"], tmp_path / "refused")
    err = capsys.readouterr().err.strip().splitlines()
    assert exc.value.code == 1 and len(err) == 1 and said in err[0]
    if missing != "GENOMAD_AMD_EMBEDDINGS":
        assert "the labelled reference's labels spread along the similarity graph" in err[0]
    assert not list((tmp_path / "refused").rglob("*.npz")) and FakeSpreadEngine.calls == []


def test_bad_values_and_a_bad_reference(world, tmp_path, monkeypatch, capsys):
    on = world["env"]
    for env, match in ((dict(on, GENOMAD_AMD_SPREAD="0.3"), "GENOMAD_AMD_SPREAD='0.3'"), (dict(on, GENOMAD_AMD_SPREAD="1"), "multiple of 1/64"),
                       (dict(on, GENOMAD_AMD_SPREAD="x"), "GENOMAD_AMD_SPREAD='x'"), (dict(on, GENOMAD_AMD_SPREAD_MAX_ITER="0"), "GENOMAD_AMD_SPREAD_MAX_ITER"),
                       (dict(on, GENOMAD_AMD_SPREAD_MAX_ITER="10001"), "GENOMAD_AMD_SPREAD_MAX_ITER"),
                       (dict(BASE, GENOMAD_AMD_SPREAD_MAX_ITER="5"), "GENOMAD_AMD_SPREAD_MAX_ITER='5' needs GENOMAD_AMD_SPREAD")):
        set_env(monkeypatch, env)
        with pytest.raises(ValueError, match=match):
            fake_main(world["fa"], tmp_path / "bad")
    set_env(monkeypatch, dict(on, GENOMAD_AMD_SPREAD="0.984375", GENOMAD_AMD_SPREAD_MAX_ITER="10000"))
    assert nnc.spread_requested() == (63 / 64, float(np.float32(0.999)), 10000)
    set_env(monkeypatch, BASE)
    assert nnc.spread_requested() is None
    plain = tmp_path / "plain.npz"                               # an embeddings file without labels: the message names the spread's switch
    z = _npz(world["ref"])
    np.savez_compressed(plain, embeddings=z["embeddings"], contig_names=z["contig_names"])
    set_env(monkeypatch, dict(on, GENOMAD_AMD_SPREAD_BASE=str(plain)))
    capsys.readouterr()
    with pytest.raises(SystemExit):
        fake_main(world["fa"], tmp_path / "bad")
    err = capsys.readouterr().err
    assert f"GENOMAD_AMD_SPREAD_BASE={str(plain)!r}: it must hold 'labels'" in err and "GENOMAD_AMD_VOTE" not in err
    assert "or unset GENOMAD_AMD_SPREAD and GENOMAD_AMD_SPREAD_BASE." in err
    with pytest.raises(ValueError, match="GENOMAD_AMD_VOTE_BASE="):
        nnc.load_vote_base(plain)                                # the vote's own messages are what they were
