"""Record the reference calls the CPU tests compare against (run where the reference checkout exists).

TEST INFRASTRUCTURE ONLY — see oracle/__init__.py.

    python -m oracle.make_golden_reference_calls

The tests below used to call the reference's functions in place; they now read what those calls
returned, so that the suite needs nothing outside the repository.  Every input is rebuilt here
exactly as the test builds it, and stored with its output (or keyed by its sha256) so that a test
can tell when its inputs no longer are the recorded ones.

* reference_calls.json
  - ``tokenize`` / ``windows`` (tests/test_oracle.py::test_oracle_against_live_reference_functions):
    genomad/sequence.py tokenize_dna(s, 4) on 200 random byte strings, and the window lengths of
    seq_windows(Sequence("x", "A" * L), 6000, 2500) for 40 random lengths;
  - ``fasta`` (tests/test_host.py::test_native_fasta_packer_equals_the_python_rules_and_the_reference):
    per FASTA text (keyed by its sha256), the accessions and the joined sequence read_fasta(p, strip_n)
    yields for strip_n True / False, and check_fasta(p) - or "IndexError" where the reference raises it.
* reference_calls.npz
  - ``net7_tokens_sha256``, ``net7_scores64`` / ``net7_scores32``
    (tests/test_oracle.py::test_oracle_matches_reference_network_code_live): create_classifier() of
    model.py / igloo.py over the numpy stand-ins of oracle/keras_shim.py, seed-7 weights, two windows
    with N runs;
  - ``torch16_tokens_sha256``, ``torch16_scores64``
    (tests/test_oracle.py::test_whole_graph_against_an_independent_torch_implementation): the same graph,
    seed-42 weights, the test's 16 windows;
  - ``patches_seed5`` (tests/test_host.py::test_gen_patches_follows_the_reference_initializer):
    igloo.py gen_filters_igloo(4, 2100, 5997, return_sequences=False, build_backbone=False) after
    np.random.seed(5).
"""
import hashlib
import importlib
import json
import os
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")

from genomad_amd import synthetic  # noqa: E402
from oracle import reference_harness, sequence_oracle  # noqa: E402


def sha256(b: bytes) -> str:
    return hashlib.sha256(b).hexdigest()


def live_function_cases():
    """the inputs of test_oracle_against_live_reference_functions, in its order"""
    rng = np.random.default_rng(11)
    alpha = np.frombuffer(b"ACGTNacgtnRY-", dtype=np.uint8)
    strings = [bytes(alpha[rng.integers(0, len(alpha), int(rng.integers(0, 60)))]) for _ in range(200)]
    lengths = [int(L) for L in rng.integers(1, 40000, 40)]
    return strings, lengths


def fasta_cases():
    """the FASTA texts of test_native_fasta_packer_equals_the_python_rules_and_the_reference"""
    cases = [
        b"", b"\n", b">", b">\n", b">a", b">a\n", b">a\nACGT", b">a\nACGT\n", b"ACGT\n>a\nAC\n\nGT\n",
        b">a\n\n\n>b\nNNNN\n>c\nnNACGTNn\n>d\nN\nA\nN\n", b">a desc here\n AC GT \n>b\tq\nAC>GT\n>>c\n>\nAC\n",
        b"\n>a\nACGT\n>a\nACGT\n", b">a\nNNNN\n>a\nNN\n", b">x\n" + b"N" * 5000 + b"\n" + b"ACGT" * 10 + b"\n" + b"n" * 70 + b"\n",
        b">a\r\nAC\r\nGT\r\n>b\rACGT\r", b">only header no newline", b"no header at all\nACGT\n",
        b">a\nACGT\n>b\n>c\n\n>d\nTTTT",
    ]
    rng = np.random.default_rng(11)
    alphabet = np.frombuffer(b"ACGTNnacgt>>\n\n\n xyz", dtype=np.uint8)
    for k in range(60):
        body = alphabet[rng.integers(0, len(alphabet), int(rng.integers(1, 400)))].tobytes()
        cases.append((b">r%d\n" % k if k % 3 else b"") + body)
    return cases


def torch16_tokens():
    bases = synthetic.synth_windows(0, 16).copy()
    bases[2, 777:790] = np.frombuffer(b"RYKMSWacgtnN-", dtype=np.uint8)
    bases[3, :3] = ord("N")
    return sequence_oracle.tokenize_closed_form(bases)


def net7_tokens():
    bases = synthetic.synth_windows(5000, 2)
    bases[0, 100:140] = ord("N")
    bases[1, 5990:] = ord("N")
    return sequence_oracle.tokenize_closed_form(bases)


def main():
    ref = reference_harness.load_reference_sequence()
    strings, lengths = live_function_cases()
    out = {"source": "outputs of the reference's genomad/sequence.py executed in place (oracle/make_golden_reference_calls.py)",
           "tokenize": [{"s": s.hex(), "tokens": list(ref.tokenize_dna(s, 4))} for s in strings],
           "windows": [{"L": L, "lens": [len(w) for w in ref.seq_windows(ref.Sequence("x", "A" * L), 6000, 2500)]} for L in lengths],
           "fasta": {}}

    def attempt(f, *a):
        try:
            return f(*a)
        except IndexError:
            return "IndexError"

    with tempfile.TemporaryDirectory() as tmp:
        for i, text in enumerate(fasta_cases()):
            p = Path(tmp) / f"case{i}.fna"
            with open(p, "wb") as f:
                f.write(text)
            rec = {}
            for strip in (True, False):
                got = attempt(lambda: [(r.accession, r.seq) for r in ref.read_fasta(p, strip_n=strip)])
                rec[f"strip_{str(strip).lower()}"] = got if isinstance(got, str) else \
                    {"accessions": [a for a, _ in got], "seq": "".join(s for _, s in got)}
            rec["check_fasta"] = attempt(ref.check_fasta, p)
            out["fasta"][sha256(text)] = rec
    with open(os.path.join(GOLDEN, "reference_calls.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))

    nn = reference_harness.load_reference_network()
    assert nn is not None
    igloo = importlib.import_module("genomad.neural_network.igloo")
    np.random.seed(5)
    patches = np.asarray(igloo.gen_filters_igloo(4, 2100, 5997, return_sequences=False, build_backbone=False))
    t7, t16 = net7_tokens(), torch16_tokens()
    w7 = synthetic.synth_weights(seed=7)
    np.savez_compressed(
        os.path.join(GOLDEN, "reference_calls.npz"),
        net7_tokens_sha256=sha256(t7.astype(np.int64).tobytes()),
        net7_scores64=reference_harness.reference_classifier_scores(t7, w7, np.float64),
        net7_scores32=reference_harness.reference_classifier_scores(t7, w7, np.float32),
        torch16_tokens_sha256=sha256(t16.astype(np.int64).tobytes()),
        torch16_scores64=reference_harness.reference_classifier_scores(t16, synthetic.synth_weights(), np.float64),
        patches_seed5=patches)
    print("wrote", os.path.join(GOLDEN, "reference_calls.json"), "and reference_calls.npz")


if __name__ == "__main__":
    main()
