"""Generate tests/golden/encoder_golden.npz: the encoder embedding of the reference's own graph.

Run where the reference checkout exists (oracle/reference_harness.py finds it):

    python scripts/make_encoder_golden.py [--n 64] [--threads 4]

For synthetic windows 0 .. n-1 (seed 1234, the windows of BASELINE config 2) and the seed-42 synthetic weights it
stores

* ``emb_refgraph32`` (n, 512) f32 - outputs of the REFERENCE'S OWN ``create_encoder()`` (genomad/neural_network/
  model.py:14-31: one-hot -> IGLOO block -> Dense512 -> BatchNorm -> ReLU) executed in place in float32 over the numpy
  stand-ins of oracle/keras_shim.py;
* ``emb_refgraph64`` (n, 512) f64 - the same graph evaluated in float64.

``keras_shim.schema_provider`` hands out weights by per-class layer ordinal; a stand-alone encoder instantiates
Dense #0 and BatchNormalization #0 only, which are ``enc_dense`` and ``enc_bn`` of the classifier, so it gets the
encoder's weights.  The network package's ``__init__`` exports only ``create_classifier``, hence the import of
``genomad.neural_network.model``.
"""
import argparse
import hashlib
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def reference_encoder(tokens, weights, dtype):
    """(n, 512) output of the reference's create_encoder() for (n, 5997) tokens."""
    import numpy as np
    from oracle import keras_shim, reference_harness
    reference_harness.load_reference_network()
    model = importlib.import_module("genomad.neural_network.model")
    keras_shim.new_session(keras_shim.schema_provider(weights), dtype)
    enc = model.create_encoder()
    return np.asarray(enc.predict(np.asarray(tokens, dtype=np.int64), verbose=0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--threads", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "encoder_golden.npz"))
    args = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", str(args.threads))
    import numpy as np
    from genomad_amd import synthetic
    from oracle import sequence_oracle

    weights = synthetic.synth_weights()
    bases = synthetic.synth_windows(0, args.n)
    tokens = sequence_oracle.tokenize_closed_form(bases)
    e32, e64 = [], []
    for a in range(0, args.n, args.chunk):
        t = tokens[a:a + args.chunk]
        e32.append(reference_encoder(t, weights, np.float32).astype(np.float32))
        e64.append(reference_encoder(t, weights, np.float64).astype(np.float64))
        print(f"{a + len(t)} / {args.n} windows", flush=True)
    wsha = hashlib.sha256(b"".join(np.ascontiguousarray(weights[k]).tobytes() for k in sorted(weights))).hexdigest()
    np.savez_compressed(args.out, emb_refgraph32=np.concatenate(e32), emb_refgraph64=np.concatenate(e64),
                        n=np.int64(args.n), data_seed=np.int64(1234), weights_sha256=np.array(wsha))
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
