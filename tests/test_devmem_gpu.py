"""Ownership of device memory (csrc/gnn_devmem.h): a context that is destroyed gives back what it allocated."""
import ctypes as C

import numpy as np
import pytest

from genomad_amd import _lib, synthetic

pytestmark = pytest.mark.gpu

PARENT_RESIDUE = 14680064     # bytes (14 MiB); measured at the parent commit (see the docstring below)
SLACK = 64 << 20              # what test_kmer_tables_that_do_not_fit_leave_the_default_arithmetic grants the same comparison


def _contigs():
    """packed contigs: short ones, a window that is all N, long ones that take several windows, an empty record"""
    rng = np.random.default_rng(5)
    acgt = lambda k: "".join(rng.choice(list("ACGT"), k))          # noqa: E731
    recs = [acgt(2000), acgt(33000), acgt(6000) + "N" * 6000 + acgt(7000), acgt(100), "", acgt(70000), acgt(2600), acgt(8000) + "N" * 5000]
    seq = np.frombuffer("".join(recs).encode(), dtype=np.uint8).copy()
    return seq, np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)


def _exercise(eng):
    """one call of every entry point that owns device or pinned memory (the k-mer tables apart: their release has a test)"""
    _lib.check(eng.lib.gnn_phase_cycles(eng.ctx, 1, None))                 # left on: gnn_destroy has to free it
    for n in (8, 300, 700):                                                # the stage grows twice
        eng.classify(synthetic.synth_windows(0, n))
    n = 1024
    bases, a, b, emb = eng.alloc(n * 6000 + 8), eng.alloc(n * 12), eng.alloc(n * 12), eng.alloc(n * 512 * 4)
    eng.synth_windows_dev(11, n, bases.ptr)
    eng.classify_dev(bases.ptr, n, a.ptr)
    eng.classify_dev_async(bases.ptr, 512, b.ptr)
    eng.classify_dev_async(bases.ptr + 512 * 6000, 512, b.ptr + 512 * 12)
    eng.flush()
    eng.sync()
    assert np.array_equal(a.download((n, 3), np.float32), b.download((n, 3), np.float32))
    host = bases.download((n * 6000,), np.uint8)
    eng.embed(host.reshape(n, 6000)[:40], with_scores=True)
    eng.embed(host.reshape(n, 6000)[:48], dtype="bf16")                    # NULL scores pointer
    eng.embed_dev(bases.ptr, 64, emb.ptr)                                  # no scores pointer: the ctx's own scratch
    eng.sync()
    bases.upload(np.concatenate([np.zeros(1, np.uint8), host[:300 * 6000]]))
    eng.classify_dev(bases.ptr + 1, 300, b.ptr)                            # a misaligned device buffer
    eng.sync()
    assert np.array_equal(b.download((300, 3), np.float32), a.download((300, 3), np.float32))
    seq, offsets = _contigs()
    s0, _ = eng.classify_contigs(seq, offsets)
    s1, _, _ = eng.embed_contigs(seq, offsets)
    res = eng.scan_contigs(seq, offsets, 2000)
    assert np.array_equal(s0, s1) and res.track.shape[1] == 3
    dseq = eng.alloc(seq.nbytes)
    dseq.upload(seq)
    s2, _ = eng.classify_contigs_spans(dseq.ptr, offsets)
    assert np.array_equal(s0, s2)
    eng.tokenize(host.reshape(n, 6000)[:4])
    out = (C.c_uint64 * 16)()
    _lib.check(eng.lib.gnn_phase_cycles(eng.ctx, 1, out))
    for buf in (bases, a, b, emb, dseq):
        buf.free()


def test_destroying_a_context_gives_its_memory_back(engine, synth_weights):
    """With the session engine open as the observer (mem_info needs a context): free memory before a second engine exists and
    after it has run every memory-owning entry point and was closed.  What stays behind is the runtime's (code objects, its own
    pools), not the context's.  The bound is the parent commit's residue of this same test plus the 64 MB the k-mer table test
    grants the same comparison.  Measured on one MI355X, this test alone in its session: 14 680 064 bytes (14 MiB) at the parent
    commit, 10 485 760 bytes (10 MiB) here; the second engine held 2 720 MiB before it was closed
    (profiles/devmem/README.md)."""
    from genomad_amd.engine import NNEngine
    engine.sync()
    free0 = engine.mem_info()[0]
    with NNEngine(0, synth_weights) as eng:
        _exercise(eng)
        held = free0 - engine.mem_info()[0]
    residue = free0 - engine.mem_info()[0]
    print(f"devmem: the second engine held {held / 2**20:.1f} MiB before it was closed, residue after gnn_destroy {residue} bytes "
          f"({residue / 2**20:.2f} MiB), parent {PARENT_RESIDUE} bytes")
    assert held > (256 << 20)                  # the exercise did allocate: workspaces of 1024 windows alone are 0.9 GB
    assert residue <= PARENT_RESIDUE + SLACK
