"""The limits round of Markov clustering on the MI355X.  Every comparison is bit for bit, dtypes included (assert_equal of
tests/test_mcl_gpu.py: the five arrays, iterations, converged, changed and the matrix); the fixtures are tests/mcl_limits_data.py's,
and tests/test_mcl_limits_host.py holds them and the definition to the brute force and to Python integers.  By the issue's sections:

0. a cutoff that keeps nothing: ``precision=1`` on the path empties every valid column on the device as in the definition (part of 4).
1. ``NNEngine.mcl_pow`` (``gnn_debug_mcl_pow``: the passes' own ``mc_pow`` / ``mc_isqrt``) equals Python integers with ``math.isqrt`` on
   about 6000 values - the ends, the powers of two, the squares and the k^4 >> 30 where the roots step - at all 28 exponents; its
   range errors.
2. every inflation 1.25 .. 8 through the passes: the 40-node random graph with invalid rows at ``select=8`` and the planted graph at
   ``select=64``, table sizes 4096 and 0, the default grid.
3. the selection's ends: stars whose hub has 1023, 1024, 1025 and 1101 equal entries at ``select=1024`` (the radix select at the sort
   buffer's size, the full buffer, the 1024-key sort; kept == select and select + 1); ``select`` 1 and 2; every knob.
4. the cutoff's ends: ``precision`` 1, 2, 3 and 2^20 on the path, the planted graph and a graph of isolated, invalid and joined rows;
   every knob.
5. the loop entry that alone does not fit: stars of 4095 / 4096 leaves at 4096 slots and 63 / 64 at 64, in the initial pass.
6. rows beyond 2^16: the equal-weight clique at rows 65486 .. 65585 of 65600, the cut at 64 falling across 65536; table sizes 4096 and
   0, the default grid and 3 workgroups; one ``matrix()`` per configuration.
7. weights over the whole admitted range (times 60; q = 1 and q = 2^30 - 64 with the rounding ties, -0.0 and a denormal; all at the
   top) and parallel entries (the ring, spread_data.PARALLEL, a star whose leaves are listed twice: the dense maximum at 64 slots);
   every knob.
8. the same weights for the other consumers: the fixtures ``heavy`` and ``ranged`` of tests/avglink_data.py, tests/communities_data.py
   and tests/spread_data.py, which the sweeps of those suites pick up.
No knob combination was cut."""
import numpy as np
import pytest

from genomad_amd import _lib
from tests import mcl_limits_data as D
from tests.test_mcl_gpu import assert_equal, knobs  # noqa: F401 - knobs is a fixture

pytestmark = pytest.mark.gpu


def run(engine, name, slots, groups):
    """the fixture at one table size and grid, held to the definition: (the result, the overflow counts)"""
    graph, valid, kw, want = D.case(name)
    engine.set_mcl_lds(slots)
    engine.set_mcl_groups(groups)
    res = engine.mcl(*graph, valid, **kw)
    assert_equal(res, want, (name, slots, groups))
    over = engine.mcl_overflow()
    assert len(over) == res.iterations + 1
    if slots == 0:                                      # every valid column took the overflow path in the initial pass
        assert over[0] == (len(graph[0]) - 1 if valid is None else int(valid.sum()))
    return res, over


# ---- 1 -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("a4", D.A4)
def test_the_devices_power_equals_python_integers(engine, a4):
    got = engine.mcl_pow(D.pow_values(), a4 / 4)
    want = D.pow_reference(a4)
    wrong = np.flatnonzero(got != want)
    assert got.dtype == np.uint64 and not len(wrong), (a4, D.pow_values()[wrong[:5]], got[wrong[:5]], want[wrong[:5]])


def test_the_powers_range_errors(engine):
    u, out = np.array([0, 1 << 30], np.uint64), np.full(2, 0x5A, np.uint64)
    fn = engine.lib.gnn_debug_mcl_pow
    assert fn(engine.ctx, u.ctypes.data, 2, 8, out.ctypes.data) == 0 and out.tolist() == [0, 1 << 30]
    assert fn(engine.ctx, None, 0, 8, None) == 0 and len(engine.mcl_pow(np.zeros(0, np.uint64), 2.0)) == 0
    above = np.array([5, (1 << 30) + 1], np.uint64)
    huge = np.array([1 << 63], np.uint64)
    out[:] = 0x5A
    # the library's own range checks come before the ctx is looked at
    for ctx in (engine.ctx, None):
        for args in ((u.ctypes.data, 2, 4, out.ctypes.data), (u.ctypes.data, 2, 33, out.ctypes.data), (u.ctypes.data, -1, 8, out.ctypes.data),
                     (u.ctypes.data, (1 << 24) + 1, 8, out.ctypes.data), (None, 2, 8, out.ctypes.data), (u.ctypes.data, 2, 8, None),
                     (above.ctypes.data, 2, 8, out.ctypes.data), (huge.ctypes.data, 1, 8, out.ctypes.data)):
            assert fn(ctx, *args) == _lib.ERR_ARG, args
            assert b"gnn_debug_mcl_pow" in engine.lib.gnn_last_error()
    assert (out == 0x5A).all()
    assert fn(None, u.ctypes.data, 2, 8, out.ctypes.data) < 0 and (out == 0x5A).all()          # no ctx: an error, nothing written
    for bad in (1.0, 1.3, 8.25):
        with pytest.raises(ValueError, match="inflation"):
            engine.mcl_pow(u, bad)
    with pytest.raises(ValueError):
        engine.mcl_pow(u.reshape(1, 2), 2.0)
    with pytest.raises(_lib.GnnError):
        engine.mcl_pow(above, 2.0)


# ---- 2 -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("a4", D.A4)
def test_every_inflation_through_the_passes(knobs, a4):
    for name in (f"inflation{a4}-random", f"inflation{a4}-planted"):
        for slots in (4096, 0):
            run(knobs, name, slots, 0)


# ---- 3, 4, 7 ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", D.EVERY_KNOB)
def test_every_output_equals_the_definition_on_every_knob(knobs, name):
    assert knobs.set_mcl_lds(-1) == 4096
    for slots, groups in D.KNOBS:
        _, over = run(knobs, name, slots, groups)
        if name == "double-star" and slots == 64:       # the hub's 71 distinct rows do not fit: the maximum is taken in global memory
            assert over[0] == 1
    want = D.case(name)[3]
    print(f"\n{name}: {want['iterations']} iterations, changed {want['changed'].tolist()[:4]}, longest column {want['length'].max()}")


# ---- 5 -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("slots", (4096, 64))
def test_the_loop_is_the_entry_that_does_not_fit(knobs, slots):
    for extra in (0, 1):                                # the neighbours and the loop fill the table; the neighbours alone do
        res, over = run(knobs, f"loop-{slots - 1 + extra}", slots, 0)
        print(f"\n{slots} slots, {slots - 1 + extra} leaves: overflow columns per pass {over.tolist()}")
        assert res.iterations == 1 and over[0] == extra


# ---- 6 -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("beyond-some", "beyond-all"))
def test_a_tie_at_the_cut_between_rows_on_either_side_of_two_to_the_sixteenth(knobs, name):
    for slots, groups in ((4096, 0), (0, 0), (4096, 3), (0, 3)):
        run(knobs, name, slots, groups)
