"""Graphs whose rows stand exactly on the class borders of the row table (genomad_amd/csrc/gnn_row_table.h), for
tests/test_avglink_gpu.py and tests/test_communities_gpu.py: disjoint stars of weight 0.5, built once and never written to."""
import functools

import numpy as np

from tests.mcl_data import csr_of_edges

# (hub degrees, slots (-1: the library's own 4096), wave_limit = min(the library's 256 wave rows, slots / 4), rows by class): a hub at
# wave_limit, wave_limit + 1, slots and slots + 1 each, the leaves with the waves
BORDERS = (((15, 16, 17, 63, 64, 65), 64, 16, [242, 3, 1]), ((256, 257, 4096, 4097), -1, 256, [8707, 2, 1]))


@functools.lru_cache(maxsize=None)
def stars(degrees):
    """(csr, the nodes' degrees): the hubs first, then their leaves"""
    edges, leaf = [], len(degrees)
    for hub, d in enumerate(degrees):
        edges += [(hub, leaf + x, 0.5) for x in range(d)]
        leaf += d
    return csr_of_edges(leaf, edges), np.array(list(degrees) + [1] * sum(degrees))


def histogram(degree, slots, wave_limit):
    """the rows by class under the rule: wave for a bound u <= wave_limit, workgroup for u <= slots, else dense (u < 1: none)"""
    slots = 4096 if slots < 0 else slots
    return [int(((degree >= 1) & (degree <= wave_limit)).sum()), int(((degree > wave_limit) & (degree <= slots)).sum()),
            int((degree > max(slots, wave_limit)).sum())]
