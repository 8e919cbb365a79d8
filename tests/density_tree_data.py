"""For the density-tree tests: the mutual-reachability values of a given value matrix and core list, the last finite entry of a
neighbour list, what the device tests compare two trees by, a brute-force HDBSCAN by levels that uses no tree and no union-find, and
the plant of the HDBSCAN tests.  Nothing here shares code with sequence.mutual_reachability_tree / hdbscan_clusters."""
import numpy as np

from tests.linkage_data import bits
from tests.neighbours_data import rows


def mutual(values, core):
    """w (n, n) in the dtype of ``values``: min(values[i, j], core[i], core[j]); a NaN value stays NaN (no edge), whatever core is"""
    values = np.asarray(values)
    core = np.asarray(core, values.dtype)
    with np.errstate(invalid="ignore"):
        w = np.fmin(np.fmin(values, core[:, None]), core[None, :])
    w[np.isnan(values)] = np.nan
    return w


def last_finite(sim):
    """per row of a NaN-padded neighbour list (n, k) float32: its last entry that is a number, NaN where there is none"""
    sim = np.asarray(sim, np.float32)
    out = np.full(len(sim), np.nan, np.float32)
    for i, row in enumerate(sim):
        ok = np.flatnonzero(~np.isnan(row))
        if len(ok):
            out[i] = row[ok[-1]]
    return out


def same_tree(got, want):
    """two DensityTreeResults: indices, the bits of sim and core, flags and rounds"""
    return (np.array_equal(got.a, want.a) and np.array_equal(got.b, want.b) and np.array_equal(bits(got.sim), bits(want.sim))
            and np.array_equal(bits(got.core), bits(want.core)) and np.array_equal(got.valid, want.valid) and got.rounds == want.rounds)


def _components(adj, members):
    """the connected components of ``members`` under the adjacency ``adj``, by flooding; each a sorted list"""
    left, out = set(members), []
    while left:
        seed = min(left)
        comp, front = {seed}, [seed]
        while front:
            x = front.pop()
            for y in list(left):
                if y not in comp and adj[x, y]:
                    comp.add(y)
                    front.append(y)
        left -= comp
        out.append(sorted(comp))
    return out


def brute_hdbscan(w, min_cluster_size, allow_single_cluster=False):
    """HDBSCAN by levels from the FULL symmetric value matrix ``w`` (n, n; the diagonal ignored), all rows valid: at every distinct
    value of w (float32), in ascending order, the components of every current cluster under the pairs with a larger value are
    recomputed by flooding.  Returns (label, lambda_out, clusters): clusters is a list of dicts (members, birth, stability, parent,
    children) in order of creation."""
    w = np.asarray(w, np.float32)
    n = len(w)
    lam_of = lambda s: 1.0 / max(1.0 - float(s), 2.0 ** -24)
    levels = np.unique(w[np.triu_indices(n, 1)])
    clusters = [{"members": list(range(n)), "birth": 0.0, "stability": 0.0, "parent": -1, "children": [], "now": list(range(n))}]
    home = [0] * n                                       # the deepest cluster of the row
    lambda_out = [None] * n
    for s in levels:
        adj = w > s
        lam = lam_of(s)
        for c in range(len(clusters)):                   # clusters born at this level are not looked at again at it
            cl = clusters[c]
            if not cl["now"]:
                continue
            comps = _components(adj, cl["now"])
            if len(comps) == 1:                          # nothing falls apart at this level
                continue
            big = [k for k in comps if len(k) >= min_cluster_size]
            for k in comps:
                if len(big) == 1 and k is big[0]:
                    continue
                cl["stability"] += len(k) * (lam - cl["birth"])
                if len(big) >= 2 and len(k) >= min_cluster_size:
                    clusters.append({"members": k, "birth": lam, "stability": 0.0, "parent": c, "children": [], "now": k})
                    cl["children"].append(len(clusters) - 1)
                    for p in k:
                        home[p] = len(clusters) - 1
                else:
                    for p in k:
                        lambda_out[p] = lam
            cl["now"] = big[0] if len(big) == 1 else []

    def best(c):
        """(stability selected in c's subtree, the selected clusters there)"""
        cl = clusters[c]
        below = [best(k) for k in cl["children"]]
        total, chosen = sum(b[0] for b in below), [x for b in below for x in b[1]]
        if (c or allow_single_cluster) and (not cl["children"] or cl["stability"] >= total):
            return cl["stability"], [c]
        return total, chosen
    chosen = best(0)[1] if n else []
    label = np.full(n, -1, np.int64)
    for c in chosen:
        inside, stack = [], [c]
        while stack:
            x = stack.pop()
            inside.append(x)
            stack += clusters[x]["children"]
        for p in range(n):
            if home[p] in inside:
                label[p] = min(clusters[c]["members"])
    return label, np.asarray([np.nan if x is None else x for x in lambda_out], np.float64), clusters


def hdbscan_plant(seed=3):
    """(rows (46, 512) float32, family (46,) int64): three families of 12, 14 and 16 rows (centre + 0.2 * noise: pairwise cosine about
    0.96 inside, about 0.3 across) and four isolated background rows (family -1), scattered by a fixed permutation"""
    sizes = (12, 14, 16)
    pool = rows(3 + sum(sizes) + 4, seed)
    centres, noise, lone = pool[:3], pool[3:3 + sum(sizes)], pool[3 + sum(sizes):]
    out, fam, o = [], [], 0
    for f, m in enumerate(sizes):
        out.append(centres[f] + np.float32(0.2) * noise[o:o + m])
        fam += [f] * m
        o += m
    r = np.concatenate(out + [lone]).astype(np.float32)
    fam = np.asarray(fam + [-1] * 4, np.int64)
    perm = np.random.default_rng(seed + 1).permutation(len(r))
    return np.ascontiguousarray(r[perm]), fam[perm]
