"""NNEngine — thin host wrapper over the C ABI: one engine = one gnn_ctx = one GPU.

Mirrors what the reference does with a Keras model inside
genomad/modules/nn_classification.py:309-320: build, load weights, predict batches,
segment-mean per contig.  All arithmetic happens in libgenomad_nn_hip.so.
"""
import ctypes as C

import numpy as np

from . import _lib, sequence as _sequence, weights as _weights
from ._lib import GnnError, check  # noqa: F401  (re-export)


class DeviceBuffer:
    """A raw device allocation owned by an engine (no torch needed for buffers)."""

    def __init__(self, engine, nbytes: int):
        self.engine, self.nbytes = engine, int(nbytes)
        p = C.c_void_p()
        check(engine.lib.gnn_dev_alloc(engine.ctx, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def upload(self, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        check(self.engine.lib.gnn_memcpy_h2d(self.engine.ctx, self.ptr, arr.ctypes.data, arr.nbytes))

    def download(self, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        check(self.engine.lib.gnn_memcpy_d2h(self.engine.ctx, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            check(self.engine.lib.gnn_dev_free(self.engine.ctx, self.ptr))
            self.ptr = None


class _Result:
    """The base of what the engine's calls return: one attribute per name of ``FIELDS`` (None for one that is not given)."""
    FIELDS = ()

    def __init__(self, **kw):
        for k in self.FIELDS:
            setattr(self, k, kw.get(k))

    def asdict(self) -> dict:
        return {k: getattr(self, k) for k in self.FIELDS}


class ScanResult(_Result):
    """What :meth:`NNEngine.scan_contigs` returns.  Windows (CSR over contigs by ``win_offsets``): ``starts`` (contig-relative),
    ``lens``, ``kept`` (bool: the N rule's mask), ``scores`` (n_windows, 3).  Bins (CSR by ``bin_offsets``, ``stride`` bases each):
    ``track`` (n_bins, 3; NaN where ``cover`` == 0), ``cover`` (kept windows averaged into the bin).  ``contig_scores``
    (n_contigs, 3): the mean of each contig's kept windows."""
    FIELDS = ("stride", "win_offsets", "starts", "lens", "kept", "scores", "bin_offsets", "track", "cover", "contig_scores")


class StrandScanResult(ScanResult):
    """What :meth:`NNEngine.scan_contigs_strand` returns: the fields of :class:`ScanResult` for the strand mode ``strand``
    ("forward", "reverse" or "both": ``scores``, ``track`` and ``contig_scores`` carry it; the window tables, ``kept`` and ``cover``
    do not depend on it) plus ``scores_fwd`` and ``scores_rev`` (n_windows, 3): each strand's own window scores."""
    FIELDS = ScanResult.FIELDS + ("strand", "scores_fwd", "scores_rev")


class OcclusionResult(_Result):
    """What :meth:`NNEngine.occlude_contigs` returns.  Windows (CSR over contigs by ``win_offsets``): ``starts`` (contig-relative),
    ``lens``, ``kept`` (bool: the N rule's mask), ``scores`` (n_windows, 3: the windows' ordinary scores).  Pairs (CSR over windows
    by ``blk_offsets``, ``block`` bases each - ``sequence.occlusion_blocks``): ``delta`` (n_pairs, 3) = scores[window] - the score
    of the window with that block set to N; positive where the block supports the class.  ``contig_scores`` (n_contigs, 3): the
    mean of each contig's kept windows."""
    FIELDS = ("block", "win_offsets", "starts", "lens", "kept", "scores", "blk_offsets", "delta", "contig_scores")


class AttributionResult(_Result):
    """What :meth:`NNEngine.attribute_contigs` returns.  Windows (CSR over contigs by ``win_offsets``): ``starts`` (contig-relative),
    ``lens``, ``kept`` (bool: the N rule's mask), ``window_scores`` (n_windows, 3).  Maps: ``contrib`` (n_windows, 2, nb, 3) - head A,
    B; bins of ``bin`` pooled positions (a position = 8 tokens; nb = ceil(749 / bin)); class - each bin's signed share of the
    window's pre-softmax ``logits`` (n_windows, 3), and ``bias`` (n_windows, 3), the remainder: contrib.sum((1, 2)) + bias = logits.
    ``contig_scores`` (n_contigs, 3): the mean of each contig's kept windows."""
    FIELDS = ("bin", "win_offsets", "starts", "lens", "kept", "window_scores", "contrib", "bias", "logits", "contig_scores")


class RegionResult(_Result):
    """What :meth:`NNEngine.call_regions` returns (the definition is ``sequence.call_regions``).  ``penalty``; bins (CSR over contigs
    by ``bin_offsets``): ``state`` (n_bins,) uint8, the path's class per bin.  Regions, ordered by contig, then position:
    ``region_contig``, ``region_lo``, ``region_hi`` (int64; contig-relative bins, half-open), ``region_state`` (uint8),
    ``region_evidence`` (int64) and ``region_qsum`` (n_regions, 3) int64.  With ``offsets`` and ``stride`` given also the derived
    table of ``sequence.region_table``: ``stride``, ``start``, ``end`` (bases), ``mean`` (n_regions, 3), ``margin``; None otherwise."""
    FIELDS = ("penalty", "bin_offsets", "state", "region_contig", "region_lo", "region_hi", "region_state", "region_evidence",
              "region_qsum", "stride", "start", "end", "mean", "margin")

    @property
    def regions(self) -> dict:
        """the six region arrays under the names of ``sequence.call_regions``"""
        return {k: getattr(self, "region_" + k) for k in ("contig", "lo", "hi", "state", "evidence", "qsum")}

    @classmethod
    def build(cls, penalty, bin_offsets, state, regions, offsets=None, stride=None):
        """from the output of ``sequence.call_regions`` or the library; the table where ``offsets`` and ``stride`` are given"""
        table = _sequence.region_table(regions, offsets, stride) if offsets is not None and stride is not None else {}
        return cls(penalty=float(penalty), bin_offsets=bin_offsets, state=state, **{"region_" + k: v for k, v in regions.items()},
                   stride=None if stride is None else int(stride), **table)


class IntervalResult(_Result):
    """What :meth:`NNEngine.embed_intervals` returns (the definition is ``sequence.interval_embeddings``).  ``stride`` and ``strand``
    of the pass; per interval ``contig``, ``start``, ``end`` (int64; 0-based half-open bases within the contig), its member windows
    [``w_lo``, ``w_hi``) in the window order of a scan at ``stride``, ``count`` (int32: the kept members), ``embedding``
    (n_intervals, 512) float32 - their mean encoder embedding, a zero row where count == 0: ordinary rows for
    :meth:`NNEngine.neighbours`, :meth:`NNEngine.cluster` and :meth:`NNEngine.representatives` -, ``coherence`` (float32 in [0, 1]:
    the mean resultant length of the members' unit rows; low where the mean averages unlike windows) and ``scores``
    (n_intervals, 3): the mean of the members' window scores."""
    FIELDS = ("stride", "strand", "contig", "start", "end", "w_lo", "w_hi", "count", "embedding", "coherence", "scores")


class ClusterResult(_Result):
    """What :meth:`NNEngine.cluster` returns (the definition is ``sequence.threshold_clusters``): ``label``, ``degree``, ``size``,
    ``rep`` (int64 (n,); -1 / 0 / 0 / -1 for an invalid row), the ``threshold`` as the float32 it was compared as, and ``metric``."""
    FIELDS = ("label", "degree", "size", "rep", "threshold", "metric")

    @property
    def n_clusters(self) -> int:
        """clusters, singletons included: the rows that are their own label"""
        return int((self.label == np.arange(len(self.label))).sum())

    @property
    def n_edges(self) -> int:
        return int(self.degree.sum()) // 2

    def table(self, names=None):
        """``sequence.cluster_table``: one record per cluster, ordered by label"""
        return _sequence.cluster_table(self, names)

    @classmethod
    def build(cls, arrays, threshold, metric):
        """from the four arrays of ``sequence.threshold_clusters`` or the library"""
        label, degree, size, rep = arrays
        return cls(label=label, degree=degree, size=size, rep=rep, threshold=float(_sequence.cluster_threshold(threshold)), metric=str(metric))


class DensityResult(_Result):
    """What :meth:`NNEngine.density` returns (the definition is ``sequence.density_clusters``): ``label``, ``degree``, ``size``,
    ``anchor`` (int64 (n,)), ``sim`` (float32 from the device; a border row's similarity to its anchor, NaN otherwise), ``kind``
    (uint8: 0 invalid, 1 noise, 2 border, 3 core), the ``threshold`` as the float32 it was compared as, ``min_points`` and
    ``metric``."""
    FIELDS = ("label", "degree", "size", "anchor", "sim", "kind", "threshold", "min_points", "metric")

    @property
    def n_clusters(self) -> int:
        """clusters: the core rows that are their own label"""
        return int((self.label == np.arange(len(self.label))).sum())

    @property
    def n_core(self) -> int:
        return int((self.kind == 3).sum())

    @property
    def n_border(self) -> int:
        return int((self.kind == 2).sum())

    @property
    def n_noise(self) -> int:
        return int((self.kind == 1).sum())

    def table(self, names=None):
        """``sequence.density_table``: one record per cluster, ordered by label"""
        return _sequence.density_table(self, names)

    @classmethod
    def build(cls, arrays, threshold, min_points, metric):
        """from the six arrays of ``sequence.density_clusters`` or the library"""
        label, degree, size, anchor, sim, kind = arrays
        return cls(label=label, degree=degree, size=size, anchor=anchor, sim=sim, kind=kind,
                   threshold=float(_sequence.cluster_threshold(threshold)), min_points=int(min_points), metric=str(metric))


class KMeansResult(_Result):
    """What :meth:`NNEngine.kmeans` returns (the definition is ``sequence.spherical_kmeans``): ``label`` (int64 (n,); -1 for an
    invalid row), ``sim`` (float32 (n,): the similarity to the row's own centroid, NaN for an invalid row), ``centroids`` (float32
    (k, 512), unit rows), ``size`` (int64 (k,)), ``iterations``, ``converged`` and ``init_rows`` (int64 (k,): the rows the
    farthest-first traversal picked, -1 for a given init)."""
    FIELDS = ("label", "sim", "centroids", "size", "iterations", "converged", "init_rows")

    @property
    def k(self) -> int:
        return len(self.size)

    @property
    def objective(self) -> float:
        """the sum of ``sim`` over the valid rows, in float64"""
        return float(np.asarray(self.sim, dtype=np.float64)[np.asarray(self.label) >= 0].sum())

    def table(self, names=None):
        """``sequence.kmeans_table``: one record per cluster, by cluster index"""
        return _sequence.kmeans_table(self, names)

    @classmethod
    def build(cls, arrays):
        """from the seven values of ``sequence.spherical_kmeans`` or the library"""
        label, sim, centroids, size, iterations, converged, init_rows = arrays
        return cls(label=label, sim=sim, centroids=centroids, size=size, iterations=int(iterations), converged=bool(converged),
                   init_rows=init_rows)


class PCAResult(_Result):
    """What :meth:`NNEngine.pca` returns: ``mean`` (float64 (512,): the mean of the valid rows' unit vectors; zeros for
    ``center=False``), ``components`` (float32 (c, 512), unit rows, by eigenvalue descending, the entry of largest magnitude
    positive), ``explained_variance`` / ``explained_variance_ratio`` (float64 (c,)), ``total_variance``, ``n_valid``, ``valid``
    (bool (n,)) and ``projection`` (float32 (n, c): the rows' scores, NaN for an invalid row)."""
    FIELDS = ("mean", "components", "explained_variance", "explained_variance_ratio", "total_variance", "n_valid", "valid", "projection")

    def __init__(self, engine=None, **kw):
        super().__init__(**kw)
        self._engine = engine

    @property
    def n_components(self) -> int:
        return len(self.components)

    def transform(self, rows) -> np.ndarray:
        """new rows onto the same axes (float32 (m, c)): :meth:`NNEngine.project` with this result's components and mean"""
        if self._engine is None:
            raise ValueError("this PCAResult has no engine: call NNEngine.project(rows, result.components, result.mean)")
        return self._engine.project(rows, self.components, self.mean)

    def table(self, names=None):
        """``sequence.pca_table``: one record per row"""
        return _sequence.pca_table(self.projection, self.valid, names)


class RepresentativeResult(_Result):
    """What :meth:`NNEngine.representatives` returns (the definition is ``sequence.greedy_representatives``), in the caller's index
    space: ``rep`` (int64; a representative names itself, -1 for an invalid row), ``sim`` (float32; a member's similarity to its
    representative, NaN otherwise), ``size`` (int64; 0 for an invalid row), ``rank`` (int64; the row's place in the priority order),
    ``rounds`` (the synchronous rounds the device ran: a property of the graph and the order), the ``threshold`` as the float32 it
    was compared as, and ``metric``."""
    FIELDS = ("rep", "sim", "size", "rank", "rounds", "threshold", "metric")

    @property
    def is_rep(self) -> np.ndarray:
        return self.rep == np.arange(len(self.rep))

    @property
    def n_clusters(self) -> int:
        return int(self.is_rep.sum())

    def table(self, names=None):
        """``sequence.representative_table``: one record per cluster, ordered by the representative's rank"""
        return _sequence.representative_table(self, names)

    @classmethod
    def build(cls, arrays, threshold, metric):
        """from the (rep, sim, size, rank, rounds) of ``sequence.greedy_representatives`` or the library"""
        rep, sim, size, rank, rounds = arrays
        return cls(rep=rep, sim=sim, size=size, rank=rank, rounds=int(rounds), threshold=float(_sequence.cluster_threshold(threshold)),
                   metric=str(metric))


class LinkageResult(_Result):
    """What :meth:`NNEngine.linkage` returns (the definition is ``sequence.single_linkage_tree``): the single-linkage tree's edges,
    best first - ``a`` (int64, the smaller row), ``b`` (int64, the larger), ``sim`` (float32), trimmed to ``n_edges`` -, ``valid``
    (uint8 (n,)), ``n``, ``n_valid``, ``rounds`` (the Boruvka rounds of the device that added an edge) and ``metric``."""
    FIELDS = ("a", "b", "sim", "valid", "n", "n_valid", "rounds", "metric")

    @property
    def n_edges(self) -> int:
        return len(self.a)

    def cut(self, threshold) -> np.ndarray:
        """``sequence.linkage_cut``: the ``label`` of :meth:`NNEngine.cluster` at ``threshold``"""
        return _sequence.linkage_cut(self.a, self.b, self.sim, self.valid, threshold)

    def cluster_counts(self, thresholds) -> np.ndarray:
        """``sequence.linkage_cluster_counts``: the clusters a cut leaves at each threshold"""
        return _sequence.linkage_cluster_counts(self.sim, self.n_valid, thresholds)

    def matrix(self) -> np.ndarray:
        """``sequence.linkage_matrix``: SciPy's convention, distance = 1 - sim; cosine, all rows valid and a spanning tree only"""
        if self.metric != "cosine":
            raise ValueError(f"metric {self.metric!r}: 1 - sim is a distance under cosine only")
        if self.n_valid != self.n:
            raise ValueError(f"{self.n - self.n_valid} of {self.n} rows are invalid: a linkage matrix needs every row")
        return _sequence.linkage_matrix(self.a, self.b, self.sim, self.n)

    def table(self, names=None):
        """``sequence.linkage_table``: one record per merge - rank, a, b, sim, clusters left"""
        return _sequence.linkage_table(self.a, self.b, self.sim, self.n_valid, names)

    @classmethod
    def build(cls, arrays, metric, rounds=0):
        """from the (a, b, sim, valid) of ``sequence.single_linkage_tree`` or the library, already trimmed"""
        a, b, sim, valid = arrays
        return cls(a=a, b=b, sim=sim, valid=valid, n=len(valid), n_valid=int(np.count_nonzero(valid)), rounds=int(rounds), metric=str(metric))


class DensityTreeResult(_Result):
    """What :meth:`NNEngine.density_tree` returns (the definition is ``sequence.mutual_reachability_tree``): the tree's edges, best
    first - ``a`` (int64, the smaller row), ``b`` (int64, the larger), ``sim`` (float32, the mutual-reachability value), trimmed to
    ``n_edges`` -, ``core`` (float32 (n,): the row's core similarity, NaN for an invalid row), ``valid`` (uint8 (n,)), ``n``,
    ``n_valid``, ``rounds``, ``min_points`` and ``metric``."""
    FIELDS = ("a", "b", "sim", "core", "valid", "n", "n_valid", "rounds", "min_points", "metric")

    @property
    def n_edges(self) -> int:
        return len(self.a)

    def cut(self, threshold) -> np.ndarray:
        """``sequence.density_tree_cut``: the ``label`` of :meth:`NNEngine.density` at (``threshold``, ``min_points``) at its core
        rows, -1 at every other row"""
        return _sequence.density_tree_cut(self.a, self.b, self.sim, self.core, self.valid, threshold)

    def cluster_counts(self, thresholds) -> np.ndarray:
        """``sequence.density_tree_cluster_counts``: the clusters of core rows a cut leaves at each threshold"""
        return _sequence.density_tree_cluster_counts(self.sim, self.core, self.valid, thresholds)

    def hdbscan(self, min_cluster_size=5, allow_single_cluster=False) -> dict:
        """``sequence.hdbscan_clusters`` of this tree: ``label``, ``lambda_out`` and the cluster table.  Cosine only (1 - sim is a
        distance); a forest - which only ``dot`` can give - is a ValueError there."""
        if self.metric != "cosine":
            raise ValueError(f"metric {self.metric!r}: 1 - sim is a distance under cosine only")
        return _sequence.hdbscan_clusters(self.a, self.b, self.sim, self.valid, min_cluster_size, allow_single_cluster)

    def matrix(self) -> np.ndarray:
        """``sequence.linkage_matrix`` of the mutual-reachability values: SciPy's convention, distance = 1 - sim; cosine, all rows
        valid and a spanning tree only"""
        if self.metric != "cosine":
            raise ValueError(f"metric {self.metric!r}: 1 - sim is a distance under cosine only")
        if self.n_valid != self.n:
            raise ValueError(f"{self.n - self.n_valid} of {self.n} rows are invalid: a linkage matrix needs every row")
        return _sequence.linkage_matrix(self.a, self.b, self.sim, self.n)

    def table(self, names=None):
        """``sequence.linkage_table``: one record per merge - rank, a, b, sim, clusters left"""
        return _sequence.linkage_table(self.a, self.b, self.sim, self.n_valid, names)

    @classmethod
    def build(cls, arrays, min_points, metric, rounds=0):
        """from the (a, b, sim, core, valid) of ``sequence.mutual_reachability_tree`` or the library, already trimmed"""
        a, b, sim, core, valid = arrays
        return cls(a=a, b=b, sim=sim, core=core, valid=valid, n=len(valid), n_valid=int(np.count_nonzero(valid)), rounds=int(rounds),
                   min_points=int(min_points), metric=str(metric))


class GraphResult(_Result):
    """What :meth:`NNEngine.graph` returns (the definition is ``sequence.threshold_graph``): the similarity graph's upper triangle in
    CSR form - ``indptr`` (int64 (n + 1,)), ``col`` (int32: row i owns ``col[indptr[i]:indptr[i + 1]]``, its partners j > i in
    ascending order) and ``sim`` (float32, the device's own values) -, ``valid`` (bool (n,): the rows that took part; it cannot be
    read off the graph), ``n``, ``n_edges``, the ``threshold`` as the float32 it was compared as, and ``metric``."""
    FIELDS = ("indptr", "col", "sim", "valid", "n", "n_edges", "threshold", "metric")

    def edges(self):
        """COO: (a int64, b int64, sim) with a < b, in the CSR's order"""
        a, b = _sequence.graph_edges(self.indptr, self.col)
        return a, b, self.sim

    def degree(self) -> np.ndarray:
        """int64 (n,), both ends counted: what :meth:`NNEngine.cluster` returns as ``degree``"""
        return _sequence.graph_degree(self.indptr, self.col)

    def symmetric(self):
        """the full CSR (indptr int64, col int32, sim): every edge at both its rows, a row's partners ascending"""
        return _sequence.graph_symmetric(self.indptr, self.col, self.sim)

    def components(self) -> np.ndarray:
        """int64 (n,): what :meth:`NNEngine.cluster` returns as ``label`` - the smallest index of the row's component, -1 for an
        invalid row - by a union-find on the host"""
        return _sequence.graph_components(self.indptr, self.col, self.valid)

    def table(self, names=None):
        """``sequence.graph_table``: one record per edge - a, b, sim"""
        return _sequence.graph_table(self.indptr, self.col, self.sim, names)

    def mcl(self, engine, **kw) -> "MCLResult":
        """:meth:`NNEngine.mcl` of this graph and its rows' validity: Markov clusters, with ``inflation``, ``select``, ``precision``
        and ``max_iter`` as there"""
        return engine.mcl(self.indptr, self.col, self.sim, self.valid, **kw)

    def spread(self, engine, label, n_classes, **kw) -> "SpreadResult":
        """:meth:`NNEngine.spread` of this graph and its rows' validity: the labels of the seed rows spread along its edges, with
        ``alpha``, ``clamp``, ``max_iter`` and ``scores`` as there"""
        return engine.spread(self.indptr, self.col, self.sim, label, n_classes, valid=self.valid, **kw)

    def average_linkage(self, engine, **kw) -> "AverageLinkageResult":
        """:meth:`NNEngine.average_linkage` of this graph and its rows' validity: the UPGMA tree, with ``stop`` and ``max_rounds``
        as there"""
        return engine.average_linkage(self.indptr, self.col, self.sim, valid=self.valid, **kw)

    def communities(self, engine, **kw) -> "CommunityResult":
        """:meth:`NNEngine.communities` of this graph and its rows' validity: modularity communities, with ``resolution``,
        ``max_levels`` and ``max_sweeps`` as there"""
        return engine.communities(self.indptr, self.col, self.sim, valid=self.valid, **kw)

    def label_components(self, engine, label) -> np.ndarray:
        """:meth:`NNEngine.label_components` of this graph and its rows' validity: the connected parts of every label's rows"""
        return engine.label_components(self.indptr, self.col, self.sim, label, valid=self.valid)

    def tsne(self, engine, init=None, **kw) -> "TSNEResult":
        """:meth:`NNEngine.tsne` of this graph and its rows' validity: the exact t-SNE layout, with ``n_iter``, ``exaggeration_iter``,
        ``exaggeration`` and ``learning_rate`` as there; ``init`` None: ``sequence.tsne_init``"""
        return engine.tsne(self.indptr, self.col, self.sim, _sequence.tsne_init(self.n) if init is None else init, valid=self.valid, **kw)

    @classmethod
    def build(cls, arrays, valid, threshold, metric):
        """from the (indptr, col, sim) of ``sequence.threshold_graph`` or the library, and the rows' validity"""
        indptr, col, sim = arrays
        return cls(indptr=indptr, col=col, sim=sim, valid=np.asarray(valid, dtype=bool), n=len(indptr) - 1, n_edges=len(col),
                   threshold=float(_sequence.cluster_threshold(threshold)), metric=str(metric))

    def extend(self, cross: "MatchResult", new: "GraphResult") -> "GraphResult":
        """The graph of the concatenated rows [this graph's rows; ``new``'s rows] (``sequence.graph_extend``), where ``cross`` =
        ``match(query=these rows, base=new's rows)`` at the same threshold and metric: a pair's value depends on its two rows only,
        so the result equals ``graph(concatenation)`` bit for bit and the old x old products are not computed again.  Its
        :meth:`components` is the assignment of the new rows to the old clusters.  ``ValueError`` when sizes, threshold bits or
        metric disagree."""
        if cross.n_query != self.n or cross.n_base != new.n:
            raise ValueError(f"the cross matches are {cross.n_query} x {cross.n_base}, the graphs have {self.n} and {new.n} rows: "
                             "match(query=the old rows, base=the new rows) is required")
        bits = [np.float32(x.threshold).view(np.uint32) for x in (self, cross, new)]
        if bits[0] != bits[1] or bits[0] != bits[2]:
            raise ValueError(f"the thresholds {self.threshold!r}, {cross.threshold!r} and {new.threshold!r} differ")
        if not self.metric == cross.metric == new.metric:
            raise ValueError(f"the metrics {self.metric!r}, {cross.metric!r} and {new.metric!r} differ")
        arrays = _sequence.graph_extend(*((x.indptr, x.col, x.sim) for x in (self, cross, new)))
        return GraphResult.build(arrays, np.concatenate([self.valid, new.valid]), self.threshold, self.metric)


class KNNGraphResult(GraphResult):
    """What :meth:`NNEngine.knn_graph` returns (the definition is ``sequence.knn_graph``): a :class:`GraphResult` - the same CSR over
    the upper triangle, so everything said there holds, the four consumers included - whose edges join rows that list each other
    among their ``k`` nearest neighbours: ``mode`` ("union": either lists the other; "mutual": both), ``weight`` ("similarity": ``sim``
    is the similarity the lists carry; "jaccard": the overlap of the two neighbourhoods) and ``mutual`` (uint8 per edge: both ends
    list each other).  ``threshold`` is NaN: there is none."""
    FIELDS = GraphResult.FIELDS + ("k", "mode", "weight", "mutual")

    def table(self, names=None):
        """``sequence.knn_graph_table``: one record per edge - a, b, weight, mutual"""
        return _sequence.knn_graph_table(self.indptr, self.col, self.sim, self.mutual, names)

    @classmethod
    def build(cls, arrays, valid, k, mode, weight, metric):
        """from the (indptr, col, sim, mutual) of ``sequence.knn_graph`` or the library, and the rows' validity"""
        indptr, col, sim, mutual = arrays
        return cls(indptr=indptr, col=col, sim=sim, valid=np.asarray(valid, dtype=bool), n=len(indptr) - 1, n_edges=len(col),
                   threshold=float("nan"), metric=str(metric), k=int(k), mode=str(mode), weight=str(weight), mutual=mutual)


class MatchResult(_Result):
    """What :meth:`NNEngine.match` returns (the definition is ``sequence.threshold_matches``): the bipartite similarity graph query x
    base in CSR form by query row - ``indptr`` (int64 (n_query + 1,)), ``col`` (int32: query i owns ``col[indptr[i]:indptr[i + 1]]``,
    its base partners in ascending order) and ``sim`` (float32, the device's own values: what :meth:`NNEngine.neighbours` returns for
    query i and base row j) -, ``query_valid`` and ``base_valid`` (bool: the rows that took part), ``n_query``, ``n_base``,
    ``n_edges``, the ``threshold`` as the float32 it was compared as, and ``metric``."""
    FIELDS = ("indptr", "col", "sim", "query_valid", "base_valid", "n_query", "n_base", "n_edges", "threshold", "metric")

    def edges(self):
        """COO: (query int64, base int64, sim), in the CSR's order"""
        a, b = _sequence.graph_edges(self.indptr, self.col)
        return a, b, self.sim

    def hits(self) -> np.ndarray:
        """int64 (n_query,): the partners of every query"""
        return np.diff(self.indptr).astype(np.int64)

    def base_hits(self) -> np.ndarray:
        """int64 (n_base,): the queries that matched every base row"""
        return np.bincount(np.asarray(self.col, dtype=np.int64), minlength=self.n_base).astype(np.int64)

    def best(self):
        """``sequence.match_best``: (idx int64 (n_query,), sim (n_query,)) - per query the partner with the largest ``sim``, ties to
        the smaller index, -1 / NaN where there is none.  It is ``neighbours(query, base, 1)`` wherever that similarity is >= the
        threshold."""
        return _sequence.match_best(self.indptr, self.col, self.sim)

    def transpose(self):
        """``sequence.match_transpose``: the CSR by base row (indptr int64 (n_base + 1,), col int32: the queries, ascending; sim) -
        on the host; a pair's value keeps its orientation (query i, base row j)"""
        return _sequence.match_transpose(self.indptr, self.col, self.sim, self.n_base)

    def table(self, query_names=None, base_names=None):
        """``sequence.match_table``: one record per match - query, base, sim"""
        return _sequence.match_table(self.indptr, self.col, self.sim, query_names, base_names)

    @classmethod
    def build(cls, arrays, query_valid, base_valid, threshold, metric):
        """from the (indptr, col, sim) of ``sequence.threshold_matches`` or the library, and the validity of both sides"""
        indptr, col, sim = arrays
        query_valid, base_valid = np.asarray(query_valid, dtype=bool), np.asarray(base_valid, dtype=bool)
        if len(query_valid) != len(indptr) - 1:
            raise ValueError(f"query_valid has {len(query_valid)} flags, indptr {len(indptr) - 1} rows")
        return cls(indptr=indptr, col=col, sim=sim, query_valid=query_valid, base_valid=base_valid, n_query=len(indptr) - 1,
                   n_base=len(base_valid), n_edges=len(col), threshold=float(_sequence.cluster_threshold(threshold)), metric=str(metric))


class MCLResult(_Result):
    """What :meth:`NNEngine.mcl` returns (the definition is ``sequence.markov_clusters``), per row: ``label`` (int64: the smallest
    index of the row's cluster; -1 for an invalid row), ``size`` (int64: rows of its cluster), ``attractor`` (int64: the row most of
    its flow ends at; -1), ``flow`` (uint32: that share, in units of 2^-30) and ``is_attractor`` (bool: the row keeps flow to itself);
    ``iterations``, ``converged``, ``changed`` (int64: the columns every iteration changed), ``n`` and the ``inflation``, ``select``,
    ``precision`` it ran with.  :meth:`NNEngine.mcl_dev` leaves the per-row arrays on the device: they are None here."""
    FIELDS = _sequence.MCL_FIELDS + ("iterations", "converged", "changed", "n", "inflation", "select", "precision")

    def __init__(self, engine=None, serial=0, **kw):
        super().__init__(**kw)
        self._engine, self._serial, self._matrix = engine, serial, None

    @property
    def n_clusters(self) -> int:
        return int(np.count_nonzero(self.label == np.arange(self.n)))

    def matrix(self):
        """The final matrix (``gnn_mcl_matrix``) as ``sequence.markov_clusters`` returns it: (length int64 (n,), idx int32, val
        uint32) - column j owns the next ``length[j]`` entries, rows ascending.  It is read from the engine on the first call, which
        must come before the engine's next Markov clustering (``GnnError`` otherwise)."""
        if self._matrix is None:
            self._matrix = self._engine._mcl_matrix(self.n, self.select, self._serial)
        return self._matrix

    def table(self, names=None):
        """``sequence.mcl_table``: one record per cluster - label, size, members, attractors"""
        return _sequence.mcl_table(self.label, self.size, self.is_attractor, names)


class SpreadResult(_Result):
    """What :meth:`NNEngine.spread` returns (the definition is ``sequence.label_spread``), per row: ``score`` (uint32 (n, n_classes),
    units of 2^-30; None where it was not asked for), ``best`` (int32: the class of the largest score, ties to the smaller class; -1
    where every score is 0), ``best_score``, ``second_score`` (uint32), ``total`` (uint64) and ``first`` (int32: the first iteration
    behind which the row's total was not 0; -1); ``seed`` (bool: the valid rows that carried a label); ``iterations``, ``converged``,
    ``changed`` (int64: the rows every iteration changed), ``n``, ``n_classes`` and the ``alpha`` and ``clamp`` it ran with.
    :meth:`NNEngine.spread_dev` leaves the per-row arrays on the device: they are None here."""
    FIELDS = _sequence.SPREAD_FIELDS + ("seed", "iterations", "converged", "changed", "n", "n_classes", "alpha", "clamp")

    def predict(self, min_score=0.0):
        """``sequence.spread_predict``: (label int64, confidence = best_score / total, margin = (best_score - second_score) / total)
        per row; -1 / NaN where no class reached the row or its best score is below ``min_score``.  No calibrated probability."""
        return _sequence.spread_predict(self.best, self.best_score, self.second_score, self.total, min_score)

    def table(self, names=None, class_names=None, min_score=0.0):
        """``sequence.spread_table``: one record per row - label, confidence, score, total_score, first"""
        return _sequence.spread_table(self.best, self.best_score, self.second_score, self.total, self.first, names, class_names, min_score)


class AverageLinkageResult(_Result):
    """What :meth:`NNEngine.average_linkage` returns (the definition is ``sequence.average_linkage``), per merge, best first -
    the average descending as an exact rational, then the round, then ``a``; children before parents: ``a`` < ``b`` (int64: the
    absorbing and the absorbed cluster, each named by its smallest member), ``weight`` (uint64: S, the sum of the integer weights
    between them), ``size_a``, ``size_b``, ``round`` (int64) and ``sim`` (float64: S / (size_a * size_b) / 2^24); ``valid`` (bool
    per row), ``rounds``, ``merged_per_round`` (int64), ``complete`` (the rounds ended because one merged nothing), ``n`` and the
    ``stop`` it ran with.  :meth:`NNEngine.average_linkage_dev` leaves the per-node records on the device: the per-merge arrays and
    ``valid`` are None here."""
    FIELDS = _sequence.AVGLINK_FIELDS + ("sim", "valid", "rounds", "merged_per_round", "complete", "n", "stop")

    def _arrays(self):
        return {k: getattr(self, k) for k in _sequence.AVGLINK_FIELDS + ("sim", "valid")}

    def cut(self, t) -> np.ndarray:
        """``sequence.average_linkage_cut``: int64 label per row at the similarity ``t`` - the smallest member, -1 for an invalid row"""
        return _sequence.average_linkage_cut(self._arrays(), t)

    def cluster_counts(self, thresholds) -> np.ndarray:
        """``sequence.average_linkage_cluster_counts``: the clusters a cut leaves at each threshold"""
        return _sequence.average_linkage_cluster_counts(self._arrays(), thresholds)

    def matrix(self) -> np.ndarray:
        """``sequence.average_linkage_matrix``: SciPy's convention, distance = 1 - sim; all rows valid and a whole tree only"""
        return _sequence.average_linkage_matrix(self._arrays())

    def table(self, names=None):
        """``sequence.average_linkage_table``: one record per merge - rank, a, b, sim, size, round, clusters left"""
        return _sequence.average_linkage_table(self._arrays(), names)


class CommunityResult(_Result):
    """What :meth:`NNEngine.communities` returns (the definition is ``sequence.modularity_communities``), per row: ``label`` (int64:
    the smallest row of its community; -1 for an invalid row) and ``size`` (int64); ``level_label`` (int64 (levels, n)): the labelling
    behind each level, every level's communities nested in the next one's; per level (int64) ``nodes``, ``communities``, ``sweeps``,
    ``accepted``, ``moved``, ``rejected``, ``split`` and ``qnum`` (a list of Python ints; ``qnum_words`` uint64 (levels, 2): the
    device's low and high word, two's complement); ``levels``, ``complete``, ``m2``, ``resolution``, ``modularity`` (float64: the last
    qnum / (64 * m2^2); 0.0 without a level), ``valid`` and ``n``.  :meth:`NNEngine.communities_dev` leaves ``label``, ``size`` and
    ``level_label`` on the device: they and ``valid`` are None here."""
    FIELDS = (("label", "size", "level_label") + _sequence.COMM_LEVEL_FIELDS +
              ("qnum", "qnum_words", "levels", "complete", "m2", "resolution", "modularity", "valid", "n"))

    @property
    def n_communities(self) -> int:
        return int(np.count_nonzero(self.label == np.arange(self.n)))

    def at_level(self, level) -> np.ndarray:
        """int64 label per row behind level ``level`` (negative: from the last): the finest partition is level 0"""
        return self.level_label[level]

    def table(self, names=None):
        """``sequence.communities_table``: one record per community - label, size, members"""
        return _sequence.communities_table({"label": self.label, "size": self.size}, names)

    @classmethod
    def build(cls, result):
        """from the dict of ``sequence.modularity_communities``"""
        words = np.array([[q & (2 ** 64 - 1), (q >> 64) & (2 ** 64 - 1)] for q in result["qnum"]], dtype=np.uint64).reshape(-1, 2)
        return cls(**{k: result[k] for k in cls.FIELDS if k in result}, qnum_words=words, n=len(result["label"]))


class TSNEResult(_Result):
    """What :meth:`NNEngine.tsne` returns (the definition is ``sequence.tsne_layout``): ``layout`` (float32 (n, 2), NaN at an invalid
    row), ``z_trace`` (uint64 (n_iter + 1,): the integer Z - the sum of 1 / (1 + d^2) over all ordered pairs in units of 2^-20 - of
    every iterate, the final one included), ``kl_divergence`` (float64: ``sequence.tsne_kl`` of the final layout), ``iterations``,
    ``valid`` (bool (n,)), ``n`` and the knobs it ran with: ``exaggeration_iter``, ``exaggeration``, ``learning_rate``.  From
    :meth:`NNEngine.tsne_dev` the per-row arrays stay on the device and ``layout``, ``z_trace``, ``kl_divergence`` and ``valid`` are
    None."""
    FIELDS = ("layout", "z_trace", "kl_divergence", "iterations", "valid", "n", "exaggeration_iter", "exaggeration", "learning_rate")

    def table(self, names=None):
        """``sequence.tsne_table``: one record per row - name, x, y"""
        return _sequence.tsne_table(self.layout, self.valid, names)


class VoteResult(_Result):
    """What :meth:`NNEngine.vote` returns (the definition is ``sequence.class_votes``): per query row and class of a labelled base,
    over the voters - the valid base rows of the class whose cosine similarity reaches the threshold - ``count`` (int64: how many),
    ``weight`` (int64: their similarities summed in units of 2^-32), ``nearest`` (int64) and ``nearest_sim`` (float32, the device's
    own value): the most similar voter, ties to the smaller index, -1 / NaN where the class has none -, each (n_query, n_classes);
    ``query_valid`` (bool: the rows that took part; the others have 0 / 0 / -1 / NaN), ``n_classes`` and the ``threshold`` as the
    float32 it was compared as."""
    FIELDS = ("count", "weight", "nearest", "nearest_sim", "query_valid", "n_classes", "threshold")

    def similarity_sum(self) -> np.ndarray:
        """float64 (n_query, n_classes): ``weight`` / 2^32 - the voters' similarities summed"""
        return self.weight.astype(np.float64) / _sequence.VOTE_UNIT

    def mean_similarity(self) -> np.ndarray:
        """float64 (n_query, n_classes): the voters' mean similarity, NaN where the class has none"""
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(self.count > 0, self.similarity_sum() / self.count, np.nan)

    def predict(self, rule="weight", min_votes=1):
        """``sequence.vote_predict``: (label int64, confidence float64, margin float64) per query - the class with the largest
        ``weight`` / ``count`` / ``nearest_sim``, ties to the smaller class, -1 where fewer than ``min_votes`` voters are within the
        threshold.  A share of votes, no calibrated probability."""
        return _sequence.vote_predict(self.count, self.weight, rule, self.nearest_sim, min_votes)

    def table(self, names=None, class_names=None, base_names=None, rule="weight", min_votes=1):
        """``sequence.vote_table``: one record per query - label, confidence, votes of the winner, votes in all, the nearest voter
        of the winning class and its similarity"""
        return _sequence.vote_table(self.count, self.weight, self.nearest, self.nearest_sim, names, class_names, base_names, rule, min_votes)

    @classmethod
    def build(cls, arrays, query_valid, n_classes, threshold):
        """from the (count, weight, nearest, nearest_sim) of ``sequence.class_votes`` or the library, and the queries' validity"""
        count, weight, nearest, nearest_sim = arrays
        query_valid = np.asarray(query_valid, dtype=bool)
        if count.shape != (len(query_valid), int(n_classes)):
            raise ValueError(f"count has the shape {count.shape}, expected {(len(query_valid), int(n_classes))}")
        return cls(count=count, weight=weight, nearest=nearest, nearest_sim=nearest_sim, query_valid=query_valid, n_classes=int(n_classes),
                   threshold=float(_sequence.cluster_threshold(threshold)))


class NNEngine:
    def __init__(self, device: int = 0, weights: dict = None, chunk: int = None):
        self.lib = _lib.load()
        ctx = C.c_void_p()
        check(self.lib.gnn_create(int(device), C.byref(ctx)))
        self.ctx = ctx
        self.device = int(device)
        self._weights_keepalive = None
        self._mcl_serial = 0                         # Markov clusterings so far: an MCLResult's matrix belongs to the last one
        if chunk:
            check(self.lib.gnn_set_chunk(self.ctx, int(chunk)))
        if weights is not None:
            self.load_weights(weights)

    # -- life cycle ---------------------------------------------------------------------
    def close(self):
        if getattr(self, "ctx", None):
            self.lib.gnn_destroy(self.ctx)
            self.ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def pci_bus_id(self) -> str:
        buf = C.create_string_buffer(32)
        check(self.lib.gnn_device_pci_bus_id(self.ctx, buf, 32))
        return buf.value.decode()

    def device_info(self) -> dict:
        name = C.create_string_buffer(256)
        cus, mem = C.c_int(), C.c_int64()
        check(self.lib.gnn_device_info(self.ctx, name, 256, C.byref(cus), C.byref(mem)))
        return {"name": name.value.decode(), "cus": cus.value, "hbm_bytes": mem.value}

    def mem_info(self):
        """(free, total) bytes of the engine's device."""
        f, t = C.c_int64(), C.c_int64()
        check(self.lib.gnn_device_mem_info(self.ctx, C.byref(f), C.byref(t)))
        return f.value, t.value

    def load_weights(self, weights: dict):
        w = _weights.validate(weights)
        s, keep = _weights.to_struct(w)
        check(self.lib.gnn_load_weights(self.ctx, C.byref(s)))
        self._weights_keepalive = keep

    def build_kmer_tables(self, reserve_bytes: int = -1) -> bool:
        """The k-mer tables of "f16x3tk" (156 GB: x2 per 14-mer, head A's pair products per (entry, 9-mer), conv2's tap tables and x1 over head A's index space); False - with nothing
        allocated - on a device that cannot hold them behind `reserve_bytes` (< 0: the library's default reserve)."""
        rc = self.lib.gnn_build_kmer_tables(self.ctx, int(reserve_bytes))
        if rc == _lib.ERR_NOMEM:
            return False
        check(rc)
        return True

    def has_kmer_tables(self) -> bool:
        return bool(self.lib.gnn_has_kmer_tables(self.ctx))

    def drop_kmer_tables(self):
        check(self.lib.gnn_drop_kmer_tables(self.ctx))

    def sync(self):
        check(self.lib.gnn_sync(self.ctx))

    def alloc(self, nbytes: int) -> DeviceBuffer:
        return DeviceBuffer(self, nbytes)

    # -- hot path -----------------------------------------------------------------------
    @staticmethod
    def _check_bases(bases) -> np.ndarray:
        b = np.ascontiguousarray(bases, dtype=np.uint8)
        if b.ndim != 2 or b.shape[1] != _lib.WINDOW:
            raise ValueError(f"bases must have shape (n, {_lib.WINDOW}), got {b.shape}")
        return b

    def tokenize(self, bases) -> np.ndarray:
        """(n,6000) uint8 padded upper-case windows -> (n,5997) uint16 tokens (sequence.py:170-193)."""
        b = self._check_bases(bases)
        out = np.empty((len(b), _lib.TOKENS), dtype=np.uint16)
        check(self.lib.gnn_tokenize(self.ctx, b.ctypes.data, len(b), out.ctypes.data))
        return out

    def onehot(self, bases, dtype="u8") -> np.ndarray:
        """Stand-alone encoder: (n,6000) bases -> (n,5997,257) one-hot (model.py:9-11)."""
        b = self._check_bases(bases)
        code, npdt = {"u8": (_lib.OH_U8, np.uint8), "bf16": (_lib.OH_BF16, np.uint16),
                      "f32": (_lib.OH_F32, np.float32)}[dtype]
        shape = (len(b), _lib.TOKENS, _lib.DEPTH)
        nbytes = int(np.prod(shape)) * np.dtype(npdt).itemsize
        db, do = self.alloc(max(b.nbytes, 1)), self.alloc(max(nbytes, 1))
        try:
            if len(b):
                db.upload(b)
            check(self.lib.gnn_onehot_dev(self.ctx, db.ptr, len(b), code, do.ptr))
            self.sync()
            return do.download(shape, npdt)
        finally:
            db.free()
            do.free()

    def classify(self, bases, precision=_lib.DEFAULT_PRECISION) -> np.ndarray:
        """(n,6000) uint8 windows -> (n,3) float32 class scores (chromosome, plasmid, virus)."""
        b = self._check_bases(bases)
        out = np.empty((len(b), _lib.CLASSES), dtype=np.float32)
        check(self.lib.gnn_classify(self.ctx, b.ctypes.data, len(b), _lib.PRECISIONS[precision],
                                    out.ctypes.data))
        return out

    def classify_dev(self, bases_ptr: int, n: int, scores_ptr: int, precision=_lib.DEFAULT_PRECISION):
        """Asynchronous: device pointers in and out, enqueued on the engine's stream."""
        check(self.lib.gnn_classify_dev(self.ctx, bases_ptr, int(n), _lib.PRECISIONS[precision],
                                        scores_ptr))

    def classify_dev_async(self, bases_ptr: int, n: int, scores_ptr: int, precision=_lib.DEFAULT_PRECISION):
        """classify_dev whose last back end may still run beside the next call's front end; call :meth:`flush`
        (or sync / download / a collective) before reading the scores."""
        check(self.lib.gnn_classify_dev_async(self.ctx, bases_ptr, int(n), _lib.PRECISIONS[precision], scores_ptr))

    def flush(self):
        check(self.lib.gnn_classify_flush(self.ctx))

    # -- encoder embeddings ---------------------------------------------------------------
    def embed(self, bases, precision=_lib.DEFAULT_PRECISION, dtype="f32", with_scores=False):
        """(n,6000) uint8 windows -> (n,512) encoder embeddings: create_encoder()'s output (model.py:14-31), the h1 the
        classifier reads.  dtype "f32" -> float32; "bf16" -> uint16 bit patterns (the f32 values rounded to nearest even).
        with_scores: also the (n,3) class scores of the same pass (bit-identical to :meth:`classify`), as (emb, scores)."""
        b = self._check_bases(bases)
        npdt = np.float32 if _lib.EMB_DTYPES[dtype] == _lib.EMB_F32 else np.uint16
        emb = np.empty((len(b), _lib.EMBED_DIM), dtype=npdt)
        scores = np.empty((len(b), _lib.CLASSES), dtype=np.float32) if with_scores else None
        check(self.lib.gnn_embed(self.ctx, b.ctypes.data, len(b), _lib.PRECISIONS[precision], _lib.EMB_DTYPES[dtype],
                                 emb.ctypes.data, scores.ctypes.data if with_scores else None))
        return (emb, scores) if with_scores else emb

    def embed_dev(self, bases_ptr: int, n: int, emb_ptr: int, precision=_lib.DEFAULT_PRECISION, dtype="f32", scores_ptr=None):
        """Asynchronous: device pointers in and out (emb: n x 512 of ``dtype``; scores: n x 3 f32 or None), enqueued on the
        engine's stream."""
        check(self.lib.gnn_embed_dev(self.ctx, bases_ptr, int(n), _lib.PRECISIONS[precision], _lib.EMB_DTYPES[dtype], emb_ptr,
                                     scores_ptr))

    def debug_forward(self, bases, precision="f32", taps=("m_a", "m_b", "yp_a", "yp_b",
                                                         "alpha_a", "alpha_b", "feat")):
        """Scores plus the requested intermediates as a dict of numpy arrays."""
        b = self._check_bases(bases)
        n = len(b)
        shapes = {"x1": (n, _lib.TOKENS, _lib.CH), "x2": (n, _lib.TOKENS, _lib.CH),
                  "x3": (n, _lib.TOKENS, _lib.CH), "m_a": (n, _lib.PATCHES), "m_b": (n, _lib.PATCHES),
                  "yp_a": (n, _lib.POOLED, _lib.CH), "yp_b": (n, _lib.POOLED, _lib.CH),
                  "alpha_a": (n, _lib.POOLED), "alpha_b": (n, _lib.POOLED), "feat": (n, _lib.FEAT)}
        arrays = {k: np.empty(shapes[k], dtype=np.float32) for k in taps}
        t = _lib.Taps(**{k: v.ctypes.data_as(C.POINTER(C.c_float)) for k, v in arrays.items()})
        scores = np.empty((n, _lib.CLASSES), dtype=np.float32)
        check(self.lib.gnn_debug_forward(self.ctx, b.ctypes.data, n, _lib.PRECISIONS[precision],
                                         scores.ctypes.data, C.byref(t)))
        return scores, arrays

    # -- packed contigs: what every contig method is given ---------------------------------
    @staticmethod
    def _offsets(offsets) -> np.ndarray:
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if offsets.ndim != 1 or len(offsets) < 1:
            raise ValueError("offsets must hold n_contigs + 1 byte offsets")
        return offsets

    @classmethod
    def _packed(cls, seq, offsets):
        """(packed bytes, offsets) as the contig entry points take them: (ptr, on_host, bytes, offsets, n_contigs).  ``seq`` is a
        host array (any dtype / layout numpy converts to contiguous uint8) or the device address of byte 0; the returned ``keep``
        owns the bytes ``ptr`` points at."""
        offsets = cls._offsets(offsets)
        if isinstance(seq, np.ndarray):
            keep = np.ascontiguousarray(seq, dtype=np.uint8)
            return (keep.ctypes.data, 1, keep.nbytes, offsets, len(offsets) - 1), keep
        return (seq, 0, int(offsets[-1]), offsets, len(offsets) - 1), None

    @staticmethod
    def _strand_code(strand) -> int:
        return _lib.STRANDS[strand] if isinstance(strand, str) else int(strand)       # an int goes to the library as it is

    def _classify_contigs(self, seq, offsets, single_window, precision, embed=False, strand=None):
        """gnn_classify_contigs / _embed / _strand -> (scores, ids, emb or None, fwd or None, rev or None)"""
        (ptr, on_host, nbytes, offsets, n_contigs), _keep = self._packed(seq, offsets)
        scores = np.zeros((n_contigs, _lib.CLASSES), dtype=np.float32)
        emb = np.zeros((n_contigs, _lib.EMBED_DIM), dtype=np.float32) if embed else None
        cap = int(((np.diff(offsets) + _lib.WINDOW - 1) // _lib.WINDOW).sum()) if n_contigs else 0
        ids = np.empty(max(cap, 1), dtype=np.int64)
        n = C.c_int64()
        args = (self.ctx, ptr, on_host, nbytes, offsets.ctypes.data, n_contigs, int(bool(single_window)),
                _lib.PRECISIONS[precision], scores.ctypes.data, ids.ctypes.data, cap, C.byref(n))
        fwd = rev = None
        if strand is not None:
            fwd, rev = (np.zeros((n_contigs, _lib.CLASSES), dtype=np.float32) for _ in range(2))
            check(self.lib.gnn_classify_contigs_strand(*args, emb.ctypes.data if embed else None, self._strand_code(strand),
                                                       fwd.ctypes.data, rev.ctypes.data))
        elif embed:
            check(self.lib.gnn_classify_contigs_embed(*args, emb.ctypes.data))
        else:
            check(self.lib.gnn_classify_contigs(*args))
        return scores, ids[:n.value].copy(), emb, fwd, rev

    def _scan_contigs(self, seq, offsets, stride, single_window, precision, strand=None):
        """gnn_scan_contigs / _strand -> ScanResult / StrandScanResult"""
        (ptr, on_host, nbytes, offsets, n_contigs), _keep = self._packed(seq, offsets)
        win_off, bin_off, starts, lens = self.scan_plan(offsets, stride, single_window)
        n, n_bins = len(starts), int(bin_off[-1])
        scores = np.zeros((n, _lib.CLASSES), dtype=np.float32)
        kept = np.zeros(n, dtype=np.uint8)
        track = np.zeros((n_bins, _lib.CLASSES), dtype=np.float32)
        cover = np.zeros(n_bins, dtype=np.int32)
        contig_scores = np.zeros((n_contigs, _lib.CLASSES), dtype=np.float32)
        args = (self.ctx, ptr, on_host, nbytes, offsets.ctypes.data, n_contigs, int(stride), int(bool(single_window)),
                _lib.PRECISIONS[precision], scores.ctypes.data, kept.ctypes.data, n, track.ctypes.data, cover.ctypes.data, n_bins,
                contig_scores.ctypes.data)
        if strand is None:
            check(self.lib.gnn_scan_contigs(*args))
        else:
            code = self._strand_code(strand)
            fwd, rev = (np.zeros((n, _lib.CLASSES), dtype=np.float32) for _ in range(2))
            check(self.lib.gnn_scan_contigs_strand(*args, code, fwd.ctypes.data, rev.ctypes.data))
        fields = dict(stride=int(stride), win_offsets=win_off, starts=starts, lens=lens, kept=kept.astype(bool), scores=scores,
                      bin_offsets=bin_off, track=track, cover=cover, contig_scores=contig_scores)
        if strand is None:
            return ScanResult(**fields)
        name = {v: k for k, v in _lib.STRANDS.items()}[code]
        return StrandScanResult(**fields, strand=name, scores_fwd=fwd, scores_rev=rev)

    def _occlude_contigs(self, seq, offsets, block, single_window, precision):
        """gnn_occlude_contigs -> OcclusionResult"""
        (ptr, on_host, nbytes, offsets, n_contigs), _keep = self._packed(seq, offsets)
        win_off, starts, lens, blk_off = self.occlusion_plan(offsets, block, single_window)
        n, n_pairs = len(starts), int(blk_off[-1])
        scores = np.zeros((n, _lib.CLASSES), dtype=np.float32)
        kept = np.zeros(n, dtype=np.uint8)
        delta = np.zeros((n_pairs, _lib.CLASSES), dtype=np.float32)
        contig_scores = np.zeros((n_contigs, _lib.CLASSES), dtype=np.float32)
        check(self.lib.gnn_occlude_contigs(self.ctx, ptr, on_host, nbytes, offsets.ctypes.data, n_contigs, int(block),
                                           int(bool(single_window)), _lib.PRECISIONS[precision], scores.ctypes.data, kept.ctypes.data, n,
                                           delta.ctypes.data, n_pairs, contig_scores.ctypes.data))
        return OcclusionResult(block=int(block), win_offsets=win_off, starts=starts, lens=lens, kept=kept.astype(bool), scores=scores,
                               blk_offsets=blk_off, delta=delta, contig_scores=contig_scores)

    # -- contig scores and embeddings ------------------------------------------------------
    def classify_contigs(self, seq: np.ndarray, offsets: np.ndarray, single_window: bool = False,
                         precision=_lib.DEFAULT_PRECISION):
        """Contig front end: packed raw contig bytes -> per-contig scores.

        Does what generate_data + the predict loop + segment_mean do (nn_classification.py:54-82,
        :316-320) in ONE library call (``gnn_classify_contigs``): candidate windows are cut in native code,
        the packed buffer goes up in pieces on a copy stream while earlier pieces are classified, the
        N-content rule, upper-casing, padding, tokenising, classification and the per-contig mean run on the
        device and the window scores never leave it.  Returns (contig_scores (n_contigs, 3), contig ids of
        the kept windows).
        """
        return self._classify_contigs(np.asarray(seq), offsets, single_window, precision)[:2]

    def classify_contigs_dev(self, seq_ptr: int, offsets: np.ndarray, single_window: bool = False,
                             precision=_lib.DEFAULT_PRECISION):
        """Same as :meth:`classify_contigs` for a packed contig buffer that is already resident in
        HBM (``seq_ptr`` = device address of byte 0, ``offsets`` = (n_contigs+1,) byte offsets)."""
        return self._classify_contigs(seq_ptr, offsets, single_window, precision)[:2]

    def embed_contigs(self, seq: np.ndarray, offsets: np.ndarray, single_window: bool = False,
                      precision=_lib.DEFAULT_PRECISION):
        """:meth:`classify_contigs` plus the per-contig embedding (``gnn_classify_contigs_embed``): the f32 mean of the encoder
        embeddings of the contig's kept windows, a zero row for a contig without one.  Returns (contig_scores (n_contigs, 3),
        contig_embeddings (n_contigs, 512), contig ids of the kept windows); scores and ids are those of classify_contigs."""
        scores, ids, emb = self._classify_contigs(np.asarray(seq), offsets, single_window, precision, embed=True)[:3]
        return scores, emb, ids

    def embed_contigs_dev(self, seq_ptr: int, offsets: np.ndarray, single_window: bool = False,
                          precision=_lib.DEFAULT_PRECISION):
        """Same as :meth:`embed_contigs` for a packed contig buffer that is already resident in HBM."""
        scores, ids, emb = self._classify_contigs(seq_ptr, offsets, single_window, precision, embed=True)[:3]
        return scores, emb, ids

    # -- score tracks --------------------------------------------------------------------
    def scan_plan(self, offsets: np.ndarray, stride: int, single_window: bool = False):
        """``gnn_scan_plan`` (host only): (win_offsets, bin_offsets, contig-relative starts, lens) of a scan at ``stride``."""
        offsets = self._offsets(offsets)
        n_contigs = len(offsets) - 1
        nw, nb = C.c_int64(), C.c_int64()
        head = (offsets.ctypes.data, n_contigs, int(stride), int(bool(single_window)), C.byref(nw), C.byref(nb))
        check(self.lib.gnn_scan_plan(*head, None, None, None, None))
        win_off, bin_off = np.zeros(n_contigs + 1, np.int64), np.zeros(n_contigs + 1, np.int64)
        starts, lens = np.zeros(nw.value, np.int64), np.zeros(nw.value, np.int32)
        check(self.lib.gnn_scan_plan(*head, win_off.ctypes.data, bin_off.ctypes.data, starts.ctypes.data, lens.ctypes.data))
        return win_off, bin_off, starts, lens

    def scan_contigs(self, seq: np.ndarray, offsets: np.ndarray, stride: int, single_window: bool = False,
                     precision=_lib.DEFAULT_PRECISION) -> ScanResult:
        """Score track along every contig (``gnn_scan_contigs``): overlapping 6000-base windows every ``stride`` bases
        (1 <= stride <= 6000), each scored by the forward pass of :meth:`classify`, and their mean per stride-wide bin - where in
        a contig the signal is, which :meth:`classify_contigs` averages away.  The window and bin rules are those of
        ``sequence.scan_spans`` / ``sequence.scan_track``; at stride 6000 windows and ``contig_scores`` are those of
        classify_contigs.  Overlapping windows are classified independently: 6000 / stride times the work."""
        return self._scan_contigs(np.asarray(seq), offsets, stride, single_window, precision)

    def scan_contigs_dev(self, seq_ptr: int, offsets: np.ndarray, stride: int, single_window: bool = False,
                         precision=_lib.DEFAULT_PRECISION) -> ScanResult:
        """Same as :meth:`scan_contigs` for a packed contig buffer that is already resident in HBM."""
        return self._scan_contigs(seq_ptr, offsets, stride, single_window, precision)

    # -- region calls --------------------------------------------------------------------
    def set_region_tile(self, bins: int):
        """test aid (``gnn_debug_set_region_tile``): bins per tile of the region kernels' scan, 1..4096; no result depends on it."""
        check(self.lib.gnn_debug_set_region_tile(self.ctx, int(bins)))

    def call_regions(self, track, bin_offsets, penalty, offsets=None, stride=None) -> RegionResult:
        """Region calls along contigs (``gnn_call_regions``; the definition is ``sequence.call_regions``): one 3-state Viterbi path
        per contig over the track of a scan (``track`` (n_bins, 3), ``bin_offsets``: any strand mode's), a switch between classes
        costing ``penalty`` (0..4096, in score x bins: a run of n bins is split off when its summed advantage exceeds 2 x penalty).
        Integer arithmetic on the device: bit-identical to the numpy definition.  ``offsets`` (the contigs' byte offsets) and
        ``stride`` add base coordinates, means and margins (``sequence.region_table``)."""
        track = np.ascontiguousarray(track, dtype=np.float32).reshape(-1, _lib.CLASSES)
        bin_off = self._offsets(bin_offsets)
        n_contigs, n_bins = len(bin_off) - 1, int(bin_off[-1])
        if len(track) != n_bins:
            raise ValueError(f"the track has {len(track)} bins, bin_offsets end at {n_bins}")
        state = np.zeros(n_bins, dtype=np.uint8)
        n = C.c_int64(0)
        cap = n_contigs + n_bins // 16 + 1024           # a guess: the call says what it needs when this is too small
        while True:
            arrs = {"contig": np.zeros(cap, np.int64), "lo": np.zeros(cap, np.int64), "hi": np.zeros(cap, np.int64),
                    "state": np.zeros(cap, np.uint8), "evidence": np.zeros(cap, np.int64), "qsum": np.zeros((cap, _lib.CLASSES), np.int64)}
            rc = self.lib.gnn_call_regions(self.ctx, track.ctypes.data, bin_off.ctypes.data, n_contigs, float(penalty), state.ctypes.data,
                                           *(a.ctypes.data for a in arrs.values()), cap, C.byref(n))
            if rc == _lib.ERR_ARG and n.value > cap:
                cap = n.value
                continue
            check(rc)
            break
        regions = {k: a[:n.value].copy() for k, a in arrs.items()}
        return RegionResult.build(penalty, bin_off, state, regions, offsets, stride)

    def region_states_dev(self, track_ptr: int, bin_offsets, penalty, state_ptr: int):
        """Asynchronous building block (``gnn_region_states_dev``): track (n_bins x 3 f32) and states (n_bins uint8) are device
        pointers; the path's state per bin is enqueued on the engine's stream."""
        bin_off = self._offsets(bin_offsets)
        check(self.lib.gnn_region_states_dev(self.ctx, track_ptr, bin_off.ctypes.data, len(bin_off) - 1, float(penalty), state_ptr))

    def scan_regions(self, seq: np.ndarray, offsets: np.ndarray, stride: int, penalty, single_window: bool = False,
                     precision=_lib.DEFAULT_PRECISION, strand=None):
        """:meth:`scan_contigs` (``strand`` given: :meth:`scan_contigs_strand`) followed by :meth:`call_regions` on its track.
        Returns (the scan's result, RegionResult with the derived table)."""
        scan = self._scan_contigs(np.asarray(seq), offsets, stride, single_window, precision, strand)
        return scan, self.call_regions(scan.track, scan.bin_offsets, penalty, self._offsets(offsets), stride)

    # -- interval embeddings ---------------------------------------------------------------
    def interval_plan(self, offsets: np.ndarray, stride: int, contig, start, end, single_window: bool = False):
        """``gnn_interval_plan`` (host only): the member windows (w_lo, w_hi) of the intervals, validated
        (``sequence.interval_windows`` is the numpy mirror)."""
        offsets = self._offsets(offsets)
        contig, start, end = self._intervals(contig, start, end)
        w_lo, w_hi = np.zeros(len(contig), np.int64), np.zeros(len(contig), np.int64)
        check(self.lib.gnn_interval_plan(offsets.ctypes.data, len(offsets) - 1, int(stride), int(bool(single_window)), contig.ctypes.data,
                                         start.ctypes.data, end.ctypes.data, len(contig), w_lo.ctypes.data, w_hi.ctypes.data))
        return w_lo, w_hi

    @staticmethod
    def _intervals(contig, start, end):
        arrs = tuple(np.ascontiguousarray(a, dtype=np.int64).reshape(-1) for a in (contig, start, end))
        if not len(arrs[0]) == len(arrs[1]) == len(arrs[2]):
            raise ValueError("contig, start and end differ in length")
        return arrs

    def _embed_intervals(self, seq, offsets, stride, contig, start, end, strand, single_window, precision) -> IntervalResult:
        (ptr, on_host, nbytes, offsets, n_contigs), _keep = self._packed(seq, offsets)
        contig, start, end = self._intervals(contig, start, end)
        n = len(contig)
        code = self._strand_code(strand)
        emb = np.zeros((n, _lib.EMBED_DIM), dtype=np.float32)
        count = np.zeros(n, dtype=np.int32)
        coherence = np.zeros(n, dtype=np.float32)
        scores = np.zeros((n, _lib.CLASSES), dtype=np.float32)
        check(self.lib.gnn_embed_intervals(self.ctx, ptr, on_host, nbytes, offsets.ctypes.data, n_contigs, int(stride),
                                           int(bool(single_window)), _lib.PRECISIONS[precision], code, contig.ctypes.data, start.ctypes.data,
                                           end.ctypes.data, n, emb.ctypes.data, count.ctypes.data, coherence.ctypes.data, scores.ctypes.data))
        w_lo, w_hi = self.interval_plan(offsets, stride, contig, start, end, single_window) if n and n_contigs else (
            np.zeros(n, np.int64), np.zeros(n, np.int64))
        name = {v: k for k, v in _lib.STRANDS.items()}[code]
        return IntervalResult(stride=int(stride), strand=name, contig=contig, start=start, end=end, w_lo=w_lo, w_hi=w_hi, count=count,
                              embedding=emb, coherence=coherence, scores=scores)

    def embed_intervals(self, seq: np.ndarray, offsets: np.ndarray, stride: int, contig, start, end, strand="forward",
                        single_window: bool = False, precision=_lib.DEFAULT_PRECISION) -> IntervalResult:
        """Encoder embeddings for parts of contigs (``gnn_embed_intervals``; the definition is ``sequence.interval_windows`` +
        ``sequence.interval_embeddings``): the windows of a scan at ``stride`` go through the forward pass once more, and the rows of
        the kept windows whose centre base lies in an interval (``contig``, ``start``, ``end``: sorted, disjoint, 0-based half-open
        bases) are folded on the device into that interval's mean embedding, mean scores and coherence.  What
        :meth:`embed_contigs` answers per contig, for the regions :meth:`call_regions` names.  Costs one scan of the same windows;
        no window row leaves the device."""
        return self._embed_intervals(np.asarray(seq), offsets, stride, contig, start, end, strand, single_window, precision)

    def embed_intervals_dev(self, seq_ptr: int, offsets: np.ndarray, stride: int, contig, start, end, strand="forward",
                            single_window: bool = False, precision=_lib.DEFAULT_PRECISION) -> IntervalResult:
        """Same as :meth:`embed_intervals` for a packed contig buffer that is already resident in HBM."""
        return self._embed_intervals(seq_ptr, offsets, stride, contig, start, end, strand, single_window, precision)

    def embed_regions(self, seq: np.ndarray, offsets: np.ndarray, regions: RegionResult, strand="forward", single_window: bool = False,
                      precision=_lib.DEFAULT_PRECISION) -> IntervalResult:
        """:meth:`embed_intervals` on the regions of a :class:`RegionResult` built with ``offsets`` and ``stride`` (its
        ``region_contig``, ``start``, ``end``): one embedding per called region.  Regions of a contig are sorted and disjoint by
        construction.  A result without the derived table is refused."""
        if regions.stride is None or regions.start is None or regions.end is None:
            raise ValueError("the RegionResult has no base coordinates: call_regions(..., offsets=, stride=) builds them")
        return self.embed_intervals(seq, offsets, regions.stride, regions.region_contig, regions.start, regions.end, strand, single_window,
                                    precision)

    def fold_intervals(self, rows, kept, w_lo, w_hi, scores=None, rows_per_call=None, rows_rev=None):
        """The building blocks (``gnn_interval_fold_dev`` + ``gnn_interval_finish_dev``) on rows of the caller's choosing: ``rows``
        (n, 512) float32, ``kept`` (n,) the mask, [w_lo[i], w_hi[i]) the member rows of interval i, ``scores`` (n, 3) or None.  The
        rows are fed in slices of ``rows_per_call`` (None: all at once); no result depends on it.  ``rows_rev`` (n, 512) selects strand
        mode ``both`` as ``gnn_embed_intervals`` runs it: the reverse rows are folded slice by slice into sums of their own (no scores,
        a count that is ignored) and the finish adds the two; ``scores`` are then the combined window scores.  Returns a dict of
        ``count``, ``embedding``, ``coherence`` (float32) and ``scores`` as ``sequence.interval_embeddings``."""
        rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, _lib.EMBED_DIM)
        n = len(rows)
        if rows_rev is not None:
            rows_rev = np.ascontiguousarray(rows_rev, dtype=np.float32).reshape(-1, _lib.EMBED_DIM)
            if len(rows_rev) != n:
                raise ValueError(f"rows_rev has {len(rows_rev)} rows, rows has {n}")
        kept = np.ascontiguousarray(np.asarray(kept).astype(bool), dtype=np.uint8)
        w_lo, w_hi = (np.ascontiguousarray(a, dtype=np.int64).reshape(-1) for a in (w_lo, w_hi))
        if len(kept) != n or len(w_lo) != len(w_hi):
            raise ValueError("kept has one flag per row, and w_lo and w_hi one entry per interval")
        if len(w_hi) and int(w_hi.max()) > n:
            raise ValueError(f"a member range ends at {int(w_hi.max())}, beyond the {n} rows")
        if scores is not None:
            scores = np.ascontiguousarray(scores, dtype=np.float32).reshape(n, _lib.CLASSES)
        ni = len(w_lo)
        out = {"count": np.zeros(ni, np.int32), "embedding": np.zeros((ni, _lib.EMBED_DIM), np.float32),
               "coherence": np.zeros(ni, np.float32), "scores": np.zeros((ni, _lib.CLASSES), np.float32)}
        if ni == 0 or n == 0:
            return out
        step = n if rows_per_call is None else max(1, int(rows_per_call))
        sizes = {"rows": rows.nbytes, "scores": n * 12, "sum": ni * 2048, "unit": ni * 2048, "score_sum": ni * 12, "count": ni * 4,
                 "coherence": ni * 4}
        zeroed = ["sum", "unit", "score_sum", "count"]
        if rows_rev is not None:         # the second strand: its own rows and sums, and the count the entry point insists on
            sizes.update({"rows_rev": rows_rev.nbytes, "sum_rev": ni * 2048, "unit_rev": ni * 2048, "count_rev": ni * 4})
            zeroed += ["sum_rev", "unit_rev", "count_rev"]
        bufs = {}
        try:
            for k, v in sizes.items():
                bufs[k] = self.alloc(v)
            bufs["rows"].upload(rows)
            if rows_rev is not None:
                bufs["rows_rev"].upload(rows_rev)
            if scores is not None:
                bufs["scores"].upload(scores)
            for k in zeroed:
                bufs[k].upload(np.zeros(sizes[k], np.uint8))
            sc = bufs["scores"].ptr if scores is not None else None
            ssum = bufs["score_sum"].ptr if scores is not None else None
            sum_rev, unit_rev = (bufs["sum_rev"].ptr, bufs["unit_rev"].ptr) if rows_rev is not None else (None, None)
            for a in range(0, n, step):
                check(self.lib.gnn_interval_fold_dev(self.ctx, bufs["rows"].ptr, sc, a, min(step, n - a), kept.ctypes.data, w_lo.ctypes.data,
                                                     w_hi.ctypes.data, ni, bufs["sum"].ptr, bufs["unit"].ptr, ssum, bufs["count"].ptr))
                if rows_rev is not None:
                    check(self.lib.gnn_interval_fold_dev(self.ctx, bufs["rows_rev"].ptr, None, a, min(step, n - a), kept.ctypes.data,
                                                         w_lo.ctypes.data, w_hi.ctypes.data, ni, sum_rev, unit_rev, None,
                                                         bufs["count_rev"].ptr))
            check(self.lib.gnn_interval_finish_dev(self.ctx, bufs["sum"].ptr, bufs["unit"].ptr, sum_rev, unit_rev, ssum, bufs["count"].ptr,
                                                   ni, bufs["sum"].ptr, bufs["coherence"].ptr, ssum))
            self.sync()
            out["embedding"] = bufs["sum"].download((ni, _lib.EMBED_DIM), np.float32)
            out["count"] = bufs["count"].download((ni,), np.int32)
            out["coherence"] = bufs["coherence"].download((ni,), np.float32)
            if scores is not None:
                out["scores"] = bufs["score_sum"].download((ni, _lib.CLASSES), np.float32)
        finally:
            for b in bufs.values():
                b.free()
        return out

    # -- nearest neighbours ---------------------------------------------------------------
    def set_neighbour_split(self, rows: int):
        """test aid (``gnn_debug_set_neighbour_split``): base rows per workgroup of the neighbour search (0: the library's choice); no
        result depends on it."""
        check(self.lib.gnn_debug_set_neighbour_split(self.ctx, int(rows)))

    @staticmethod
    def _knn_metric(metric) -> int:
        return _lib.KNN_METRICS[metric] if isinstance(metric, str) else int(metric)

    @staticmethod
    def _check_metric(metric):
        """an unknown metric name is a ``ValueError`` before anything is allocated or launched"""
        if isinstance(metric, str) and metric not in _lib.KNN_METRICS:
            raise ValueError(f"metric {metric!r}: expected one of {tuple(_lib.KNN_METRICS)}")

    @staticmethod
    def _metric_name(metric) -> str:
        """the name of a metric given by name or by the library's code"""
        return metric if isinstance(metric, str) else {v: k for k, v in _lib.KNN_METRICS.items()}[int(metric)]

    def _debug_ms(self, fn, dtype=np.float64) -> np.ndarray:
        """the float64 milliseconds a ``gnn_debug_*_ms`` entry point keeps (or the ``dtype`` values of another entry point of that
        shape): ask for their number, allocate, ask again"""
        n = C.c_int64(0)
        check(fn(self.ctx, None, 0, C.addressof(n)))
        ms = np.zeros(n.value, dtype)
        if n.value:
            check(fn(self.ctx, ms.ctypes.data, n.value, C.addressof(n)))
        return ms

    def _count_then_fill(self, count, fill, n_indptr, max_edges, too_many):
        """what :meth:`graph` and :meth:`match` share: ``count(indptr_ptr, total_ptr)``, the verdict on ``max_edges`` (``too_many``
        words the ``ValueError``), then ``fill(col_ptr, sim_ptr, m)`` into arrays of the counted size.  Returns (indptr, col, sim)."""
        indptr = np.empty(n_indptr, dtype=np.int64)
        total = C.c_int64(0)
        check(count(indptr.ctypes.data, C.addressof(total)))
        m = int(total.value)
        if m > int(max_edges):
            raise ValueError(f"{too_many(m)}, more than max_edges = {int(max_edges)}: raise the threshold or max_edges")
        col, sim = np.empty(m, dtype=np.int32), np.empty(m, dtype=np.float32)
        check(fill(col.ctypes.data, sim.ctypes.data, m))
        return indptr, col, sim

    def neighbours(self, query, base=None, k=10, metric="cosine"):
        """Nearest neighbours among encoder embeddings (``gnn_neighbours``; the definition is ``sequence.nearest_neighbours``): for
        every row of ``query`` (nq, 512) its ``k`` (1..64) most similar rows of ``base`` (nb, 512) under ``metric`` ("cosine" or
        "dot"), exact search on the matrix pipe.  ``base=None``: the self-search, pair (i, i) excluded.  Returns (idx int64 (nq, k),
        sim float32 (nq, k)), each row ordered by (similarity descending, base index ascending), padded with -1 / NaN; rows that
        are not finite (under cosine: or zero) neither match nor are matched."""
        q = _sequence.neighbour_rows(query)
        b = None if base is None else _sequence.neighbour_rows(base, "base")
        idx = np.empty((len(q), max(int(k), 0)), dtype=np.int64)         # a k outside [1, 64] is the library's error
        sim = np.empty((len(q), max(int(k), 0)), dtype=np.float32)
        check(self.lib.gnn_neighbours(self.ctx, q.ctypes.data, len(q), None if b is None else b.ctypes.data, 0 if b is None else len(b),
                                      int(k), self._knn_metric(metric), idx.ctypes.data, sim.ctypes.data))
        return idx, sim

    def neighbours_dev(self, query_ptr: int, n_query: int, base_ptr, n_base: int, idx_ptr: int, sim_ptr: int, k=10, metric="cosine"):
        """Asynchronous (``gnn_neighbours_dev``): device pointers in (query n_query x 512 f32; base n_base x 512 f32, or None for
        the self-search) and out (idx n_query x k int64, sim n_query x k f32), enqueued on the engine's stream."""
        check(self.lib.gnn_neighbours_dev(self.ctx, query_ptr, int(n_query), base_ptr, int(n_base), int(k), self._knn_metric(metric),
                                          idx_ptr, sim_ptr))

    # -- clusters ------------------------------------------------------------------------
    def cluster(self, rows, threshold, metric="cosine") -> ClusterResult:
        """Clusters among encoder embeddings (``gnn_cluster``; the definition is ``sequence.threshold_clusters``): the connected
        components of the graph with an edge between two valid rows of ``rows`` (n, 512) whose similarity under ``metric`` is >=
        ``threshold`` - single linkage, exact search over the upper triangle on the matrix pipe.  The similarity of the pair i < j
        is the float32 :meth:`neighbours` returns for query i and base row j.  Clusters chain: ``degree`` and ``rep`` tell a chain
        (a representative with few edges for its cluster's size) from a clique.  :meth:`set_neighbour_split` sets the range of
        this search too; no result depends on it."""
        r = _sequence.neighbour_rows(rows, "rows")
        self._check_metric(metric)
        out = [np.empty(len(r), dtype=np.int64) for _ in range(4)]
        check(self.lib.gnn_cluster(self.ctx, r.ctypes.data, len(r), float(threshold), self._knn_metric(metric),
                                   *(a.ctypes.data for a in out)))
        return ClusterResult.build(out, np.float32(threshold), metric)

    def cluster_dev(self, rows_ptr: int, n: int, threshold, label_ptr: int, degree_ptr: int, size_ptr: int, rep_ptr: int,
                    metric="cosine"):
        """Asynchronous (``gnn_cluster_dev``): device pointers in (rows n x 512 f32) and out (label, degree, size, rep: n int64
        each), enqueued on the engine's stream."""
        check(self.lib.gnn_cluster_dev(self.ctx, rows_ptr, int(n), float(threshold), self._knn_metric(metric), label_ptr, degree_ptr,
                                       size_ptr, rep_ptr))

    # -- density clusters ----------------------------------------------------------------
    def density(self, rows, threshold, min_points=5, metric="cosine") -> DensityResult:
        """Density clusters among encoder embeddings (``gnn_density``; the definition is ``sequence.density_clusters``): DBSCAN at
        one (``threshold``, ``min_points``) on the graph :meth:`cluster` acts on.  A valid row of ``rows`` (n, 512) with ``degree``
        + 1 >= ``min_points`` is core; clusters are the components of the core rows; a row that is not core hangs on to its most
        similar core neighbour as a border row (ties to the smaller index) and joins nothing; the rest is noise (label -1).  A row
        between two dense families no longer merges them.  Exact, two passes over the upper triangle on the matrix pipe; the
        similarity of the pair i < j is the float32 :meth:`neighbours` returns for query i and base row j.  Unlike textbook DBSCAN
        the result depends on no visiting order.  :meth:`set_neighbour_split` sets the range of this search too; no result depends
        on it."""
        r = _sequence.neighbour_rows(rows, "rows")
        self._check_metric(metric)
        n = len(r)
        out = [np.empty(n, dtype=np.int64) for _ in range(4)] + [np.empty(n, dtype=np.float32), np.empty(n, dtype=np.uint8)]
        check(self.lib.gnn_density(self.ctx, r.ctypes.data, n, float(threshold), int(min_points), self._knn_metric(metric),
                                   *(a.ctypes.data for a in out)))
        return DensityResult.build(out, np.float32(threshold), min_points, metric)

    def density_dev(self, rows_ptr: int, n: int, threshold, min_points, label_ptr: int, degree_ptr: int, size_ptr: int, anchor_ptr: int,
                    sim_ptr: int, kind_ptr: int, metric="cosine"):
        """Asynchronous (``gnn_density_dev``): device pointers in (rows n x 512 f32) and out (label, degree, size, anchor: n int64
        each; sim: n f32; kind: n uint8), enqueued on the engine's stream."""
        check(self.lib.gnn_density_dev(self.ctx, rows_ptr, int(n), float(threshold), int(min_points), self._knn_metric(metric), label_ptr,
                                       degree_ptr, size_ptr, anchor_ptr, sim_ptr, kind_ptr))

    # -- similarity graph ----------------------------------------------------------------
    def graph(self, rows, threshold, metric="cosine", max_edges=1 << 28) -> GraphResult:
        """The similarity graph among encoder embeddings (``gnn_graph_count`` + ``gnn_graph_fill``; the definition is
        ``sequence.threshold_graph``): every pair i < j of valid rows of ``rows`` (n, 512) whose similarity under ``metric`` is >=
        ``threshold``, with that similarity - the edges :meth:`cluster` joins, kept; exact, two passes over the upper triangle on
        the matrix pipe.  The similarity of the pair i < j is the float32 :meth:`neighbours` returns for query i and base row j.
        The count runs first: more than ``max_edges`` edges raise ``ValueError`` before anything is allocated for them (a
        threshold of -1 on 262 144 rows is 3.4e10 edges).  :meth:`set_neighbour_split` sets the range of this search too; no
        result depends on it."""
        r = _sequence.neighbour_rows(rows, "rows")
        self._check_metric(metric)
        code = self._knn_metric(metric)
        n, t = len(r), float(threshold)
        csr = self._count_then_fill(
            lambda indptr, total: self.lib.gnn_graph_count(self.ctx, r.ctypes.data, n, t, code, indptr, total),
            lambda col, sim, m: self.lib.gnn_graph_fill(self.ctx, n, t, code, col, sim, m), n + 1, max_edges,
            lambda m: f"the graph has {m} edges at the threshold {float(np.float32(threshold)):g}")
        name = self._metric_name(metric)
        return GraphResult.build(csr, _sequence.valid_rows(r, name), np.float32(threshold), name)

    def graph_count_dev(self, rows_ptr: int, n: int, threshold, indptr_ptr: int, metric="cosine") -> int:
        """``gnn_graph_count_dev``: device pointers in (rows n x 512 f32) and out (indptr n + 1 int64); the engine's stream is
        synchronised once.  Returns the number of edges: what ``col`` and ``sim`` of :meth:`graph_fill_dev` must hold."""
        total = C.c_int64(0)
        check(self.lib.gnn_graph_count_dev(self.ctx, rows_ptr, int(n), float(threshold), self._knn_metric(metric), indptr_ptr,
                                           C.addressof(total)))
        return int(total.value)

    def graph_fill_dev(self, rows_ptr: int, n: int, threshold, col_ptr, sim_ptr, capacity: int, metric="cosine"):
        """Asynchronous (``gnn_graph_fill_dev``): the edges of the engine's last :meth:`graph_count_dev`, which must have had the
        same rows, n, threshold and metric - col (int32) and sim (f32) of ``capacity`` elements each on the device, enqueued on
        the engine's stream."""
        check(self.lib.gnn_graph_fill_dev(self.ctx, rows_ptr, int(n), float(threshold), self._knn_metric(metric), col_ptr, sim_ptr,
                                          int(capacity)))

    def graph_pass_ms(self):
        """measurement only (``gnn_debug_graph_pass_ms``): with profiling enabled, the HIP-event milliseconds of the last count call's
        [count pass, scan]"""
        return self._debug_ms(self.lib.gnn_debug_graph_pass_ms)

    # -- k-nearest-neighbour graph --------------------------------------------------------
    @staticmethod
    def _knn_graph_codes(k, mode, weight):
        """(k, mode code, weight code): an unknown name is a ``ValueError`` before anything is allocated or launched; a k outside
        [1, 64] is one too, with the value and the range"""
        return (_sequence.neighbour_k(k), _lib.KNN_GRAPH_MODES[_sequence.knn_graph_mode(mode)],
                _lib.KNN_GRAPH_WEIGHTS[_sequence.knn_graph_weight(weight)])

    def knn_graph(self, rows, k=15, mode="union", weight="similarity", metric="cosine") -> KNNGraphResult:
        """The k-nearest-neighbour graph among encoder embeddings (``gnn_knn_graph_count`` + ``gnn_knn_graph_fill``; the definition is
        ``sequence.knn_graph``): the lists of :meth:`neighbours`' self-search at ``k`` (1..64), joined on the device into the CSR
        :meth:`graph` returns - a pair i < j of valid rows is an edge when either lists the other (``mode`` "union") or both do
        ("mutual").  At most n k edges whatever the data, and a density that adapts per row: what a single threshold cannot give.
        ``weight`` "similarity": where j is among i's neighbours, the float32 :meth:`graph` gives the pair, bit for bit; otherwise
        the float32 row j's list holds for i - the other orientation, which may differ from the graph's value in the last bit.
        Negative similarities are kept; the consumers drop weights <= 0.  "jaccard": the overlap of the two neighbourhoods, each
        with its own row, |A & B| / |A | B| in (0, 1] - shared nearest neighbours.  The result's :meth:`~GraphResult.mcl`,
        :meth:`~GraphResult.spread`, :meth:`~GraphResult.average_linkage` and :meth:`~GraphResult.communities` run the consumers
        on it.  :meth:`set_neighbour_split` sets the range of this search too; no result depends on it."""
        r = _sequence.neighbour_rows(rows, "rows")
        self._check_metric(metric)
        k, m, w = self._knn_graph_codes(k, mode, weight)
        code = self._knn_metric(metric)
        n = len(r)
        flags = []

        def fill(col, sim, total):
            flags.append(np.empty(total, dtype=np.uint8))
            return self.lib.gnn_knn_graph_fill(self.ctx, n, k, m, w, code, col, sim, flags[0].ctypes.data, total)

        csr = self._count_then_fill(
            lambda indptr, total: self.lib.gnn_knn_graph_count(self.ctx, r.ctypes.data, n, k, m, w, code, indptr, total),
            fill, n + 1, n * k, lambda total: f"the graph has {total} edges")          # the cap cannot be met: at most n k edges
        name = self._metric_name(metric)
        return KNNGraphResult.build(csr + (flags[0],), _sequence.valid_rows(r, name), k, mode, weight, name)

    def knn_graph_count_dev(self, rows_ptr: int, n: int, indptr_ptr: int, k=15, mode="union", weight="similarity", metric="cosine") -> int:
        """``gnn_knn_graph_count_dev``: device pointers in (rows n x 512 f32) and out (indptr n + 1 int64); the engine's stream is
        synchronised.  Returns the number of edges: what ``col``, ``sim`` and ``mutual`` of :meth:`knn_graph_fill_dev` must hold."""
        k, m, w = self._knn_graph_codes(k, mode, weight)
        total = C.c_int64(0)
        check(self.lib.gnn_knn_graph_count_dev(self.ctx, rows_ptr, int(n), k, m, w, self._knn_metric(metric), indptr_ptr, C.addressof(total)))
        return int(total.value)

    def knn_graph_fill_dev(self, n: int, col_ptr, sim_ptr, mutual_ptr, capacity: int, k=15, mode="union", weight="similarity",
                           metric="cosine"):
        """Asynchronous (``gnn_knn_graph_fill_dev``): the edges of the engine's last :meth:`knn_graph_count_dev`, which must have had
        the same n, k, mode, weight and metric - col (int32), sim (f32) and mutual (uint8, or None) of ``capacity`` elements each on
        the device, enqueued on the engine's stream.  It reads the lists the count left in the engine, not the rows."""
        k, m, w = self._knn_graph_codes(k, mode, weight)
        check(self.lib.gnn_knn_graph_fill_dev(self.ctx, int(n), k, m, w, self._knn_metric(metric), col_ptr, sim_ptr, mutual_ptr, int(capacity)))

    def set_knn_graph_wave_rows(self, entries: int) -> int:
        """test aid (``gnn_debug_knn_graph_wave_rows``): the longest row one wave orders, 1..64 (the default 64); no result depends on
        it."""
        return self._knob(self.lib.gnn_debug_knn_graph_wave_rows, entries, answers_before=False)

    def set_knn_graph_group_rows(self, entries: int) -> int:
        """test aid (``gnn_debug_knn_graph_group_rows``): the longest row a workgroup orders in LDS, 1..4096 (the default 2048); no
        result depends on it."""
        return self._knob(self.lib.gnn_debug_knn_graph_group_rows, entries, answers_before=False)

    def knn_graph_classes(self) -> np.ndarray:
        """measurement only (``gnn_debug_knn_graph_classes``): the rows the last count gave the [LDS, radix] class"""
        out = np.zeros(2, dtype=np.int64)
        check(self.lib.gnn_debug_knn_graph_classes(self.ctx, out.ctypes.data))
        return out

    def knn_graph_pass_ms(self):
        """measurement only (``gnn_debug_knn_graph_ms``): with profiling enabled, the HIP-event milliseconds of the last count call's
        [search, lists, count, scan] and, behind them, of every fill's [fill, order, finish] since"""
        return self._debug_ms(self.lib.gnn_debug_knn_graph_ms)

    # -- matches against a reference -----------------------------------------------------
    def match(self, query, base, threshold, metric="cosine", max_edges=1 << 28) -> MatchResult:
        """Matches against a reference (``gnn_match_count`` + ``gnn_match_fill``; the definition is ``sequence.threshold_matches``):
        every pair of a valid row i of ``query`` (nq, 512) and a valid row j of ``base`` (nb, 512) whose similarity under ``metric``
        is >= ``threshold``, with that similarity - ALL the reference rows a query is within the threshold of, where
        :meth:`neighbours` stops at 64; exact, the passes of :meth:`graph` over the rectangle.  The similarity of the pair (i, j) is
        the float32 :meth:`neighbours` returns for query i and base row j; no pair is excluded.  The count runs first: more than
        ``max_edges`` matches raise ``ValueError`` before anything is allocated for them.  With :meth:`GraphResult.extend` it adds
        rows to a graph without computing old x old again.  :meth:`set_neighbour_split` sets the range of this search too; no
        result depends on it."""
        q = _sequence.neighbour_rows(query)
        b = _sequence.neighbour_rows(base, "base")
        self._check_metric(metric)
        code = self._knn_metric(metric)
        nq, nb, t = len(q), len(b), float(threshold)
        csr = self._count_then_fill(
            lambda indptr, total: self.lib.gnn_match_count(self.ctx, q.ctypes.data, nq, b.ctypes.data, nb, t, code, indptr, total),
            lambda col, sim, m: self.lib.gnn_match_fill(self.ctx, nq, nb, t, code, col, sim, m), nq + 1, max_edges,
            lambda m: f"there are {m} matches at the threshold {float(np.float32(threshold)):g}")
        name = self._metric_name(metric)
        return MatchResult.build(csr, _sequence.valid_rows(q, name), _sequence.valid_rows(b, name), np.float32(threshold), name)

    def match_count_dev(self, query_ptr: int, n_query: int, base_ptr: int, n_base: int, threshold, indptr_ptr: int, metric="cosine") -> int:
        """``gnn_match_count_dev``: device pointers in (query n_query x 512 f32, base n_base x 512 f32) and out (indptr n_query + 1
        int64); the engine's stream is synchronised once.  Returns the number of matches: what ``col`` and ``sim`` of
        :meth:`match_fill_dev` must hold."""
        total = C.c_int64(0)
        check(self.lib.gnn_match_count_dev(self.ctx, query_ptr, int(n_query), base_ptr, int(n_base), float(threshold),
                                           self._knn_metric(metric), indptr_ptr, C.addressof(total)))
        return int(total.value)

    def match_fill_dev(self, query_ptr: int, n_query: int, base_ptr: int, n_base: int, threshold, col_ptr, sim_ptr, capacity: int,
                       metric="cosine"):
        """Asynchronous (``gnn_match_fill_dev``): the matches of the engine's last :meth:`match_count_dev`, which must have had the
        same rows, sizes, threshold and metric - col (int32) and sim (f32) of ``capacity`` elements each on the device, enqueued on
        the engine's stream."""
        check(self.lib.gnn_match_fill_dev(self.ctx, query_ptr, int(n_query), base_ptr, int(n_base), float(threshold),
                                          self._knn_metric(metric), col_ptr, sim_ptr, int(capacity)))

    def match_pass_ms(self):
        """measurement only (``gnn_debug_match_pass_ms``): with profiling enabled, the HIP-event milliseconds of the last count call's
        [count pass, scan]"""
        return self._debug_ms(self.lib.gnn_debug_match_pass_ms)

    # -- label transfer ------------------------------------------------------------------
    def vote(self, query, base, label, n_classes, threshold) -> VoteResult:
        """Label transfer among encoder embeddings (``gnn_vote``; the definition is ``sequence.class_votes``): for every valid row i
        of ``query`` (nq, 512) and every class c, the voters - the valid rows j of ``base`` (nb, 512) with ``label[j]`` == c whose
        cosine similarity to i is >= ``threshold`` - counted, their similarities summed as integers in units of 2^-32, and the most
        similar one named: n_query x n_classes numbers where :meth:`match` would write every edge.  ``label``: int64 per base row
        in [0, ``n_classes``), or -1 for an unlabelled row, which is ignored; 1 <= ``n_classes`` <= 1024.  ``base=None``: the rows
        vote among themselves, ``label`` runs over them and the pair (i, i) is left out - leave-one-out over a labelled set.  The
        similarity of the pair (i, j) is the float32 :meth:`neighbours` and :meth:`match` return for it, and the sums are integer
        sums: no bit of the result depends on the order of execution, and a permutation of the base with its labels changes no
        bit of ``count``, ``weight`` or ``nearest_sim``.  Not a top-k vote, not the dot metric, not approximate, no calibrated
        probability.  :meth:`set_neighbour_split` sets the range of this search too; no result depends on it."""
        q = _sequence.neighbour_rows(query)
        b = None if base is None else _sequence.neighbour_rows(base, "base")
        nc = _sequence.vote_classes(n_classes)
        thr = _sequence.cluster_threshold(threshold)
        lab = _sequence.vote_labels(label, len(q) if b is None else len(b), nc)
        shape = (len(q), nc)
        count, weight, nearest = (np.empty(shape, dtype=np.int64) for _ in range(3))
        nearest_sim = np.empty(shape, dtype=np.float32)
        check(self.lib.gnn_vote(self.ctx, q.ctypes.data, len(q), None if b is None else b.ctypes.data, 0 if b is None else len(b),
                                lab.ctypes.data, nc, float(thr), count.ctypes.data, weight.ctypes.data, nearest.ctypes.data,
                                nearest_sim.ctypes.data))
        return VoteResult.build((count, weight, nearest, nearest_sim), _sequence.valid_rows(q), nc, thr)

    def vote_dev(self, query_ptr: int, n_query: int, base_ptr, n_base: int, label_ptr: int, n_classes: int, threshold, count_ptr: int,
                 weight_ptr: int, nearest_ptr: int, nearest_sim_ptr: int):
        """``gnn_vote_dev``: device pointers in (query n_query x 512 f32; base n_base x 512 f32, or None for the self form; label
        int64 per base row) and out (count, weight, nearest: n_query x n_classes int64 each; nearest_sim: the same in f32); the
        engine's stream is synchronised once (the labels' verdict), the rest is enqueued on it."""
        check(self.lib.gnn_vote_dev(self.ctx, query_ptr, int(n_query), base_ptr, int(n_base), label_ptr, int(n_classes), float(threshold),
                                    count_ptr, weight_ptr, nearest_ptr, nearest_sim_ptr))

    def set_vote_lds(self, max_classes: int):
        """test aid (``gnn_debug_set_vote_lds``): up to ``max_classes`` (0..16, the default) classes a workgroup of :meth:`vote` adds
        in LDS before it adds to memory; no result depends on it."""
        check(self.lib.gnn_debug_set_vote_lds(self.ctx, int(max_classes)))

    def vote_pass_ms(self):
        """measurement only (``gnn_debug_vote_pass_ms``): with profiling enabled, the HIP-event milliseconds of the last
        :meth:`vote` / :meth:`vote_dev` call - [labels, then per slab of 262 144 queries: votes, finish]"""
        return self._debug_ms(self.lib.gnn_debug_vote_pass_ms)

    # -- the similarity graph's consumers ---------------------------------------------------
    @staticmethod
    def _csr_arrays(indptr, col, sim, valid):
        """the graph as the library takes it: (indptr, col, sim, valid as uint8 or None, n); a ``ValueError`` for arrays that are no CSR"""
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        col = np.ascontiguousarray(col, dtype=np.int32)
        with np.errstate(over="ignore"):
            sim = np.ascontiguousarray(sim, dtype=np.float32)
        n = len(indptr) - 1
        if indptr.ndim != 1 or n < 0 or col.ndim != 1 or sim.shape != col.shape:
            raise ValueError("indptr (n + 1,), col (nnz,) and sim (nnz,) are required")
        ok = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
        if ok is not None and ok.shape != (n,):
            raise ValueError(f"valid must have one entry per row ({n})")
        return indptr, col, sim, ok, n

    def _knob(self, fn, value, answers_before=True) -> int:
        """a debug knob's setter: ``GnnError`` for a value out of range.  Returns what the library answers, the value before the call,
        or - where it answers ``GNN_OK`` - the value set."""
        rc = fn(self.ctx, int(value))
        if rc < 0:
            check(rc)
        return int(rc) if answers_before else int(value)

    # -- Markov clusters -----------------------------------------------------------------
    @staticmethod
    def _mcl_params(inflation, select, precision, max_iter):
        """the four knobs as the library takes them; a ``ValueError`` for one out of range, before anything is allocated"""
        return (_sequence.mcl_inflation(inflation), _sequence._whole(select, "select", 1, _sequence.MCL_SELECT_MAX),
                _sequence._whole(precision, "precision", 1, _sequence.MCL_PRECISION_MAX),
                _sequence._whole(max_iter, "max_iter", 0, _sequence.MCL_MAX_ITER_MAX))

    def _mcl_call(self, fn, graph, n, nnz, knobs, outs, inflation):
        changed = np.zeros(knobs[3], dtype=np.int64)
        iterations, converged = C.c_int64(0), C.c_int(0)
        self._mcl_serial += 1
        check(fn(self.ctx, *graph, int(n), int(nnz), *knobs, *outs, changed.ctypes.data, C.addressof(iterations), C.addressof(converged)))
        return dict(iterations=int(iterations.value), converged=bool(converged.value), changed=changed[:iterations.value], n=int(n),
                    inflation=float(inflation), select=knobs[1], precision=knobs[2], engine=self, serial=self._mcl_serial)

    def mcl(self, indptr, col, sim, valid=None, inflation=2.0, select=256, precision=10000, max_iter=100) -> MCLResult:
        """Markov clusters of a similarity graph (``gnn_mcl``; the definition is ``sequence.markov_clusters``): van Dongen's MCL of
        the upper-triangle CSR (``indptr``, ``col``, ``sim``) :meth:`graph` returns - flow-based families that survive a few bridge
        edges, with one knob, the ``inflation`` (a multiple of 0.25 in [1.25, 8]; larger: smaller clusters).  In integers throughout:
        every output equals the definition bit for bit.  ``valid``: bool per row (None: all); ``select`` (1..1024): the entries a
        column keeps at the most; ``precision`` (1..2^20): an entry below 1 / precision of its column is cut; ``max_iter`` (0..10000).
        ``ValueError`` for a knob out of range, ``GnnError`` for a graph that is no such CSR."""
        knobs = self._mcl_params(inflation, select, precision, max_iter)
        indptr, col, sim, ok, n = self._csr_arrays(indptr, col, sim, valid)
        out = [np.empty(n, dtype=np.int64) for _ in range(3)] + [np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint8)]
        kw = self._mcl_call(self.lib.gnn_mcl, (indptr.ctypes.data, col.ctypes.data, sim.ctypes.data, None if ok is None else ok.ctypes.data),
                            n, len(col), knobs, [a.ctypes.data for a in out], inflation)
        out[4] = out[4].astype(bool)
        return MCLResult(**dict(zip(_sequence.MCL_FIELDS, out)), **kw)

    def mcl_dev(self, indptr_ptr: int, col_ptr, sim_ptr, n: int, nnz: int, label_ptr: int, size_ptr: int, attractor_ptr: int, flow_ptr: int,
                is_attractor_ptr: int, valid_ptr=None, inflation=2.0, select=256, precision=10000, max_iter=100) -> MCLResult:
        """``gnn_mcl_dev``: device pointers in - indptr (n + 1 int64), col (nnz int32) and sim (nnz f32) exactly as
        :meth:`graph_count_dev` and :meth:`graph_fill_dev` wrote them, valid (n uint8, or None) - and out (label, size, attractor: n
        int64 each; flow: n uint32; is_attractor: n uint8); the engine's stream is synchronised once per iteration.  Returns an
        :class:`MCLResult` without the per-row arrays."""
        knobs = self._mcl_params(inflation, select, precision, max_iter)
        return MCLResult(**self._mcl_call(self.lib.gnn_mcl_dev, (indptr_ptr, col_ptr, sim_ptr, valid_ptr), n, nnz, knobs,
                                          [label_ptr, size_ptr, attractor_ptr, flow_ptr, is_attractor_ptr], inflation))

    def _mcl_matrix(self, n, select, serial):
        if serial != self._mcl_serial:
            raise GnnError("the engine has run another Markov clustering since: its matrix is gone")
        length = np.zeros(n, dtype=np.int32)
        idx, val = np.zeros((n, select), dtype=np.int32), np.zeros((n, select), dtype=np.uint32)
        check(self.lib.gnn_mcl_matrix(self.ctx, int(n), int(select), length.ctypes.data, idx.ctypes.data, val.ctypes.data))
        keep = np.arange(select)[None, :] < length[:, None]
        return length.astype(np.int64), idx[keep], val[keep]

    def set_mcl_lds(self, slots: int) -> int:
        """test aid (``gnn_debug_mcl_lds``): the slots (0..4096, the default) of the LDS table :meth:`mcl` sums a column's products in
        - a column that needs more takes the overflow path, with 0 every column; -1 changes nothing.  Returns the value before the
        call.  No result depends on it."""
        before = self.lib.gnn_debug_mcl_lds(self.ctx, int(slots))
        if before < 0:
            check(before)
        return int(before)

    def set_mcl_groups(self, groups: int):
        """test aid (``gnn_debug_mcl_groups``): the workgroups of a pass of :meth:`mcl` (0: the library's choice); no result depends
        on it."""
        check(self.lib.gnn_debug_mcl_groups(self.ctx, int(groups)))

    def mcl_pow(self, u, inflation) -> np.ndarray:
        """test aid (``gnn_debug_mcl_pow``): the device's integer power over ``u`` (m,) uint64 <= 2^30: uint64 (m,) of u ^ inflation
        in 2^-30 fixed point, by the function the passes of :meth:`mcl` call"""
        a4 = _sequence.mcl_inflation(inflation)
        u = np.ascontiguousarray(u, dtype=np.uint64)
        if u.ndim != 1:
            raise ValueError("u (m,) uint64 is required")
        out = np.empty(len(u), dtype=np.uint64)
        check(self.lib.gnn_debug_mcl_pow(self.ctx, u.ctypes.data, len(u), a4, out.ctypes.data))
        return out

    def mcl_pass_ms(self):
        """measurement only (``gnn_debug_mcl_ms``): with profiling enabled, the HIP-event milliseconds of the last :meth:`mcl` /
        :meth:`mcl_dev` call - [validate and symmetrise, the initial matrix, then every iteration]"""
        return self._debug_ms(self.lib.gnn_debug_mcl_ms)

    def mcl_overflow(self) -> np.ndarray:
        """measurement only (``gnn_debug_mcl_overflow``): the columns that took the overflow path in the last :meth:`mcl` /
        :meth:`mcl_dev` call - int64 [the initial matrix, then every iteration]"""
        return self._debug_ms(self.lib.gnn_debug_mcl_overflow, np.int64)

    # -- t-SNE layout --------------------------------------------------------------------
    @staticmethod
    def _tsne_init(init, n):
        with np.errstate(over="ignore"):
            y = np.ascontiguousarray(init, dtype=np.float32)
        if y.shape != (n, 2):
            raise ValueError(f"the layout must be ({n}, 2)")
        return y

    def tsne(self, indptr, col, sim, init, valid=None, n_iter=750, exaggeration_iter=250, exaggeration=12.0, learning_rate=None) -> TSNEResult:
        """The exact t-SNE layout of a similarity graph (``gnn_tsne``; the definition is ``sequence.tsne_layout``): a 2-D picture of
        the upper-triangle CSR (``indptr``, ``col``, ``sim``) :meth:`graph` / :meth:`knn_graph` return, from ``init`` (float32 (n, 2),
        finite at every valid row).  The affinities are the graph's own weights, the repulsion the exact all-pairs pass; every output
        equals the definition bit for bit, whatever the grid.  ``valid``: bool per row (None: all); ``n_iter`` (0..100000) iterations,
        the first ``exaggeration_iter`` with the attraction times ``exaggeration`` (1..1024) and momentum 0.5, the others with
        momentum 0.8; ``learning_rate`` None: max(n_valid / exaggeration / 4, 50).  ``ValueError`` for a knob out of range,
        ``GnnError`` for a graph that is no such CSR, more than 2^21 rows or an init that is not finite.  Not Barnes-Hut, not
        perplexity-calibrated, not UMAP; n^2 pairs per iteration."""
        indptr, col, sim, ok, n = self._csr_arrays(indptr, col, sim, valid)
        y = self._tsne_init(init, n)
        n_valid = n if ok is None else int(np.count_nonzero(ok))
        n_iter, ex_iter, e, lr = _sequence.tsne_params(n_iter, exaggeration_iter, exaggeration, learning_rate, n_valid)
        layout, z_trace, valid_out = np.empty((n, 2), dtype=np.float32), np.empty(n_iter + 1, dtype=np.uint64), np.empty(n, dtype=np.uint8)
        check(self.lib.gnn_tsne(self.ctx, indptr.ctypes.data, col.ctypes.data, sim.ctypes.data, None if ok is None else ok.ctypes.data, n, len(col),
                                y.ctypes.data, n_iter, ex_iter, e, float(lr), layout.ctypes.data, z_trace.ctypes.data, valid_out.ctypes.data))
        valid_out = valid_out.astype(bool)
        kl = _sequence.tsne_kl(indptr, col, sim, layout, z_trace[-1], valid_out)
        return TSNEResult(layout=layout, z_trace=z_trace, kl_divergence=kl, iterations=n_iter, valid=valid_out, n=n, exaggeration_iter=ex_iter,
                          exaggeration=e, learning_rate=float(lr))

    def tsne_dev(self, indptr_ptr: int, col_ptr, sim_ptr, n: int, nnz: int, init_ptr: int, layout_ptr: int, z_trace_ptr: int, valid_out_ptr: int,
                 valid_ptr=None, n_valid=None, n_iter=750, exaggeration_iter=250, exaggeration=12.0, learning_rate=None) -> TSNEResult:
        """``gnn_tsne_dev``: device pointers in - indptr (n + 1 int64), col (nnz int32) and sim (nnz f32) exactly as the graph's fill
        wrote them, valid (n uint8, or None), init (n x 2 f32) - and out (layout: n x 2 f32; z_trace: n_iter + 1 uint64; valid_out: n
        uint8); the engine's stream is synchronised once, before the loop is enqueued.  ``n_valid`` (None: n) is what the default
        ``learning_rate`` counts.  Returns a :class:`TSNEResult` without the arrays."""
        n_iter, ex_iter, e, lr = _sequence.tsne_params(n_iter, exaggeration_iter, exaggeration, learning_rate, int(n if n_valid is None else n_valid))
        check(self.lib.gnn_tsne_dev(self.ctx, indptr_ptr, col_ptr, sim_ptr, valid_ptr, int(n), int(nnz), init_ptr, n_iter, ex_iter, e, float(lr),
                                    layout_ptr, z_trace_ptr, valid_out_ptr))
        return TSNEResult(layout=None, z_trace=None, kl_divergence=None, iterations=n_iter, valid=None, n=int(n), exaggeration_iter=ex_iter,
                          exaggeration=e, learning_rate=float(lr))

    def tsne_forces(self, indptr, col, sim, y, valid=None) -> dict:
        """One evaluation of the layout's forces at ``y`` (float32 (n, 2)) (``gnn_tsne_forces``; the definition is
        ``sequence.tsne_forces`` over ``sequence.tsne_affinities``): a dict of int64 (n,) ``zi``, ``rx``, ``ry`` (the repulsion's
        sums in units of 2^-20 and 2^-32), ``ax``, ``ay`` (the attraction's, 2^-32) and ``m2`` (the integer sum of the weights) -
        what every iteration of :meth:`tsne` computes, by the same kernels."""
        indptr, col, sim, ok, n = self._csr_arrays(indptr, col, sim, valid)
        y = self._tsne_init(y, n)
        out = {k: np.zeros(n, dtype=np.int64) for k in ("zi", "rx", "ry", "ax", "ay")}
        m2 = C.c_int64(0)
        check(self.lib.gnn_tsne_forces(self.ctx, indptr.ctypes.data, col.ctypes.data, sim.ctypes.data, None if ok is None else ok.ctypes.data, n,
                                       len(col), y.ctypes.data, *(a.ctypes.data for a in out.values()), C.addressof(m2)))
        out["m2"] = int(m2.value)
        return out

    def tsne_rows(self, rows, k=15, mode="union", weight="similarity", **kw) -> TSNEResult:
        """The chain in one call: :meth:`knn_graph` of ``rows`` (n, 512) with ``k``, ``mode`` and ``weight``, :meth:`pca` onto two
        components scaled so that the first has standard deviation 1e-4 over the valid rows as the init (0 at an invalid row), then
        :meth:`tsne` with ``**kw``."""
        g = self.knn_graph(rows, k, mode, weight)
        return g.tsne(self, init=self.tsne_pca_init(rows), **kw)

    def tsne_pca_init(self, rows) -> np.ndarray:
        """float32 (n, 2): the rows' scores on their first two principal components (:meth:`pca`), scaled in float64 so that the first
        has standard deviation 1e-4 over the valid rows; 0 at an invalid row, and everywhere when that deviation is 0"""
        res = self.pca(rows, 2)
        proj = np.where(res.valid[:, None], res.projection, 0).astype(np.float64)
        sd = float(proj[res.valid, 0].std()) if res.valid.any() else 0.0
        return (proj * (1e-4 / sd) if sd > 0 else np.zeros_like(proj)).astype(np.float32)

    def set_tsne_split(self, splits: int):
        """test aid (``gnn_debug_tsne_split``): the workgroups the repel pass of :meth:`tsne` splits the columns over, at granule
        boundaries (0: the library's choice); no result depends on it."""
        check(self.lib.gnn_debug_tsne_split(self.ctx, int(splits)))

    def tsne_pass_ms(self):
        """measurement only (``gnn_debug_tsne_ms``): with profiling enabled, the HIP-event milliseconds of the last :meth:`tsne` /
        :meth:`tsne_dev` call - [validate, symmetrise and affinities; the whole loop; the final Z and the results]"""
        return self._debug_ms(self.lib.gnn_debug_tsne_ms)

    # -- label spreading -----------------------------------------------------------------
    def _spread_call(self, fn, graph, n, nnz, knobs, outs, alpha):
        nc, a, clamp, max_iter = knobs
        changed = np.zeros(max_iter, dtype=np.int64)
        iterations, converged = C.c_int64(0), C.c_int(0)
        check(fn(self.ctx, *graph, int(n), int(nnz), nc, a, int(clamp), max_iter, *outs, changed.ctypes.data, C.addressof(iterations),
                 C.addressof(converged)))
        return dict(iterations=int(iterations.value), converged=bool(converged.value), changed=changed[:iterations.value], n=int(n),
                    n_classes=nc, alpha=float(alpha), clamp=bool(clamp))

    @staticmethod
    def _spread_params(n_classes, alpha, clamp, max_iter):
        """the knobs as the library takes them; a ``ValueError`` for one out of range, before anything is allocated"""
        return (_sequence.vote_classes(n_classes), _sequence.spread_alpha(alpha), bool(clamp),
                _sequence._whole(max_iter, "max_iter", 1, _sequence.SPREAD_MAX_ITER_MAX))

    def spread(self, indptr, col, sim, label, n_classes, valid=None, alpha=0.5, clamp=True, max_iter=200, scores=True) -> SpreadResult:
        """Label spreading over a similarity graph (``gnn_spread``; the definition is ``sequence.label_spread``): the labels of the
        seed rows - ``label`` int64 per row in [-1, ``n_classes``), -1: unlabelled - spread along the edges of the upper-triangle CSR
        (``indptr``, ``col``, ``sim``) :meth:`graph` returns until nothing changes: a row gets a class through any number of
        unlabelled rows, where :meth:`vote` crosses one edge.  ``alpha``: a multiple of 1/64 in (0, 1), the share a row takes from
        its neighbours; ``clamp``: a seed keeps its label's full score; ``max_iter`` (1..10000); ``scores=False``: the n x n_classes
        matrix is not copied back (``score`` is None).  In integers throughout: every output equals the definition bit for bit.
        Random-walk rows, not the symmetric normalisation; no calibrated probability.  ``ValueError`` for a knob out of range,
        ``GnnError`` for a graph that is no such CSR."""
        knobs = self._spread_params(n_classes, alpha, clamp, max_iter)
        indptr, col, sim, ok, n = self._csr_arrays(indptr, col, sim, valid)
        lab = _sequence.vote_labels(label, n, knobs[0])
        score = np.empty((n, knobs[0]), dtype=np.uint32) if scores else None
        out = [np.empty(n, dtype=np.int32), np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint64),
               np.empty(n, dtype=np.int32)]
        kw = self._spread_call(self.lib.gnn_spread, (indptr.ctypes.data, col.ctypes.data, sim.ctypes.data, None if ok is None else ok.ctypes.data,
                                                     lab.ctypes.data), n, len(col), knobs,
                               [None if score is None else score.ctypes.data] + [a.ctypes.data for a in out], alpha)
        seed = (lab >= 0) & (np.ones(n, dtype=bool) if ok is None else ok.astype(bool))
        return SpreadResult(score=score, **dict(zip(_sequence.SPREAD_FIELDS[1:], out)), seed=seed, **kw)

    def spread_dev(self, indptr_ptr: int, col_ptr, sim_ptr, label_ptr: int, n: int, nnz: int, n_classes: int, best_ptr: int, best_score_ptr: int,
                   second_score_ptr: int, total_ptr: int, first_ptr: int, score_ptr=None, valid_ptr=None, alpha=0.5, clamp=True,
                   max_iter=200) -> SpreadResult:
        """``gnn_spread_dev``: device pointers in - indptr (n + 1 int64), col (nnz int32) and sim (nnz f32) exactly as
        :meth:`graph_count_dev` and :meth:`graph_fill_dev` wrote them, label (n int64), valid (n uint8, or None) - and out (best,
        first: n int32; best_score, second_score: n uint32; total: n uint64; score: n x n_classes uint32, or None); the engine's
        stream is synchronised once per iteration.  Returns a :class:`SpreadResult` without the per-row arrays."""
        knobs = self._spread_params(n_classes, alpha, clamp, max_iter)
        return SpreadResult(**self._spread_call(self.lib.gnn_spread_dev, (indptr_ptr, col_ptr, sim_ptr, valid_ptr, label_ptr), n, nnz, knobs,
                                                [score_ptr, best_ptr, best_score_ptr, second_score_ptr, total_ptr, first_ptr], alpha))

    def set_spread_groups(self, groups: int):
        """test aid (``gnn_debug_spread_groups``): the workgroups of an iteration of :meth:`spread` (0: the library's choice); no
        result depends on it."""
        check(self.lib.gnn_debug_spread_groups(self.ctx, int(groups)))

    def set_spread_skip(self, on: bool):
        """test aid (``gnn_debug_spread_skip``): the dirty-row rule of :meth:`spread` - a row none of whose neighbours changed is not
        computed again - on (the default) or off; no result depends on it."""
        check(self.lib.gnn_debug_spread_skip(self.ctx, int(bool(on))))

    def spread_pass_ms(self):
        """measurement only (``gnn_debug_spread_ms``): with profiling enabled, the HIP-event milliseconds of the last :meth:`spread`
        / :meth:`spread_dev` call - [validate and symmetrise, then every iteration]"""
        return self._debug_ms(self.lib.gnn_debug_spread_ms)

    # -- average linkage -----------------------------------------------------------------
    @staticmethod
    def _avglink_params(stop, max_rounds):
        """the knobs as the library takes them; a ``ValueError`` for one out of range, before anything is allocated"""
        return (_sequence.average_linkage_stop(stop), _sequence._whole(max_rounds, "max_rounds", 1, _sequence.AVGLINK_MAX_ROUNDS_MAX))

    def _avglink_call(self, fn, graph, n, nnz, knobs, outs):
        stop_q, max_rounds = knobs
        merged = np.zeros(min(max_rounds, int(n) + 1), dtype=np.int64)      # a round that is not the last merges a pair
        rounds, complete = C.c_int64(0), C.c_int(0)
        check(fn(self.ctx, *graph, int(n), int(nnz), stop_q, max_rounds, *outs, merged.ctypes.data, C.addressof(rounds), C.addressof(complete)))
        return dict(rounds=int(rounds.value), complete=bool(complete.value), merged_per_round=merged[:rounds.value], n=int(n),
                    stop=stop_q / _sequence.MCL_W)

    def average_linkage(self, indptr, col, sim, valid=None, stop=_sequence.AVGLINK_STOP_DEFAULT,
                        max_rounds=_sequence.AVGLINK_MAX_ROUNDS_MAX) -> AverageLinkageResult:
        """Average linkage over a similarity graph (``gnn_avglink``; the definition is ``sequence.average_linkage``): the UPGMA tree
        of the upper-triangle CSR (``indptr``, ``col``, ``sim``) :meth:`graph` returns, by rounds of reciprocal best pairs - two
        groups merge by their *mean* similarity, so one bridge pair chains nothing, there is no knob to guess, and the tree answers
        every cut level at once (:meth:`AverageLinkageResult.cut`).  A pair of rows without an entry counts as similarity 0.
        ``stop``: a similarity in (0, 64), the smallest average that still merges; ``max_rounds`` (1..2^20).  In integers throughout:
        every output equals the definition bit for bit.  ``ValueError`` for a knob out of range, ``GnnError`` for a graph that is
        no such CSR."""
        knobs = self._avglink_params(stop, max_rounds)
        indptr, col, sim, ok, n = self._csr_arrays(indptr, col, sim, valid)
        parent, weight = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.uint64)
        size_a, size_b, rnd = (np.empty(n, dtype=np.int32) for _ in range(3))
        kw = self._avglink_call(self.lib.gnn_avglink, (indptr.ctypes.data, col.ctypes.data, sim.ctypes.data, None if ok is None else ok.ctypes.data),
                                n, len(col), knobs, [a.ctypes.data for a in (parent, weight, size_a, size_b, rnd)])
        b = np.flatnonzero(parent >= 0)                   # the host's part: the per-node records as the ordered merge list
        merges = _sequence.average_linkage_order(parent[b], b, weight[b], size_a[b], size_b[b], rnd[b])
        return AverageLinkageResult(**merges, valid=np.ones(n, dtype=bool) if ok is None else ok.astype(bool), **kw)

    def average_linkage_dev(self, indptr_ptr: int, col_ptr, sim_ptr, n: int, nnz: int, parent_ptr: int, weight_ptr: int, size_a_ptr: int,
                            size_b_ptr: int, round_ptr: int, valid_ptr=None, stop=_sequence.AVGLINK_STOP_DEFAULT,
                            max_rounds=_sequence.AVGLINK_MAX_ROUNDS_MAX) -> AverageLinkageResult:
        """``gnn_avglink_dev``: device pointers in - indptr (n + 1 int64), col (nnz int32) and sim (nnz f32) exactly as
        :meth:`graph_count_dev` and :meth:`graph_fill_dev` wrote them, valid (n uint8, or None) - and out, per node, written where
        the node was absorbed (parent: n int32, -1 for a node never absorbed; weight: n uint64; size_a, size_b, round: n int32); the
        engine's stream is synchronised once per round.  Returns an :class:`AverageLinkageResult` without the per-merge arrays."""
        knobs = self._avglink_params(stop, max_rounds)
        return AverageLinkageResult(**self._avglink_call(self.lib.gnn_avglink_dev, (indptr_ptr, col_ptr, sim_ptr, valid_ptr), n, nnz, knobs,
                                                         [parent_ptr, weight_ptr, size_a_ptr, size_b_ptr, round_ptr]))

    def set_average_linkage_slots(self, slots: int) -> int:
        """test aid (``gnn_debug_avglink_slots``): the slots (0..4096, the default) of the LDS table :meth:`average_linkage` sums a
        row's entries in - a row with more entries takes the accumulator in global memory, with 0 every row; -1 changes nothing.
        Returns the value before the call.  No result depends on it."""
        return self._knob(self.lib.gnn_debug_avglink_slots, slots)

    def set_average_linkage_wave_rows(self, entries: int) -> int:
        """test aid (``gnn_debug_avglink_wave_rows``): the longest upper bound (0..4096; the default is 256) of a row that one wave
        of :meth:`average_linkage` takes with its quarter of the table; 0: none; -1 changes nothing.  Returns the value before the
        call.  No result depends on it."""
        return self._knob(self.lib.gnn_debug_avglink_wave_rows, entries)

    def set_average_linkage_groups(self, groups: int):
        """test aid (``gnn_debug_avglink_groups``): the workgroups of a contraction of :meth:`average_linkage` (0: the library's
        choice); no result depends on it."""
        check(self.lib.gnn_debug_avglink_groups(self.ctx, int(groups)))

    def average_linkage_order(self, quads) -> np.ndarray:
        """test aid (``gnn_debug_avglink_order``): the device's order function over ``quads`` (m, 4) uint64 = (s1, d1, s2, d2):
        int32 (m,) of -1 / 0 / 1 as s1 / d1 is below, equal to or above s2 / d2"""
        quads = np.ascontiguousarray(quads, dtype=np.uint64)
        if quads.ndim != 2 or quads.shape[1] != 4:
            raise ValueError("quads (m, 4) uint64 is required")
        out = np.empty(len(quads), dtype=np.int32)
        check(self.lib.gnn_debug_avglink_order(self.ctx, quads.ctypes.data, len(quads), out.ctypes.data))
        return out

    def average_linkage_pass_ms(self):
        """measurement only (``gnn_debug_avglink_ms``): with profiling enabled, the HIP-event milliseconds of the last
        :meth:`average_linkage` / :meth:`average_linkage_dev` call - [validate and symmetrise, then every round]"""
        return self._debug_ms(self.lib.gnn_debug_avglink_ms)

    def average_linkage_classes(self) -> np.ndarray:
        """measurement only (``gnn_debug_avglink_classes``): the rows the contractions of the last call took by class, all rounds
        together - int64 [one wave, one workgroup, the accumulator in global memory]"""
        out = np.zeros(3, dtype=np.int64)
        check(self.lib.gnn_debug_avglink_classes(self.ctx, out.ctypes.data))
        return out

    # -- modularity communities ------------------------------------------------------------
    @staticmethod
    def _communities_params(resolution, max_levels, max_sweeps):
        """the knobs as the library takes them; a ``ValueError`` for one out of range, before anything is allocated"""
        return (_sequence.communities_resolution(resolution), _sequence._whole(max_levels, "max_levels", 1, _sequence.COMM_LEVELS_MAX),
                _sequence._whole(max_sweeps, "max_sweeps", 1, _sequence.COMM_SWEEPS_MAX))

    def _communities_call(self, fn, graph, n, nnz, knobs, outs):
        r, max_levels, max_sweeps = knobs
        stats = np.zeros((max_levels, len(_sequence.COMM_LEVEL_FIELDS)), dtype=np.int64)
        words = np.zeros((max_levels, 2), dtype=np.uint64)
        levels, complete, m2 = C.c_int64(0), C.c_int(0), C.c_uint64(0)
        check(fn(self.ctx, *graph, int(n), int(nnz), r, max_levels, max_sweeps, *outs, stats.ctypes.data, words.ctypes.data,
                 C.addressof(levels), C.addressof(complete), C.addressof(m2)))
        lv, m2 = int(levels.value), int(m2.value)
        qnum = [((int(hi) << 64) | int(lo)) - ((1 << 128) if int(hi) >> 63 else 0) for lo, hi in words[:lv]]
        from fractions import Fraction
        out = {f: stats[:lv, k].copy() for k, f in enumerate(_sequence.COMM_LEVEL_FIELDS)}
        out.update(qnum=qnum, qnum_words=words[:lv].copy(), levels=lv, complete=bool(complete.value), m2=m2, resolution=r / _sequence.COMM_R_ONE,
                   modularity=float(Fraction(qnum[-1], 64 * m2 * m2)) if qnum else 0.0, n=int(n))
        return out

    def communities(self, indptr, col, sim, valid=None, resolution=1.0, max_levels=_sequence.COMM_LEVELS_MAX,
                    max_sweeps=_sequence.COMM_SWEEPS_MAX) -> CommunityResult:
        """Modularity communities of a similarity graph (``gnn_communities``; the definition is
        ``sequence.modularity_communities``): Louvain's levels over the upper-triangle CSR (``indptr``, ``col``, ``sim``)
        :meth:`graph` returns - a partition that scores itself (``modularity``), with one knob that has a natural default
        (``resolution`` 1, a multiple of 1/64 in [1/64, 4]) and a coarse-to-fine hierarchy (``level_label``).  ``max_levels`` (1..32),
        ``max_sweeps`` per level (1..2^20).  In integers throughout: every output equals the definition bit for bit.  Every community
        is connected (the split at a level's end), which is not Leiden's refinement: well-connectedness is not guaranteed.
        ``ValueError`` for a knob out of range, ``GnnError`` for a graph that is no such CSR or whose doubled weight reaches 2^58."""
        knobs = self._communities_params(resolution, max_levels, max_sweeps)
        indptr, col, sim, ok, n = self._csr_arrays(indptr, col, sim, valid)
        label, size = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
        level_label = np.empty((knobs[1], n), dtype=np.int64)
        kw = self._communities_call(self.lib.gnn_communities,
                                    (indptr.ctypes.data, col.ctypes.data, sim.ctypes.data, None if ok is None else ok.ctypes.data), n, len(col),
                                    knobs, [a.ctypes.data for a in (label, size, level_label)])
        return CommunityResult(label=label, size=size, level_label=level_label[:kw["levels"]].copy(),
                               valid=np.ones(n, dtype=bool) if ok is None else ok.astype(bool), **kw)

    def communities_dev(self, indptr_ptr: int, col_ptr, sim_ptr, n: int, nnz: int, label_ptr: int, size_ptr: int, level_label_ptr: int,
                        valid_ptr=None, resolution=1.0, max_levels=_sequence.COMM_LEVELS_MAX,
                        max_sweeps=_sequence.COMM_SWEEPS_MAX) -> CommunityResult:
        """``gnn_communities_dev``: device pointers in - indptr (n + 1 int64), col (nnz int32) and sim (nnz f32) exactly as
        :meth:`graph_count_dev` and :meth:`graph_fill_dev` wrote them, valid (n uint8, or None) - and out: label and size (n int64
        each) and level_label (``max_levels`` x n int64, of which the first ``levels`` rows are written); the engine's stream is
        synchronised once per sweep.  Returns a :class:`CommunityResult` without the per-row arrays."""
        knobs = self._communities_params(resolution, max_levels, max_sweeps)
        return CommunityResult(**self._communities_call(self.lib.gnn_communities_dev, (indptr_ptr, col_ptr, sim_ptr, valid_ptr), n, nnz, knobs,
                                                        [label_ptr, size_ptr, level_label_ptr]))

    def label_components(self, indptr, col, sim, label, valid=None) -> np.ndarray:
        """``gnn_label_components`` (the definition is ``sequence.label_components``): for any labelling of the rows (int64, -1:
        none) the connected components of every label's induced subgraph over the graph's existing entries - int64 per row, the
        smallest row of its component; -1 for label -1 and for an invalid row."""
        indptr, col, sim, ok, n = self._csr_arrays(indptr, col, sim, valid)
        label = np.asarray(label)
        if label.shape != (n,) or label.dtype.kind not in "iu" or (label < -1).any():
            raise ValueError(f"label must be an integer array of {n} with values >= -1")
        label = np.ascontiguousarray(label, dtype=np.int64)
        out = np.empty(n, dtype=np.int64)
        check(self.lib.gnn_label_components(self.ctx, indptr.ctypes.data, col.ctypes.data, sim.ctypes.data, None if ok is None else ok.ctypes.data,
                                            n, len(col), label.ctypes.data, out.ctypes.data))
        return out

    def label_components_dev(self, indptr_ptr: int, col_ptr, sim_ptr, n: int, nnz: int, label_ptr: int, out_ptr: int, valid_ptr=None):
        """``gnn_label_components_dev``: device pointers in (the graph as :meth:`graph_fill_dev` wrote it, label: n int64) and out
        (n int64); enqueued on the engine's stream behind one synchronise for the verdict on the graph."""
        check(self.lib.gnn_label_components_dev(self.ctx, indptr_ptr, col_ptr, sim_ptr, valid_ptr, int(n), int(nnz), label_ptr, out_ptr))

    def set_communities_slots(self, slots: int) -> int:
        """test aid (``gnn_debug_communities_slots``): the slots (0..4096, the default) of the LDS table :meth:`communities` sums a
        row's entries in - a longer row takes the accumulator in global memory, with 0 every row; -1 changes nothing.  Returns the
        value before the call.  No result depends on it."""
        return self._knob(self.lib.gnn_debug_communities_slots, slots)

    def set_communities_wave_rows(self, entries: int) -> int:
        """test aid (``gnn_debug_communities_wave_rows``): the longest row (0..4096; the default is 256) that one wave of
        :meth:`communities` takes with its quarter of the table; 0: none; -1 changes nothing.  Returns the value before the call.
        No result depends on it."""
        return self._knob(self.lib.gnn_debug_communities_wave_rows, entries)

    def set_communities_groups(self, groups: int):
        """test aid (``gnn_debug_communities_groups``): the workgroups of a launch of :meth:`communities` (0: the library's
        choice); no result depends on it."""
        check(self.lib.gnn_debug_communities_groups(self.ctx, int(groups)))

    def communities_gain(self, operands) -> np.ndarray:
        """test aid (``gnn_debug_communities_gain``): the device's gain and score arithmetic over ``operands`` (m, 12) uint64 =
        (64 * M2, r, k, w_ic, w_ia, tot_c, tot_a, in, sq low, sq high, previous Qnum low, high): uint64 (m, 5) = (D low, D high,
        Qnum low, Qnum high, Qnum > previous), 128-bit values in two's complement"""
        operands = np.ascontiguousarray(operands, dtype=np.uint64)
        if operands.ndim != 2 or operands.shape[1] != 12:
            raise ValueError("operands (m, 12) uint64 is required")
        out = np.empty((len(operands), 5), dtype=np.uint64)
        check(self.lib.gnn_debug_communities_gain(self.ctx, operands.ctypes.data, len(operands), out.ctypes.data))
        return out

    def communities_pass_ms(self):
        """measurement only (``gnn_debug_communities_ms``): with profiling enabled, the HIP-event milliseconds of the last
        :meth:`communities` / :meth:`communities_dev` call - [setup, then per level every sweep and, behind a level with an accepted
        sweep, its end (split, contraction and the next level's start)]"""
        return self._debug_ms(self.lib.gnn_debug_communities_ms)

    def communities_classes(self) -> np.ndarray:
        """measurement only (``gnn_debug_communities_classes``): the rows the last call took by class, all launches together - int64
        [one wave, one workgroup, the accumulator in global memory] of the want launches, then of the contractions"""
        out = np.zeros(6, dtype=np.int64)
        check(self.lib.gnn_debug_communities_classes(self.ctx, out.ctypes.data))
        return out

    # -- spherical k-means ---------------------------------------------------------------
    def kmeans(self, rows, k, init=None, max_iter=_sequence.KMEANS_MAX_ITER_DEFAULT) -> KMeansResult:
        """Spherical k-means among encoder embeddings (``gnn_kmeans``; the definition is ``sequence.spherical_kmeans``): the valid
        rows of ``rows`` (n, 512) in exactly ``k`` (1..65535, at most the valid rows) groups under cosine similarity, and one unit
        centroid per group - a new row that stands for it, ordinary input for :meth:`match` and :meth:`neighbours`.  A row's label
        is its most similar centroid (ties to the smaller index), a centroid the unit vector of the sum of its members' unit rows;
        assignments and updates alternate on the device until no label changes or ``max_iter`` (0..1000) updates were made, and
        the labels returned are always the assignment to the centroids returned.  ``init``: (k, 512) valid rows, or None for the
        farthest-first traversal (no random numbers: the same rows give the same result).  ``label`` / ``sim`` are what
        :meth:`neighbours` returns for (rows, centroids, k=1), bit for bit; the centroids are sums of exact integers, so a
        permutation of the rows changes no bit of them.  Not Euclidean k-means, not the dot metric, not k-means++, not
        mini-batch.  :meth:`set_neighbour_split` sets the range of this search too; no result depends on it."""
        r = _sequence.neighbour_rows(rows, "rows")
        k, max_iter = _sequence.kmeans_k(k), _sequence.kmeans_max_iter(max_iter)
        b = None
        if init is not None:
            b = _sequence.neighbour_rows(init, "init")
            if len(b) != k:
                raise ValueError(f"init has {len(b)} rows: k = {k} are required")
            bad = int((~_sequence.valid_rows(b)).sum())
            if bad:
                raise ValueError(f"{bad} of the {k} init rows are not valid (finite, norm > 0)")
        n = len(r)
        label, sim = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.float32)
        cent, size, picks = np.empty((k, _lib.EMBED_DIM), dtype=np.float32), np.empty(k, dtype=np.int64), np.empty(k, dtype=np.int64)
        iterations, converged = C.c_int64(0), C.c_int(0)
        check(self.lib.gnn_kmeans(self.ctx, r.ctypes.data, n, k, None if b is None else b.ctypes.data, max_iter, label.ctypes.data,
                                  sim.ctypes.data, cent.ctypes.data, size.ctypes.data, picks.ctypes.data, C.addressof(iterations),
                                  C.addressof(converged)))
        return KMeansResult.build((label, sim, cent, size, iterations.value, converged.value, picks))

    def kmeans_dev(self, rows_ptr: int, n: int, k: int, label_ptr: int, sim_ptr: int, centroids_ptr: int, size_ptr: int, init_rows_ptr: int,
                   init_ptr=None, max_iter=_sequence.KMEANS_MAX_ITER_DEFAULT):
        """``gnn_kmeans_dev``: device pointers in (rows n x 512 f32; init k x 512 f32 or None) and out (label n int64, sim n f32,
        centroids k x 512 f32, size k int64, init_rows k int64), enqueued on the engine's stream - which is synchronised once at
        the start and once per assignment; the arrays are ready when the stream is.  Returns (iterations, converged)."""
        iterations, converged = C.c_int64(0), C.c_int(0)
        check(self.lib.gnn_kmeans_dev(self.ctx, rows_ptr, int(n), int(k), init_ptr, int(max_iter), label_ptr, sim_ptr, centroids_ptr,
                                      size_ptr, init_rows_ptr, C.addressof(iterations), C.addressof(converged)))
        return int(iterations.value), bool(converged.value)

    def centroids(self, rows, label, k):
        """One unit row per group (``gnn_centroids``; the definition is ``sequence.group_centroids``): the k-means update alone, for
        any int64 ``label`` in [-1, k) over ``rows`` (n, 512) - the clusters of :meth:`cluster`, :meth:`density` or
        :meth:`representatives` after a relabel to 0 .. k - 1.  Label -1 and invalid rows are skipped; a group without members or
        with a zero sum is a zero row.  Returns (centroids float32 (k, 512), size int64 (k,)); a permutation of the rows changes no
        bit of either."""
        r = _sequence.neighbour_rows(rows, "rows")
        k = _sequence.kmeans_k(k)
        lab = np.ascontiguousarray(label, dtype=np.int64)
        if lab.shape != (len(r),):
            raise ValueError(f"label has the shape {lab.shape}: one label per row ({len(r)}) is required")
        cent, size = np.full((k, _lib.EMBED_DIM), np.nan, dtype=np.float32), np.full(k, -1, dtype=np.int64)
        check(self.lib.gnn_centroids(self.ctx, r.ctypes.data, len(r), lab.ctypes.data, k, cent.ctypes.data, size.ctypes.data))
        return cent, size

    def centroids_dev(self, rows_ptr: int, n: int, label_ptr: int, k: int, centroids_ptr: int, size_ptr: int):
        """``gnn_centroids_dev``: device pointers in (rows n x 512 f32, label n int64) and out (centroids k x 512 f32, size k
        int64); the engine's stream is synchronised once (the labels' verdict), the rest is enqueued on it."""
        check(self.lib.gnn_centroids_dev(self.ctx, rows_ptr, int(n), label_ptr, int(k), centroids_ptr, size_ptr))

    def set_kmeans_lds(self, max_k: int):
        """test aid (``gnn_debug_set_kmeans_lds``): up to ``max_k`` (0..128, the default) groups the k-means update adds in LDS before it adds to
        memory; no result depends on it."""
        check(self.lib.gnn_debug_set_kmeans_lds(self.ctx, int(max_k)))

    def kmeans_pass_ms(self):
        """measurement only (``gnn_debug_kmeans_pass_ms``): with profiling enabled, the HIP-event milliseconds of the last
        :meth:`kmeans` / :meth:`kmeans_dev` call - [init, then per assignment: assign, and behind every assignment but the last:
        update, finish, prepare]"""
        return self._debug_ms(self.lib.gnn_debug_kmeans_pass_ms)

    # -- principal components ------------------------------------------------------------
    def pca_moments(self, rows):
        """The second moments of the unit rows (``gnn_pca_moments``; the definition is ``sequence.pca_moments``): ``G`` (float64
        (512, 512): the sum of u uT over the valid rows' unit vectors), ``S`` (float64 (512,): the sum of u) and ``n_valid``.  The
        device sums int64 fixed-point values in units of 2^-32 - S exactly, G from f32 product chains over granules of 256 rows
        turned into integers once - so no bit depends on how the rows are split over workgroups (:meth:`set_pca_split`).
        :meth:`pca_moments_fixed` returns the integers themselves."""
        G, S, n_valid = self.pca_moments_fixed(rows)
        return G.astype(np.float64) / 2.0 ** 32, S.astype(np.float64) / 2.0 ** 32, n_valid

    def pca_moments_fixed(self, rows):
        """:meth:`pca_moments` as the library returns it: int64 ``G`` (512, 512) and ``S`` (512,) in units of 2^-32, and ``n_valid``"""
        r = _sequence.neighbour_rows(rows, "rows")
        if not 1 <= len(r) <= _sequence.PCA_ROWS_MAX:
            raise ValueError(f"{len(r)} rows: 1 to 2^30 are required")
        G, S = np.empty((_lib.EMBED_DIM, _lib.EMBED_DIM), dtype=np.int64), np.empty(_lib.EMBED_DIM, dtype=np.int64)
        n_valid = C.c_int64(0)
        check(self.lib.gnn_pca_moments(self.ctx, r.ctypes.data, len(r), G.ctypes.data, S.ctypes.data, C.addressof(n_valid)))
        return G, S, int(n_valid.value)

    def pca_moments_dev(self, rows_ptr: int, n: int, G_ptr: int, S_ptr: int, n_valid_ptr: int):
        """``gnn_pca_moments_dev``: device pointers in (rows n x 512 f32) and out (G 512 x 512 int64, S 512 int64, n_valid 1 int64,
        all in units of 2^-32 but the last), enqueued on the engine's stream."""
        check(self.lib.gnn_pca_moments_dev(self.ctx, rows_ptr, int(n), G_ptr, S_ptr, n_valid_ptr))

    def project(self, rows, components, mean=None) -> np.ndarray:
        """Scores of ``rows`` (n, 512) on ``components`` (c, 512; 1 <= c <= 64 valid rows: directions, renormalised)
        (``gnn_pca_project``; the definition is ``sequence.pca_project``): float32 (n, c), the f32 cosine that :meth:`neighbours`
        returns for (row, component) minus ``mean`` . component - computed in float64 on the host and rounded to f32 once, then one
        f32 subtraction per value on the device -; NaN for an invalid row.  ``mean`` None: the cosines themselves."""
        r = _sequence.neighbour_rows(rows, "rows")
        if not 1 <= len(r) <= _sequence.PCA_ROWS_MAX:
            raise ValueError(f"{len(r)} rows: 1 to 2^30 are required")
        c32, _ = _sequence.pca_directions(components)
        off = None if mean is None else np.ascontiguousarray(_sequence.pca_offsets(c32, mean), dtype=np.float32)
        out = np.empty((len(r), len(c32)), dtype=np.float32)
        check(self.lib.gnn_pca_project(self.ctx, r.ctypes.data, len(r), c32.ctypes.data, len(c32), None if off is None else off.ctypes.data,
                                       out.ctypes.data))
        return out

    def project_dev(self, rows_ptr: int, n: int, components_ptr: int, ncomp: int, out_ptr: int, off_ptr=None):
        """``gnn_pca_project_dev``: device pointers in (rows n x 512 f32, components ncomp x 512 f32, off ncomp f32 or None) and
        out (n x ncomp f32), enqueued on the engine's stream."""
        check(self.lib.gnn_pca_project_dev(self.ctx, rows_ptr, int(n), components_ptr, int(ncomp), off_ptr, out_ptr))

    def pca(self, rows, n_components=2, center=True) -> PCAResult:
        """Principal components among encoder embeddings: the directions of largest variance of the valid rows' UNIT vectors - the
        geometry every search here works in - and the rows' scores on them.  :meth:`pca_moments` on the device, the 512 x 512
        eigenproblem on the host (``sequence.pca_from_moments``, float64: the matrix is 2 MB whatever n is), :meth:`project` on the
        device.  1 <= ``n_components`` <= 64; fewer than two valid rows is a ValueError.  ``center=False``: the second moments about
        the origin.  Not PCA of the raw (un-normalised) rows, not kernel PCA, not t-SNE / UMAP."""
        r = _sequence.neighbour_rows(rows, "rows")
        c = _sequence.pca_components(n_components)
        G, S, n_valid = self.pca_moments(r)
        m = _sequence.pca_from_moments(G, S, n_valid, c, center)
        comp = np.ascontiguousarray(m["components"], dtype=np.float32)
        proj = self.project(r, comp, m["mean"] if center else None)
        return PCAResult(engine=self, mean=m["mean"], components=comp, explained_variance=m["explained_variance"],
                         explained_variance_ratio=m["explained_variance_ratio"], total_variance=m["total_variance"], n_valid=n_valid,
                         valid=~np.isnan(proj[:, 0]), projection=proj)

    def set_pca_split(self, rows: int):
        """test aid (``gnn_debug_set_pca_split``): the rows a workgroup of the Gram pass takes, a multiple of 256; 0 = the
        library's choice; no result depends on it."""
        check(self.lib.gnn_debug_set_pca_split(self.ctx, int(rows)))

    def pca_pass_ms(self):
        """measurement only (``gnn_debug_pca_pass_ms``): with profiling enabled, the HIP-event milliseconds of the last moments
        call - [prepare, sums, gram, mirror] - or projection - [prepare rows, prepare components, project]"""
        return self._debug_ms(self.lib.gnn_debug_pca_pass_ms)

    # -- representatives -----------------------------------------------------------------
    def representatives(self, rows, threshold, weight=None, metric="cosine") -> RepresentativeResult:
        """Representatives among encoder embeddings (``gnn_representatives``; the definition is
        ``sequence.greedy_representatives``): greedy incremental clusters of ``rows`` (n, 512).  The rows are walked by (``weight``
        descending, index ascending) - ``None``: index order -; a row founds a cluster unless an earlier representative has a
        similarity >= ``threshold`` to it, otherwise it joins the most similar such representative.  Stars, not chains: every
        member is within the threshold of its representative, no two representatives are within it of each other.  The rows are
        permuted by rank before the call and ``rep`` is mapped back: the similarity of a pair is the float32 :meth:`neighbours`
        returns for query = the row of smaller rank and base row = the other, in the permuted order.  The device runs synchronous
        rounds (``rounds``; a path walked end to end takes as many as it has rows), one stream synchronise each.
        :meth:`set_neighbour_split` sets the range of this search too; no result depends on it."""
        r = _sequence.neighbour_rows(rows, "rows")
        self._check_metric(metric)
        n = len(r)
        order = _sequence.priority_order(weight, n)
        rank = np.empty(n, dtype=np.int64)
        rank[order] = np.arange(n)
        p = r if weight is None else np.ascontiguousarray(r[order])
        rep_p, sim_p, size_p = np.empty(n, np.int64), np.empty(n, np.float32), np.empty(n, np.int64)
        rounds = C.c_int64(0)
        check(self.lib.gnn_representatives(self.ctx, p.ctypes.data, n, float(threshold), self._knn_metric(metric), rep_p.ctypes.data,
                                           sim_p.ctypes.data, size_p.ctypes.data, C.addressof(rounds)))
        rep, sim, size = np.empty(n, np.int64), np.empty(n, np.float32), np.empty(n, np.int64)
        rep[order] = np.where(rep_p >= 0, order[np.maximum(rep_p, 0)], -1)
        sim[order], size[order] = sim_p, size_p
        return RepresentativeResult.build((rep, sim, size, rank, rounds.value), np.float32(threshold), metric)

    def representatives_dev(self, rows_ptr: int, n: int, threshold, rep_ptr: int, sim_ptr: int, size_ptr: int, metric="cosine") -> int:
        """``gnn_representatives_dev``: device pointers in (rows n x 512 f32 IN PRIORITY ORDER: index = rank) and out (rep int64,
        sim f32, size int64, n each, in that order's index space), enqueued on the engine's stream - which is synchronised once per
        round; the arrays are ready when the stream is.  Returns ``rounds``."""
        rounds = C.c_int64(0)
        check(self.lib.gnn_representatives_dev(self.ctx, rows_ptr, int(n), float(threshold), self._knn_metric(metric), rep_ptr, sim_ptr,
                                               size_ptr, C.addressof(rounds)))
        return int(rounds.value)

    def representative_round_ms(self):
        """measurement only (``gnn_debug_representative_round_ms``): with profiling enabled, the HIP-event milliseconds of every
        round of the last ``representatives`` / ``representatives_dev`` call"""
        return self._debug_ms(self.lib.gnn_debug_representative_round_ms)

    # -- single-linkage tree -------------------------------------------------------------
    def _linkage(self, fn, rows_ptr, n, metric) -> LinkageResult:
        self._check_metric(metric)
        cap = max(int(n) - 1, 0)
        a, b, sim = np.empty(cap, np.int64), np.empty(cap, np.int64), np.empty(cap, np.float32)
        valid = np.zeros(max(int(n), 0), np.uint8)
        n_edges, rounds = C.c_int64(0), C.c_int64(0)
        check(fn(self.ctx, rows_ptr, int(n), self._knn_metric(metric), a.ctypes.data, b.ctypes.data, sim.ctypes.data, valid.ctypes.data,
                 C.addressof(n_edges), C.addressof(rounds)))
        m = n_edges.value
        name = self._metric_name(metric)
        return LinkageResult.build((a[:m].copy(), b[:m].copy(), sim[:m].copy(), valid), name, rounds.value)

    def linkage(self, rows, metric="cosine") -> LinkageResult:
        """The single-linkage tree among encoder embeddings (``gnn_linkage``; the definition is ``sequence.single_linkage_tree``):
        the maximum-similarity spanning tree over the valid rows of ``rows`` (n, 512), edges ordered by (similarity descending, smaller
        row, larger row) - Boruvka rounds over the upper triangle on the matrix pipe, exact.  It answers :meth:`cluster` at every
        threshold: ``result.cut(t)`` is ``cluster(rows, t).label`` and ``result.cluster_counts`` the number of clusters, without
        another pass.  The similarity of the pair i < j is the float32 :meth:`neighbours` returns for query i and base row j.
        :meth:`set_neighbour_split` sets the range of this search too; no result depends on it."""
        r = _sequence.neighbour_rows(rows, "rows")
        return self._linkage(self.lib.gnn_linkage, r.ctypes.data, len(r), metric)

    def linkage_dev(self, rows_ptr: int, n: int, metric="cosine") -> LinkageResult:
        """``gnn_linkage_dev``: the rows (n x 512 f32) on the device, the result on the host; the engine's stream is synchronised once
        per round and the call returns with the result."""
        return self._linkage(self.lib.gnn_linkage_dev, rows_ptr, n, metric)

    def linkage_round_ms(self):
        """measurement only (``gnn_debug_linkage_round_ms``): with profiling enabled, the HIP-event milliseconds of every round of the
        last ``linkage`` / ``linkage_dev`` call, a last round that added no edge included"""
        return self._debug_ms(self.lib.gnn_debug_linkage_round_ms)

    # -- density-aware linkage tree ------------------------------------------------------
    def _density_tree(self, fn, rows_ptr, n, min_points, metric) -> DensityTreeResult:
        self._check_metric(metric)
        m = _sequence.density_tree_min_points(min_points)
        cap = max(int(n) - 1, 0)
        a, b, sim = np.empty(cap, np.int64), np.empty(cap, np.int64), np.empty(cap, np.float32)
        core = np.full(max(int(n), 0), np.nan, np.float32)
        valid = np.zeros(max(int(n), 0), np.uint8)
        n_edges, rounds = C.c_int64(0), C.c_int64(0)
        check(fn(self.ctx, rows_ptr, int(n), m, self._knn_metric(metric), a.ctypes.data, b.ctypes.data, sim.ctypes.data, core.ctypes.data,
                 valid.ctypes.data, C.addressof(n_edges), C.addressof(rounds)))
        e = n_edges.value
        return DensityTreeResult.build((a[:e].copy(), b[:e].copy(), sim[:e].copy(), core, valid), m, self._metric_name(metric), rounds.value)

    def density_tree(self, rows, min_points=5, metric="cosine") -> DensityTreeResult:
        """The density-aware linkage tree among encoder embeddings (``gnn_density_tree``; the definition is
        ``sequence.mutual_reachability_tree``): :meth:`linkage` over the mutual-reachability values min(v(i, j), core_i, core_j),
        where core_i is row i's similarity to its (``min_points`` - 1)-th nearest neighbour - the last finite entry of row i of
        ``neighbours(rows, None, min_points - 1).sim``, bit for bit.  A bridge row between two families no longer merges them
        early, and a straggler joins late: ``result.cut(t)`` is the core rows' ``label`` of :meth:`density` at (t, min_points) for
        every t without another pass, and ``result.hdbscan(min_cluster_size)`` picks the clusters without a threshold.  Exact;
        1 <= ``min_points`` <= 65; ``min_points`` 1 is :meth:`linkage`, bit for bit.  :meth:`set_neighbour_split` sets the range of
        this search too; no result depends on it."""
        r = _sequence.neighbour_rows(rows, "rows")
        return self._density_tree(self.lib.gnn_density_tree, r.ctypes.data, len(r), min_points, metric)

    def density_tree_dev(self, rows_ptr: int, n: int, min_points=5, metric="cosine") -> DensityTreeResult:
        """``gnn_density_tree_dev``: the rows (n x 512 f32) on the device, the result on the host; the engine's stream is synchronised
        once per round and the call returns with the result."""
        return self._density_tree(self.lib.gnn_density_tree_dev, rows_ptr, n, min_points, metric)

    def density_tree_round_ms(self):
        """measurement only (``gnn_debug_density_tree_round_ms``): with profiling enabled, the HIP-event milliseconds of every round
        of the last ``density_tree`` / ``density_tree_dev`` call, a last round that added no edge included"""
        return self._debug_ms(self.lib.gnn_debug_density_tree_round_ms)

    # -- occlusion maps ------------------------------------------------------------------
    def occlusion_plan(self, offsets: np.ndarray, block: int, single_window: bool = False):
        """``gnn_occlusion_plan`` (host only): (win_offsets, contig-relative starts, lens, blk_offsets) of an occlusion map with
        blocks of ``block`` bases - the windows of :meth:`classify_contigs` and the CSR of their (window, block) pairs."""
        offsets = self._offsets(offsets)
        n_contigs = len(offsets) - 1
        nw, npairs = C.c_int64(), C.c_int64()
        head = (offsets.ctypes.data, n_contigs, int(block), int(bool(single_window)), C.byref(nw), C.byref(npairs))
        check(self.lib.gnn_occlusion_plan(*head, None, None, None, None))
        win_off, blk_off = np.zeros(n_contigs + 1, np.int64), np.zeros(nw.value + 1, np.int64)
        starts, lens = np.zeros(nw.value, np.int64), np.zeros(nw.value, np.int32)
        check(self.lib.gnn_occlusion_plan(*head, win_off.ctypes.data, starts.ctypes.data, lens.ctypes.data, blk_off.ctypes.data))
        return win_off, starts, lens, blk_off

    def occlude_spans_dev(self, seq_ptr: int, starts, lens, lo, hi, bases_ptr: int):
        """``gnn_occlude_spans_dev``: the occluded windows (``sequence.occlude_spans``) of the spans (start, len <= 6000) of a packed
        buffer in HBM - each materialised with its window-relative interval [lo, hi) set to N - written to ``bases_ptr`` (n x 6000
        bytes on the device, 4-byte aligned), ready for :meth:`classify_dev` / :meth:`embed_dev`.  Returns when they are written."""
        starts = np.ascontiguousarray(starts, dtype=np.int64)
        lens, lo, hi = (np.ascontiguousarray(a, dtype=np.int32) for a in (lens, lo, hi))
        if starts.ndim != 1 or not (starts.shape == lens.shape == lo.shape == hi.shape):
            raise ValueError("starts, lens, lo and hi must be 1-d arrays of one length")
        check(self.lib.gnn_occlude_spans_dev(self.ctx, seq_ptr, starts.ctypes.data, lens.ctypes.data, lo.ctypes.data, hi.ctypes.data,
                                             len(starts), bases_ptr))

    def occlude_contigs(self, seq: np.ndarray, offsets: np.ndarray, block: int, single_window: bool = False,
                        precision=_lib.DEFAULT_PRECISION) -> OcclusionResult:
        """Occlusion map of every contig (``gnn_occlude_contigs``): each window of :meth:`classify_contigs` is scored as it is and
        once per block of ``block`` bases (1 <= block <= 6000) with that block set to N, the model's own "unknown"; ``delta`` is how
        far each class moved - which bases the score rests on.  Windows, ``kept`` and ``contig_scores`` are those of
        classify_contigs, ``scores`` those of ``scan_contigs(stride=6000)``, every occluded score that of :meth:`classify` on the
        same bytes (``sequence.occlude_spans``).  1 + ceil(6000 / block) forward passes per window."""
        return self._occlude_contigs(np.asarray(seq), offsets, block, single_window, precision)

    def occlude_contigs_dev(self, seq_ptr: int, offsets: np.ndarray, block: int, single_window: bool = False,
                            precision=_lib.DEFAULT_PRECISION) -> OcclusionResult:
        """Same as :meth:`occlude_contigs` for a packed contig buffer that is already resident in HBM."""
        return self._occlude_contigs(seq_ptr, offsets, block, single_window, precision)

    # -- attention contribution maps ------------------------------------------------------
    @staticmethod
    def attribution_bins(bin: int) -> int:
        """nb = ceil(749 / bin): the bins of a contribution map with ``bin`` pooled positions each (the last one may be short)."""
        return -(-_lib.POOLED // int(bin))

    def attribute(self, bases, bin: int = 1, precision=_lib.DEFAULT_PRECISION):
        """(n,6000) uint8 windows -> (contrib (n, 2, nb, 3), bias (n, 3), logits (n, 3), scores (n, 3)), all float32
        (``gnn_attribute``): each pooled position's share of each pre-softmax logit, per attention head - gradient x input at the
        attention layer with the attention weights held fixed.  contrib.sum((1, 2)) + bias = logits; the scores are those of
        :meth:`classify`, bit for bit.  ``bin`` pooled positions (8 tokens each) per output bin, 1 <= bin <= 749.  The map decomposes
        the logit exactly; it does not predict what an edit of the window would do (:meth:`occlude_contigs` does)."""
        b = self._check_bases(bases)
        nb = self.attribution_bins(bin) if 1 <= int(bin) <= _lib.POOLED else 1      # a bad bin is the library's to refuse
        contrib = np.zeros((len(b), 2, nb, _lib.CLASSES), dtype=np.float32)
        bias, logits, scores = (np.zeros((len(b), _lib.CLASSES), dtype=np.float32) for _ in range(3))
        check(self.lib.gnn_attribute(self.ctx, b.ctypes.data, len(b), _lib.PRECISIONS[precision], int(bin), contrib.ctypes.data,
                                     bias.ctypes.data, logits.ctypes.data, scores.ctypes.data))
        return contrib, bias, logits, scores

    def attribute_dev(self, bases_ptr: int, n: int, bin: int, contrib_ptr: int, precision=_lib.DEFAULT_PRECISION, bias_ptr=None,
                      logits_ptr=None, scores_ptr=None):
        """Asynchronous: device pointers in and out (contrib: n x 2 x nb x 3 f32; bias, logits, scores: n x 3 f32 or None),
        enqueued on the engine's stream (``gnn_attribute_dev``)."""
        check(self.lib.gnn_attribute_dev(self.ctx, bases_ptr, int(n), _lib.PRECISIONS[precision], int(bin), contrib_ptr, bias_ptr,
                                         logits_ptr, scores_ptr))

    def _attribute_contigs(self, seq, offsets, bin, single_window, precision):
        """gnn_attribute_contigs -> AttributionResult"""
        (ptr, on_host, nbytes, offsets, n_contigs), _keep = self._packed(seq, offsets)
        win_off, _, starts, lens = self.scan_plan(offsets, _lib.WINDOW, single_window)
        n = len(starts)
        nb = self.attribution_bins(bin) if 1 <= int(bin) <= _lib.POOLED else 1
        contrib = np.zeros((n, 2, nb, _lib.CLASSES), dtype=np.float32)
        bias, logits, scores = (np.zeros((n, _lib.CLASSES), dtype=np.float32) for _ in range(3))
        kept = np.zeros(n, dtype=np.uint8)
        contig_scores = np.zeros((n_contigs, _lib.CLASSES), dtype=np.float32)
        check(self.lib.gnn_attribute_contigs(self.ctx, ptr, on_host, nbytes, offsets.ctypes.data, n_contigs, int(bin),
                                             int(bool(single_window)), _lib.PRECISIONS[precision], contrib.ctypes.data, n,
                                             bias.ctypes.data, logits.ctypes.data, scores.ctypes.data, kept.ctypes.data,
                                             contig_scores.ctypes.data))
        return AttributionResult(bin=int(bin), win_offsets=win_off, starts=starts, lens=lens, kept=kept.astype(bool),
                                 window_scores=scores, contrib=contrib, bias=bias, logits=logits, contig_scores=contig_scores)

    def attribute_contigs(self, seq: np.ndarray, offsets: np.ndarray, bin: int = 1, single_window: bool = False,
                          precision=_lib.DEFAULT_PRECISION) -> AttributionResult:
        """Contribution maps of every window of every contig (``gnn_attribute_contigs``): the windows, ``kept`` and
        ``contig_scores`` of :meth:`classify_contigs`, the window scores of ``scan_contigs(stride=6000)``, and per window the maps
        of :meth:`attribute` - in the same forward pass, with no extra one."""
        return self._attribute_contigs(np.asarray(seq), offsets, bin, single_window, precision)

    def attribute_contigs_dev(self, seq_ptr: int, offsets: np.ndarray, bin: int = 1, single_window: bool = False,
                              precision=_lib.DEFAULT_PRECISION) -> AttributionResult:
        """Same as :meth:`attribute_contigs` for a packed contig buffer that is already resident in HBM."""
        return self._attribute_contigs(seq_ptr, offsets, bin, single_window, precision)

    # -- both strands --------------------------------------------------------------------
    def revcomp_spans_dev(self, seq_ptr: int, starts, lens, bases_ptr: int):
        """``gnn_revcomp_spans_dev``: the reverse windows (``sequence.revcomp_spans``) of the spans (start, len <= 6000) of a packed
        buffer in HBM, written to ``bases_ptr`` (n x 6000 bytes on the device, 4-byte aligned) - ready for :meth:`classify_dev` /
        :meth:`embed_dev`.  Returns when they are written."""
        starts = np.ascontiguousarray(starts, dtype=np.int64)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        if starts.shape != lens.shape or starts.ndim != 1:
            raise ValueError("starts and lens must be 1-d arrays of one length")
        check(self.lib.gnn_revcomp_spans_dev(self.ctx, seq_ptr, starts.ctypes.data, lens.ctypes.data, len(starts), bases_ptr))

    def classify_contigs_strand(self, seq: np.ndarray, offsets: np.ndarray, strand="both", single_window: bool = False,
                                precision=_lib.DEFAULT_PRECISION, embed: bool = False):
        """:meth:`classify_contigs` on the forward windows, their reverse complements, or both (``gnn_classify_contigs_strand``;
        the definitions are ``sequence.revcomp_spans`` and ``sequence.strand_mean``).  The windows, the N rule and the window ids
        are the forward ones; under "both" a window's score is the f32 mean of its two strands and the contig score the mean of
        those.  Returns (contig_scores (n_contigs, 3) of the mode, contig ids of the kept windows, contig embeddings
        (n_contigs, 512) of the mode or None without ``embed``, forward contig scores, reverse contig scores); a strand the
        mode does not need is computed for its own scores.  "forward" is bit-identical to classify_contigs / embed_contigs."""
        return self._classify_contigs(np.asarray(seq), offsets, single_window, precision, embed, strand)

    def classify_contigs_strand_dev(self, seq_ptr: int, offsets: np.ndarray, strand="both", single_window: bool = False,
                                    precision=_lib.DEFAULT_PRECISION, embed: bool = False):
        """Same as :meth:`classify_contigs_strand` for a packed contig buffer that is already resident in HBM."""
        return self._classify_contigs(seq_ptr, offsets, single_window, precision, embed, strand)

    def scan_contigs_strand(self, seq: np.ndarray, offsets: np.ndarray, stride: int, strand="both", single_window: bool = False,
                            precision=_lib.DEFAULT_PRECISION) -> StrandScanResult:
        """:meth:`scan_contigs` with a strand mode (``gnn_scan_contigs_strand``): ``scores``, ``track`` and ``contig_scores`` carry
        the mode, ``scores_fwd`` / ``scores_rev`` each strand's own window scores; everything else is the forward scan's."""
        return self._scan_contigs(np.asarray(seq), offsets, stride, single_window, precision, strand)

    def scan_contigs_strand_dev(self, seq_ptr: int, offsets: np.ndarray, stride: int, strand="both", single_window: bool = False,
                                precision=_lib.DEFAULT_PRECISION) -> StrandScanResult:
        """Same as :meth:`scan_contigs_strand` for a packed contig buffer that is already resident in HBM."""
        return self._scan_contigs(seq_ptr, offsets, stride, single_window, precision, strand)

    def classify_contigs_spans(self, seq_ptr: int, offsets: np.ndarray, single_window: bool = False,
                               precision=_lib.DEFAULT_PRECISION):
        """The same result assembled on the host from the span-level entry points (gnn_span_byte_count,
        gnn_classify_spans, gnn_segment_mean) — kept as an independently coded cross-check for the tests."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n_contigs = len(offsets) - 1
        starts, lens, ids, window_n = _sequence.candidate_spans(offsets, single_window)
        if not len(starts):
            return np.zeros((n_contigs, _lib.CLASSES), np.float32), ids
        later = np.flatnonzero(window_n > 0)              # window 0 is never skipped (:70)
        keep = np.ones(len(starts), dtype=bool)
        if len(later):
            st, ln = np.ascontiguousarray(starts[later]), np.ascontiguousarray(lens[later])
            counts = np.empty(len(later), dtype=np.int32)
            check(self.lib.gnn_span_byte_count(self.ctx, seq_ptr, st.ctypes.data, ln.ctypes.data, len(later),
                                               ord("N"), counts.ctypes.data))
            keep[later[counts > _sequence.MAX_N]] = False
        starts, lens, ids = (np.ascontiguousarray(a[keep]) for a in (starts, lens, ids))
        scores = np.empty((len(starts), _lib.CLASSES), dtype=np.float32)
        check(self.lib.gnn_classify_spans(self.ctx, seq_ptr, starts.ctypes.data, lens.ctypes.data, len(starts),
                                          _lib.PRECISIONS[precision], scores.ctypes.data))
        return self.segment_mean(scores, ids, n_contigs), ids

    def segment_mean(self, scores, ids, n_segments=None) -> np.ndarray:
        """tf.math.segment_mean(scores, ids) (nn_classification.py:320); ids sorted ascending."""
        s = np.ascontiguousarray(scores, dtype=np.float32)
        i = np.ascontiguousarray(ids, dtype=np.int64)
        if n_segments is None:
            n_segments = int(i.max()) + 1 if len(i) else 0
        out = np.zeros((n_segments, _lib.CLASSES), dtype=np.float32)
        check(self.lib.gnn_segment_mean(self.ctx, s.ctypes.data, i.ctypes.data, len(i), n_segments,
                                        out.ctypes.data))
        return out

    def synth_windows_dev(self, first: int, n: int, bases_ptr: int, seed: int = 1234):
        check(self.lib.gnn_synth_windows_dev(self.ctx, seed, int(first), int(n), bases_ptr))

    def synth_windows(self, first: int, n: int, seed: int = 1234) -> np.ndarray:
        buf = self.alloc(max(n * _lib.WINDOW, 1))
        try:
            self.synth_windows_dev(first, n, buf.ptr, seed)
            self.sync()
            return buf.download((n, _lib.WINDOW), np.uint8)
        finally:
            buf.free()

    # -- measurement --------------------------------------------------------------------
    def profile_enable(self, on=True):
        check(self.lib.gnn_profile_enable(self.ctx, 1 if on else 0))

    def profile_reset(self):
        check(self.lib.gnn_profile_reset(self.ctx))

    def profile_get(self, kernel_id: int):
        ms, n = C.c_double(), C.c_int64()
        check(self.lib.gnn_profile_get(self.ctx, kernel_id, C.byref(ms), C.byref(n)))
        return ms.value, n.value
