"""ctypes binding of libgenomad_nn_hip.so (include/genomad_nn.h).

There is no CPU fallback: if the shared library is missing, or no gfx950 device is
visible, the product path raises.  Loading the library itself needs no GPU (used by
the CPU test-suite to check the exported symbols).
"""
import ctypes as C
import os
from pathlib import Path

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("GENOMAD_AMD_LIB", _HERE / "csrc" / "libgenomad_nn_hip.so"))

WINDOW, TOKENS, DEPTH, CH = 6000, 5997, 257, 128
PATCHES, PATCH_SIZE, POOLED, FEAT, HIDDEN, CLASSES = 2100, 4, 749, 256, 512, 3
EMBED_DIM = 512                                  # GNN_EMBED_DIM: create_encoder()'s output (model.py:14-31)
EMB_F32, EMB_BF16 = 0, 1                         # gnn_emb_dtype
EMB_DTYPES = {"f32": EMB_F32, "bf16": EMB_BF16}

PREC_F32, PREC_BF16X3, PREC_BF16, PREC_F16C8, PREC_F16X3, PREC_F16C6, PREC_F16X3TC, PREC_F16X3TK = 0, 1, 2, 3, 4, 5, 6, 7
# PREC_BF16 (single bf16 pass) and PREC_F16C8 (f16 + fp8 corrections) were removed in round 6: both fail the 1e-4 tolerance; the
# library keeps the enum values and answers GNN_ERR_STATE, the Python side no longer knows their names
PRECISIONS = {"f32": PREC_F32, "bf16x3": PREC_BF16X3, "f16x3": PREC_F16X3, "f16c6": PREC_F16C6, "f16x3tc": PREC_F16X3TC,
              "f16x3tk": PREC_F16X3TK}
# Arithmetics that are KNOWN to leave the 1e-4 score tolerance at scale (f16c6: 1.2e-4 on a few of 10^6 windows, profiles/history/
# r02c6_tails.txt): selectable for measurements only - main() refuses them unless GENOMAD_AMD_ALLOW_OUT_OF_TOLERANCE=1 is set
OUT_OF_TOLERANCE = {"f16c6": 1.2e-4}
# Arithmetic of the fused front end when the caller names none.  "f16x3tc" (round 4): split-f16 limbs, three MFMA products per operand
# pair, conv2 / conv3 by Toom-Cook F(3,6) minimal filtering over time (0.444x their MFMAs, f32 transforms), split-f16 logits GEMM and
# exact-f32 dense head.  Class scores within 2e-5 (weight seed 42) / 4e-5 (seed 43) of the exact-f32 path on every one of 1 M windows -
# the figures of "f16x3", the direct three-pass form it replaced as the default (profiles/r04_tails.txt) - and 1.16x its speed.
# "f16c6" (f16 + 4-bit correction MFMAs) stays opt-in behind OUT_OF_TOLERANCE: 1.2e-4 on a handful of 10^6 windows.  "bf16x3": f32 range; "f32": exact.
# "f16x3tk" (round 6): f16x3tc with conv2 read from a 137 GB table of all 14-mers and head A's pair products from an 8.8 GB (entry, 9-mer)
# table - 1.4x the speed, scores equal to 1e-6 - on an engine whose device could hold them (NNEngine.build_kmer_tables); main() and
# bench.py promote the default to it when the tables are there or worth building (nn_classification.select_arithmetic).
DEFAULT_PRECISION = "f16x3tc"
ERR_ARG, ERR_HIP, ERR_STATE, ERR_WEIGHTS, ERR_NOMEM = -1, -2, -3, -4, -5      # gnn_status
OH_U8, OH_BF16, OH_F32 = 0, 1, 2
STRAND_FORWARD, STRAND_REVERSE, STRAND_BOTH = 0, 1, 2       # gnn_strand
STRANDS = {"forward": STRAND_FORWARD, "reverse": STRAND_REVERSE, "both": STRAND_BOTH}
K_FUSED, K_BACKEND, K_ENCODER, K_F32_FRONT, K_ATTR_HEAD, K_ATTR_CONTRIB, K_REGIONS, K_NEIGHBOURS = 0, 1, 2, 3, 4, 5, 6, 7
KNN_COSINE, KNN_DOT = 0, 1                                  # gnn_knn_metric
KNN_METRICS = {"cosine": KNN_COSINE, "dot": KNN_DOT}
KNN_GRAPH_MODES = {"union": 0, "mutual": 1}                    # gnn_knn_graph_mode
KNN_GRAPH_WEIGHTS = {"similarity": 0, "jaccard": 1}            # gnn_knn_graph_weight
KNN_K_MAX = 64

_f32p = C.POINTER(C.c_float)
_i32p = C.POINTER(C.c_int32)


class IglooWeights(C.Structure):
    _fields_ = [("patches", _i32p), ("w_mult", _f32p), ("w_summer", _f32p), ("w_bias", _f32p),
                ("w_qk", _f32p), ("w_v", _f32p)]


class DenseBN(C.Structure):
    _fields_ = [("kernel", _f32p), ("bias", _f32p), ("gamma", _f32p), ("beta", _f32p),
                ("mean", _f32p), ("var", _f32p)]


class Weights(C.Structure):
    _fields_ = [("conv1_kernel", _f32p), ("conv1_bias", _f32p), ("conv2_kernel", _f32p),
                ("conv2_bias", _f32p), ("conv3_kernel", _f32p), ("conv3_bias", _f32p),
                ("igloo_a", IglooWeights), ("igloo_b", IglooWeights), ("enc", DenseBN),
                ("head", DenseBN), ("out_kernel", _f32p), ("out_bias", _f32p)]


class Taps(C.Structure):
    _fields_ = [(k, _f32p) for k in ("x1", "x2", "x3", "m_a", "m_b", "yp_a", "yp_b",
                                     "alpha_a", "alpha_b", "feat")]


# name -> (restype, argtypes); every entry is declared in include/genomad_nn.h
_vp, _i64, _int, _sz, _u64 = C.c_void_p, C.c_int64, C.c_int, C.c_size_t, C.c_uint64
SIGNATURES = {
    "gnn_last_error": (C.c_char_p, []),
    "gnn_version": (_int, []),
    "gnn_has_experimental": (_int, []),
    "gnn_device_count": (_int, [C.POINTER(_int)]),
    "gnn_create": (_int, [_int, C.POINTER(_vp)]),
    "gnn_destroy": (_int, [_vp]),
    "gnn_sync": (_int, [_vp]),
    "gnn_device_info": (_int, [_vp, C.c_char_p, _sz, C.POINTER(_int), C.POINTER(_i64)]),
    "gnn_device_mem_info": (_int, [_vp, C.POINTER(_i64), C.POINTER(_i64)]),
    "gnn_device_pci_bus_id": (_int, [_vp, C.c_char_p, _sz]),
    "gnn_load_weights": (_int, [_vp, C.POINTER(Weights)]),
    "gnn_build_kmer_tables": (_int, [_vp, _i64]),
    "gnn_has_kmer_tables": (_int, [_vp]),
    "gnn_drop_kmer_tables": (_int, [_vp]),
    "gnn_kmer_tables_bytes": (_i64, []),
    "gnn_debug_kmer_table_row": (_int, [_vp, _int, _u64, _vp]),
    "gnn_dev_alloc": (_int, [_vp, _sz, C.POINTER(_vp)]),
    "gnn_dev_free": (_int, [_vp, _vp]),
    "gnn_memcpy_h2d": (_int, [_vp, _vp, _vp, _sz]),
    "gnn_memcpy_d2h": (_int, [_vp, _vp, _vp, _sz]),
    "gnn_tokenize": (_int, [_vp, _vp, _i64, _vp]),
    "gnn_tokenize_dev": (_int, [_vp, _vp, _i64, _vp]),
    "gnn_onehot_dev": (_int, [_vp, _vp, _i64, _int, _vp]),
    "gnn_classify": (_int, [_vp, _vp, _i64, _int, _vp]),
    "gnn_classify_dev": (_int, [_vp, _vp, _i64, _int, _vp]),
    "gnn_classify_dev_async": (_int, [_vp, _vp, _i64, _int, _vp]),
    "gnn_classify_flush": (_int, [_vp]),
    "gnn_segment_mean": (_int, [_vp, _vp, _vp, _i64, _i64, _vp]),
    "gnn_span_byte_count": (_int, [_vp, _vp, _vp, _vp, _i64, _int, _vp]),
    "gnn_classify_spans": (_int, [_vp, _vp, _vp, _vp, _i64, _int, _vp]),
    "gnn_classify_contigs": (_int, [_vp, _vp, _int, _i64, _vp, _i64, _int, _int, _vp, _vp, _i64, C.POINTER(_i64)]),
    "gnn_classify_contigs_embed": (_int, [_vp, _vp, _int, _i64, _vp, _i64, _int, _int, _vp, _vp, _i64, C.POINTER(_i64), _vp]),
    "gnn_scan_plan": (_int, [_vp, _i64, _int, _int, C.POINTER(_i64), C.POINTER(_i64), _vp, _vp, _vp, _vp]),
    "gnn_scan_contigs": (_int, [_vp, _vp, _int, _i64, _vp, _i64, _int, _int, _int, _vp, _vp, _i64, _vp, _vp, _i64, _vp]),
    "gnn_revcomp_spans_dev": (_int, [_vp, _vp, _vp, _vp, _i64, _vp]),
    "gnn_classify_contigs_strand": (_int, [_vp, _vp, _int, _i64, _vp, _i64, _int, _int, _vp, _vp, _i64, C.POINTER(_i64), _vp, _int, _vp,
                                           _vp]),
    "gnn_scan_contigs_strand": (_int, [_vp, _vp, _int, _i64, _vp, _i64, _int, _int, _int, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _int, _vp,
                                       _vp]),
    "gnn_occlusion_plan": (_int, [_vp, _i64, _int, _int, C.POINTER(_i64), C.POINTER(_i64), _vp, _vp, _vp, _vp]),
    "gnn_occlude_spans_dev": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "gnn_occlude_contigs": (_int, [_vp, _vp, _int, _i64, _vp, _i64, _int, _int, _int, _vp, _vp, _i64, _vp, _i64, _vp]),
    "gnn_attribute": (_int, [_vp, _vp, _i64, _int, _int, _vp, _vp, _vp, _vp]),
    "gnn_attribute_dev": (_int, [_vp, _vp, _i64, _int, _int, _vp, _vp, _vp, _vp]),
    "gnn_attribute_contigs": (_int, [_vp, _vp, _int, _i64, _vp, _i64, _int, _int, _int, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "gnn_call_regions": (_int, [_vp, _vp, _vp, _i64, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, C.POINTER(_i64)]),
    "gnn_region_states_dev": (_int, [_vp, _vp, _vp, _i64, C.c_double, _vp]),
    "gnn_debug_set_region_tile": (_int, [_vp, _int]),
    "gnn_interval_plan": (_int, [_vp, _i64, _int, _int, _vp, _vp, _vp, _i64, _vp, _vp]),
    "gnn_embed_intervals": (_int, [_vp, _vp, _int, _i64, _vp, _i64, _int, _int, _int, _int, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "gnn_interval_fold_dev": (_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "gnn_interval_finish_dev": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "gnn_neighbours": (_int, [_vp, _vp, _i64, _vp, _i64, _int, _int, _vp, _vp]),
    "gnn_neighbours_dev": (_int, [_vp, _vp, _i64, _vp, _i64, _int, _int, _vp, _vp]),
    "gnn_debug_set_neighbour_split": (_int, [_vp, _i64]),
    "gnn_cluster": (_int, [_vp, _vp, _i64, C.c_float, _int, _vp, _vp, _vp, _vp]),
    "gnn_cluster_dev": (_int, [_vp, _vp, _i64, C.c_float, _int, _vp, _vp, _vp, _vp]),
    "gnn_density": (_int, [_vp, _vp, _i64, C.c_float, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gnn_density_dev": (_int, [_vp, _vp, _i64, C.c_float, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gnn_representatives": (_int, [_vp, _vp, _i64, C.c_float, _int, _vp, _vp, _vp, _vp]),
    "gnn_representatives_dev": (_int, [_vp, _vp, _i64, C.c_float, _int, _vp, _vp, _vp, _vp]),
    "gnn_debug_representative_round_ms": (_int, [_vp, _vp, _i64, _vp]),
    "gnn_linkage": (_int, [_vp, _vp, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gnn_linkage_dev": (_int, [_vp, _vp, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gnn_debug_linkage_round_ms": (_int, [_vp, _vp, _i64, _vp]),
    "gnn_density_tree": (_int, [_vp, _vp, _i64, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gnn_density_tree_dev": (_int, [_vp, _vp, _i64, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gnn_debug_density_tree_round_ms": (_int, [_vp, _vp, _i64, _vp]),
    "gnn_graph_count": (_int, [_vp, _vp, _i64, C.c_float, _int, _vp, _vp]),
    "gnn_graph_fill": (_int, [_vp, _i64, C.c_float, _int, _vp, _vp, _i64]),
    "gnn_graph_count_dev": (_int, [_vp, _vp, _i64, C.c_float, _int, _vp, _vp]),
    "gnn_graph_fill_dev": (_int, [_vp, _vp, _i64, C.c_float, _int, _vp, _vp, _i64]),
    "gnn_debug_graph_pass_ms": (_int, [_vp, _vp, _i64, _vp]),
    "gnn_match_count": (_int, [_vp, _vp, _i64, _vp, _i64, C.c_float, _int, _vp, _vp]),
    "gnn_match_fill": (_int, [_vp, _i64, _i64, C.c_float, _int, _vp, _vp, _i64]),
    "gnn_match_count_dev": (_int, [_vp, _vp, _i64, _vp, _i64, C.c_float, _int, _vp, _vp]),
    "gnn_match_fill_dev": (_int, [_vp, _vp, _i64, _vp, _i64, C.c_float, _int, _vp, _vp, _i64]),
    "gnn_debug_match_pass_ms": (_int, [_vp, _vp, _i64, _vp]),
    "gnn_mcl": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gnn_mcl_dev": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gnn_mcl_matrix": (_int, [_vp, _i64, _int, _vp, _vp, _vp]),
    "gnn_debug_mcl_lds": (_int, [_vp, _int]),
    "gnn_debug_mcl_groups": (_int, [_vp, _int]),
    "gnn_debug_mcl_pow": (_int, [_vp, _vp, _i64, _int, _vp]),
    "gnn_debug_mcl_ms": (_int, [_vp, _vp, _i64, _vp]),
    "gnn_debug_mcl_overflow": (_int, [_vp, _vp, _i64, _vp]),
    "gnn_spread": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gnn_spread_dev": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gnn_debug_spread_groups": (_int, [_vp, _int]),
    "gnn_debug_spread_skip": (_int, [_vp, _int]),
    "gnn_debug_spread_ms": (_int, [_vp, _vp, _i64, _vp]),
    "gnn_avglink": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gnn_avglink_dev": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gnn_debug_avglink_slots": (_int, [_vp, _int]),
    "gnn_debug_avglink_wave_rows": (_int, [_vp, _int]),
    "gnn_debug_avglink_groups": (_int, [_vp, _int]),
    "gnn_debug_avglink_order": (_int, [_vp, _vp, _i64, _vp]),
    "gnn_debug_avglink_ms": (_int, [_vp, _vp, _i64, _vp]),
    "gnn_debug_avglink_classes": (_int, [_vp, _vp]),
    "gnn_communities": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gnn_communities_dev": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gnn_label_components": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp]),
    "gnn_label_components_dev": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp]),
    "gnn_debug_communities_slots": (_int, [_vp, _int]),
    "gnn_debug_communities_wave_rows": (_int, [_vp, _int]),
    "gnn_debug_communities_groups": (_int, [_vp, _int]),
    "gnn_debug_communities_gain": (_int, [_vp, _vp, _i64, _vp]),
    "gnn_debug_communities_ms": (_int, [_vp, _vp, _i64, _vp]),
    "gnn_debug_communities_classes": (_int, [_vp, _vp]),
    "gnn_knn_graph_count": (_int, [_vp, _vp, _i64, _int, _int, _int, _int, _vp, _vp]),
    "gnn_knn_graph_fill": (_int, [_vp, _i64, _int, _int, _int, _int, _vp, _vp, _vp, _i64]),
    "gnn_knn_graph_count_dev": (_int, [_vp, _vp, _i64, _int, _int, _int, _int, _vp, _vp]),
    "gnn_knn_graph_fill_dev": (_int, [_vp, _i64, _int, _int, _int, _int, _vp, _vp, _vp, _i64]),
    "gnn_debug_knn_graph_wave_rows": (_int, [_vp, _int]),
    "gnn_debug_knn_graph_group_rows": (_int, [_vp, _int]),
    "gnn_debug_knn_graph_classes": (_int, [_vp, _vp]),
    "gnn_debug_knn_graph_ms": (_int, [_vp, _vp, _i64, _vp]),
    "gnn_tsne": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _int, _int, C.c_double, C.c_float, _vp, _vp, _vp]),
    "gnn_tsne_dev": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _int, _int, C.c_double, C.c_float, _vp, _vp, _vp]),
    "gnn_tsne_forces": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gnn_tsne_forces_dev": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gnn_debug_tsne_split": (_int, [_vp, _int]),
    "gnn_debug_tsne_ms": (_int, [_vp, _vp, _i64, _vp]),
    "gnn_kmeans": (_int, [_vp, _vp, _i64, _int, _vp, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gnn_kmeans_dev": (_int, [_vp, _vp, _i64, _int, _vp, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gnn_centroids": (_int, [_vp, _vp, _i64, _vp, _int, _vp, _vp]),
    "gnn_centroids_dev": (_int, [_vp, _vp, _i64, _vp, _int, _vp, _vp]),
    "gnn_debug_set_kmeans_lds": (_int, [_vp, _int]),
    "gnn_debug_kmeans_pass_ms": (_int, [_vp, _vp, _i64, _vp]),
    "gnn_vote": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _int, C.c_float, _vp, _vp, _vp, _vp]),
    "gnn_vote_dev": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _int, C.c_float, _vp, _vp, _vp, _vp]),
    "gnn_debug_set_vote_lds": (_int, [_vp, _int]),
    "gnn_debug_vote_pass_ms": (_int, [_vp, _vp, _i64, _vp]),
    "gnn_pca_moments": (_int, [_vp, _vp, _i64, _vp, _vp, _vp]),
    "gnn_pca_moments_dev": (_int, [_vp, _vp, _i64, _vp, _vp, _vp]),
    "gnn_pca_project": (_int, [_vp, _vp, _i64, _vp, _int, _vp, _vp]),
    "gnn_pca_project_dev": (_int, [_vp, _vp, _i64, _vp, _int, _vp, _vp]),
    "gnn_debug_set_pca_split": (_int, [_vp, _i64]),
    "gnn_debug_pca_pass_ms": (_int, [_vp, _vp, _i64, _vp]),
    "gnn_embed": (_int, [_vp, _vp, _i64, _int, _int, _vp, _vp]),
    "gnn_embed_dev": (_int, [_vp, _vp, _i64, _int, _int, _vp, _vp]),
    "gnn_debug_forward": (_int, [_vp, _vp, _i64, _int, _vp, C.POINTER(Taps)]),
    "gnn_synth_windows_dev": (_int, [_vp, _u64, _i64, _i64, _vp]),
    "gnn_profile_enable": (_int, [_vp, _int]),
    "gnn_profile_reset": (_int, [_vp]),
    "gnn_profile_get": (_int, [_vp, _int, C.POINTER(C.c_double), C.POINTER(_i64)]),
    "gnn_set_chunk": (_int, [_vp, _i64]),
    "gnn_phase_cycles": (_int, [_vp, _int, C.POINTER(C.c_uint64)]),
    "gnn_mfma_probe": (_int, [_vp, _int, C.POINTER(C.c_double)]),
    "gnn_mfma_probe_kind": (_int, [_vp, _int, _int, C.POINTER(C.c_double)]),
    "gnn_fused_rows_per_step": (_int, [_int]),
    "gnn_debug_set_pad_skip": (_int, [_vp, _int]),
    "gnn_debug_set_time_split": (_int, [_vp, _int]),
    "gnn_debug_last_split": (_int, [_vp, C.POINTER(_int)]),
    "gnn_debug_pack_c6": (_int, [_f32p, _int, _int, C.POINTER(C.c_uint32), _sz, C.POINTER(_sz)]),
    "gnn_crc32c": (C.c_uint32, [_vp, _sz]),
    "gnn_fasta_scan": (_int, [_vp, _i64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "gnn_fasta_pack": (_int, [_vp, _i64, _int, _vp, _vp, _vp, _vp, _i64, C.POINTER(C.c_int64)]),
    "gnn_fasta_accession_digests": (_int, [_vp, _i64, _vp, _i64, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "gnn_comm_unique_id": (_int, [_vp]),
    "gnn_comm_init": (_int, [_vp, _int, _int, _vp]),
    "gnn_comm_destroy": (_int, [_vp]),
    "gnn_comm_info": (_int, [_vp, C.POINTER(_int), C.POINTER(_int)]),
    "gnn_comm_gather_dev": (_int, [_vp, _vp, _vp, _sz, _int]),
    "gnn_comm_gather": (_int, [_vp, _vp, _vp, _sz, _int]),
    "gnn_comm_allgather": (_int, [_vp, _vp, _vp, _sz]),
    "gnn_comm_allreduce_max": (_int, [_vp, C.POINTER(C.c_double), _int]),
    "gnn_comm_barrier": (_int, [_vp]),
    "gnn_branch_attention": (_int, [_vp, _vp, _vp, _vp, _i64, C.c_double, _vp]),
    "gnn_score_calibration": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
}

_lib = None


class GnnError(RuntimeError):
    pass


def load():
    """dlopen the C-ABI library and attach the prototypes.  Raises if it was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.is_file():
        raise GnnError(
            f"{LIB_PATH} not found: build it with genomad_amd/csrc/build.sh (or "
            "python -c 'import __graft_entry__ as g; g.build()').  There is no CPU fallback.")
    lib = C.CDLL(str(LIB_PATH))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def check(rc: int):
    if rc != 0:
        msg = load().gnn_last_error()
        raise GnnError(f"libgenomad_nn_hip error {rc}: {msg.decode() if msg else '?'}")
