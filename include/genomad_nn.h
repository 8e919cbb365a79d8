/*
 * genomad_nn.h — C ABI of libgenomad_nn_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the nn-classification hot path of geNomad.  The reference
 * has no FFI of its own: the seam is the Python function
 *   genomad/modules/nn_classification.py:21-30  main(input_path, output_path, ...)
 * and, inside it, the TensorFlow/numba calls listed per entry point below.  A
 * maintainer binds these functions with ctypes; all arguments
 * are plain pointers and sizes, no torch/numpy types.
 *
 * Conventions: every function returns 0 on success or a negative gnn_status; the
 * message for the last failure on the calling thread is gnn_last_error().  The
 * caller allocates all outputs.  One gnn_ctx is bound to one HIP device and one
 * HIP stream; a ctx is not thread safe, different ctxs are independent (one process
 * per GPU, or one ctx per device in one process).  "host"/"dev" in a parameter name
 * says where the pointer must live.  No exceptions cross the ABI.
 */
#ifndef GENOMAD_NN_H
#define GENOMAD_NN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNN_WINDOW 6000      /* nn_classification.py:68,72  window length / ljust width   */
#define GNN_TOKENS 5997      /* model.py:15                 6000 - 4 + 1 tokens            */
#define GNN_DEPTH 257        /* model.py:11                 one-hot depth (token 0 = N)    */
#define GNN_CH 128           /* model.py:20                 nb_filters_conv1d              */
#define GNN_KSIZE 6          /* model.py:22                 conv1d_kernel                  */
#define GNN_PATCHES 2100     /* model.py:19                 nb_patches                     */
#define GNN_PATCH_SIZE 4     /* igloo.py:33                 patch_size                     */
#define GNN_POOL 8           /* model.py:23                 pooling_size                   */
#define GNN_POOLED 749       /* igloo.py:176                int(5997 / 8)                  */
#define GNN_FEAT 256         /* igloo.py:83                 concat of the two IGLOO heads  */
#define GNN_HIDDEN 512       /* model.py:28,40                                             */
#define GNN_CLASSES 3        /* model.py:44                 chromosome, plasmid, virus     */
#define GNN_EMBED_DIM 512    /* model.py:28                 create_encoder()'s output width (= GNN_HIDDEN) */

typedef enum gnn_status {
    GNN_OK = 0,
    GNN_ERR_ARG = -1,        /* bad argument (null pointer, negative size, bad enum) */
    GNN_ERR_HIP = -2,        /* a HIP runtime call failed (message has the HIP error)  */
    GNN_ERR_STATE = -3,      /* e.g. classify before gnn_load_weights                  */
    GNN_ERR_WEIGHTS = -4,    /* weight tensor invalid (patch index out of range ...)   */
    GNN_ERR_NOMEM = -5
} gnn_status;

/* Arithmetic of the conv / w_v contractions (everything else is always f32). */
typedef enum gnn_precision {
    GNN_PREC_F32 = 0,        /* f32 reference path: unfused f32 kernels, activations in HBM   */
    GNN_PREC_BF16X3 = 1,     /* fused path: split-bf16 (hi+lo), 3 MFMA passes, f32 accumulate (gnn_fused_x3.hip); f32 range:
                                what main() recomputes a batch with when an f16-operand mode returns non-finite scores */
    GNN_PREC_BF16 = 2,       /* REMOVED in round 6 (single bf16 MFMA pass, 7e-3: a roofline experiment).  The value is kept so that
                                an old caller gets GNN_ERR_STATE with a message instead of another arithmetic                    */
    GNN_PREC_F16C8 = 3,      /* REMOVED in round 6 (f16 + MX-fp8 correction MFMAs, 1.3e-4 on 10^6 windows).  GNN_ERR_STATE          */
    GNN_PREC_F16C6 = 5,      /* FROZEN opt-in fast mode (gnn_fused_c6.hip, not tuned any more): one f16 MFMA pass + MX-scaled fp6
                                (e2m3) correction MFMAs, both operands block scaled = 1.5 pass equivalents; 8.2e-5 on config 2,
                                1.2e-4 on a few of 10^6 windows - NO head-room under the 1e-4 tolerance (bench.py exits non-zero
                                with it), so it cannot be a default; needs |activation| < 65504 and a 4-byte aligned buffer   */
    GNN_PREC_F16X3TC = 6,    /* THE DEFAULT of main(), NNEngine and bench.py since round 4 (gnn_fused_tc.hip): the F16X3 arithmetic (split-f16
                                hi + lo limbs, three MFMA products per operand pair, f32 accumulate) with conv2 / conv3 evaluated by
                                Toom-Cook minimal filtering F(3,6) over the time axis - 0.444x their MFMAs, f32 transforms; y @ w_v direct,
                                logits GEMM split-f16 x 3 on the matrix pipe, dense head exact f32.  Class scores as F16X3's: within
                                2e-5 / 4e-5 of the exact-f32 path on every one of 10^6 windows for two weight sets
                                (profiles/r04_tails.txt).  Needs |activation| < ~2000 (the transformed activations, up to 32x the
                                activations, are f16 operands): beyond that the scores are non-finite, never silently wrong, and
                                main() recomputes the batch along the chain F16X3TC -> F16X3 (f16 range, 65504) -> BF16X3 (f32
                                range), logging every hop with the arithmetic that failed.  Since round 6 head A's y @ w_v rows
                                are not computed but gathered from a 1.38 GB table of all 9-mers that gnn_load_weights builds on
                                the device (x1[t] is a function of the bases t-5 .. t+3; f64 accumulation, rounded once).  A window
                                buffer that is not 4-byte aligned goes through one aligned staging copy and the same kernel: the
                                scores do not depend on the buffer's address                                                   */
    GNN_PREC_F16X3TK = 7,    /* round 6 (gnn_fused_tk.hip): F16X3TC with everything that is a function of a short k-mer READ FROM TABLES IN HBM
                                instead of computed - x2[t] = LeakyReLU(conv2(x1))[t] depends on the bases t-10 .. t+3, so conv2 (43 % of a
                                window's FLOPs) is one 512-byte row gather per position from a table of all 4^14 fourteen-mers (137.4 GB),
                                head A's pair products one 4-byte read per entry from an (entry, 9-mer) table (8.8 GB), rows no 14-mer
                                indexes (window starts, k-mers with a non-ACGT byte) <= 6 row reads of conv2's tap tables (8.3 GB); conv3 and head B's
                                y @ w_v stay on the matrix pipe with the F16X3TC arithmetic.  The tables are built on the device by
                                gnn_build_kmer_tables (f64 accumulation, rounded once: closer to exact f32 than the three f16 products);
                                without them this value answers GNN_ERR_STATE and the caller stays on F16X3TC.  Same range rule as F16X3TC */
    GNN_PREC_F16X3 = 4       /* the direct three-pass form (gnn_fused_x3.hip), the default of round 3: split-f16 (hi+lo, 11+11 significant
                                bits), 3 MFMA passes, logits GEMM split-f16 x 3 on the matrix pipe, dense head exact f32: f32-class
                                accuracy (within 2e-5 of the exact-f32 path on every one of 10^6 windows); needs |activation| < 65504
                                (f16 range)                                   */
} gnn_precision;

/* Kept for ABI compatibility: rounds 4 and 5 could link an experimental f16c8 kernel (GNN_EXPERIMENTAL=1); round 6 deleted it
 * together with the round-1 kernel.  Always 0. */
int gnn_has_experimental(void);

typedef enum gnn_onehot_dtype { GNN_OH_U8 = 0, GNN_OH_BF16 = 1, GNN_OH_F32 = 2 } gnn_onehot_dtype;

/* dtype of an embedding row: f32, or bf16 (the f32 value rounded to nearest even; a NaN stays a NaN) */
typedef enum gnn_emb_dtype { GNN_EMB_F32 = 0, GNN_EMB_BF16 = 1 } gnn_emb_dtype;

/*
 * Weights in the reference's own layouts (what Keras load_weights would put into the
 * graph of model.py:34-45; nn_classification.py:309-310).  All pointers are HOST
 * pointers, C-contiguous, float32 unless noted; the library copies and re-packs them.
 */
typedef struct gnn_igloo_weights {
    const int32_t* patches;  /* (2100,4,1) int32  igloo.py:129-135 "random_patches" */
    const float* w_mult;     /* (1,2100,4,128)    igloo.py:137-143                  */
    const float* w_summer;   /* (1,512,1)         igloo.py:144-150                  */
    const float* w_bias;     /* (1,2100)          igloo.py:166-172                  */
    const float* w_qk;       /* (2100,749)        igloo.py:174-180                  */
    const float* w_v;        /* (1,128,128)       igloo.py:182-188                  */
} gnn_igloo_weights;

typedef struct gnn_dense_bn {
    const float* kernel;     /* (in,out) Keras Dense kernel          model.py:28,40 */
    const float* bias;       /* (out,)                                              */
    const float* gamma;      /* (out,) BatchNormalization, eps=1e-3  model.py:29,41 */
    const float* beta;
    const float* mean;       /* moving_mean     */
    const float* var;        /* moving_variance */
} gnn_dense_bn;

typedef struct gnn_weights {
    const float* conv1_kernel;   /* (6,257,128)  igloo.py:45-47 on the one-hot input */
    const float* conv1_bias;     /* (128,)                                           */
    const float* conv2_kernel;   /* (6,128,128)  igloo.py:66 (loop iteration 1)      */
    const float* conv2_bias;
    const float* conv3_kernel;   /* (6,128,128)  igloo.py:66 (loop iteration 2)      */
    const float* conv3_bias;
    gnn_igloo_weights igloo_a;   /* igloo.py:54-62, applied to conv1 output           */
    gnn_igloo_weights igloo_b;   /* igloo.py:73-81, applied to conv3 output           */
    gnn_dense_bn enc;            /* Dense(512)+BN, in=256   model.py:28-30            */
    gnn_dense_bn head;           /* Dense(512)+BN, in=512   model.py:40-42            */
    const float* out_kernel;     /* (512,3)                 model.py:44               */
    const float* out_bias;       /* (3,)                                              */
} gnn_weights;

/* Host pointers that receive intermediates of gnn_debug_forward (any may be NULL). */
typedef struct gnn_taps {
    float* x1;       /* (n,5997,128) conv1+LeakyReLU            (F32 path only) */
    float* x2;       /* (n,5997,128)                            (F32 path only) */
    float* x3;       /* (n,5997,128)                            (F32 path only) */
    float* m_a;      /* (n,2100)   igloo.py:205-206 "mpi" of head A             */
    float* m_b;
    float* yp_a;     /* (n,749,128) max-pooled y @ w_v   igloo.py:208-210       */
    float* yp_b;
    float* alpha_a;  /* (n,749)    igloo.py:211-212                             */
    float* alpha_b;
    float* feat;     /* (n,256)    igloo.py:83 concat                           */
} gnn_taps;

typedef struct gnn_ctx gnn_ctx;

/* ---- life cycle -------------------------------------------------------------------- */
const char* gnn_last_error(void);
int gnn_version(void);
int gnn_device_count(int* count);
int gnn_create(int device, gnn_ctx** out);
int gnn_destroy(gnn_ctx* ctx);
int gnn_sync(gnn_ctx* ctx);                      /* hipStreamSynchronize on the ctx stream */
int gnn_device_info(gnn_ctx* ctx, char* name, size_t name_len, int* cus, int64_t* hbm_bytes);
int gnn_device_pci_bus_id(gnn_ctx* ctx, char* out, size_t out_len);   /* "0000:05:00.0" of the ctx's device (hipDeviceGetPCIBusId): what bench.py
                                                                         prints per rank, so that two ranks bound to one GPU are visible */
int gnn_device_mem_info(gnn_ctx* ctx, int64_t* free_bytes, int64_t* total_bytes);   /* hipMemGetInfo of the ctx's device (what the default launch size is clamped against) */

/* replaces nn_model.load_weights(GenomadData.nn_model_file), nn_classification.py:310 */
int gnn_load_weights(gnn_ctx* ctx, const gnn_weights* w);

/* The k-mer tables of GNN_PREC_F16X3TK: gnn_kmer_tables_bytes() bytes (155.9 GB) of device memory + 1.7 GB of temporaries while they
 * are built (about a second).  reserve_bytes = device memory that must stay free behind them (the workspaces of the launches to come and
 * the caller's own buffers; < 0 = the library's default: two workspaces of the ctx's launch size + 8 GiB).  GNN_ERR_NOMEM - nothing
 * allocated, message says how much is missing - on a device that cannot hold them: the caller keeps GNN_PREC_F16X3TC.  Idempotent.
 * gnn_drop_kmer_tables frees them (gnn_destroy does too). */
int gnn_build_kmer_tables(gnn_ctx* ctx, int64_t reserve_bytes);
int gnn_has_kmer_tables(gnn_ctx* ctx);
int gnn_drop_kmer_tables(gnn_ctx* ctx);
int64_t gnn_kmer_tables_bytes(void);
/* test aid: which = 0: row `row` (a 14-mer, first base in the top two of 28 bits; 4^14 = the all-N-token row) of the x2 table -> 128
 * floats; which = 1: head A's table, entry row >> 32 at the 9-mer row & 0xffffffff (4^9 = all-N-token) -> 1 float */
int gnn_debug_kmer_table_row(gnn_ctx* ctx, int which, uint64_t row, float* out_host);

/* ---- raw device memory (so a ctypes host needs no torch for buffers) ------------------ */
int gnn_dev_alloc(gnn_ctx* ctx, size_t bytes, void** dev_ptr);
int gnn_dev_free(gnn_ctx* ctx, void* dev_ptr);
int gnn_memcpy_h2d(gnn_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int gnn_memcpy_d2h(gnn_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);

/* ---- hot path ------------------------------------------------------------------------ */
/* replaces sequence.tokenize_dna(window, 4) (sequence.py:170-193) on n padded, upper-cased
 * 6000-byte windows: tokens_out[n][5997] in [0,256].  Host in / host out. */
int gnn_tokenize(gnn_ctx* ctx, const uint8_t* bases_host, int64_t n_windows, uint16_t* tokens_host);
int gnn_tokenize_dev(gnn_ctx* ctx, const uint8_t* bases_dev, int64_t n_windows, uint16_t* tokens_dev);

/* replaces OneHotLayer (model.py:9-11): bases -> tokens -> one-hot depth 257, written to
 * onehot_dev[n][5997][257] of the requested dtype (device pointer, caller-allocated). */
int gnn_onehot_dev(gnn_ctx* ctx, const uint8_t* bases_dev, int64_t n_windows, int onehot_dtype,
                   void* onehot_dev);

/* replaces the predict loop nn_classification.py:316-317 (+ tokenisation :72-73):
 * scores[n][3] = softmax class scores per window.  precision: gnn_precision. */
int gnn_classify(gnn_ctx* ctx, const uint8_t* bases_host, int64_t n_windows, int precision,
                 float* scores_host);
/* gnn_classify_dev_async: the same, but the back end (pair-product reduction, logits, attention sum, dense head) of the call's
 * last chunk may still be running on the library's second stream when the call returns, beside the front end of the NEXT
 * asynchronous call — for loops over batches that fit one launch.  scores_dev is complete once gnn_classify_flush (or any
 * other entry point of this ctx: gnn_sync, gnn_memcpy_d2h, gnn_comm_gather_dev, gnn_classify_dev ...) has been called — they
 * wait on the host for what is pending on the second stream — and the ctx stream has been synchronised; results are
 * bit-identical to gnn_classify_dev (bench.py checks every window of every run).  Worth +8-10 % for F16C6 at 2048 windows per
 * call, nothing for the power-bound default arithmetic.
 * Debug switches of the library (environment, read once): GNN_NO_BACKEND_OVERLAP=1 keeps every back end on the ctx stream;
 * GNN_BACKEND_OVERLAP=1 also overlaps the chunks of a synchronous multi-chunk call (the policy of rounds 2-4, slower beside the
 * power-bound default kernel: profiles/r04/backend_overlap_ab.txt);
 * GNN_DEBUG_POISON=1 fills the workspaces with NaN patterns before every launch (a kernel reading what its launch has not
 * written turns the scores into NaN); GNN_X3_ROUND1=1 serves F16X3 / BF16X3 with the round-1 kernel (A/B measurements);
 * GNN_NO_PAD_SKIP=1 / GNN_NO_TIME_SPLIT=1 start every ctx with the padding skip / the time split off (gnn_debug_set_*);
 * GNN_LOGITS_F32=1 keeps the logits GEMM on the f32 FMA path.  Each switch is read once and announced on stderr.
 * Memory: the asynchronous entry point alternates TWO workspaces (2 x 0.86 MB per window of a launch, see gnn_set_chunk). */
int gnn_classify_dev_async(gnn_ctx* ctx, const uint8_t* bases_dev, int64_t n_windows, int precision, float* scores_dev);
int gnn_classify_flush(gnn_ctx* ctx);

int gnn_classify_dev(gnn_ctx* ctx, const uint8_t* bases_dev, int64_t n_windows, int precision,
                     float* scores_dev);   /* asynchronous on the ctx stream */

/* ---- encoder embeddings: create_encoder()'s output (model.py:14-31: one-hot -> IGLOO block -> Dense512 -> BatchNorm -> ReLU),
 * the h1 of the dense head, which the classifier (model.py:34-45) reads and then drops.  The same forward pass as gnn_classify:
 * emb[n][GNN_EMBED_DIM] of emb_dtype (gnn_emb_dtype) per window, and - when the scores pointer is not NULL - the class scores,
 * bit-identical to gnn_classify / gnn_classify_dev.  A NaN of an f16 arithmetic's overflow stays a NaN in both (the range fallback
 * of main() recomputes the batch).  GNN_PREC_F16C6 (frozen, outside the tolerance) has no embedding path: GNN_ERR_ARG.
 * gnn_embed: host pointers, synchronous, chunked like gnn_classify.  gnn_embed_dev: device pointers, asynchronous on the ctx
 * stream like gnn_classify_dev. */
int gnn_embed(gnn_ctx* ctx, const uint8_t* bases_host, int64_t n_windows, int precision, int emb_dtype, void* emb_host,
              float* scores_host_or_null);
int gnn_embed_dev(gnn_ctx* ctx, const uint8_t* bases_dev, int64_t n_windows, int precision, int emb_dtype, void* emb_dev,
                  float* scores_dev_or_null);

/* replaces tf.math.segment_mean(pred, contig_ids) nn_classification.py:320.
 * ids sorted ascending, out has n_segments rows (zero row for an id with no window). */
int gnn_segment_mean(gnn_ctx* ctx, const float* scores_host, const int64_t* ids_host, int64_t n,
                     int64_t n_segments, float* out_host);

/* ---- contig front end: windows are spans of one packed contig buffer ------ */
/* counts[i] = number of bytes equal to `byte` in seq_dev[starts[i] .. starts[i]+lens[i]); used for the
 * window skip rule `window_n > 0 and seq_window.count("N") > 4000` (nn_classification.py:70-71, counted
 * on the raw, not upper-cased, sequence: sequence.py:38-39). */
int gnn_span_byte_count(gnn_ctx* ctx, const uint8_t* seq_dev, const int64_t* starts_host,
                        const int32_t* lens_host, int64_t n_spans, int byte, int32_t* counts_host);
/* replaces seq_window.seq_ascii.ljust(6000, b"N") + tokenize + predict for windows given as spans
 * (start, len <= 6000) of the raw contig buffer on the device (nn_classification.py:72-73, :316-317):
 * each span is upper-cased (sequence.py:35-36) and right-padded with 'N' on the device. */
int gnn_classify_spans(gnn_ctx* ctx, const uint8_t* seq_dev, const int64_t* starts_host,
                       const int32_t* lens_host, int64_t n_spans, int precision, float* scores_host);

/* The whole contig front end in one call: replaces generate_data (window cutting seq_windows(seq, 6000, 2500,
 * max_windows), the skip rule, upper-casing, padding, tokenising: nn_classification.py:54-82), the predict loop
 * (:316-318) and tf.math.segment_mean (:320) for a packed buffer of raw contig bytes: contig c =
 * seq[offsets[c] .. offsets[c+1]) (n_contigs + 1 offsets, non-decreasing).  seq is a HOST pointer when
 * seq_on_host != 0 (uploaded in pieces on a copy stream while earlier pieces are classified) and a device
 * pointer otherwise.  contig_scores_host[n_contigs][3] = mean class scores of the contig's kept windows;
 * window_ids_host (capacity >= number of CANDIDATE windows, sum over contigs of ceil(len / 6000) is enough)
 * receives the contig index of every KEPT window in order, *n_windows_out their number — the `contig_ids` the
 * reference stores in <prefix>_seq_window_id.npz.  Window scores never leave the device; every buffer is
 * persistent in the ctx.  Synchronous (returns when the scores are on the host). */
int gnn_classify_contigs(gnn_ctx* ctx, const uint8_t* seq, int seq_on_host, int64_t seq_bytes,
                         const int64_t* offsets_host, int64_t n_contigs, int single_window, int precision,
                         float* contig_scores_host, int64_t* window_ids_host, int64_t ids_capacity,
                         int64_t* n_windows_out);
/* gnn_classify_contigs plus the per-contig embedding: contig_emb_host[n_contigs][GNN_EMBED_DIM] f32 = mean of the encoder
 * embeddings (see gnn_embed) of the contig's KEPT windows - the windows and the N rule of the scores' mean - and a zero row for a
 * contig without one.  Window embeddings are folded into per-contig f32 sums on the device after every slab of windows, added in
 * window order (a contig may straddle slabs), so the result does not depend on gnn_set_chunk; they never leave the device.
 * Scores and window ids are bit-identical to gnn_classify_contigs.  GNN_PREC_F16C6: GNN_ERR_ARG. */
int gnn_classify_contigs_embed(gnn_ctx* ctx, const uint8_t* seq, int seq_on_host, int64_t seq_bytes,
                               const int64_t* offsets_host, int64_t n_contigs, int single_window, int precision,
                               float* contig_scores_host, int64_t* window_ids_host, int64_t ids_capacity,
                               int64_t* n_windows_out, float* contig_emb_host);

/* ---- score tracks: the contig front end at a stride ("Score tracks along contigs") -----------------------------------
 * Overlapping 6000-base windows every `stride` bases (1 <= stride <= 6000) along every contig, each scored by the same forward
 * pass as gnn_classify, folded into one score triple per stride-wide bin.  For a contig of length L > 0:
 *   windows  window k starts at k * stride and is min(6000, L - k * stride) long.  Window 0 always exists; window k > 0 exists
 *            while no earlier window reached the contig's end ((k - 1) * stride + 6000 < L) and it is at least 2500 long;
 *            single_window keeps window 0 only.  At stride 6000: seq_windows(seq, 6000, 2500, max_windows), the table of
 *            gnn_classify_contigs.  Content: the span upper-cased and right-padded with 'N', as gnn_classify_spans.
 *   kept     window k is kept unless k > 0 and it holds more than 4000 literal 'N' bytes (the rule of gnn_classify_contigs).  Every
 *            window is scored; kept is a mask.
 *   bins     bin b = [b * stride, min((b + 1) * stride, L)), ceil(L / stride) of them.  Window k covers bin b iff k <= b and
 *            b * stride < k * stride + its length.  track[b][c] = f32 sum, in increasing k, of class c over the kept windows that
 *            cover b, divided once by their number cover[b]; NaN in all three classes where cover[b] == 0 (a dropped tail, or every
 *            covering window masked).
 *   contig   mean over the contig's kept scan windows, in the arithmetic and order of gnn_classify_contigs (bit-identical to it at
 *            stride 6000); a zero row for a contig without a window.
 * gnn_scan_plan - host only, no ctx, no GPU - answers the sizes: the number of windows and bins of all contigs, and, where the
 * pointers are not NULL, the CSR offsets per contig (n_contigs + 1 entries each) and the contig-relative start and the length of
 * every window (*n_windows_out entries: call once for the sizes, then again with the arrays).  GNN_ERR_ARG for a stride outside
 * [1, 6000] or decreasing offsets. */
int gnn_scan_plan(const int64_t* offsets_host, int64_t n_contigs, int stride, int single_window, int64_t* n_windows_out,
                  int64_t* n_bins_out, int64_t* win_offsets_or_null, int64_t* bin_offsets_or_null, int64_t* starts_or_null,
                  int32_t* lens_or_null);
/* The scan of a packed contig buffer (seq, seq_on_host, seq_bytes, offsets_host as gnn_classify_contigs; every arithmetic it
 * accepts).  window_scores_host[n_windows][3] and window_kept_host[n_windows] (1 = kept) in the order of gnn_scan_plan, capacity
 * windows_capacity windows; track_host[n_bins][3] and cover_host[n_bins], capacity bins_capacity bins; contig_scores_host
 * [n_contigs][3].  Every output except window_scores_host may be NULL; a capacity that is too small is GNN_ERR_ARG and the message
 * names the size needed.  Synchronous.  Device memory, persistent in the ctx and grow-only: the 40 B per window of
 * gnn_classify_contigs' own table (spans, N counts, 12 B of scores - the scan adds nothing per window) and 16 B per bin.  Overlapping windows are
 * classified independently: a scan at stride S costs 6000 / S times the windows of gnn_classify_contigs. */
int gnn_scan_contigs(gnn_ctx* ctx, const uint8_t* seq, int seq_on_host, int64_t seq_bytes, const int64_t* offsets_host,
                     int64_t n_contigs, int stride, int single_window, int precision, float* window_scores_host,
                     uint8_t* window_kept_host_or_null, int64_t windows_capacity, float* track_host_or_null,
                     int32_t* cover_host_or_null, int64_t bins_capacity, float* contig_scores_host_or_null);

/* ---- both strands: reverse-complement windows on the device ("Both strands") ------------------------------------------
 * The classifier is not strand-symmetric (causal convolutions, window-relative patch positions): a window and its reverse
 * complement are two inputs, and which strand a contig was written on is arbitrary.  These entry points score either strand, or
 * both and their mean, with the forward pass of gnn_classify.
 *   complement   of an upper-cased byte: A <-> T, C <-> G, every other byte unchanged.  The tokenizer maps any non-ACGT byte to
 *                token 0 on either strand, so an IUPAC-exact table would change no score.
 *   reverse      window of a span (start, len <= 6000) of the packed buffer: out[i] = comp(upper(seq[start + len - 1 - i])) for
 *                i < len and 'N' for len <= i < 6000 - right-padded like the forward window; the pad is NOT reversed to the front.
 *   windows      spans, window ids, bins and the kept mask are the FORWARD ones: the reverse complement is taken per window, not per
 *                contig (a reverse-complemented contig would be cut into other windows).  The N rule counts literal 'N' once on the
 *                raw forward span - N maps to N, so the count is that of the reverse window too.  window ids, kept, the CSR offsets
 *                and cover therefore do not depend on the strand, and every output aligns element by element.
 *   modes        gnn_strand.  Window score under GNN_STRAND_BOTH: (f + r) * 0.5f per class in f32 - one rounding.
 *   contig       the masked mean of gnn_classify_contigs over the kept windows' scores OF THE MODE: under BOTH the mean of the
 *                combined window scores, not the half-sum of the two contig means.  Track: the fold of gnn_scan_contigs over them.
 *   embedding    per strand the slab fold of gnn_classify_contigs_embed into its own f32 sum: REVERSE = sum_r / kept, BOTH =
 *                (sum_f + sum_r) / (2 kept) - two independent sums, so independent of gnn_set_chunk; zero row without a kept window.
 * GNN_STRAND_FORWARD is bit-identical to the entry points without a strand.  A strand is computed when the mode needs it or one of
 * its own output buffers is given (REVERSE with contig_scores_fwd_host: both strands run, the mode's outputs are the reverse ones).
 * When both run, a slab's forward and reverse windows go through the front end as one batch, forward windows first; the front
 * ends are batch-invariant, so no score depends on it.  A strand outside the enum: GNN_ERR_ARG, the message names the value.
 * Device memory, persistent in the ctx and grow-only: 24 B per window (reverse and combined scores), 12 B per window of one slab,
 * 24 B per contig, and a second embedding sum (2 KB per contig) when an embedding is asked for under REVERSE or BOTH. */
typedef enum gnn_strand { GNN_STRAND_FORWARD = 0, GNN_STRAND_REVERSE = 1, GNN_STRAND_BOTH = 2 } gnn_strand;
/* The building block and the window-level route: bases_dev_out[n_spans][6000] = the reverse windows of the spans (start, len) of
 * seq_dev, ready for gnn_classify_dev / gnn_embed_dev.  bases_dev_out: device pointer, 4-byte aligned.  Spans as
 * gnn_classify_spans (host arrays, lengths in [0, 6000]).  Returns when the windows are written. */
int gnn_revcomp_spans_dev(gnn_ctx* ctx, const uint8_t* seq_dev, const int64_t* starts_host, const int32_t* lens_host, int64_t n_spans,
                          uint8_t* bases_dev_out);
/* gnn_classify_contigs_embed with a strand: contig_scores_host, and contig_emb_host_or_null (may be NULL: no embedding is computed;
 * with it GNN_PREC_F16C6 is GNN_ERR_ARG) carry the mode; window ids as gnn_classify_contigs.  contig_scores_fwd_host_or_null /
 * contig_scores_rev_host_or_null [n_contigs][3]: each strand's own masked mean. */
int gnn_classify_contigs_strand(gnn_ctx* ctx, const uint8_t* seq, int seq_on_host, int64_t seq_bytes, const int64_t* offsets_host,
                                int64_t n_contigs, int single_window, int precision, float* contig_scores_host,
                                int64_t* window_ids_host, int64_t ids_capacity, int64_t* n_windows_out, float* contig_emb_host_or_null,
                                int strand, float* contig_scores_fwd_host_or_null, float* contig_scores_rev_host_or_null);
/* gnn_scan_contigs with a strand: window_scores_host, track_host, contig_scores_host carry the mode; kept and cover are those of
 * gnn_scan_contigs.  window_scores_fwd_host_or_null / window_scores_rev_host_or_null [n_windows][3] (capacity windows_capacity):
 * each strand's own window scores. */
int gnn_scan_contigs_strand(gnn_ctx* ctx, const uint8_t* seq, int seq_on_host, int64_t seq_bytes, const int64_t* offsets_host,
                            int64_t n_contigs, int stride, int single_window, int precision, float* window_scores_host,
                            uint8_t* window_kept_host_or_null, int64_t windows_capacity, float* track_host_or_null,
                            int32_t* cover_host_or_null, int64_t bins_capacity, float* contig_scores_host_or_null, int strand,
                            float* window_scores_fwd_host_or_null, float* window_scores_rev_host_or_null);

/* ---- occlusion maps: per-block score change along contigs ("Occlusion maps") -------------------------------------------
 * Which bases a score rests on, answered with the forward pass of gnn_classify alone: mask a block of a window with 'N' - the
 * model's own "unknown": every 4-mer that touches a non-ACGT byte is token 0, and 'N' is the byte short windows are padded with -
 * score the window again and report how far each class moved.
 *   block     B, 1 <= B <= 6000.
 *   windows   the table of gnn_classify_contigs: seq_windows(seq, 6000, 2500, max_windows) per contig, honouring single_window.
 *             Window ids, the N rule and the kept mask are unchanged.  Every window is occluded; kept is a mask, as in the scan.
 *   blocks    window i of length len_i has nb_i = ceil(len_i / B) blocks; block j is the window-relative interval
 *             [j B, min((j + 1) B, len_i)).  The pad is never a block.
 *   pairs     all (window, block) pairs in window order, then block order: P = sum nb_i, indexed through the CSR
 *             blk_offsets[n_windows + 1].
 *   occluded  window: the forward window as gnn_classify_spans materialises it (upper-cased, right-padded with 'N') with the
 *             block's bytes set to 'N'.
 *   delta     delta[p][c] = base[i][c] - occ[p][c], one f32 subtraction; base is the window's ordinary score.  Positive: the block
 *             supports class c.  A block that holds no ACGT byte yields exactly +0.0: its tokens are the window's own, and every
 *             arithmetic is batch-invariant.
 *   identity  base is bit-identical to gnn_scan_contigs at stride 6000, the contig scores and kept to gnn_classify_contigs, occ to
 *             gnn_classify on the same bytes - whatever gnn_set_chunk, where seq lives, or what ran on the ctx before.
 * Cost: 1 + ceil(6000 / B) forward passes per full window.  Forward strand only.
 * gnn_occlusion_plan - host only, no ctx, no GPU, like gnn_scan_plan - answers the sizes: the number of windows and of pairs, and,
 * where the pointers are not NULL, win_offsets (n_contigs + 1), the contig-relative start and the length of every window
 * (*n_windows_out entries) and blk_offsets (*n_windows_out + 1): call once for the sizes, then again with the arrays.  GNN_ERR_ARG
 * (the message says [1, 6000]) for a block outside that range, and for decreasing offsets. */
int gnn_occlusion_plan(const int64_t* offsets_host, int64_t n_contigs, int block, int single_window,
                       int64_t* n_windows_out, int64_t* n_pairs_out, int64_t* win_offsets_or_null,
                       int64_t* starts_or_null, int32_t* lens_or_null, int64_t* blk_offsets_or_null);
/* The building block, the counterpart of gnn_revcomp_spans_dev: bases_dev_out[n_spans][6000] = each span (start, len) of seq_dev
 * materialised with the window-relative interval [lo, hi) set to 'N', ready for gnn_classify_dev / gnn_embed_dev.  0 <= lo <= hi <=
 * 6000; an empty interval gives the plain forward window, an interval that reaches into the pad changes nothing there.
 * bases_dev_out: device pointer, 4-byte aligned.  Spans as gnn_classify_spans (host arrays, lengths in [0, 6000]); a violation is
 * GNN_ERR_ARG and the message names the offending value.  Returns when the windows are written. */
int gnn_occlude_spans_dev(gnn_ctx* ctx, const uint8_t* seq_dev, const int64_t* starts_host, const int32_t* lens_host,
                          const int32_t* lo_host, const int32_t* hi_host, int64_t n_spans, uint8_t* bases_dev_out);
/* The occlusion map of a packed contig buffer (seq, seq_on_host, seq_bytes, offsets_host as gnn_scan_contigs; every arithmetic
 * gnn_classify_contigs accepts).  window_scores_host[n_windows][3] (base) and window_kept_host[n_windows] (1 = kept) in the order of
 * gnn_occlusion_plan, capacity windows_capacity windows; delta_host[n_pairs][3], capacity pairs_capacity pairs; contig_scores_host
 * [n_contigs][3].  A capacity that is too small is GNN_ERR_ARG and the message names the size needed; n_contigs == 0, or no window
 * at all, is GNN_OK.  Synchronous.  The base windows go first; then the pairs in slabs of at most 4 launches, each materialised,
 * scored, differenced and copied out.  Device memory, persistent in the ctx and grow-only, does not grow with the number of pairs:
 * 6000 B + 12 B per pair of ONE slab, the 40 B per window of gnn_classify_contigs' table and 8 B per window of blk_offsets. */
int gnn_occlude_contigs(gnn_ctx* ctx, const uint8_t* seq, int seq_on_host, int64_t seq_bytes, const int64_t* offsets_host,
                        int64_t n_contigs, int block, int single_window, int precision, float* window_scores_host,
                        uint8_t* window_kept_host_or_null, int64_t windows_capacity, float* delta_host,
                        int64_t pairs_capacity, float* contig_scores_host_or_null);

/* ---- attention contribution maps: each pooled position's share of a logit ("Attention contribution maps") -------------
 * The encoder ends in two attention sums over 749 pooled positions, feat[h*128 + ch] = sum_q alpha[h][q] yp[h][q][ch] (h = head A, B;
 * igloo.py:208-214), and the dense head behind them is piecewise linear.  For the window's own ReLU pattern logit_c = g_c . feat +
 * bias_c with g_c = d logit_c / d feat, so every logit decomposes exactly, signed and per class, over (head, pooled position):
 *   contrib   contrib[h][q][c] = alpha[h][q] * sum_ch yp[h][q][ch] g_c[h*128 + ch]; sum_h sum_q contrib + bias_c = logit_c.
 *             Gradient x input at the attention layer with alpha held fixed, in logit units; bias is the same-sign-pattern remainder.
 *   masks     the device's own: a hidden unit is active iff the value the dense head stores for it is > 0.
 *   bins      `bin` pooled positions per output bin, 1 <= bin <= 749: nb = ceil(749 / bin), bin b = [b bin, min((b + 1) bin, 749)),
 *             the last one may be short.  A position's value does not depend on bin: the map at bin = k is, bit for bit, the f32
 *             sums in increasing q of the bin = 1 map.
 *   position  q of either head is the max-pool of tokens 8q .. 8q + 7, whose 4-mers span bases 8q .. 8q + 10; each token's features
 *             see further back through the causal convolutions (5 tokens for head A, 15 for head B).  Tokens 5992 .. 5996 belong to
 *             no position.  The pad positions of a short window carry contributions like any other.
 *   not       a prediction of what an edit would do: alpha depends on the whole window (gnn_occlude_contigs answers that).
 * Costs no extra forward pass: the maps are computed from the back end's workspace of the launch that scores the window; the scores
 * of this path are bit-identical to gnn_classify.  Every arithmetic with the f32 dense head; GNN_PREC_F16C6: GNN_ERR_ARG, the
 * message names it.  A bin outside [1, 749]: GNN_ERR_ARG, the message gives the range.  Forward strand only.
 * contrib[n][2][nb][3] f32; bias[n][3], logits[n][3] (pre-softmax) and scores[n][3] may be NULL.
 * gnn_attribute: host pointers, synchronous, chunked like gnn_embed.  gnn_attribute_dev: device pointers, asynchronous on the ctx
 * stream like gnn_embed_dev. */
int gnn_attribute(gnn_ctx* ctx, const uint8_t* bases_host, int64_t n_windows, int precision, int bin, float* contrib_host,
                  float* bias_host_or_null, float* logits_host_or_null, float* scores_host_or_null);
int gnn_attribute_dev(gnn_ctx* ctx, const uint8_t* bases_dev, int64_t n_windows, int precision, int bin, float* contrib_dev,
                      float* bias_dev_or_null, float* logits_dev_or_null, float* scores_dev_or_null);
/* The maps of a packed contig buffer (seq, seq_on_host, seq_bytes, offsets_host as gnn_classify_contigs).  The window table is that
 * of gnn_classify_contigs: its sizes, starts and lengths are gnn_scan_plan's at stride 6000.  Every window is attributed; kept is a
 * mask, as in the scan.  contrib_host[n_windows][2][nb][3], capacity windows_capacity windows - too small is GNN_ERR_ARG and the
 * message names the size needed; bias, logits, window_scores [n_windows][3], window_kept [n_windows], contig_scores [n_contigs][3] may
 * be NULL.  Window scores are bit-identical to gnn_scan_contigs at stride 6000, contig scores and kept to gnn_classify_contigs, maps,
 * bias and logits to gnn_attribute on the same bytes.  Synchronous.  The maps are copied out slab by slab (4 launches): device
 * memory, persistent in the ctx and grow-only, is 24 nb + 24 B per window of ONE slab beside gnn_classify_contigs' own tables. */
int gnn_attribute_contigs(gnn_ctx* ctx, const uint8_t* seq, int seq_on_host, int64_t seq_bytes, const int64_t* offsets_host,
                          int64_t n_contigs, int bin, int single_window, int precision, float* contrib_host, int64_t windows_capacity,
                          float* bias_host_or_null, float* logits_host_or_null, float* window_scores_host_or_null,
                          uint8_t* window_kept_host_or_null, float* contig_scores_host_or_null);

/* ---- region calls along contigs: Viterbi over score tracks ----------------------------------------------------------
 * From a track to "bins 41-78 of this contig look viral": a segmentation with a switch cost, one 3-state Viterbi path per contig,
 * bit-exact.  The input is any track (gnn_scan_contigs, gnn_scan_contigs_strand under any mode).
 * Inputs.
 *   - track[n_bins][3] f32 and bin_offsets[n_contigs + 1], the CSR of gnn_scan_plan / gnn_scan_contigs.
 *   - A switch penalty `penalty`, a double, 0 <= penalty <= 4096, in units of score x bins.
 * Emissions (exact, no transcendental on either side).
 *   - Bin b is an *evidence* bin iff all three values of track[b] are finite.
 *   - For an evidence bin, q[b][s] = rint(min(max(track[b][s], 0), 1) * 2^20) as an integer.  The f32 product with a power of two
 *     is exact, and the rounding is to nearest, ties to even.
 *   - For any other bin q[b][.] = 0.  This covers an uncovered bin (NaN by construction) and a NaN from an f16 overflow.
 *   - P = rint(penalty * 2^20) as int64, computed once on the host in double.
 *   - Linear scores rather than log scores make the objective the expected number of correctly labelled bins minus `penalty` per
 *     switch.  They also make every quantity an integer: max and + on int64 are associative, so a parallel scan and the
 *     sequential definition give identical results.
 * Path, per contig with n > 0 bins, K = 3 states in class order.
 *   - d[0][s] = q[0][s].
 *   - d[b][s] = q[b][s] + max(d[b-1][s], max_{s' != s} d[b-1][s'] - P).
 *   - Back pointer psi[b][s] = s if d[b-1][s] >= max_{s' != s}(d[b-1][s'] - P).  A tie stays.  Otherwise it is the lowest s'
 *     attaining the maximum.
 *   - The last bin's state is the lowest s with maximal d[n-1][s], and the path follows psi backwards.
 *   - All DP values are int64.
 *   - Consequences, which are also tests:
 *       - At P = 0, every evidence bin gets its lowest-index argmax.
 *       - At penalty = 4096, on contigs of fewer than 4096 bins, every contig is one region.
 *       - A contig without any evidence bin is one region of state 0 with evidence = 0.
 *       - An interior uncovered run takes a state from its neighbours and never forces a switch.
 * Regions.
 *   - A region is a maximal run of equal states within one contig.
 *   - Regions are ordered by contig, then by position.
 *   - An empty contig has no region.
 *   - Each region has these fields: contig (int64); lo, hi (int64, contig-relative bins, half-open); state (uint8); evidence
 *     (int64, the number of evidence bins in the region); qsum[3] (int64, the sum of q over the region).
 *   - The sums are integer, so they are exact and independent of order.
 *   - The Python layer derives these from the fields above: base coordinates lo * stride, min(hi * stride, L);
 *     mean = qsum / (evidence * 2^20), NaN where evidence == 0; margin = (qsum[state] - max other) / 2^20.
 * The kernels (gnn_regions.hip) are a chunked max-plus scan over tiles of 256 bins; no result depends on the tile size.  Device
 * memory, persistent in the ctx and grow-only: 16 B per contig, 98 B per tile and 1 B per bin for gnn_region_states_dev;
 * gnn_call_regions adds 14 B per bin (the track, the states, the flags), 12 B per 256 bins and 65 B per region.
 * bin_offsets_host[0] may be positive: the bins below it belong to no contig, are not read and their states are not written.
 *
 * gnn_call_regions: host pointers, synchronous.  state_host_or_null[n_bins]: the path's state per bin.  The six region arrays
 * (region_qsum[regions_capacity][3], the others [regions_capacity]) may all be NULL together: only *n_regions_out is then written -
 * this is how a caller sizes them.  A capacity that is too small is GNN_ERR_ARG and the message names the size needed; nothing is
 * written to the arrays then.  n_contigs == 0 or n_bins == 0 is GNN_OK with 0 regions.  GNN_ERR_ARG, with the range in the message,
 * for a penalty outside [0, 4096] or not finite, for decreasing offsets and for a negative first offset - checked before the ctx. */
int gnn_call_regions(gnn_ctx* ctx, const float* track_host, const int64_t* bin_offsets_host, int64_t n_contigs, double penalty,
                     uint8_t* state_host_or_null, int64_t* region_contig, int64_t* region_lo, int64_t* region_hi,
                     uint8_t* region_state, int64_t* region_evidence, int64_t* region_qsum, int64_t regions_capacity,
                     int64_t* n_regions_out);
/* The building block on device pointers: track_dev[n_bins][3] -> state_dev[n_bins], asynchronous on the ctx stream like
 * gnn_classify_dev (the offsets are read before the call returns).  Arguments are checked as above. */
int gnn_region_states_dev(gnn_ctx* ctx, const float* track_dev, const int64_t* bin_offsets_host, int64_t n_contigs, double penalty,
                          uint8_t* state_dev);
/* test aid: bins per tile of the scan, 1 <= bins <= 4096, default 256.  Results do not depend on it. */
int gnn_debug_set_region_tile(gnn_ctx* ctx, int bins);

/* ---- interval embeddings: encoder rows for parts of contigs ---------------------------------------------------
 * gnn_classify_contigs_embed answers one embedding per contig; a region call (gnn_call_regions) names a PART of a contig.  These
 * entry points fold the window embeddings of a scan into caller-given intervals, on the device; their rows are ordinary
 * [n][GNN_EMBED_DIM] f32 input for gnn_neighbours / gnn_cluster / gnn_representatives.
 *   windows     those of gnn_scan_plan at `stride` (1 .. 6000), honouring single_window; kept is the N rule's mask of gnn_scan_contigs.
 *   intervals   n_intervals triples (iv_contig, iv_start, iv_end), int64, 0-based half-open bases within the contig:
 *               0 <= start <= end <= L_contig, sorted by (contig, start), pairwise disjoint within a contig.  Gaps and empty intervals
 *               (start == end) are allowed.  Anything else is GNN_ERR_ARG; the message names the first offending interval and why.
 *   membership  window k of a contig (start k * stride, length len_k) has the centre base m_k = k * stride + len_k / 2 (integer
 *               division) and belongs to the interval of its contig with start <= m_k < end, or to none.  m_k is strictly increasing
 *               in k, so an interval's members are one range [w_lo, w_hi) of the global window order, possibly empty, and a window has
 *               at most one interval.  Membership does not depend on kept; kept decides what is summed.  No overlap weights.
 *   outputs     per interval, with e_0, e_1, ... the f32 rows gnn_embed returns for its KEPT members, in window order:
 *               count      int32, the number of kept members.
 *               embedding  [GNN_EMBED_DIM] f32: ((0 + e_0) + e_1) + ... in f32, divided once by (float)count - the arithmetic of
 *                          gnn_classify_contigs_embed; a zero row when count == 0.
 *               scores     [3] f32: the same sequential sum and single divide over the members' window scores of the strand mode.
 *               coherence  f32 in [0, 1], the mean resultant length of the members' unit rows: u_i = e_i / sqrt(sum_j e_i[j]^2), or a
 *                          zero row when e_i has a non-finite element or is all zeros - the rows gnn_neighbours calls invalid under
 *                          cosine; every other row has a unit row whatever its scale, from all-subnormal to FLT_MAX, and coherence
 *                          does not change when a row is multiplied by a power of two; U = ((0 + u_0) + u_1) + ...;
 *                          coherence = |U| / count, 0 when count == 0.  1: the members point one way; low: the mean averages
 *                          unlike rows.  The device computes it in f32 (a fixed reduction order per row, rsqrt); with n kept
 *                          members it agrees with a float64 evaluation of the definition to (17 + (n + 1) / 2) * 2^-24, and to
 *                          (18 + (n + 1) / 2) * 2^-24 under GNN_STRAND_BOTH: 3.0e-6 at n = 64, 6.1e-5 at n = 2000.
 *   strand      gnn_strand, as gnn_classify_contigs_strand.  REVERSE folds the reverse windows' rows and scores.  BOTH keeps two
 *               independent sums per interval: embedding = (S_f + S_r) / (2 count), coherence = |U_f + U_r| / (2 count), scores fold
 *               the combined window scores (f + r) * 0.5f.  Windows, membership, kept and count are the forward ones in every mode.
 * No result depends on gnn_set_chunk, on where seq lives, or on what ran on the ctx before: every sum is sequential in window order
 * and continues, slab by slab, from what the slabs before left in device memory.
 *
 * gnn_interval_plan - host only, no ctx, no GPU, like gnn_scan_plan - validates the intervals and answers w_lo_out / w_hi_out
 * [n_intervals]: the member range of every interval in the window order of gnn_scan_plan.  GNN_ERR_ARG also for a stride outside
 * [1, 6000] and decreasing offsets. */
int gnn_interval_plan(const int64_t* offsets_host, int64_t n_contigs, int stride, int single_window, const int64_t* iv_contig,
                      const int64_t* iv_start, const int64_t* iv_end, int64_t n_intervals, int64_t* w_lo_out, int64_t* w_hi_out);
/* The pass over a packed contig buffer (seq, seq_on_host, seq_bytes, offsets_host as gnn_scan_contigs): the windows of the scan go
 * through the forward pass slab by slab - under REVERSE / BOTH a slab's forward and reverse windows as one batch - and every slab's
 * rows are folded into the intervals it touches before the next slab overwrites them.  emb_host[n_intervals][GNN_EMBED_DIM],
 * count_host[n_intervals]; coherence_host_or_null[n_intervals] and scores_host_or_null[n_intervals][3] may be NULL.  Synchronous.
 * n_intervals == 0 or n_contigs == 0 is GNN_OK and writes nothing.  GNN_PREC_F16C6: GNN_ERR_ARG, as for every embedding entry
 * point.  Device memory, persistent in the ctx and grow-only: gnn_scan_contigs' window table, one slab of rows (2 KB per window of
 * the slab) and, per interval, 4 KB for the two sums (8 KB under BOTH), 16 B for the member range and 20 B of scores, count and
 * coherence.  Nothing grows with the number of windows beyond the table. */
int gnn_embed_intervals(gnn_ctx* ctx, const uint8_t* seq, int seq_on_host, int64_t seq_bytes, const int64_t* offsets_host,
                        int64_t n_contigs, int stride, int single_window, int precision, int strand, const int64_t* iv_contig,
                        const int64_t* iv_start, const int64_t* iv_end, int64_t n_intervals, float* emb_host, int32_t* count_host,
                        float* coherence_host_or_null, float* scores_host_or_null);
/* The building block on device pointers, asynchronous on the ctx stream (the host arrays are read before the call returns).  Rows
 * [first_window, first_window + n_rows) of ANY f32 matrix rows_dev[n][GNN_EMBED_DIM] (16-byte aligned) - and of scores_dev_or_null
 * [n][3] - are folded into the running sums sum_dev / unit_dev [n_intervals][GNN_EMBED_DIM], score_sum_dev_or_null[n_intervals][3]
 * and count_dev[n_intervals], which the caller zeroed before the first slice; slices are fed in increasing window order.
 * kept_host[n] (1 = kept) is read at those rows; w_lo_host / w_hi_host[n_intervals] are member ranges as gnn_interval_plan answers
 * them: 0 <= w_lo[i] <= w_hi[i] <= w_lo[i + 1], anything else is GNN_ERR_ARG naming the interval.  A range may reach beyond the
 * slice: only its rows inside the slice are read.  n_rows == 0 or n_intervals == 0 is GNN_OK. */
int gnn_interval_fold_dev(gnn_ctx* ctx, const float* rows_dev, const float* scores_dev_or_null, int64_t first_window, int64_t n_rows,
                          const uint8_t* kept_host, const int64_t* w_lo_host, const int64_t* w_hi_host, int64_t n_intervals,
                          float* sum_dev, float* unit_dev, float* score_sum_dev_or_null, int32_t* count_dev);
/* The sums of gnn_interval_fold_dev -> the outputs, asynchronous on the ctx stream: emb_dev[n_intervals][GNN_EMBED_DIM],
 * coherence_dev_or_null[n_intervals], scores_dev_or_null[n_intervals][3] (needs score_sum_dev).  sum_rev_dev_or_null and
 * unit_rev_dev_or_null, given together, are a second strand's sums: the combination of GNN_STRAND_BOTH.  An output may be the sum
 * it is made from (emb_dev == sum_dev, scores_dev == score_sum_dev): every element is read before it is written. */
int gnn_interval_finish_dev(gnn_ctx* ctx, const float* sum_dev, const float* unit_dev, const float* sum_rev_dev_or_null,
                            const float* unit_rev_dev_or_null, const float* score_sum_dev_or_null, const int32_t* count_dev,
                            int64_t n_intervals, float* emb_dev, float* coherence_dev_or_null, float* scores_dev_or_null);

/* ---- nearest neighbours among encoder embeddings: cosine top-k on the device ---------------------------------
 * "What is this contig like": for every query row the k most similar base rows, exact search (every pair is computed).  The rows are
 * what gnn_embed / gnn_classify_contigs_embed write; no forward pass runs and no other entry point's result changes.
 *   rows      query[n_query][GNN_EMBED_DIM] and base[n_base][GNN_EMBED_DIM], f32, C-contiguous (device pointers: 16-byte aligned).
 *             base == NULL is the self-search: base = query (n_base is ignored) and the pair (i, i) is excluded.
 *   valid     a row is valid iff every element is finite and, under GNN_KNN_COSINE, its norm is > 0 (a contig without a kept window
 *             has a zero row: it neither matches nor is matched).  An invalid query gets no neighbours; an invalid base row is nobody's.
 *   metric    GNN_KNN_COSINE: x.y / (|x| |y|).  GNN_KNN_DOT: x.y; a zero row is valid under it.
 *   outputs   idx[n_query][k] int64 (base row) and sim[n_query][k] f32, each row ordered by (similarity descending, base index
 *             ascending) on the device's own f32 similarities - a total order, so the result depends neither on how the base is split
 *             over workgroups nor on the slabs the queries are walked in.  Fewer than k candidates: padded with idx = -1, sim = NaN.
 *   ranges    1 <= k <= 64, n_query >= 0, 0 <= base rows < 2^31.  n_query == 0 is GNN_OK; no base row gives all -1 / NaN.
 *             GNN_ERR_ARG, with the range in the message, for k, the metric and the sizes - checked before the ctx is looked at.
 *   values    split-f16 limbs (hi + lo), three v_mfma_f32_32x32x16_f16 products per k-step, f32 accumulation in a fixed order: a
 *             pair's similarity depends on its two rows only.  Cosine: the f32 norm is taken in a fixed order, the normalised row is
 *             scaled by 2^8 before the split and the f32 result by 2^-16 (both exact: the low limbs stay f16 normals) - within 1e-5 of
 *             the fp64 cosine, 1e-6 typical; a power of two per row changes no bit, from rows whose elements are all subnormal to
 *             rows at FLT_MAX.  Dot: the rows are split unscaled: exact for small integers; within 1e-5 sum_i |x_i y_i| of the fp64
 *             dot where every non-zero element has 2^-7 <= |element| < 65504 (the limbs carry an element to
 *             max(2^-22 |element|, 2^-25): below 2^-3 the low limb is an f16 subnormal and the error is absolute - measured 0.09 of
 *             that bound on heavy-tailed rows up to 6e4, 10 times the bound for elements below 2^-9: scale such rows first);
 *             needs |element| < 65504 (f16 range) - beyond it a pair's similarity is not finite, and a NaN similarity is never
 *             returned: such a row is nobody's neighbour, has none, and is a cluster of its own.
 * Device memory, persistent in the ctx and grow-only: per base row 2 KB of f16 fragments + 1 B (gnn_neighbours: + the row's 2 KB of
 * f32); the queries are walked in slabs of 16384 rows, and per query row of ONE slab: 2 KB of fragments (+ 2 KB of f32 for
 * gnn_neighbours; nothing in the self-search, which reads the base's), 8 k B per base range of partial lists (a range is at most
 * 65280 base rows) and, for gnn_neighbours, 12 k B of results.  Nothing grows with n_query.
 * gnn_neighbours: host pointers, synchronous; the base goes up once, the queries slab by slab.  gnn_neighbours_dev: device pointers,
 * asynchronous on the ctx stream like gnn_classify_dev. */
typedef enum gnn_knn_metric { GNN_KNN_COSINE = 0, GNN_KNN_DOT = 1 } gnn_knn_metric;
int gnn_neighbours(gnn_ctx* ctx, const float* query_host, int64_t n_query, const float* base_host_or_null, int64_t n_base, int k,
                   int metric, int64_t* idx_host, float* sim_host);
int gnn_neighbours_dev(gnn_ctx* ctx, const float* query_dev, int64_t n_query, const float* base_dev_or_null, int64_t n_base, int k,
                       int metric, int64_t* idx_dev, float* sim_dev);
/* test aid: base rows per workgroup of the search (rounded up to a multiple of 32, at most 65280); 0, the default: the library's
 * choice, two workgroups per CU.  Results do not depend on it. */
int gnn_debug_set_neighbour_split(gnn_ctx* ctx, int64_t base_rows_per_workgroup);

/* ---- clusters among encoder embeddings: threshold components on the device ----------------------------------
 * "Which rows belong together, and which one stands for the group": the connected components of the graph that has an edge {i, j},
 * i != j, iff both rows are valid and sim(i, j) >= threshold - single linkage at the threshold, exact (every pair i < j is computed,
 * no pair twice).  Rows, validity and metric are those of the nearest neighbours above; no forward pass runs and no other entry
 * point's result changes.
 *   value     the similarity of the pair {i, j}, i < j, is the f32 that gnn_neighbours returns for query i and base row j (the same
 *             fragments, k-steps and order); (j, i) is never computed - the limb products are not symmetric in the last bit.  A
 *             similarity that is not a number is no edge.  The threshold is compared as the f32 given; a tie is an edge.
 *   outputs   four int64 arrays of n: label = the smallest index of the row's cluster; degree = the number of edges at the row; size
 *             = the rows of its cluster; rep = the member of its cluster with the largest degree, ties to the smallest index.  A
 *             valid row without an edge is a cluster of one (label = rep = itself, size 1).  An invalid row: -1, 0, 0, -1.
 *   ranges    0 <= n < 2^31, a finite threshold, a metric in [0, 1]; GNN_ERR_ARG with the value and the range in the message - checked
 *             before the ctx is looked at, nothing is written.  n == 0 is GNN_OK and writes nothing.
 *   exact     degrees, sizes and representatives are integer sums and maxima, the label is the root of a union-find whose links point
 *             to the smaller index: nothing depends on the order workgroups run in or on how the base is split over them
 *             (gnn_debug_set_neighbour_split sets the range for this search too).
 * Single linkage chains: two rows far below the threshold share a cluster when a path of edges joins them.  degree and rep are there
 * so that a caller sees it - a chain's representative has few edges for its cluster's size.
 * Device memory, persistent in the ctx and grow-only: the 2 KB of fragments + 1 B per row of the neighbour search (shared with it;
 * gnn_cluster: + the row's 2 KB of f32) and 20 B per row of parent, degree, size and key (gnn_cluster: + 32 B of results).  Nothing is
 * n x n and no edge list is stored.
 * gnn_cluster: host pointers, synchronous.  gnn_cluster_dev: device pointers, asynchronous on the ctx stream like gnn_classify_dev. */
int gnn_cluster(gnn_ctx* ctx, const float* rows_host, int64_t n, float threshold, int metric, int64_t* label_host, int64_t* degree_host,
                int64_t* size_host, int64_t* rep_host);
int gnn_cluster_dev(gnn_ctx* ctx, const float* rows_dev, int64_t n, float threshold, int metric, int64_t* label_dev, int64_t* degree_dev,
                    int64_t* size_dev, int64_t* rep_dev);

/* ---- density clusters among encoder embeddings: DBSCAN on the device ----------------------------------------
 * "Which rows form dense groups, which hang on to one, and which are alone": DBSCAN at one (threshold, min_points) pair on the graph
 * of gnn_cluster above - an edge {i, j}, i != j, iff both rows are valid and sim(i, j) >= threshold.  Rows, validity, metric, the value
 * of a pair (the f32 gnn_neighbours returns for query i < base row j; (j, i) is never computed) and the threshold (compared as the f32
 * given, a tie is an edge) are those of gnn_cluster; no forward pass runs and no other entry point's result changes.
 *   core      a valid row with degree + 1 >= min_points: the row counts itself, as scikit-learn's min_samples does.
 *   clusters  the connected components of the core rows under core-core edges; a cluster's label is its smallest core row.
 *   border    a valid row that is not core and has a core neighbour: anchor = the core neighbour with the largest similarity, ties to
 *             the smaller index; label = the anchor's; sim = that similarity (the f32's bits, -0 reported as +0).  A border row joins
 *             nothing: a border-border edge has no effect, and a row between two dense families no longer merges them.
 *   noise     a valid row that is not core and has no core neighbour: label = anchor = -1.
 *   outputs   label, degree, size, anchor: int64 arrays of n; sim: f32; kind: uint8, 0 invalid, 1 noise, 2 border, 3 core.  degree IS
 *             gnn_cluster's.  size = the rows, core and border, that carry the row's label; 0 for noise.  A core row has anchor =
 *             itself and sim = NaN.  An invalid row: -1, 0, 0, -1, NaN, 0.
 *   ranges    0 <= n < 2^31, a finite threshold, 1 <= min_points < 2^31, a metric in [0, 1], in this order; GNN_ERR_ARG with the value
 *             and the range in the message - checked before the ctx is looked at, nothing is written.  n == 0 is GNN_OK, needs a ctx
 *             and no pointers, and writes nothing.
 *   exact     degrees and sizes are integer sums, the anchor a 64-bit integer maximum over ALL core neighbours, the label the root of a
 *             union-find whose links point to the smaller index: nothing depends on the order workgroups run in or on how the base
 *             is split over them (gnn_debug_set_neighbour_split sets the range for this search too).  Unlike textbook DBSCAN, where
 *             a border row goes to the cluster that reaches it first, there is no visiting order for the result to depend on.
 * min_points = 1: label is gnn_cluster's label.  min_points = 2: the core rows are the rows with an edge and carry gnn_cluster's labels,
 * the noise rows are its clusters of one, and there is no border row.
 * What it is not: not HDBSCAN - one (threshold, min_points), no hierarchy over thresholds (gnn_density_tree is that); not approximate; no width other than
 * GNN_EMBED_DIM; not multi-GPU.
 * Two passes over the upper triangle (degrees first: who is core is known only when every edge is counted), no rounds.  Device memory,
 * persistent in the ctx and grow-only: the 2 KB of fragments + 1 B per row of the neighbour search (shared with it; gnn_density: + the
 * row's 2 KB of f32), 21 B per row of parent, degree, size, key and core flag, one byte per (64-row tile, base range) (gnn_density: +
 * 37 B of results).  Nothing is n x n and no edge list is stored.
 * gnn_density: host pointers, synchronous.  gnn_density_dev: device pointers, asynchronous on the ctx stream like gnn_classify_dev. */
int gnn_density(gnn_ctx* ctx, const float* rows_host, int64_t n, float threshold, int64_t min_points, int metric, int64_t* label_host,
                int64_t* degree_host, int64_t* size_host, int64_t* anchor_host, float* sim_host, uint8_t* kind_host);
int gnn_density_dev(gnn_ctx* ctx, const float* rows_dev, int64_t n, float threshold, int64_t min_points, int metric, int64_t* label_dev,
                    int64_t* degree_dev, int64_t* size_dev, int64_t* anchor_dev, float* sim_dev, uint8_t* kind_dev);

/* ---- representatives among encoder embeddings: greedy clusters on the device --------------------------------
 * "Which rows stand for the others": greedy incremental clustering, as dereplication tools do it.  THE ROWS ARRIVE IN PRIORITY ORDER
 * (index = rank; NNEngine.representatives sorts by weight and maps the answer back).  Walked in that order, a valid row is a
 * representative iff no representative of smaller rank has sim >= threshold to it; otherwise it is a member of the representative of
 * smaller rank with the largest similarity, ties to the smaller rank.  Every member is within the threshold of its representative, no
 * two representatives are within the threshold of each other, no cluster chains (gnn_cluster above is single linkage and does).  Rows,
 * validity, metric and threshold are those of gnn_cluster; no forward pass runs and no other entry point's result changes.
 *   value     the similarity of the pair i < j is the f32 that gnn_neighbours returns for query i and base row j (the same fragments,
 *             k-steps, order and scale as gnn_cluster); (j, i) is never computed.  A tie with the threshold is an edge.
 *   outputs   rep (int64): the row's representative, a representative names itself; sim (f32): a member's similarity to rep, NaN for a
 *             representative; size (int64): the rows of its cluster.  An invalid row: -1, NaN, 0.
 *   rounds    the device replaces the walk by synchronous rounds over the states of their start: an undecided row with an edge to a
 *             smaller-rank row that became a representative in the previous round turns member; otherwise an undecided row with no
 *             edge to a smaller-rank undecided row turns representative; otherwise it waits.  The representatives are the walk's.
 *             *rounds_host = the rounds until no row is undecided: a property of the graph and the order, not of the device.  WORST
 *             CASE: a path walked end to end takes as many rounds as it has rows, each a launch over the rows still live and one
 *             synchronise.  The undecided row of smallest rank is decided in every round, so at most n rounds run; a round that does
 *             not lower the count of undecided rows returns GNN_ERR_STATE with a message instead of going on.
 *   ranges    0 <= n < 2^31, a finite threshold, a metric in [0, 1]; GNN_ERR_ARG with the value and the range in the message - checked
 *             before the ctx is looked at, nothing is written.  n == 0 is GNN_OK, *rounds_host = 0 where the pointer is given.
 *   exact     flags are ORs, keys 64-bit maxima, sizes integer adds: bit-identical for every split of the base
 *             (gnn_debug_set_neighbour_split sets the range for this search too).
 * Device memory, persistent in the ctx and grow-only: the 2 KB of fragments + 1 B per row of the neighbour search (shared with it;
 * gnn_representatives: + the row's 2 KB of f32), 21 B per row of state, flag, key and size, one live byte per 64 and per 32 rows, 16 B
 * of counters (gnn_representatives: + 20 B of results per row).  Nothing is n x n and no edge list is stored.
 * gnn_representatives: host pointers, synchronous.  gnn_representatives_dev: device pointers (rounds_host stays a host pointer); it
 * enqueues on the ctx stream but SYNCHRONISES IT ONCE PER ROUND - the host reads 8 bytes, the undecided count - and is asynchronous
 * only in its last launches: the three arrays are ready when the stream is. */
int gnn_representatives(gnn_ctx* ctx, const float* rows_host, int64_t n, float threshold, int metric, int64_t* rep_host, float* sim_host,
                        int64_t* size_host, int64_t* rounds_host);
int gnn_representatives_dev(gnn_ctx* ctx, const float* rows_dev, int64_t n, float threshold, int metric, int64_t* rep_dev, float* sim_dev,
                            int64_t* size_dev, int64_t* rounds_host);
/* measurement only: with gnn_profile_enable on, the HIP-event milliseconds of every round (its tile and decide launches) of the ctx's
 * last gnn_representatives* call; *n_out = the rounds recorded, at most `capacity` of them are written. */
int gnn_debug_representative_round_ms(gnn_ctx* ctx, double* ms_out, int64_t capacity, int64_t* n_out);

/* ---- single-linkage tree among encoder embeddings: Boruvka on the device ------------------------------------
 * "Which rows belong together AT EVERY THRESHOLD": the single-linkage dendrogram = the maximum-similarity spanning tree of the complete
 * graph over the valid rows.  Cutting it at t - the union of its edges with sim >= t - gives exactly gnn_cluster's label at t, and the
 * clusters at t number n_valid - #(edges >= t).  Rows, validity and metric are those of gnn_cluster; no forward pass runs and no other
 * entry point's result changes.
 *   value     the weight of the pair {i, j}, i < j, is the f32 that gnn_neighbours returns for query i and base row j (the same
 *             fragments, k-steps, order and scale as gnn_cluster); (j, i) is never computed.  -0 counts as +0.  A pair whose value is
 *             not a number is no edge: the result is then a forest.
 *             Under GNN_KNN_DOT a finite row with an element beyond the f16 range is a valid, isolated row of that forest.
 *   order     an edge is better when its value is larger; ties go to the smaller lo = min(i, j), then to the smaller hi = max(i, j).
 *             The order holds for negative values as for positive ones: a negative edge ranks below every zero and positive one.
 *   tree      Kruskal over the valid pairs in that order: an edge is taken iff it joins two different components.  The order is
 *             strict, so the tree is unique.
 *   outputs   the tree's edges in that order, best first: a (int64, lo), b (int64, hi), sim (f32), each of capacity max(n - 1, 0),
 *             entries past *n_edges_host are -1 / -1 / NaN; *n_edges_host = n_valid - 1 unless NaN pairs split the forest (0 where no
 *             row is valid); valid (uint8 [n]): 1 for a valid row; *rounds_host: the passes of the device that added an edge.
 *   rounds    Boruvka: in a round every component picks its best outgoing edge in the order above - one pass over the upper triangle
 *             that keeps a 64-bit maximum per row, two launches that reduce them per component - and the picked edges join.  The
 *             components that are not final at least halve per round: at most ceil(log2 n_valid) rounds add an edge, one more finds
 *             none (it is not run where the tree already spans all n rows).  A 33rd round returns GNN_ERR_STATE with a message
 *             naming the round: n < 2^31 halves at most 31 times.  The host sorts the <= n - 1 records at the end.
 *   ranges    0 <= n < 2^31, a metric in [0, 1]; GNN_ERR_ARG with the value and the range in the message - checked before the ctx is
 *             looked at, nothing is written.  n == 0 is GNN_OK with zero edges and zero rounds.
 *   exact     every key is an integer maximum or minimum of values that depend on the pair alone, and the records are sorted:
 *             bit-identical, rounds included, for every split of the base (gnn_debug_set_neighbour_split sets the range for this
 *             search too).
 * What it is not: not approximate; not average or complete linkage (single linkage chains, see gnn_cluster); no width other than
 * GNN_EMBED_DIM; not multi-GPU.
 * Device memory, persistent in the ctx and grow-only: the 2 KB of fragments + 1 B per row of the neighbour search (shared with it;
 * gnn_linkage: + the row's 2 KB of f32) and 40 B per row of parent, component, the two keys, hi and the edge records.  Nothing is n x n.
 * gnn_linkage: host pointers, synchronous.  gnn_linkage_dev: the rows on the device, every output on the host; it enqueues on the ctx
 * stream, SYNCHRONISES IT ONCE PER ROUND - the host reads 8 bytes, the number of edges - and returns with the results written. */
int gnn_linkage(gnn_ctx* ctx, const float* rows_host, int64_t n, int metric, int64_t* a_host, int64_t* b_host, float* sim_host,
                uint8_t* valid_host, int64_t* n_edges_host, int64_t* rounds_host);
int gnn_linkage_dev(gnn_ctx* ctx, const float* rows_dev, int64_t n, int metric, int64_t* a_host, int64_t* b_host, float* sim_host,
                    uint8_t* valid_host, int64_t* n_edges_host, int64_t* rounds_host);
/* measurement only: with gnn_profile_enable on, the HIP-event milliseconds of every round (its six launches; the last one may have
 * added no edge) of the ctx's last gnn_linkage* call; *n_out = the rounds recorded, at most `capacity` of them are written. */
int gnn_debug_linkage_round_ms(gnn_ctx* ctx, double* ms_out, int64_t capacity, int64_t* n_out);

/* ---- density-aware linkage tree among encoder embeddings: mutual-reachability Boruvka ------------------------
 * "Which rows belong together at every threshold, bridges and stragglers aside": the tree that answers the core-only form of
 * gnn_density at every threshold at once, as gnn_linkage answers gnn_cluster - the input of HDBSCAN.  Rows, validity and metric are
 * those of gnn_linkage; no forward pass runs and no other entry point's result changes.
 *   core      core[i] of a valid row i: its similarity to its (min_points - 1)-th most similar partner - the row itself counts
 *             towards min_points, as in gnn_density and scikit-learn's min_samples.  It is the last entry that is a number of row i
 *             of the sim that the self-search gnn_neighbours(rows, NULL, k = min_points - 1, metric) returns, bit for bit: fewer
 *             valid partners than that give the least similar partner there is, min_points == 1 gives +inf, an invalid row or a row
 *             without a partner whose value is a number gives NaN.  gnn_neighbours forms (i -> j) and (j -> i) with the two cross
 *             products in opposite order, so core[i] may differ in the last bit from the k-th largest of the pair values below: that
 *             is accepted, core is what gnn_neighbours says.
 *   value     w(i, j) = fminf(fminf(v, core[i]), core[j]) for i < j, both rows valid and v a number; v is gnn_linkage's value of the
 *             pair.  A pair whose v is not a number is no edge.  With min_points == 1, w == v: a, b, sim, valid and rounds are
 *             gnn_linkage's, bit for bit.
 *   order, tree, rounds, exact: gnn_linkage's, over w.  Mutual reachability makes many pairs tie exactly; the strict order (value
 *             descending, lo ascending, hi ascending) decides every one of them, so the tree is unique and bit-identical for every
 *             split of the base.
 *   outputs   a, b, sim, valid, *n_edges_host, *rounds_host as gnn_linkage's (sim = w), and core (f32 [n]).
 *   ranges    gnn_linkage's, and 1 <= min_points <= 65 (the neighbour search stops at k = 64): GNN_ERR_ARG with the value and the
 *             range in the message before anything is launched or written.
 * Cutting the tree at t - the rows with core >= t, joined by the edges with sim >= t - gives the core rows of gnn_density at
 * (t, min_points) and their labels wherever no pair value lies within rounding of t (core comes from the (i -> j) orientation,
 * gnn_density counts the i < j one).  genomad_amd.sequence.hdbscan_clusters condenses the tree by levels of sim and selects clusters by
 * excess of mass on the host.
 * What it is: exact.  What it is not: not approximate; no width other than GNN_EMBED_DIM; not multi-GPU; not scikit-learn's handling
 * of tied merges (the condensed tree here is defined by levels, so it does not depend on which spanning tree was found); no
 * min_points above 65.
 * Device memory, persistent in the ctx and grow-only: gnn_linkage's, 4 B per row of core and 12 B per row and neighbour of the
 * self-search's lists.  Host and _dev forms and the synchronisation per round are gnn_linkage's. */
int gnn_density_tree(gnn_ctx* ctx, const float* rows_host, int64_t n, int min_points, int metric, int64_t* a_host, int64_t* b_host,
                     float* sim_host, float* core_host, uint8_t* valid_host, int64_t* n_edges_host, int64_t* rounds_host);
int gnn_density_tree_dev(gnn_ctx* ctx, const float* rows_dev, int64_t n, int min_points, int metric, int64_t* a_host, int64_t* b_host,
                         float* sim_host, float* core_host, uint8_t* valid_host, int64_t* n_edges_host, int64_t* rounds_host);
/* measurement only: gnn_debug_linkage_round_ms for the ctx's last gnn_density_tree* call (the self-search is not part of a round) */
int gnn_debug_density_tree_round_ms(gnn_ctx* ctx, double* ms_out, int64_t capacity, int64_t* n_out);

/* ---- similarity graph among encoder embeddings: every pair above a threshold --------------------------------
 * "Which pairs are the edges": the thresholded similarity graph that gnn_cluster acts on and throws away, kept - every pair i < j of
 * valid rows with sim(i, j) >= threshold and its similarity, as a CSR over the upper triangle.  Rows, validity, metric and threshold
 * are those of gnn_cluster; no forward pass runs and no other entry point's result changes.
 *   value     the similarity of the pair i < j is the f32 that gnn_neighbours returns for query i and base row j (the same fragments,
 *             k-steps, order and scale as gnn_cluster); (j, i) is never computed.  The threshold is compared as the f32 given; a tie
 *             is an edge; a similarity that is not a number is none.
 *   outputs   indptr (int64 [n + 1]): row i owns col[indptr[i] .. indptr[i + 1]), its partners j > i in ascending order, and
 *             sim[...], their similarities; an invalid row owns nothing and is nobody's partner.  col is int32 (n < 2^31), sim f32.
 *             The degree of gnn_cluster counts an edge at both ends: here it stands once, at its smaller row.
 *   passes    count: one pass over the upper triangle that counts every row's edges per base range, a prefix sum, indptr and the
 *             total (*nnz_host; the stream is synchronised once to hand it back).  fill: a second pass that computes the same
 *             products and writes every edge to its place; base ranges without an edge at a tile's rows are skipped.  The caller
 *             sizes col and sim between the two.  The fill belongs to the ctx's LAST count: GNN_ERR_STATE unless that count had
 *             the same (n, threshold, metric).  The rows must be the same; if they changed, the result is garbage, but no store
 *             leaves a row's segment.
 *   ranges    0 <= n < 2^31, a finite threshold, a metric in [0, 1]; GNN_ERR_ARG with the value and the range in the message - checked
 *             before the ctx is looked at.  n == 0: indptr = [0], *nnz_host = 0.  capacity < the total: GNN_ERR_ARG with both numbers.
 *             A total of 0: the fill launches nothing and col and sim may be NULL.
 *   exact     a counter has one owner workgroup, the offsets are integer prefix sums, an edge's place follows from its row, base
 *             range, step, wave, column block and lane: no atomics in global memory, bit-identical for every split of the base
 *             (gnn_debug_set_neighbour_split sets the range for this search too).
 * What it is not: not approximate; no width other than GNN_EMBED_DIM; not multi-GPU.  Query rows against OTHER base rows - the
 * bipartite graph - is gnn_match_count / gnn_match_fill below.  The edge list is as large as the threshold makes it - n (n - 1) / 2 at -1: look at *nnz_host before allocating.
 * Device memory, persistent in the ctx and grow-only: the 2 KB of fragments + 1 B per row of the neighbour search (shared with it;
 * gnn_graph_count: + the row's 2 KB of f32), 12 B per (row, base range) of counters and offsets (gnn_graph_count: + 8 B per row;
 * gnn_graph_fill: + 8 B per edge).  Nothing is n x n.
 * gnn_graph_count / gnn_graph_fill: host pointers, synchronous; the fill uses the rows its count uploaded and answers GNN_ERR_STATE
 * when another host-pointer search has replaced them.  gnn_graph_count_dev: device pointers, *nnz_host on the host.
 * gnn_graph_fill_dev: device pointers, asynchronous on the ctx stream like gnn_classify_dev. */
int gnn_graph_count(gnn_ctx* ctx, const float* rows_host, int64_t n, float threshold, int metric, int64_t* indptr_host, int64_t* nnz_host);
int gnn_graph_fill(gnn_ctx* ctx, int64_t n, float threshold, int metric, int32_t* col_host, float* sim_host, int64_t capacity);
int gnn_graph_count_dev(gnn_ctx* ctx, const float* rows_dev, int64_t n, float threshold, int metric, int64_t* indptr_dev,
                        int64_t* nnz_host);
int gnn_graph_fill_dev(gnn_ctx* ctx, const float* rows_dev, int64_t n, float threshold, int metric, int32_t* col_dev, float* sim_dev,
                       int64_t capacity);
/* measurement only: with gnn_profile_enable on, the HIP-event milliseconds of the ctx's last gnn_graph_count* call: [0] the clear and
 * the count pass, [1] the scan and indptr; *n_out = the figures recorded (2, or 0 for n == 0 or without profiling), at most `capacity`
 * of them are written.  The prepare kernel and the fill are timed from outside, by gnn_profile_get around the calls. */
int gnn_debug_graph_pass_ms(gnn_ctx* ctx, double* ms_out, int64_t capacity, int64_t* n_out);

/* ---- Markov clusters of a similarity graph: integer MCL on the device ---------------------------------------
 * "Which families does the flow through the graph settle in": van Dongen's Markov clustering of the graph gnn_graph_* writes, with one
 * knob, the inflation - and in integers throughout, so that every output equals the definition (sequence.markov_clusters) bit for bit,
 * for any number of workgroups, any table size and any order they run in.  No forward pass runs and no other entry point's result changes.
 *   graph     an upper-triangle CSR: indptr (int64 [n + 1]) rises from 0 to nnz, row i owns col[indptr[i] .. indptr[i + 1]), its
 *             partners in (i, n) in ANY order, and sim[...] (f32, finite, < 64); valid (uint8 [n], or NULL: every row).  Exactly what
 *             gnn_graph_fill_dev wrote is such a graph.  Anything else: GNN_ERR_ARG behind one O(nnz) kernel, before anything else runs,
 *             the outputs untouched.
 *   weights   ONE = 2^30, W = 2^24.  q = rint(sim * W); an edge with q <= 0 or an invalid end does not exist; an edge sits at both its
 *             ends; parallel edges count once, with the largest q; node j's loop is the largest q at j, W without an edge.
 *   prune     of entries (i, y > 0): S = sum y; keep y * precision >= S; of more than `select` the first `select` under (y descending,
 *             i ascending); S' = sum of the kept; p_i = y_i * ONE / S' (floor); p = 0 dropped; ascending by i.
 *   matrix    initial column of a valid node: prune(its edges' q and its loop) - pruned like any other; an invalid node's is empty.  An
 *             iteration, per column j: e_i = sum_k p_ik p_kj (exact); t_i = e_i >> 30; u_i = t_i * ONE / max t; y_i = u_i ^ (a / 4)
 *             for inflation_quarters = a in [5, 32] - from ONE, a / 4 floored products by u, one by h = isqrt(u * ONE) if a % 4 >= 2, one
 *             by isqrt(h * ONE) if a is odd -; zeros dropped; prune.  It stops behind the first iteration that changes no column
 *             (*converged_host = 1) or behind max_iter iterations; *iterations_host counts them, changed_host[it] (capacity max_iter)
 *             the columns iteration it changed.  max_iter = 0: the initial matrix is interpreted.
 *   outputs   label (int64: the smallest index of the node's connected component in the graph {i, j : p_ij > 0} of the final matrix;
 *             -1 for an invalid row - gnn_cluster's rule), size (int64: nodes of its cluster; 0), attractor (int64: the i with the
 *             largest p_ij in column j, ties to the smaller i; -1), flow (uint32: that p; 0), is_attractor (uint8: p_jj > 0).
 *   ranges    0 <= n <= 2^24, nnz >= 0, inflation_quarters in [5, 32], select in [1, 1024], precision in [1, 2^20], max_iter in
 *             [0, 10000]; GNN_ERR_ARG with the value and the range in the message - checked before the ctx is looked at.  n == 0:
 *             nothing is launched; one iteration that changes nothing.
 *   exact     the sums are 64-bit integer adds into a table keyed by row (in LDS; a column whose rows do not fit is finished with
 *             an accumulator in global memory), the selection a radix select on integer keys, the square roots corrected by integer
 *             comparisons: no float is added or compared, nothing depends on an order.
 * What it is not: not mcl's floating-point arithmetic nor its recovery / scheme options; no overlapping clusters (a node between two
 * attractor systems joins them, as the component rule says); select <= 1024; not multi-GPU.
 * Device memory, persistent in the ctx and grow-only: 16 B per (row, select) of matrices, 16 B per edge and about 40 B per row of graph,
 * lists and union-find, and at most 1.5 GB of overflow accumulators (gnn_mcl: + the graph and 29 B per row of results).
 * gnn_mcl: host pointers, synchronous.  gnn_mcl_dev: device pointers in and out; changed, iterations and converged on the host; the
 * ctx stream is synchronised once for the verdict on the graph and once per iteration (8 bytes). */
int gnn_mcl(gnn_ctx* ctx, const int64_t* indptr_host, const int32_t* col_host, const float* sim_host, const uint8_t* valid_host_or_null,
            int64_t n, int64_t nnz, int inflation_quarters, int select, int precision, int max_iter, int64_t* label_host,
            int64_t* size_host, int64_t* attractor_host, uint32_t* flow_host, uint8_t* is_attractor_host, int64_t* changed_host,
            int64_t* iterations_host, int* converged_host);
int gnn_mcl_dev(gnn_ctx* ctx, const int64_t* indptr_dev, const int32_t* col_dev, const float* sim_dev, const uint8_t* valid_dev_or_null,
                int64_t n, int64_t nnz, int inflation_quarters, int select, int precision, int max_iter, int64_t* label_dev,
                int64_t* size_dev, int64_t* attractor_dev, uint32_t* flow_dev, uint8_t* is_attractor_dev, int64_t* changed_host,
                int64_t* iterations_host, int* converged_host);
/* The final matrix of the ctx's last gnn_mcl* call, which must have had this (n, select) and succeeded - GNN_ERR_STATE otherwise: length
 * (int32 [n]), idx (int32 [n][select]) and val (uint32 [n][select]) on the host; column j owns the first length[j] cells of its row, rows
 * ascending; the cells behind them are not written.  Synchronous. */
int gnn_mcl_matrix(gnn_ctx* ctx, int64_t n, int select, int32_t* length_host, int32_t* idx_host, uint32_t* val_host);
/* test aids; no result depends on them.  gnn_debug_mcl_lds: the slots of the LDS table, 0 .. 4096 (0: every column takes the overflow
 * path; -1: leave it as it is); returns the value before the call (>= 0), or GNN_ERR_ARG.  gnn_debug_mcl_groups: the workgroups of a
 * pass, 1 .. 65535 (0: the library's choice, two per CU).  gnn_debug_mcl_pow: the integer power of the iteration, run on the device by
 * the function the passes call: out[i] = u[i] ^ (inflation_quarters / 4) in 2^-30 fixed point for n values u <= 2^30 (uint64, on the
 * host); GNN_ERR_ARG - before the ctx is looked at - for inflation_quarters outside [5, 32], n outside [0, 2^24], a u above 2^30 or a
 * missing pointer with n > 0.  Synchronous. */
int gnn_debug_mcl_lds(gnn_ctx* ctx, int slots);
int gnn_debug_mcl_groups(gnn_ctx* ctx, int groups);
int gnn_debug_mcl_pow(gnn_ctx* ctx, const uint64_t* u_host, int64_t n, int inflation_quarters, uint64_t* out_host);
/* measurement only.  gnn_debug_mcl_ms: with gnn_profile_enable on, the HIP-event milliseconds of the ctx's last gnn_mcl* call: [0]
 * validate and symmetrise, [1] the initial matrix, then one figure per iteration; *n_out = the figures recorded, at most `capacity` are
 * written.  gnn_debug_mcl_overflow: the columns each pass of that call pushed on the overflow list: [0] the initial matrix, then one
 * count per iteration. */
int gnn_debug_mcl_ms(gnn_ctx* ctx, double* ms_out, int64_t capacity, int64_t* n_out);
int gnn_debug_mcl_overflow(gnn_ctx* ctx, int64_t* count_out, int64_t capacity, int64_t* n_out);

/* ---- label spreading over a similarity graph: multi-hop label transfer on the device ----------------------------
 * "Which class reaches every row through the graph, over any number of edges": the labels of seed rows spread along the edges of the
 * graph gnn_graph_* writes until nothing changes - where gnn_vote crosses one edge - in integers throughout, so that every output equals
 * the definition (sequence.label_spread) bit for bit, for any number of workgroups and any order they run in.  No forward pass runs and
 * no other entry point's result changes.
 *   graph     gnn_mcl's: an upper-triangle CSR with sim (f32, finite, < 64) and valid (uint8 [n], or NULL); exactly what
 *             gnn_graph_fill_dev wrote is such a graph.  label (int64 [n]) in [-1, n_classes), -1: unlabelled.  Anything else:
 *             GNN_ERR_ARG behind two O(nnz + n) kernels, before anything else runs, the outputs untouched.
 *   weights   ONE = 2^30 is a score of 1, W = 2^24.  q = rint(sim * W); an entry with q <= 0 or an invalid end does not exist; an entry
 *             sits at both its ends; parallel entries are added.  d_i = the sum of q at row i; p_ij = (q_ij << 31) / d_i (floor).
 *   seeds     a valid row with label >= 0; y_i[c] = 1 where label_i == c, else 0.
 *   iteration synchronous, F^0 = 0: g_i[c] = (sum_j p_ij * F_j[c]) >> 31; F'_i[c] = ONE * y_i[c] for a seed under `clamp`, otherwise
 *             (a * g_i[c] + (64 - a) * ONE * y_i[c]) >> 6 for alpha = a / 64, alpha_64ths = a in [1, 63]; an invalid row stays 0.  It
 *             stops behind the first iteration that changes no row (*converged_host = 1) or behind max_iter iterations;
 *             *iterations_host counts them, changed_host[it] (capacity max_iter) the rows iteration it changed.  The map is monotone
 *             and F^1 >= F^0: F never falls and is bounded, so it ends - after how many iterations, nothing here says.
 *   outputs   score (uint32 [n][n_classes], units of 2^-30; NULL: the matrix is not wanted and not copied), best (int32: the class of
 *             the largest score, ties to the smaller class; -1 where every score is 0), best_score, second_score (uint32: the largest
 *             score among the other classes), total (uint64: the sum over the classes), first (int32: the first iteration, counted from
 *             1, behind which the row's total was not 0; -1: never.  The floors can make it larger than the row's distance from a seed).
 *   ranges    0 <= n <= 2^24, nnz >= 0, n_classes in [1, 1024], alpha_64ths in [1, 63], max_iter in [1, 10000]; GNN_ERR_ARG with the
 *             value and the range in the message - checked before the ctx is looked at.  n == 0: nothing is launched; one iteration
 *             that changes nothing.
 *   exact     a row's sum is below 2^61 at any degree (the p of a row sum to 2^31 at the most, a score is at most 2^30): 64-bit integer
 *             multiply-adds, reduced by shuffles and through LDS; integer add atomics on counters only.  A row neither whose own nor
 *             whose neighbours' scores changed in the previous iteration is not computed again (gnn_debug_spread_skip): no bit depends
 *             on that.
 * What it is not: not Zhou's symmetric normalisation D^-1/2 W D^-1/2 (rows are random-walk rows, D^-1 W); not float; no calibrated
 * probability (a score is a share of seed mass that reached the row); n_classes <= 1024; not multi-GPU.
 * Device memory, persistent in the ctx and grow-only: 8 B per symmetric entry (two per edge), 2 * n * n_classes * 4 B of scores, about
 * 30 B per row (gnn_spread: + the graph, the labels and 24 B per row of results).  A failed allocation: GNN_ERR_NOMEM, outputs untouched.
 * gnn_spread: host pointers, synchronous.  gnn_spread_dev: device pointers in and out; changed, iterations and converged on the host;
 * the ctx stream is synchronised once for the verdict on graph and labels and once per iteration (8 bytes). */
int gnn_spread(gnn_ctx* ctx, const int64_t* indptr_host, const int32_t* col_host, const float* sim_host, const uint8_t* valid_host_or_null,
               const int64_t* label_host, int64_t n, int64_t nnz, int n_classes, int alpha_64ths, int clamp, int max_iter,
               uint32_t* score_host_or_null, int32_t* best_host, uint32_t* best_score_host, uint32_t* second_score_host, uint64_t* total_host,
               int32_t* first_host, int64_t* changed_host, int64_t* iterations_host, int* converged_host);
int gnn_spread_dev(gnn_ctx* ctx, const int64_t* indptr_dev, const int32_t* col_dev, const float* sim_dev, const uint8_t* valid_dev_or_null,
                   const int64_t* label_dev, int64_t n, int64_t nnz, int n_classes, int alpha_64ths, int clamp, int max_iter,
                   uint32_t* score_dev_or_null, int32_t* best_dev, uint32_t* best_score_dev, uint32_t* second_score_dev, uint64_t* total_dev,
                   int32_t* first_dev, int64_t* changed_host, int64_t* iterations_host, int* converged_host);
/* test aids; no result depends on them.  gnn_debug_spread_groups: the workgroups of an iteration, 1 .. 65535 (0: the library's choice,
 * eight per CU).  gnn_debug_spread_skip: the dirty-row rule on (the default) or off. */
int gnn_debug_spread_groups(gnn_ctx* ctx, int groups);
int gnn_debug_spread_skip(gnn_ctx* ctx, int on);
/* measurement only: with gnn_profile_enable on, the HIP-event milliseconds of the ctx's last gnn_spread* call: [0] validate and
 * symmetrise, then one figure per iteration; *n_out = the figures recorded, at most `capacity` are written. */
int gnn_debug_spread_ms(gnn_ctx* ctx, double* ms_out, int64_t capacity, int64_t* n_out);

/* ---- average linkage over a similarity graph: UPGMA rounds on the device ------------------------------------
 * "Which groups have the largest mean similarity to each other, at every cut level at once": the average-linkage (UPGMA) tree of the
 * graph gnn_graph_* writes, by rounds of reciprocal best pairs - where gnn_cluster and gnn_linkage chain through one bridge pair - in
 * integers throughout, so that every output equals the definition (sequence.average_linkage) bit for bit, for any number of
 * workgroups, any table size, any row class and any order they run in.  No forward pass runs and no other entry point's result changes.
 *   graph     gnn_mcl's: an upper-triangle CSR with sim (f32, finite, < 64) and valid (uint8 [n], or NULL); exactly what
 *             gnn_graph_fill_dev wrote is such a graph.  Anything else: GNN_ERR_ARG behind one O(nnz) kernel, before anything else
 *             runs, the outputs untouched.
 *   weights   W = 2^24.  q = rint(sim * W); an entry with q <= 0 or an invalid end does not exist; parallel entries are added.
 *   clusters  a cluster's id is its smallest member.  S(A, B) = the sum of q over the entries between A and B; the average is
 *             S / (|A| * |B|): a pair of rows without an entry counts as similarity 0.
 *   round     every live cluster A with a neighbour names best[A] = the neighbour B with the largest S(A, B) / |B|, ties to the smaller
 *             id - S1 * |B2| against S2 * |B1| as exact 128-bit integers - if S(A, B) >= stop_q * |A| * |B|; every pair with best[A] =
 *             B, best[B] = A, A < B merges: B is absorbed into A.  The rows are contracted: columns relabelled, self entries dropped,
 *             duplicates summed.  It stops behind the first round that merges nothing (*complete_host = 1) or behind max_rounds rounds;
 *             *rounds_host counts them, merged_per_round_host[r] (capacity min(max_rounds, n + 1)) the pairs round r merged.  A round
 *             in which a cluster names a best merges a pair: at most n rounds.
 *   outputs   per node, written where the node was absorbed: parent (int32: the cluster that absorbed it; -1: never absorbed), weight
 *             (uint64: S of the merge), size_a, size_b (int32: the sizes of the absorbing and the absorbed cluster before the merge),
 *             round (int32, from 0).  A node never absorbed: -1, 0, 0, 0, 0.
 *   ranges    0 <= n <= 2^24, nnz >= 0, stop_q in [1, 2^30), max_rounds in [1, 2^20]; GNN_ERR_ARG with the value and the range in the
 *             message - checked before the ctx is looked at.  n == 0: nothing is launched; one round that merges nothing.
 *   exact     S < 2^63 and |A| * |B| < 2^48: every sum is a 64-bit integer add - into a table in LDS keyed by the relabelled column,
 *             or, for a row with more entries than the table has slots, into an accumulator in global memory - and every comparison
 *             a comparison of two 128-bit products.  No float is added or compared, nothing depends on an order.
 * What it is not: not the mean over existing entries only (a missing pair is a 0, so on a graph cut at a threshold the average is a
 * lower bound of the true mean); not complete linkage or Ward; not approximate; a round rewrites every live row; not multi-GPU.
 * Device memory, persistent in the ctx and grow-only: 32 B per symmetric entry (two per edge), about 70 B per row, at most 192 MB of
 * accumulators (gnn_avglink: + the graph and 24 B per row of results).  A failed allocation: GNN_ERR_NOMEM, outputs untouched.
 * gnn_avglink: host pointers, synchronous.  gnn_avglink_dev: device pointers in and out; merged_per_round, rounds and complete on the
 * host; the ctx stream is synchronised once for the verdict on the graph and once per round (8 bytes). */
int gnn_avglink(gnn_ctx* ctx, const int64_t* indptr_host, const int32_t* col_host, const float* sim_host, const uint8_t* valid_host_or_null,
                int64_t n, int64_t nnz, int64_t stop_q, int max_rounds, int32_t* parent_host, uint64_t* weight_host, int32_t* size_a_host,
                int32_t* size_b_host, int32_t* round_host, int64_t* merged_per_round_host, int64_t* rounds_host, int* complete_host);
int gnn_avglink_dev(gnn_ctx* ctx, const int64_t* indptr_dev, const int32_t* col_dev, const float* sim_dev, const uint8_t* valid_dev_or_null,
                    int64_t n, int64_t nnz, int64_t stop_q, int max_rounds, int32_t* parent_dev, uint64_t* weight_dev, int32_t* size_a_dev,
                    int32_t* size_b_dev, int32_t* round_dev, int64_t* merged_per_round_host, int64_t* rounds_host, int* complete_host);
/* test aids; no result depends on them.  gnn_debug_avglink_slots: the slots of the LDS table, 0 .. 4096 (0: every row takes the
 * accumulator in global memory; -1: leave it as it is); returns the value before the call (>= 0), or GNN_ERR_ARG.
 * gnn_debug_avglink_wave_rows: the longest upper bound of a row that a single wave takes, 0 .. 4096 (0: none; -1: leave it); returns
 * the value before the call.  gnn_debug_avglink_groups: the workgroups of a contraction, 1 .. 65535 (0: the library's choice, eight per
 * CU).  gnn_debug_avglink_order: the order function of the best scan and the stop test, run on the device over n quadruples (s1, d1,
 * s2, d2) of uint64 on the host: out_host[i] (int32) = -1, 0 or 1 as s1 / d1 is below, equal to or above s2 / d2. */
int gnn_debug_avglink_slots(gnn_ctx* ctx, int slots);
int gnn_debug_avglink_wave_rows(gnn_ctx* ctx, int entries);
int gnn_debug_avglink_groups(gnn_ctx* ctx, int groups);
int gnn_debug_avglink_order(gnn_ctx* ctx, const uint64_t* quads_host, int64_t n, int32_t* out_host);
/* measurement only.  gnn_debug_avglink_ms: with gnn_profile_enable on, the HIP-event milliseconds of the ctx's last gnn_avglink* call:
 * [0] validate and symmetrise, then one figure per round; *n_out = the figures recorded, at most `capacity` are written.
 * gnn_debug_avglink_classes: the rows the contractions of that call took by class, all rounds together: [one wave, one workgroup, the
 * accumulator in global memory]. */
int gnn_debug_avglink_ms(gnn_ctx* ctx, double* ms_out, int64_t capacity, int64_t* n_out);
int gnn_debug_avglink_classes(gnn_ctx* ctx, int64_t* rows_out);

/* ---- modularity communities of a similarity graph: Louvain's levels on the device ---------------------------
 * "Which groups does the graph fall into by itself, and how good is that partition": modularity optimisation over the graph
 * gnn_graph_* writes - one knob with a natural default (resolution 1), a partition that scores itself, a coarse-to-fine hierarchy -
 * in integers throughout, so that every output equals the definition (sequence.modularity_communities) bit for bit, for any number
 * of workgroups, any table size, any row class and any order they run in.  No forward pass runs and no other entry point's result
 * changes.
 *   graph     gnn_mcl's: an upper-triangle CSR with sim (f32, finite, < 64) and valid (uint8 [n], or NULL); exactly what
 *             gnn_graph_fill_dev wrote is such a graph.  Anything else: GNN_ERR_ARG behind one O(nnz) kernel, before anything else
 *             runs, the outputs untouched.
 *   weights   W = 2^24.  q = rint(sim * W); an entry with q <= 0 or an invalid end does not exist; parallel entries are added.
 *             k_i = the sum of node i's row (its self entry included), M2 = the sum of all k: the same at every level, < 2^58 or
 *             GNN_ERR_ARG (outputs untouched).  r = 64 * resolution, an integer in [1, 256].
 *   level     nodes: at level 0 the valid rows under their row indices, later the components of the level before, numbered by their
 *             smallest member.  comm[i] = i at its start; a community is named by its founding node; tot_c = the sum of k over c.
 *   sweep s   synchronous.  Want: node i of community a takes, over the communities c != a of its neighbours j != i, D(i, c) = 64 M2
 *             (w_ic - w_ia) - r k_i (tot_c + k_i - tot_a) (w_ic: the sum of A_ij over j in c, j != i), a signed 128-bit integer, and
 *             wants the c of the largest D > 0, ties to the smaller c.  Pick: its priority is (D, h, -i), h = ((i + 1) * 2654435761 +
 *             s * 40503) mod 2^32; i moves iff every neighbour j != i that wants to move and sits in comm[i] or in i's target has a
 *             strictly smaller priority.  Score: Qnum = 64 M2 (the weight inside communities, both directions, self entries
 *             included) - r (the sum of tot_c^2); strictly larger than the assignment's: accepted; otherwise discarded, and the
 *             level ends (rejected).  A sweep that moves nobody ends the level, and so do max_sweeps sweeps.
 *   level end behind an accepted sweep: every community is split into the connected components of its induced subgraph, the components
 *             are numbered by their smallest member, the graph is contracted (entries summed, the inner weight as the self entry).
 *             A level without an accepted sweep is the last; max_levels caps them.  M2 == 0: no level, every valid row alone.
 *   outputs   label (int64 [n]: the smallest row of the row's final community; -1 for an invalid row), size (int64 [n]), level_label
 *             (int64 [max_levels][n], rows [0, *levels_host) written: the labelling behind each level, each nested in the next);
 *             level_stats_host (int64 [max_levels][7]: nodes, communities, sweeps, accepted, moved, rejected, split = components -
 *             communities), level_qnum_host (uint64 [max_levels][2]: Qnum of the level's labelling, low and high word, two's
 *             complement), *levels_host, *complete_host (the last level had no accepted sweep and max_sweeps ended none), *m2_host.
 *             The modularity of level l is Qnum / (64 * M2^2).
 *   ranges    0 <= n <= 2^24, 0 <= nnz < 2^30, r in [1, 256], max_levels in [1, 32], max_sweeps in [1, 2^20]; GNN_ERR_ARG with the
 *             value and the range in the message - checked before the ctx is looked at.  n == 0: nothing is launched; no level.
 *   exact     every weight, k, tot and inner sum is a 64-bit integer add - into a table in LDS keyed by the neighbour's community,
 *             or, for a row longer than the table, into an accumulator in global memory; D, the squares and Qnum are 128-bit
 *             integers (|D| < 2^126, |Qnum| < 2^125 under the ranges above).  No float is added or compared, nothing depends on an
 *             order.
 * What it is not: not Leiden's refinement (connectedness is guaranteed by the split, well-connectedness is not); not the sequential
 * Louvain sweep (moves are synchronous and a sweep that does not raise the modularity ends its level); not float; not overlapping;
 * not multi-GPU; resolution <= 4; n <= 2^24.
 * Device memory, persistent in the ctx and grow-only: 28 B per symmetric entry (two per edge), about 190 B per row, at most 192 MB of
 * accumulators (gnn_communities: + the graph and 8 B * (2 + max_levels) per row of results).  A failed allocation: GNN_ERR_NOMEM,
 * outputs untouched.
 * gnn_communities: host pointers, synchronous.  gnn_communities_dev: device pointers in and out (label, size, level_label), the rest
 * on the host; the ctx stream is synchronised once for the verdict on the graph, once per level's start and end, and once per sweep
 * (56 bytes: the movers, the sums, the verdict, Qnum). */
int gnn_communities(gnn_ctx* ctx, const int64_t* indptr_host, const int32_t* col_host, const float* sim_host, const uint8_t* valid_host_or_null,
                    int64_t n, int64_t nnz, int r, int max_levels, int max_sweeps, int64_t* label_host, int64_t* size_host,
                    int64_t* level_label_host, int64_t* level_stats_host, uint64_t* level_qnum_host, int64_t* levels_host, int* complete_host,
                    uint64_t* m2_host);
int gnn_communities_dev(gnn_ctx* ctx, const int64_t* indptr_dev, const int32_t* col_dev, const float* sim_dev, const uint8_t* valid_dev_or_null,
                        int64_t n, int64_t nnz, int r, int max_levels, int max_sweeps, int64_t* label_dev, int64_t* size_dev,
                        int64_t* level_label_dev, int64_t* level_stats_host, uint64_t* level_qnum_host, int64_t* levels_host,
                        int* complete_host, uint64_t* m2_host);
/* The connected components of every label's induced subgraph over the graph's existing entries (sequence.label_components): label
 * (int64 [n], negative: none) -> out (int64 [n]): the smallest row of the row's component among the rows of its own label; -1 for a
 * row without a label and for an invalid row.  The graph, its verdict and the ranges of n and nnz are gnn_communities'; one
 * synchronise for the verdict.  Device memory: 5 B per row. */
int gnn_label_components(gnn_ctx* ctx, const int64_t* indptr_host, const int32_t* col_host, const float* sim_host,
                         const uint8_t* valid_host_or_null, int64_t n, int64_t nnz, const int64_t* label_host, int64_t* out_host);
int gnn_label_components_dev(gnn_ctx* ctx, const int64_t* indptr_dev, const int32_t* col_dev, const float* sim_dev,
                             const uint8_t* valid_dev_or_null, int64_t n, int64_t nnz, const int64_t* label_dev, int64_t* out_dev);
/* test aids; no result depends on them.  gnn_debug_communities_slots: the slots of the LDS table, 0 .. 4096 (0: every row takes the
 * accumulator in global memory; -1: leave it as it is); returns the value before the call (>= 0), or GNN_ERR_ARG.
 * gnn_debug_communities_wave_rows: the longest row that a single wave takes, 0 .. 4096 (0: none; -1: leave it); returns the value
 * before the call.  gnn_debug_communities_groups: the workgroups of a launch, 1 .. 65535 (0: the library's choice, eight per CU).
 * gnn_debug_communities_gain: the gain and the score, run on the device over n rows of 12 uint64 on the host - 64 * M2, r, k, w_ic,
 * w_ia, tot_c, tot_a, in, the squares' low and high word, the previous Qnum's low and high word -: out_host[i] (5 uint64) = D low,
 * D high, Qnum low, Qnum high (two's complement), Qnum > previous. */
int gnn_debug_communities_slots(gnn_ctx* ctx, int slots);
int gnn_debug_communities_wave_rows(gnn_ctx* ctx, int entries);
int gnn_debug_communities_groups(gnn_ctx* ctx, int groups);
int gnn_debug_communities_gain(gnn_ctx* ctx, const uint64_t* operands_host, int64_t n, uint64_t* out_host);
/* measurement only.  gnn_debug_communities_ms: with gnn_profile_enable on, the HIP-event milliseconds of the ctx's last
 * gnn_communities* call: [0] validate, symmetrise and level 0's start, then per level one figure per sweep and - behind a level with
 * an accepted sweep - one for its end (split, contraction, the next level's start); *n_out = the figures recorded, at most `capacity`
 * are written.  gnn_debug_communities_classes: the rows that call took by class, all launches together: [one wave, one workgroup, the
 * accumulator in global memory] of the want launches, then of the contractions (6 values). */
int gnn_debug_communities_ms(gnn_ctx* ctx, double* ms_out, int64_t capacity, int64_t* n_out);
int gnn_debug_communities_classes(gnn_ctx* ctx, int64_t* rows_out);

/* ---- k-nearest-neighbour graph of encoder embeddings: union / mutual, similarity / Jaccard ------------------
 * "Which rows list each other": the neighbour lists of gnn_neighbours' self-search, joined into the upper-triangle CSR of gnn_graph_* -
 * at most n k edges whatever the data, a density that adapts per row, and the graph every consumer below gnn_graph (gnn_mcl, gnn_spread,
 * gnn_avglink, gnn_communities) takes.  Rows, validity, metric and k are those of gnn_neighbours; no forward pass runs and no other
 * entry point's result changes.  N(i): the entries of row i's list other than -1; N+(i) = N(i) + {i}.
 *   edges     unordered pairs i < j of valid rows.  GNN_KNN_GRAPH_UNION: j in N(i) or i in N(j).  GNN_KNN_GRAPH_MUTUAL: both.  A pair
 *             stands once, at its smaller row; an invalid row owns nothing and is nobody's partner.  At most n_valid * k edges.
 *   mutual    uint8 per edge: 1 when both ends list each other (everywhere, under GNN_KNN_GRAPH_MUTUAL).  May be NULL.
 *   weight    GNN_KNN_GRAPH_SIMILARITY: where j is in N(i), the f32 that stands in row i's list for j - bit for bit gnn_graph's value
 *             of the pair; otherwise the f32 in row j's list for i, the other orientation, which may differ from gnn_graph's value in
 *             the last bit.  Negative similarities are kept: the consumers drop weights <= 0.  GNN_KNN_GRAPH_JACCARD: s = |N+(i) and
 *             N+(j)|, u = |N+(i)| + |N+(j)| - s, weight = (f32)s / (f32)u, one correctly rounded division; s >= 1, so it is in (0, 1].
 *   outputs   indptr (int64 [n + 1]), col (int32: a row's partners j > i strictly ascending), sim (f32), mutual (uint8).
 *   passes    count: the self-search into lists the ctx owns, every list put in ascending order, one walk over the lists that counts
 *             every row's edges (membership: a binary search), a prefix sum, indptr and the total (*nnz_host; the stream is
 *             synchronised to hand it back).  fill: the same walk files every edge in its owner's segment, every segment is put in
 *             order, and the weights and flags are written.  The caller sizes col, sim and mutual between the two.  The fill reads
 *             the lists its count left in the ctx, not the rows: it belongs to the ctx's LAST count, GNN_ERR_STATE unless that count
 *             had the same (n, k, mode, weight, metric).  No store leaves a row's segment or the total.
 *   ranges    0 <= n < 2^31, k in [1, 64], mode, weight and metric in [0, 1]; GNN_ERR_ARG with the value and the range in the message -
 *             checked before the ctx is looked at.  n == 0: indptr = [0], *nnz_host = 0.  capacity < the total: GNN_ERR_ARG with both
 *             numbers.  A total of 0: the fill launches nothing and col, sim and mutual may be NULL.
 *   exact     the edge set, an edge's owner and its weight follow from (i, j) and the lists alone, and a segment is ordered by a
 *             total order on distinct keys: integer atomics place the edges, yet no output bit depends on the order they arrive in,
 *             on the grid, on gnn_debug_set_neighbour_split or on the class limits below.
 * What it is not: not approximate; no k above 64; not multi-GPU; the consumers are not run from here.
 * Device memory, persistent in the ctx and grow-only: what gnn_neighbours_dev holds, 20 k B per row of lists, 36 B per row of lengths,
 * counters, offsets, cursors and class lists, 16 B per edge (gnn_knn_graph_count: + 8 B per row and the rows' 2 KB of f32;
 * gnn_knn_graph_fill: + 9 B per edge).  Nothing is n x n.
 * gnn_knn_graph_count / gnn_knn_graph_fill: host pointers, synchronous; the fill answers GNN_ERR_STATE unless a gnn_knn_graph_count
 * came before it.  gnn_knn_graph_count_dev: device pointers, *nnz_host on the host.  gnn_knn_graph_fill_dev: device pointers,
 * asynchronous on the ctx stream like gnn_classify_dev. */
typedef enum gnn_knn_graph_mode { GNN_KNN_GRAPH_UNION = 0, GNN_KNN_GRAPH_MUTUAL = 1 } gnn_knn_graph_mode;
typedef enum gnn_knn_graph_weight { GNN_KNN_GRAPH_SIMILARITY = 0, GNN_KNN_GRAPH_JACCARD = 1 } gnn_knn_graph_weight;
int gnn_knn_graph_count(gnn_ctx* ctx, const float* rows_host, int64_t n, int k, int mode, int weight, int metric, int64_t* indptr_host,
                        int64_t* nnz_host);
int gnn_knn_graph_fill(gnn_ctx* ctx, int64_t n, int k, int mode, int weight, int metric, int32_t* col_host, float* sim_host,
                       uint8_t* mutual_host_or_null, int64_t capacity);
int gnn_knn_graph_count_dev(gnn_ctx* ctx, const float* rows_dev, int64_t n, int k, int mode, int weight, int metric, int64_t* indptr_dev,
                            int64_t* nnz_host);
int gnn_knn_graph_fill_dev(gnn_ctx* ctx, int64_t n, int k, int mode, int weight, int metric, int32_t* col_dev, float* sim_dev,
                           uint8_t* mutual_dev_or_null, int64_t capacity);
/* test aids; no result depends on them, and a count fixes them for its fill.  A segment of up to gnn_debug_knn_graph_wave_rows entries
 * (1 .. 64, the default 64) is ordered by one wave in registers, one of up to gnn_debug_knn_graph_group_rows (1 .. 4096, the default
 * 2048) by a workgroup in LDS, a longer one by a workgroup's stable radix passes through a second buffer in global memory.
 * gnn_debug_knn_graph_classes: the rows the last count gave the [LDS, radix] class (2 values). */
int gnn_debug_knn_graph_wave_rows(gnn_ctx* ctx, int entries);
int gnn_debug_knn_graph_group_rows(gnn_ctx* ctx, int entries);
int gnn_debug_knn_graph_classes(gnn_ctx* ctx, int64_t* rows_out);
/* measurement only: with gnn_profile_enable on, the HIP-event milliseconds of the ctx's last gnn_knn_graph_count* call - [0] the
 * self-search, [1] the ordered lists, [2] the count, [3] the scan, indptr and the classes - and behind them those of every fill since:
 * [fill, order, finish]; *n_out = the figures recorded (0 for n == 0 or without profiling), at most `capacity` are written. */
int gnn_debug_knn_graph_ms(gnn_ctx* ctx, double* ms_out, int64_t capacity, int64_t* n_out);

/* ---- t-SNE layout of a similarity graph: exact, on the device ----------------------------------------------
 * "Where does every row lie in a 2-D picture of the graph": t-SNE's gradient descent with the graph's own weights as the affinities and
 * the exact all-pairs repulsion, from a given init.  The definition is sequence.tsne_layout; every output equals it bit for bit.
 *   graph     gnn_mcl's: an upper-triangle CSR with sim (f32, finite, < 64) and valid (uint8 [n], or NULL); exactly what
 *             gnn_graph_fill / gnn_knn_graph_fill write.  q = rint((f64)sim * 2^24); an entry with q <= 0 or an invalid end does not
 *             exist; an edge stands at both its ends and parallel entries stay separate.  M2 = the integer sum over all of them,
 *             p = (f32)((f64)q / (f64)M2).
 *   iterate   Y (f32 [n][2]) starts as `init`.  Per iteration, every f32 operation one IEEE operation, nothing fused: for row i and
 *             column j, dx = x_i - x_j, dy = y_i - y_j, qij = 1 / (1 + (dx dx + dy dy)) (0 where j = i, j is invalid or beyond n); per
 *             granule of 256 columns (aligned to the column index) three f32 chains in ascending column order - cz += qij,
 *             cx += (qij qij) dx, cy likewise - whose ends become integers: Zi += rint((f64)cz * 2^20), RX += rint((f64)cx * 2^32), RY
 *             likewise; Z = the sum of Zi.  Per entry (i, j): AX_i += rint((f64)((p qij) dx) * 2^32), AY likewise.  In f64, rounded
 *             to f32 once: g = 4 (e A / 2^32 - (R / 2^32) / (Z / 2^20)), e = `exaggeration` before iteration `exaggeration_iter` and 1
 *             from it on, the second term 0 where Z = 0.  In f32: gain += 0.2 where g and the previous update have strictly opposite
 *             signs, else gain *= 0.8, at least 0.01 (it starts at 1); upd = mom upd - lr (gain g), mom = 0.5 with e and 0.8 behind;
 *             Y += upd.  No recentring, no early end.
 *   outputs   layout (f32 [n][2]; NaN at an invalid row), z_trace (uint64 [n_iter + 1]: Z of every iterate, the final one included),
 *             valid_out (uint8 [n]).
 *   ranges    0 <= n <= 2^21 (Z < 2^63), n_iter and exaggeration_iter in [0, 100000], exaggeration in [1, 1024], learning_rate in
 *             (0, 2^20]: GNN_ERR_ARG with the value and the range - checked before the ctx is looked at.  A graph that is no such CSR
 *             and an init that is not finite at a valid row: GNN_ERR_ARG behind the one synchronise, before an output is written.
 *             n == 0: z_trace is n_iter + 1 zeros.
 *   exact     a granule's chains are the same whoever runs them and whatever the grid; everything behind them is a sum of integers:
 *             no output bit depends on gnn_debug_tsne_split, the grid or the order the graph's entries arrive in.
 * gnn_tsne_forces*: one evaluation at `y` (finite at every valid row) - zi, rx, ry, ax, ay (int64 [n]; 0 at an invalid row) and *m2.
 * What it is not: not Barnes-Hut nor FFT-interpolated; no perplexity-calibrated affinities; not UMAP; no transform of new rows; not
 * multi-GPU.  Cost: n^2 pairs per iteration.
 * Device memory, persistent in the ctx and grow-only: 12 B per entry at both ends, 89 B per row, 8 B per iterate (the host entry
 * points: + the graph, the init and the results).  Nothing is n x n.
 * gnn_tsne / gnn_tsne_forces: host pointers, synchronous.  gnn_tsne_dev / gnn_tsne_forces_dev: device pointers; the stream is
 * synchronised once, for the verdict on the graph and the init, and the whole loop is enqueued behind it without another read. */
int gnn_tsne(gnn_ctx* ctx, const int64_t* indptr_host, const int32_t* col_host, const float* sim_host, const uint8_t* valid_host_or_null,
             int64_t n, int64_t nnz, const float* init_host, int n_iter, int exaggeration_iter, double exaggeration, float learning_rate,
             float* layout_host, uint64_t* z_trace_host, uint8_t* valid_out_host);
int gnn_tsne_dev(gnn_ctx* ctx, const int64_t* indptr_dev, const int32_t* col_dev, const float* sim_dev, const uint8_t* valid_dev_or_null,
                 int64_t n, int64_t nnz, const float* init_dev, int n_iter, int exaggeration_iter, double exaggeration, float learning_rate,
                 float* layout_dev, uint64_t* z_trace_dev, uint8_t* valid_out_dev);
int gnn_tsne_forces(gnn_ctx* ctx, const int64_t* indptr_host, const int32_t* col_host, const float* sim_host,
                    const uint8_t* valid_host_or_null, int64_t n, int64_t nnz, const float* y_host, int64_t* zi_host, int64_t* rx_host,
                    int64_t* ry_host, int64_t* ax_host, int64_t* ay_host, int64_t* m2_host);
int gnn_tsne_forces_dev(gnn_ctx* ctx, const int64_t* indptr_dev, const int32_t* col_dev, const float* sim_dev,
                        const uint8_t* valid_dev_or_null, int64_t n, int64_t nnz, const float* y_dev, int64_t* zi_dev, int64_t* rx_dev,
                        int64_t* ry_dev, int64_t* ax_dev, int64_t* ay_dev, int64_t* m2_dev);
/* test aid; no result depends on it: the workgroups the repel pass splits the columns over, at granule boundaries (1 .. 65535; 0: the
 * library's choice). */
int gnn_debug_tsne_split(gnn_ctx* ctx, int splits);
/* measurement only: with gnn_profile_enable on, the HIP-event milliseconds of the ctx's last gnn_tsne* call - [0] validate, symmetrise
 * and affinities, [1] the whole loop, [2] the final Z and the results; *n_out = the figures recorded, at most `capacity` are written. */
int gnn_debug_tsne_ms(gnn_ctx* ctx, double* ms_out, int64_t capacity, int64_t* n_out);

/* ---- matches against a reference: the bipartite similarity graph query x base ------------------------------
 * "Which reference rows is every new row within the threshold of, all of them": every pair (i, j) of a valid query row i and a valid
 * base row j with sim(i, j) >= threshold and its similarity, as a CSR by query row.  The passes, the kernel, the workspace and the
 * contract are those of gnn_graph_* - the rectangle instead of the upper triangle -; validity, metric and threshold are those of
 * gnn_cluster; no forward pass runs and no other entry point's result changes.
 *   value     the similarity of the pair (i, j) is the f32 that gnn_neighbours returns for query i and base row j.  No pair is
 *             excluded: where query and base are the same rows, (i, i) and both orientations (i, j), (j, i) are present.  The threshold
 *             is compared as the f32 given; a tie is an edge; a similarity that is not a number is none.
 *   outputs   indptr (int64 [n_query + 1]): query row i owns col[indptr[i] .. indptr[i + 1]), its base partners in ascending order,
 *             and sim[...], their similarities; an invalid query owns nothing, an invalid base row is nobody's partner.  col is int32
 *             (n_base < 2^31), sim f32.
 *   passes    count, scan and fill as for the graph, over ceil(n_query / 64) tiles x the ranges of the base; the caller sizes col and
 *             sim between the two calls.
 *   state     the count / scan workspace is the graph's: a fill belongs to the ctx's LAST count of either kind.  gnn_match_fill* after
 *             a gnn_graph_count*, gnn_graph_fill* after a gnn_match_count*, and gnn_match_fill* for another (n_query, n_base,
 *             threshold, metric) answer GNN_ERR_STATE.  The rows must be the same; if they changed, the result is garbage, but no
 *             store leaves a row's segment.
 *   ranges    0 <= n_query, n_base < 2^31, a finite threshold, a metric in [0, 1]; GNN_ERR_ARG with the value and the range in the
 *             message - checked before the ctx is looked at.  n_query == 0 or n_base == 0: nothing is launched, indptr is n_query + 1
 *             zeros, *nnz_host = 0.  capacity < the total: GNN_ERR_ARG with both numbers.  A total of 0: the fill launches nothing and
 *             col and sim may be NULL.
 *   exact     as the graph: no atomics in global memory, bit-identical for every split of the base.
 * What it is not: not approximate; not a top-k (gnn_neighbours); no width other than GNN_EMBED_DIM; not multi-GPU.  The edge list is as
 * large as the threshold makes it - n_query * n_base at -1: look at *nnz_host before allocating.
 * Device memory, persistent in the ctx and grow-only: per base row the 2 KB of fragments + 1 B of the neighbour search (shared with it);
 * ALL query rows are prepared at once, with no slabs: 2 KB of fragments + 1 B per query row (the neighbour search's query buffers), and
 * 12 B per (query row, base range) of counters and offsets (shared with the graph).  gnn_match_count: + 2 KB of f32 per base row and per
 * query row and 8 B per query row; gnn_match_fill: + 8 B per edge.  Nothing is n_query x n_base.
 * gnn_match_count / gnn_match_fill: host pointers, synchronous; the base's rows go where every host-pointer search puts its base, the
 * query's into a buffer of the match's own; the fill prepares both again and answers GNN_ERR_STATE when another host-pointer search
 * has replaced the base's rows.  gnn_match_count_dev: device pointers, *nnz_host on the host.  gnn_match_fill_dev: device pointers,
 * asynchronous on the ctx stream like gnn_classify_dev. */
int gnn_match_count(gnn_ctx* ctx, const float* query_host, int64_t n_query, const float* base_host, int64_t n_base, float threshold,
                    int metric, int64_t* indptr_host, int64_t* nnz_host);
int gnn_match_fill(gnn_ctx* ctx, int64_t n_query, int64_t n_base, float threshold, int metric, int32_t* col_host, float* sim_host,
                   int64_t capacity);
int gnn_match_count_dev(gnn_ctx* ctx, const float* query_dev, int64_t n_query, const float* base_dev, int64_t n_base, float threshold,
                        int metric, int64_t* indptr_dev, int64_t* nnz_host);
int gnn_match_fill_dev(gnn_ctx* ctx, const float* query_dev, int64_t n_query, const float* base_dev, int64_t n_base, float threshold,
                       int metric, int32_t* col_dev, float* sim_dev, int64_t capacity);
/* measurement only: [count pass, scan] of the ctx's last gnn_match_count* call, as gnn_debug_graph_pass_ms (the figures are the
 * workspace's: those of the last count of either kind). */
int gnn_debug_match_pass_ms(gnn_ctx* ctx, double* ms_out, int64_t capacity, int64_t* n_out);

/* ---- spherical k-means among encoder embeddings: centroids on the device ------------------------------------
 * "Exactly k groups, and one new row that stands for each": a partition of the valid rows into k groups under cosine similarity and
 * one unit centroid per group (the definition is sequence.spherical_kmeans).  Validity is gnn_neighbours' under cosine; an invalid row
 * has label -1, sim NaN and contributes to nothing; no forward pass runs and no other entry point's result changes.
 *   assign    a row's label is the centroid with the largest similarity, ties to the smaller centroid index.  The similarity of (row i,
 *             centroid c) is the f32 that gnn_neighbours returns for query i and base row c of the centroid table.
 *   update    centroid c becomes the unit vector of the sum of its members' unit rows; a centroid without members, or whose sum is
 *             exactly zero, keeps its row bit for bit.  The sums are int64 sums of 32-bit fixed-point images of the rows' unit vectors
 *             (exact, a pure function of each row): no order of execution changes a bit of a centroid - a permutation of the rows
 *             gives the same table.  The norm is summed in float64 in a fixed order and the quotient rounded to f32 once.
 *   loop      label = assign(centroids); stop when no label changed against the previous assignment (*converged_host = 1) or after
 *             max_iter updates; otherwise centroids = update(label), *iterations_host += 1, again.  The labels returned are ALWAYS the
 *             assignment to the centroids returned; max_iter = 0 is a pure assignment to the init's unit rows.
 *   init      init (k x 512 f32, every row valid): its unit rows.  NULL: farthest-first traversal - the first centre is the valid row
 *             of smallest index, every next one the valid unpicked row whose largest similarity to the centres so far is smallest,
 *             ties to the smaller row index; the similarities are gnn_neighbours' for (row, that centre alone as the base).  No random
 *             number is drawn anywhere.  init_rows (int64 [k]): the rows picked, -1 for a given init.
 *   outputs   label int64 [n], sim f32 [n] (to the row's own centroid), centroids f32 [k][512] (unit rows), size int64 [k] (the
 *             members under the labels returned; 0 for a centroid nobody chose).
 *   ranges    0 <= n <= 2^30 (the int64 sums of more rows could overflow: |image| < 2^33), 1 <= k <= 65535, 0 <= max_iter <= 1000;
 *             GNN_ERR_ARG with the value and the range - checked before the ctx is looked at.  k more than the valid rows, or an init
 *             row that is not valid: GNN_ERR_ARG after one synchronise, nothing written.
 *   exact     integer add / max / min atomics only: bit-identical for every split of the centroids (gnn_debug_set_neighbour_split), for
 *             both paths of the update (gnn_debug_set_kmeans_lds) and for the host and _dev entry points.
 * gnn_centroids: the update alone, for ANY int64 labels in [-1, k) - one unit row per cluster of gnn_cluster / gnn_density /
 * gnn_representatives after a host-side relabel to 0 .. k - 1.  Label -1 and invalid rows are skipped; a group without members or with a
 * zero sum is a zero row, size = the valid members.  A label outside [-1, k): GNN_ERR_ARG, found on the device and reported after one
 * synchronise, nothing written.
 * What it is not: not Euclidean k-means and not the dot metric (rows are compared and summed as unit vectors); not k-means++ (no random
 * numbers); not mini-batch (every update sums every row); no width other than GNN_EMBED_DIM; not multi-GPU.
 * Device memory, persistent in the ctx and grow-only: per row the 2 KB of fragments + 1 B of the neighbour search (shared with it) and
 * 8 B (9 B under the farthest-first init); per centroid 2 KB + 1 B of fragments and 4 KB + 8 B of sums; 128 KB for the init.  Nothing is
 * n x k.  gnn_kmeans / gnn_centroids: host pointers, synchronous.  gnn_kmeans_dev: device pointers, iterations and converged on the host;
 * the ctx stream is synchronised once at the start and once per assignment (8 bytes each).  gnn_centroids_dev: device pointers, one
 * synchronise, then asynchronous on the ctx stream like gnn_classify_dev. */
int gnn_kmeans(gnn_ctx* ctx, const float* rows_host, int64_t n, int k, const float* init_host_or_null, int max_iter, int64_t* label_host,
               float* sim_host, float* centroids_host, int64_t* size_host, int64_t* init_rows_host, int64_t* iterations_host,
               int* converged_host);
int gnn_kmeans_dev(gnn_ctx* ctx, const float* rows_dev, int64_t n, int k, const float* init_dev_or_null, int max_iter, int64_t* label_dev,
                   float* sim_dev, float* centroids_dev, int64_t* size_dev, int64_t* init_rows_dev, int64_t* iterations_host,
                   int* converged_host);
int gnn_centroids(gnn_ctx* ctx, const float* rows_host, int64_t n, const int64_t* label_host, int k, float* centroids_host,
                  int64_t* size_host);
int gnn_centroids_dev(gnn_ctx* ctx, const float* rows_dev, int64_t n, const int64_t* label_dev, int k, float* centroids_dev,
                      int64_t* size_dev);
/* test aid: up to max_k groups (0 .. 128, default 128) a workgroup of the update adds in LDS, 16 at a time, before it adds to memory;
 * 0: every add goes straight to memory.  No result depends on it. */
int gnn_debug_set_kmeans_lds(gnn_ctx* ctx, int max_k);
/* measurement only: with profiling enabled, the HIP-event milliseconds of the ctx's last gnn_kmeans* call - [init, then per assignment:
 * assign, and behind every assignment but the last: update, finish, prepare] - as gnn_debug_graph_pass_ms. */
int gnn_debug_kmeans_pass_ms(gnn_ctx* ctx, double* ms_out, int64_t capacity, int64_t* n_out);

/* ---- principal components among encoder embeddings: Gram sums on the device ---------------------------------
 * "Look at the rows": the second moments of the UNIT rows - the geometry every search here works in - and the projection of rows onto
 * directions.  Validity is gnn_neighbours' under cosine; an invalid row contributes nothing to a moment and projects to NaN; no forward
 * pass runs and no other entry point's result changes.  The 512 x 512 eigenproblem between the two calls is the host's
 * (sequence.pca_from_moments): the matrix is 2 MB whatever n is, there is no device eigen-solver.
 *   moments   q_i = the 32-bit fixed-point image of row i's unit vector that gnn_kmeans sums: (hi + lo) * 2^24 of its own fragments,
 *             x_i = q_i * 2^-24 = unit * 2^8, exact in f32.
 *             S[d] = sum_i q_i[d], int64, exact: units of 2^-32 of sum_i u_i[d].
 *             G[a][b], int64, units of 2^-32 of sum_i u_i[a] u_i[b]: the rows are taken in granules of 256 rows aligned to the
 *             absolute row index; within a granule the products x_i[a] * x_i[b] are accumulated in f32 in ascending row order from 0
 *             (a k-ordered fmaf chain: v_mfma_f32_32x32x2_f32), the granule's f32 sum p becomes llrint((double)p * 2^16) once, and
 *             the granules' integers are added as integers.  No bit of G, S or n_valid depends on the row split
 *             (gnn_debug_set_pca_split) or on the order of execution; G is symmetric bit for bit.  Rows whose unit entries are powers
 *             of two times small integers (all products and partial sums exact in f32) give G = Q^T Q >> 32 exactly.
 *             n_valid: the valid rows.
 *   project   out[i][c] = s(i, c) - off[c], one f32 subtraction (off NULL: s itself), where s(i, c) IS the f32 that gnn_neighbours
 *             returns for query i and base row c of `components` under cosine - the components go through the prologue like any base:
 *             they are directions and are renormalised.  NaN at an invalid row or component.  out is [n][ncomp], nothing else is
 *             written.
 *   ranges    1 <= n <= 2^30 (the int64 sums of more rows could overflow), 1 <= ncomp <= 64; GNN_ERR_ARG with the value and the range
 *             - checked before the ctx is looked at.
 * What it is not: not PCA of the raw (un-normalised) rows, not kernel PCA, not t-SNE / UMAP, no width other than GNN_EMBED_DIM, not
 * more than 64 components, not multi-GPU, not incremental.
 * Device memory, persistent in the ctx and grow-only: per row the 2 KB of fragments + 1 B of the neighbour search (shared with it);
 * 128 KB for the components; the host forms' 2 MB of moments and n x ncomp f32 of output.  gnn_pca_moments / gnn_pca_project: host
 * pointers, synchronous.  The _dev forms: device pointers (G int64 [512 * 512], S int64 [512], n_valid int64 [1]; components f32
 * [ncomp][512], off f32 [ncomp] or NULL, out f32 [n][ncomp]), asynchronous on the ctx stream like gnn_classify_dev. */
int gnn_pca_moments(gnn_ctx* ctx, const float* rows_host, int64_t n, int64_t* G_host, int64_t* S_host, int64_t* n_valid_host);
int gnn_pca_moments_dev(gnn_ctx* ctx, const float* rows_dev, int64_t n, int64_t* G_dev, int64_t* S_dev, int64_t* n_valid_dev);
int gnn_pca_project(gnn_ctx* ctx, const float* rows_host, int64_t n, const float* components_host, int ncomp, const float* off_host_or_null,
                    float* out_host);
int gnn_pca_project_dev(gnn_ctx* ctx, const float* rows_dev, int64_t n, const float* components_dev, int ncomp, const float* off_dev_or_null,
                        float* out_dev);
/* test aid: the rows a workgroup of the Gram pass takes - a multiple of 256, anything else is GNN_ERR_ARG; 0: the library's choice
 * (every CU about two workgroups).  No result depends on it. */
int gnn_debug_set_pca_split(gnn_ctx* ctx, int64_t rows_per_workgroup);
/* measurement only: with profiling enabled, the HIP-event milliseconds of the ctx's last gnn_pca_* call - moments: [prepare, sums,
 * gram, mirror]; project: [prepare rows, prepare components, project] - as gnn_debug_kmeans_pass_ms.  Synchronises the ctx stream;
 * ask before the ctx's next call of any kind. */
int gnn_debug_pca_pass_ms(gnn_ctx* ctx, double* ms_out, int64_t capacity, int64_t* n_out);

/* ---- label transfer among encoder embeddings: per-class neighbourhood votes on the device -------------------
 * "Which class do this row's neighbours say it is": for every valid query row i and every class c of a labelled base, the voters - the
 * valid base rows j with label[j] == c and sim(i, j) >= threshold - counted, their similarities summed and the most similar one named
 * (the definition is sequence.class_votes).  Cosine only; validity is gnn_neighbours' under cosine; no forward pass runs and no other
 * entry point's result changes.
 *   value     the similarity of the pair (i, j) is the f32 that gnn_neighbours and gnn_match_* return for query i and base row j.  The
 *             threshold is compared as the f32 given; a tie is a vote; a similarity that is not a number is none.
 *   labels    label int64 [n_base]: a value in [0, n_classes) makes a valid row a voter, -1 means unlabelled - the row is ignored.  Any
 *             other value: GNN_ERR_ARG, found on the device and reported after one synchronise, before any output is touched.
 *   self      base NULL: the rows vote among themselves - n_base is ignored, label has n_query entries and the pair (i, i) is left
 *             out: leave-one-out over a labelled set, or a per-row agreement score for the labels of gnn_cluster / gnn_density /
 *             gnn_kmeans.
 *   outputs   four arrays [n_query][n_classes].  count int64: the voters.  weight int64: the sum of llrint((double)s * 2^32) over them -
 *             the similarity sum in units of 2^-32.  nearest int64 / nearest_sim f32: the most similar voter, ties to the smaller
 *             base index; -1 / NaN where the class has no voter.  An invalid query row has 0 / 0 / -1 / NaN in every class.
 *   exact     the product by 2^32 is exact in float64 and llrint rounds half to even, as numpy's rint does: the sums are the int64
 *             sums of the definition taken on the device's own f32 similarities, bit for bit.  Integer add / max atomics only:
 *             bit-identical for every split of the base (gnn_debug_set_neighbour_split), for both paths (gnn_debug_set_vote_lds) and
 *             for the host and _dev entry points; a permutation of the base rows with their labels changes no bit of count, weight
 *             or nearest_sim.
 *   ranges    0 <= n_query < 2^31, 0 <= n_base <= 2^30 (|llrint(s * 2^32)| <= 2^32 + 2^10: the int64 sums of more voters could
 *             overflow), 1 <= n_classes <= 1024, a finite threshold; GNN_ERR_ARG with the value and the range - checked before the ctx
 *             is looked at.  n_base == 0: every class is empty.
 * What it is not: not a top-k vote (every row within the threshold votes, however many); not the dot metric; not approximate; no width
 * other than GNN_EMBED_DIM; not multi-GPU; no calibrated probability - a share of votes is a share of votes.
 * Device memory, persistent in the ctx and grow-only: per base row the 2 KB of fragments + 1 B of the neighbour search (shared with it)
 * and 4 B of its class; the queries go in slabs of 262 144 rows: 2 KB + 1 B per row of a slab (the neighbour search's query buffers)
 * and 8 B per (row of a slab, class) of keys.  gnn_vote: + 2 KB of f32 per base row and per query row of a slab, 8 B per base row and
 * 28 B per (row of a slab, class).  Nothing is n_query x n_base.
 * gnn_vote: host pointers, synchronous.  gnn_vote_dev: device pointers; the ctx stream is synchronised once (the labels' verdict), the
 * rest is enqueued on it like gnn_classify_dev. */
int gnn_vote(gnn_ctx* ctx, const float* query_host, int64_t n_query, const float* base_host_or_null, int64_t n_base,
             const int64_t* label_host, int n_classes, float threshold, int64_t* count_host, int64_t* weight_host, int64_t* nearest_host,
             float* nearest_sim_host);
int gnn_vote_dev(gnn_ctx* ctx, const float* query_dev, int64_t n_query, const float* base_dev_or_null, int64_t n_base,
                 const int64_t* label_dev, int n_classes, float threshold, int64_t* count_dev, int64_t* weight_dev, int64_t* nearest_dev,
                 float* nearest_sim_dev);
/* test aid: up to max_classes classes (0 .. 16, default 16) a workgroup votes in LDS before it adds to memory; 0: every vote goes
 * straight to memory.  No result depends on it. */
int gnn_debug_set_vote_lds(gnn_ctx* ctx, int max_classes);
/* measurement only: with profiling enabled, the HIP-event milliseconds of the ctx's last gnn_vote* call - [labels, then per slab of
 * queries: votes, finish] - as gnn_debug_pca_pass_ms: synchronises the ctx stream; ask before the ctx's next call of any kind. */
int gnn_debug_vote_pass_ms(gnn_ctx* ctx, double* ms_out, int64_t capacity, int64_t* n_out);

/* ---- host-side FASTA record packer (no GPU needed) ------------------------------------------------ */
/* replaces the line loop of sequence.read_fasta(path, strip_n) (genomad/sequence.py:96-121) on an
 * in-memory text buffer (already decompressed, newlines normalised to '\n').
 * gnn_fasta_scan: number of header lines (= upper bound of the record count), total bytes of header
 * text, and whether the buffer contains a '\r' (the caller then normalises newlines first, as the
 * reference's text-mode read does).
 * gnn_fasta_pack: sequence bytes of every surviving record back to back into seq_out (capacity n;
 * MAY BE THE SAME BUFFER AS text: packing only moves bytes towards lower addresses), record i =
 * seq_out[offsets[i] .. offsets[i+1]) (capacity+1 entries), and its header text (without the '>')
 * = headers_out[header_offsets[i] .. header_offsets[i+1]) (headers_out: header_bytes from the scan).
 * seq_out == NULL (with strip_n == 0) is the index mode: nothing is copied, offsets hold cumulative
 * raw lengths — the headers of the non-empty records, which is what check_fasta needs
 * (sequence.py:124-131).
 * Rules: header = line starting with '>', text before the first header dropped, only '\n' removed,
 * strip_n strips leading/trailing n/N, empty records dropped. */
int gnn_fasta_scan(const uint8_t* text, int64_t n, int64_t* n_headers, int64_t* header_bytes, int* has_cr);
int gnn_fasta_pack(const uint8_t* text, int64_t n, int strip_n, uint8_t* seq_out, int64_t* offsets,
                   uint8_t* headers_out, int64_t* header_offsets, int64_t capacity, int64_t* n_records);
/* replaces, for a multi-rank run, the accession bookkeeping of sequence.check_fasta (genomad/sequence.py:124-131: no record /
 * two records with one accession = header.split()[0], sequence.py:24-25): 64-bit digests of the accessions of every record of
 * `text` whose raw sequence is non-empty, in file order, in ONE pass (capacity from gnn_fasta_scan).  *needs_python = 1 when a
 * header has a byte >= 0x80 before the end of its first token (Python's split() knows non-ASCII white space) or an empty
 * accession: the caller then recomputes this text with the Python mirror of the hash (genomad_amd/sequence.py).  Host only. */
int gnn_fasta_accession_digests(const uint8_t* text, int64_t n, uint64_t* digests, int64_t capacity, int64_t* n_records,
                                int* needs_python);

/* ---- downstream score consumers as a device epilogue, float64 like the
 * reference's numpy ------------------------------------------------------------------------------ */
/* replaces branch_attention(w, b1, b2, temperature) (aggregated_classification.py:10-34): w[n] marker
 * frequency, b1[n][3] marker scores, b2[n][3] nn scores -> out[n][3]. */
int gnn_branch_attention(gnn_ctx* ctx, const double* w_host, const double* b1_host, const double* b2_host,
                         int64_t n, double temperature, double* out_host);
/* replaces the inference part of score_batch_correction (score_calibration.py:37-43): scores[n][3] and
 * the (already smoothed, :18-21) composition[3] through the 6->20->20->3 tanh MLP whose weights are the
 * arrays of genomad/data/score_calibration_weights.npz (kernel_1 (6,20), bias_1, kernel_2 (20,20), ...). */
int gnn_score_calibration(gnn_ctx* ctx, const double* scores_host, const double* composition3,
                          const double* kernel1, const double* bias1, const double* kernel2,
                          const double* bias2, const double* kernel3, const double* bias3, int64_t n,
                          double* out_host);

/* CRC-32C (Castagnoli) of a host buffer: the checksum of the TFRecord framing that the reference's
 * write_tfrecord produces (nn_classification.py:43-52); used by genomad_amd/tfrecord.py. Host only. */
uint32_t gnn_crc32c(const void* data_host, size_t n_bytes);

/* same forward as gnn_classify, also copying intermediates out (parity tests). */
int gnn_debug_forward(gnn_ctx* ctx, const uint8_t* bases_host, int64_t n_windows, int precision,
                      float* scores_host, const gnn_taps* taps);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI ---------------------------------
 * The path shards with no data-path collective: rank r classifies its own contiguous range of windows
 * (or contigs) with the replicated weights; the only exchange is the END-OF-RUN gather of the 12 B/window
 * class scores (the `predictions` the reference concatenates at nn_classification.py:316-319) to rank 0,
 * plus small control messages.  librccl.so is dlopen()ed on first use.  All collectives are enqueued on
 * the ctx stream; the host-buffer variants stage through device memory and synchronise before returning.
 * Bootstrap: rank 0 calls gnn_comm_unique_id and hands the 128 bytes to the other ranks out of band
 * (genomad_amd/rccl.py uses a file next to the launcher's rendezvous); every rank then calls gnn_comm_init. */
#define GNN_COMM_ID_BYTES 128
int gnn_comm_unique_id(uint8_t* id128);                                   /* ncclGetUniqueId */
int gnn_comm_init(gnn_ctx* ctx, int n_ranks, int rank, const uint8_t* id128);   /* ncclCommInitRank on ctx's device */
int gnn_comm_destroy(gnn_ctx* ctx);
int gnn_comm_info(gnn_ctx* ctx, int* n_ranks, int* rank);                  /* (1, 0) without a communicator */
/* ncclGather (rccl.h:745) of bytes_per_rank bytes from every rank to `root`: recv holds n_ranks blocks in rank
 * order (ignored on other ranks).  _dev: device pointers, asynchronous on the ctx stream. */
int gnn_comm_gather_dev(gnn_ctx* ctx, const void* send_dev, void* recv_dev, size_t bytes_per_rank, int root);
int gnn_comm_gather(gnn_ctx* ctx, const void* send_host, void* recv_host, size_t bytes_per_rank, int root);
int gnn_comm_allgather(gnn_ctx* ctx, const void* send_host, void* recv_host, size_t bytes_per_rank);
int gnn_comm_allreduce_max(gnn_ctx* ctx, double* values_host, int n);      /* in place; used for max-over-ranks timing */
int gnn_comm_barrier(gnn_ctx* ctx);

/* ---- synthetic data + measurement ------------------------------------------------------ */
/* windows first..first+n of the counter-based synthetic set (genomad_amd/synthetic.py) */
int gnn_synth_windows_dev(gnn_ctx* ctx, uint64_t seed, int64_t first, int64_t n_windows,
                          uint8_t* bases_dev);

/* HIP-event timing of the kernels launched on the ctx stream.  kernel ids: */
#define GNN_K_FUSED 0        /* fused tokens->conv1..3->IGLOO front end (dominant kernel) */
#define GNN_K_BACKEND 1      /* logits GEMM + softmax + attention + dense stack           */
#define GNN_K_ENCODER 2      /* stand-alone byte -> one-hot encoder                       */
#define GNN_K_F32_FRONT 3    /* unfused f32 front end (all its kernels)                   */
#define GNN_K_ATTR_HEAD 4    /* attribution: dense head forward + backward (gnn_attribute*)  */
#define GNN_K_ATTR_CONTRIB 5 /* attribution: the contribution kernel (second read of yp)     */
#define GNN_K_REGIONS 6      /* region calls: every kernel of gnn_region_states_dev / gnn_call_regions; interval embeddings: the fold and
                              * finish kernels of gnn_embed_intervals / gnn_interval_fold_dev / gnn_interval_finish_dev */
#define GNN_K_NEIGHBOURS 7   /* nearest neighbours: the prepare, tile and merge kernels of gnn_neighbours / gnn_neighbours_dev; clusters:
                              * every kernel of gnn_cluster / gnn_cluster_dev; representatives: every kernel of gnn_representatives*;
                              * single-linkage tree: every kernel of gnn_linkage / gnn_linkage_dev; density clusters: every kernel of
                              * gnn_density / gnn_density_dev */
#define GNN_K_COUNT 8
int gnn_profile_enable(gnn_ctx* ctx, int on);
int gnn_profile_reset(gnn_ctx* ctx);
/* synchronises the stream, then total milliseconds and number of launches of kernel_id */
int gnn_profile_get(gnn_ctx* ctx, int kernel_id, double* total_ms, int64_t* launches);

/* debug aid: per-phase shader-cycle sums of the fused kernel (instrumented build).  on=1 starts
 * (zeroes the counters), on=0 stops; out16 (may be NULL) receives the 16 counters collected so far
 * (their meaning depends on the kernel variant: see GNN_TICK in gnn_fused.hip / gnn_fused2.hip). */
int gnn_phase_cycles(gnn_ctx* ctx, int on, unsigned long long* out16);

/* measurement aid: sustained dense bf16 rate (TFLOP/s) of v_mfma_f32_32x32x16_bf16 with one wave per
 * SIMD and register operands, run for about ms_target milliseconds — the practical MFMA ceiling of
 * this (power-managed) chip, reported by bench.py beside the fused kernel's issued-MFMA rate. */
int gnn_mfma_probe(gnn_ctx* ctx, int ms_target, double* tflops_out);
/* the same with the MFMA of `kind`: 0 = v_mfma_f32_32x32x16_bf16, 1 = v_mfma_f32_32x32x16_f16 (the instruction of the default
 * arithmetic: bench.py prints the issued f16 MFMA rate of the f16x3 kernel as a fraction of it, `frac_of_power_floor`), 2 = the
 * MFMA mix of f16c6 (8 f16 + 4 MX-fp6 scaled MFMAs per k32 step), reported in algorithmic TFLOP/s (the f16 MFMAs only) */
int gnn_mfma_probe_kind(gnn_ctx* ctx, int kind, int ms_target, double* tflops_out);

/* measurement aid: rows (token positions) a workgroup of the fused front end of `precision` streams per step
 * (128 for the f16c8 / x3 kernels; 32 * GNN_C6_NMB for f16c6), 0 for GNN_PREC_F32, negative on a bad enum. */
int gnn_fused_rows_per_step(int precision);

/* test aid: the f16c6 kernel does not compute the steps of a window that lie entirely in its all-N tail (the padding of a
 * contig's last window, nn_classification.py:72) — it copies the rows an all-N window produces, which the library computed
 * with the same kernel at gnn_load_weights time (bit-identical by construction).  on = 0 makes it compute everything; the
 * default is on (environment GNN_NO_PAD_SKIP=1 turns it off at gnn_create). */
int gnn_debug_set_pad_skip(gnn_ctx* ctx, int on);

/* test aid: launches of the default arithmetic with fewer windows than the device has CUs (the reference's own call shape, one
 * predict per 128 windows: nn_classification.py:316-317) deal every window's steps to up to 4 workgroups, each with one
 * warm-up step (gnn_fused_x3.hip) - bit-identical to the one-workgroup launch by construction.  on = 0 launches one workgroup per
 * window whatever the batch size; the default is on (environment GNN_NO_TIME_SPLIT=1 turns it off at gnn_create). */
int gnn_debug_set_time_split(gnn_ctx* ctx, int on);
/* workgroups per window of the ctx's last launch of a streaming kernel (F16X3TC / F16X3 / BF16X3): 1, or 2..4 under the time split */
int gnn_debug_last_split(gnn_ctx* ctx, int* workgroups_per_window);

/* test aid, host only (no GPU, no ctx): the f16c6 weight stream of a row-major K x N matrix (K multiple of 128, N of 32) as
 * gnn_load_weights builds it — per (k32 step, 32-column block) 3584 B: the f16 fragments of the two k16 halves (2 x 1 KiB:
 * lane l holds column l & 31, k = 16 s + 8 (l >> 5) + 0..7), the fp6 (e2m3) fragment dwords 0-3 (1 KiB) and 4-5 (512 B) of
 * MX block l >> 5 (0: w - f16(w), 1: w; element i of the step's 32 k in bits 6i..6i+5) — followed by the E8M0 scale words
 * [k / 128][block][lane], byte (k / 32) % 4.  need_words receives the size in 32-bit words; out may be NULL to query it. */
int gnn_debug_pack_c6(const float* w, int k, int n, uint32_t* out, size_t out_words, size_t* need_words);

/* Windows the ctx processes per launch of the fused front end.  Workspace: 0.86 MB per window of a launch (pair products, pooled
 * y @ w_v rows, logits, attention weights, features) - 14 GB at the default ceiling of 16384, allocated on the first large call and
 * TWICE that once gnn_classify_dev_async is used (two alternating workspaces).  Without a call to this function the library clamps
 * the default to a quarter of the device memory that is free when the workspace first grows (shared / partitioned GPUs) and says so
 * on stderr; with or without it, a failed workspace allocation is retried with half the launch size (down to 256 windows) before
 * GNN_ERR_NOMEM is returned, and a second workspace that does not fit makes the asynchronous path run in order on one.
 * 16384 vs 2048 windows per launch: +0.7 % throughput (profiles/r04/backend_overlap_ab.txt). */
int gnn_set_chunk(gnn_ctx* ctx, int64_t windows_per_chunk);

#ifdef __cplusplus
}
#endif
#endif /* GENOMAD_NN_H */
