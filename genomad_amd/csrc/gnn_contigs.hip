// Contig front end as ONE entry point: packed raw contig bytes + offsets -> per-contig
// class scores.  Replaces, for a whole packed buffer, generate_data (window cutting, the N-content rule,
// upper-casing, padding, tokenising: nn_classification.py:54-82), the predict loop and
// tf.math.segment_mean (:316-320) without a per-window host object and without the window scores ever
// leaving the device.
//
// Everything after the span table is asynchronous: the sequence bytes (when they start on the host) go up
// in pieces on a copy stream while earlier pieces are classified on the ctx stream; the N-content rule is
// evaluated on the device and applied as a MASK of the segment mean — every candidate window is
// classified, windows the rule drops (window_n > 0 and more than 4000 literal 'N') just do not enter their
// contig's mean, so no host round trip sits between the rule and the classification.  (Dropped windows are
// rare: they cost one window's work each.)  All buffers are persistent and grow-only (gnn_destroy frees them).
//
// gnn_scan_contigs is the same function at a stride: windows start every `stride` bases instead of every 6000, their scores DO
// leave the device, and a fold kernel turns them into a track of one score triple per stride-wide bin ("Score tracks").
// At stride 6000 the span table, and with it every bit of the contig scores, is the one of gnn_classify_contigs.
//
// The *_strand entry points are the same function with one more parameter ("Both strands"): every span is also - or only -
// materialised as its reverse complement (revcomp_kernel), a slab's forward and reverse windows go through the front end as ONE
// batch, and a split kernel files the batch's scores per strand and forms the `both` score (f + r) * 0.5f.  Spans, the N rule, ids,
// bins and the folds are the forward ones.
#include <algorithm>
#include <cstring>

#include "gnn_common.h"

namespace gnn {

// What gnn_scan_contigs adds to a call of classify_contigs: host buffers for the per-window and per-bin results.
struct ScanOut {
    float* window_scores;
    uint8_t* window_kept;       // may be NULL
    int64_t windows_capacity;
    float* track;               // may be NULL
    int32_t* cover;             // may be NULL
    int64_t bins_capacity;
};

// What the *_strand entry points add: the mode (gnn_strand) and host buffers for each strand's own results (any may be NULL).  A
// strand is computed when the mode needs it or one of its buffers is given.
struct StrandOut {
    int strand;
    float* contig_fwd;          // [n_contigs][3]: each strand's own masked mean
    float* contig_rev;
    float* window_fwd;          // scans only: [n_windows][3]
    float* window_rev;
};

void free_contig_ws(gnn_ctx* ctx) {
    ContigWorkspace* w = ctx->contig_ws;
    if (!w) return;
    for (hipEvent_t e : w->piece_done) (void)hipEventDestroy(e);
    if (w->copy_stream) (void)hipStreamDestroy(w->copy_stream);
    delete w;
    ctx->contig_ws = nullptr;
}

// tf.math.segment_mean over the windows the N-content rule keeps (nn_classification.py:70-71, :320): one thread
// per (contig, class); ids are sorted, the contig's windows are a contiguous run summed in window order —
// the same order and arithmetic as segment_mean_kernel, so the two agree bit for bit on the kept windows.
__global__ void masked_segment_mean_kernel(const float* __restrict__ scores, const int64_t* __restrict__ ids,
                                           const int32_t* __restrict__ window_n, const int32_t* __restrict__ counts,
                                           int64_t n, int64_t n_seg, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_seg * GNN_CLASSES) return;
    const int64_t seg = i / GNN_CLASSES;
    const int cl = (int)(i % GNN_CLASSES);
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ids[mid] < seg) lo = mid + 1; else hi = mid;
    }
    float s = 0.f;
    int kept = 0;
    for (int64_t k = lo; k < n && ids[k] == seg; ++k)
        if (window_n[k] == 0 || counts[k] <= MAX_N) {
            s += scores[k * GNN_CLASSES + cl];
            ++kept;
        }
    out[i] = kept ? s / (float)kept : 0.f;
}

int launch_masked_segment_mean(gnn_ctx* ctx, const float* scores, const int64_t* ids, const int32_t* window_n, const int32_t* counts,
                               int64_t n, int64_t n_seg, float* out) {
    const int64_t threads = n_seg * GNN_CLASSES;
    hipLaunchKernelGGL(masked_segment_mean_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ctx->stream, scores, ids,
                       window_n, counts, n, n_seg, out);
    GNN_HIP(hipGetLastError());
    return GNN_OK;
}

// Per-contig embedding fold of one slab [a, a + m) of the window table: one block per contig the slab touches (ids are sorted, so
// contigs ids[a] .. ids[a+m-1]), 128 lanes x 4 columns = one 2 KB row per step, read as float4s (coalesced: a row is contiguous).
// The contig's kept windows of this slab are added to its running sum in window order, starting from what the slabs before left
// there, so the sum is ((0 + e_0) + e_1) + ... whatever the slab and launch sizes.  Kept = the rule of masked_segment_mean_kernel.
constexpr int FOLD_THREADS = HID / 4;

__global__ __launch_bounds__(FOLD_THREADS) void emb_fold_kernel(const float* __restrict__ emb, const int64_t* __restrict__ ids,
                                                                const int32_t* __restrict__ window_n, const int32_t* __restrict__ counts,
                                                                int64_t a, int64_t m, float* __restrict__ sums, int32_t* __restrict__ kept) {
    const int64_t seg = ids[a] + blockIdx.x;
    int64_t lo = a, hi = a + m;                 // first window of the slab with ids >= seg
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ids[mid] < seg) lo = mid + 1; else hi = mid;
    }
    float4* row = reinterpret_cast<float4*>(sums + (size_t)seg * HID) + threadIdx.x;
    float4 s = *row;
    int k = 0;
    for (int64_t i = lo; i < a + m && ids[i] == seg; ++i)
        if (window_n[i] == 0 || counts[i] <= MAX_N) {
            const float4 v = reinterpret_cast<const float4*>(emb + (size_t)(i - a) * HID)[threadIdx.x];
            s.x += v.x;
            s.y += v.y;
            s.z += v.z;
            s.w += v.w;
            ++k;
        }
    *row = s;
    if (threadIdx.x == 0) kept[seg] += k;
}

// sums -> means in place (a contig without a kept window keeps its zero row, as the scores do)
__global__ void emb_mean_kernel(float* __restrict__ sums, const int32_t* __restrict__ kept, int64_t n_contigs) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_contigs * HID) return;
    const int k = kept[i / HID];
    sums[i] = k ? sums[i] / (float)k : 0.f;
}

// The track fold of gnn_scan_contigs: one thread per (bin, class), the output index is the thread index (coalesced stores).  Bin b
// of a contig is [b * stride, (b + 1) * stride); window k covers it iff k <= b and b * stride < k * stride + len_k, which bounds
// k from below by b - (W - 1) / stride: at most ceil(W / stride) windows, read in increasing k and added in that order in f32 (the
// order is part of the contract: no atomics), divided once.  Kept = the rule of masked_segment_mean_kernel.  A bin without a kept
// covering window (a dropped tail, or every covering window masked by the N rule) is NaN in all three classes, cover 0.
__global__ void scan_track_kernel(const float* __restrict__ scores, const int32_t* __restrict__ lens, const int32_t* __restrict__ counts,
                                  const int64_t* __restrict__ win_off, const int64_t* __restrict__ bin_off, int64_t n_contigs,
                                  int64_t n_bins, int stride, float* __restrict__ track, int32_t* __restrict__ cover) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_bins * GNN_CLASSES) return;
    const int64_t bin = i / GNN_CLASSES;
    const int cl = (int)(i % GNN_CLASSES);
    int64_t lo = 0, hi = n_contigs - 1;            // the contig with bin_off[c] <= bin < bin_off[c + 1] (empty contigs own no bin)
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (bin_off[mid + 1] <= bin) lo = mid + 1; else hi = mid;
    }
    const int64_t b = bin - bin_off[lo];
    const int64_t w0 = win_off[lo], nw = win_off[lo + 1] - w0;
    const int64_t reach = (W - 1) / stride;
    const int64_t k_lo = b > reach ? b - reach : 0, k_hi = b < nw - 1 ? b : nw - 1;
    float s = 0.f;
    int kept = 0;
    for (int64_t k = k_lo; k <= k_hi; ++k) {
        const int64_t j = w0 + k;
        if (b * stride < k * stride + lens[j] && (k == 0 || counts[j] <= MAX_N)) {
            s += scores[j * GNN_CLASSES + cl];
            ++kept;
        }
    }
    track[i] = kept ? s / (float)kept : __builtin_nanf("");
    if (cl == 0) cover[bin] = kept;
}

// The scores of one slab's batch [m forward windows | m reverse windows] -> each strand's rows of the window table, and the
// `both` score (f + r) * 0.5f: one f32 addition, one exact halving - a single rounding.  One thread per (window, class).
__global__ void strand_split_kernel(const float* __restrict__ batch, int64_t cells, float* __restrict__ fwd, float* __restrict__ rev,
                                    float* __restrict__ mix) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cells) return;
    const float f = batch[i], r = batch[cells + i];
    fwd[i] = f;
    rev[i] = r;
    mix[i] = (f + r) * 0.5f;
}

// `both`: the two strands' embedding sums -> (sum_f + sum_r) / (2 kept), in place in sum_f (zero row without a kept window)
__global__ void emb_both_mean_kernel(float* __restrict__ sums, const float* __restrict__ sums_rev, const int32_t* __restrict__ kept,
                                     int64_t n_contigs) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_contigs * HID) return;
    const int k = kept[i / HID];
    sums[i] = k ? (sums[i] + sums_rev[i]) / (float)(2 * k) : 0.f;
}

}  // namespace gnn

using namespace gnn;

static int classify_contigs(gnn_ctx* ctx, const uint8_t* seq, int seq_on_host, int64_t seq_bytes, const int64_t* offsets_host,
                            int64_t n_contigs, int single_window, int precision, float* contig_scores_host, int64_t* window_ids_host,
                            int64_t ids_capacity, int64_t* n_windows_out, float* contig_emb_host, int64_t stride = W,
                            const ScanOut* scan = nullptr, const StrandOut* so = nullptr) {
    const char* const fn = scan ? "gnn_scan_contigs" : "gnn_classify_contigs";
    const int strand = so ? so->strand : GNN_STRAND_FORWARD;
    // which strands run: what the mode averages, and what the caller asked to see on its own
    const bool need_f = strand != GNN_STRAND_REVERSE || (so && (so->contig_fwd || so->window_fwd));
    const bool need_r = strand != GNN_STRAND_FORWARD || (so && (so->contig_rev || so->window_rev));
    const int64_t ns = (need_f ? 1 : 0) + (need_r ? 1 : 0);
    if (!ctx) {
        set_error("ctx is NULL");
        return GNN_ERR_ARG;
    }
    GNN_HIP(hipSetDevice(ctx->device));
    {
        const int frc = finish_pending(ctx);
        if (frc) return frc;
    }
    if (n_contigs < 0 || seq_bytes < 0 || !offsets_host || !n_windows_out || (n_contigs > 0 && !contig_scores_host && !scan) ||
        (seq_bytes > 0 && !seq)) {
        set_error(std::string("bad argument to ") + fn);
        return GNN_ERR_ARG;
    }
    if (offsets_host[0] < 0 || offsets_host[n_contigs] > seq_bytes) {
        set_error("contig offsets outside the sequence buffer");
        return GNN_ERR_ARG;
    }
    if (!ctx->contig_ws) ctx->contig_ws = new ContigWorkspace();
    ContigWorkspace& w = *ctx->contig_ws;

    // ---- candidate windows: seq_windows(seq, 6000, 2500, max_windows) for every contig (sequence.py:150-167), at `stride`
    w.starts.clear(), w.lens.clear(), w.ids.clear(), w.window_n.clear();
    w.win_off.assign(1, 0), w.bin_off.assign(1, 0);
    for (int64_t c = 0; c < n_contigs; ++c) {
        const int64_t a = offsets_host[c], b = offsets_host[c + 1];
        if (b < a) {
            set_error("contig offsets are not non-decreasing");
            return GNN_ERR_ARG;
        }
        for_each_window(b - a, stride, single_window, [&](int64_t k, int64_t l) {
            w.starts.push_back(a + k * stride);
            w.lens.push_back((int32_t)l);
            w.ids.push_back(c);
            w.window_n.push_back((int32_t)k);
        });
        if (scan) {
            w.win_off.push_back((int64_t)w.starts.size());
            w.bin_off.push_back(w.bin_off.back() + (b - a + stride - 1) / stride);
        }
    }
    const int64_t n = (int64_t)w.starts.size();
    const int64_t n_bins = w.bin_off.back();
    const bool fold = scan && (scan->track || scan->cover);
    *n_windows_out = 0;
    if (n_contigs && contig_scores_host) std::memset(contig_scores_host, 0, (size_t)n_contigs * GNN_CLASSES * sizeof(float));
    if (n_contigs && contig_emb_host) std::memset(contig_emb_host, 0, (size_t)n_contigs * HID * sizeof(float));
    if (so)
        for (float* p : {so->contig_fwd, so->contig_rev})
            if (n_contigs && p) std::memset(p, 0, (size_t)n_contigs * GNN_CLASSES * sizeof(float));
    if (n == 0) return GNN_OK;
    if (scan) {
        if (!scan->window_scores || scan->windows_capacity < n) {
            set_error("window_scores_host holds " + std::to_string(scan->windows_capacity) + " windows, the scan has " + std::to_string(n));
            return GNN_ERR_ARG;
        }
        if (fold && scan->bins_capacity < n_bins) {
            set_error("track_host / cover_host hold " + std::to_string(scan->bins_capacity) + " bins, the scan has " + std::to_string(n_bins));
            return GNN_ERR_ARG;
        }
    } else if (!window_ids_host || ids_capacity < n) {
        set_error("window_ids_host holds " + std::to_string(ids_capacity) + " entries, " + std::to_string(n) + " candidate windows");
        return GNN_ERR_ARG;
    }

    // ---- device buffers
    int rc = GNN_OK;
    if (w.span_cap() < (size_t)n) {
        GNN_HIP(hipStreamSynchronize(ctx->stream));
        reset_all(w.d_starts, w.d_ids, w.d_lens, w.d_window_n, w.d_counts, w.d_scores);
        if (!rc) rc = reserve_roomy(w.d_starts, (size_t)n);
        if (!rc) rc = reserve_roomy(w.d_ids, (size_t)n);
        if (!rc) rc = reserve_roomy(w.d_lens, (size_t)n);
        if (!rc) rc = reserve_roomy(w.d_window_n, (size_t)n);
        if (!rc) rc = reserve_roomy(w.d_counts, (size_t)n);
        if (!rc) rc = reserve_roomy(w.d_scores, (size_t)n * GNN_CLASSES);
        if (rc) return rc;
    }
    if (need_r && w.strand_cap() < (size_t)n) {      // 24 B per window more, and only for a caller of the *_strand entry points
        GNN_HIP(hipStreamSynchronize(ctx->stream));
        reset_all(w.d_scores_rev, w.d_scores_mix);
        if (!rc) rc = reserve_roomy(w.d_scores_rev, (size_t)n * GNN_CLASSES);
        if (!rc) rc = reserve_roomy(w.d_scores_mix, (size_t)n * GNN_CLASSES);
        if (rc) return rc;
    }
    // a slab is what d_bases holds: 4 launches of windows, of one strand or - forward windows, then reverse windows - of both
    const int64_t slab = std::min<int64_t>(n, std::max<int64_t>(4 * std::max<int64_t>(ctx->chunk_fused, 1) / ns, 1));
    if ((rc = reserve_roomy(w.d_bases, (size_t)(slab * ns) * W))) return rc;
    if ((rc = reserve_roomy(w.d_out, (size_t)n_contigs * GNN_CLASSES))) return rc;
    if (ns == 2 && (rc = reserve_roomy(w.d_slab_scores, (size_t)(slab * 2) * GNN_CLASSES))) return rc;
    if (so && (so->contig_fwd || so->contig_rev) && (rc = reserve_roomy(w.d_out_strand, (size_t)n_contigs * 2 * GNN_CLASSES))) return rc;
    if (fold) {        // 16 B per contig and 16 B per bin (hipFree of a buffer that grows waits for the kernels that read it)
        if (w.off_cap() < (size_t)n_contigs + 1) {
            reset_all(w.d_win_off, w.d_bin_off);
            if (!rc) rc = reserve_roomy(w.d_win_off, (size_t)n_contigs + 1);
            if (!rc) rc = reserve_roomy(w.d_bin_off, (size_t)n_contigs + 1);
        }
        if (!rc && w.bin_cap() < (size_t)n_bins) {
            reset_all(w.d_track, w.d_cover);
            if (!rc) rc = reserve_roomy(w.d_track, (size_t)n_bins * GNN_CLASSES);
            if (!rc) rc = reserve_roomy(w.d_cover, (size_t)n_bins);
        }
        if (rc) return rc;
    }
    if (contig_emb_host) {
        // a slab's window embeddings (2 KB each) and the per-contig sums: never every window's row (10 M windows would be 20 GB)
        const bool rev_sum = strand != GNN_STRAND_FORWARD;
        if (w.d_emb.capacity() < (size_t)(slab * ns) * HID || w.d_emb_sum.capacity() < (size_t)n_contigs * HID ||
            w.d_emb_kept.capacity() < (size_t)n_contigs ||
            (rev_sum && (w.d_emb_sum_rev.capacity() < (size_t)n_contigs * HID || w.d_emb_kept_rev.capacity() < (size_t)n_contigs)))
            GNN_HIP(hipStreamSynchronize(ctx->stream));
        if ((rc = reserve_roomy(w.d_emb, (size_t)(slab * ns) * HID))) return rc;
        if (rev_sum) {       // the reverse strand folds into a sum of its own: two independent sums, whatever the slab size
            if ((rc = reserve_roomy(w.d_emb_sum_rev, (size_t)n_contigs * HID))) return rc;
            if ((rc = reserve_roomy(w.d_emb_kept_rev, (size_t)n_contigs))) return rc;
            GNN_HIP(hipMemsetAsync(w.d_emb_sum_rev, 0, (size_t)n_contigs * HID * sizeof(float), ctx->stream));
            GNN_HIP(hipMemsetAsync(w.d_emb_kept_rev, 0, (size_t)n_contigs * sizeof(int32_t), ctx->stream));
        }
        if ((rc = reserve_roomy(w.d_emb_sum, (size_t)n_contigs * HID))) return rc;
        if ((rc = reserve_roomy(w.d_emb_kept, (size_t)n_contigs))) return rc;
        GNN_HIP(hipMemsetAsync(w.d_emb_sum, 0, (size_t)n_contigs * HID * sizeof(float), ctx->stream));
        GNN_HIP(hipMemsetAsync(w.d_emb_kept, 0, (size_t)n_contigs * sizeof(int32_t), ctx->stream));
    }
    const uint8_t* seq_dev = seq;
    int64_t n_pieces = 0;
    if (seq_on_host) {
        if ((rc = reserve_roomy(w.seq, (size_t)seq_bytes))) return rc;
        seq_dev = w.seq;
        if (!w.copy_stream) GNN_HIP(hipStreamCreateWithFlags(&w.copy_stream, hipStreamNonBlocking));
        n_pieces = (seq_bytes + PIECE - 1) / PIECE;
        while ((int64_t)w.piece_done.size() < n_pieces) {
            hipEvent_t e = nullptr;
            GNN_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            w.piece_done.push_back(e);
        }
        // the previous call's kernels may still read w.seq: order the copies behind them
        hipEvent_t& first = w.piece_done[0];
        GNN_HIP(hipEventRecord(first, ctx->stream));
        GNN_HIP(hipStreamWaitEvent(w.copy_stream, first, 0));
    }
    GNN_HIP(hipMemcpyAsync(w.d_starts, w.starts.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    GNN_HIP(hipMemcpyAsync(w.d_lens, w.lens.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    GNN_HIP(hipMemcpyAsync(w.d_ids, w.ids.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    GNN_HIP(hipMemcpyAsync(w.d_window_n, w.window_n.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));

    // ---- slabs of windows: upload what they read (copy stream), count N, materialise, classify (ctx stream)
    int64_t uploaded = 0;       // pieces issued so far
    for (int64_t a = 0; a < n; a += slab) {
        const int64_t m = std::min(slab, n - a);
        if (seq_on_host) {
            const int64_t need = w.starts[a + m - 1] + w.lens[a + m - 1];       // spans are in buffer order
            const int64_t upto = std::min<int64_t>(n_pieces, (need + PIECE - 1) / PIECE);
            for (; uploaded < upto; ++uploaded) {
                const int64_t off = uploaded * PIECE, len = std::min(PIECE, seq_bytes - off);
                GNN_HIP(hipMemcpyAsync(w.seq + off, seq + off, (size_t)len, hipMemcpyHostToDevice, w.copy_stream));
                GNN_HIP(hipEventRecord(w.piece_done[uploaded], w.copy_stream));
            }
            if (upto > 0) GNN_HIP(hipStreamWaitEvent(ctx->stream, w.piece_done[upto - 1], 0));
        }
        if ((rc = launch_span_count(ctx, seq_dev, w.d_starts + a, w.d_lens + a, m, 'N', w.d_counts + a))) return rc;
        const int64_t r0 = need_f ? m : 0;      // the batch's first reverse window (the N count above served both strands)
        if (need_f && (rc = launch_materialize(ctx, seq_dev, w.d_starts + a, w.d_lens + a, m, w.d_bases))) return rc;
        if (need_r && (rc = launch_revcomp(ctx, seq_dev, w.d_starts + a, w.d_lens + a, m, w.d_bases + r0 * W))) return rc;
        float* const batch_scores = ns == 2 ? w.d_slab_scores.get() : (need_f ? w.d_scores : w.d_scores_rev) + a * GNN_CLASSES;
        if ((rc = classify_chunks(ctx, w.d_bases, m * ns, precision, batch_scores, false, contig_emb_host ? w.d_emb.get() : nullptr,
                                  GNN_EMB_F32)))
            return rc;
        if (ns == 2) {
            const int64_t cells = m * GNN_CLASSES;
            hipLaunchKernelGGL(strand_split_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, ctx->stream, w.d_slab_scores,
                               cells, w.d_scores + a * GNN_CLASSES, w.d_scores_rev + a * GNN_CLASSES, w.d_scores_mix + a * GNN_CLASSES);
            GNN_HIP(hipGetLastError());
        }
        if (contig_emb_host) {     // classify_chunks has ordered its back ends before ctx->stream: the slab's rows are complete
            const int64_t touched = w.ids[a + m - 1] - w.ids[a] + 1;
            if (strand != GNN_STRAND_REVERSE)
                hipLaunchKernelGGL(emb_fold_kernel, dim3((unsigned)touched), dim3(FOLD_THREADS), 0, ctx->stream, w.d_emb, w.d_ids,
                                   w.d_window_n, w.d_counts, a, m, w.d_emb_sum, w.d_emb_kept);
            if (strand != GNN_STRAND_FORWARD)
                hipLaunchKernelGGL(emb_fold_kernel, dim3((unsigned)touched), dim3(FOLD_THREADS), 0, ctx->stream, w.d_emb + r0 * HID, w.d_ids,
                                   w.d_window_n, w.d_counts, a, m, w.d_emb_sum_rev, w.d_emb_kept_rev);
            GNN_HIP(hipGetLastError());
        }
    }
    // the window scores of the mode: what the contig mean, the track and window_scores_host carry
    const float* const d_mode = strand == GNN_STRAND_BOTH ? w.d_scores_mix : (strand == GNN_STRAND_REVERSE ? w.d_scores_rev : w.d_scores);
    if (contig_emb_host) {
        const int64_t cells = n_contigs * HID;
        float* const d_mean = strand == GNN_STRAND_REVERSE ? w.d_emb_sum_rev : w.d_emb_sum;
        if (strand == GNN_STRAND_BOTH)
            hipLaunchKernelGGL(emb_both_mean_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, ctx->stream, w.d_emb_sum,
                               w.d_emb_sum_rev, w.d_emb_kept, n_contigs);
        else
            hipLaunchKernelGGL(emb_mean_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, ctx->stream, d_mean,
                               strand == GNN_STRAND_REVERSE ? w.d_emb_kept_rev : w.d_emb_kept, n_contigs);
        GNN_HIP(hipGetLastError());
        GNN_HIP(hipMemcpyAsync(contig_emb_host, d_mean, (size_t)cells * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    }
    const int64_t threads = n_contigs * GNN_CLASSES;
    hipLaunchKernelGGL(masked_segment_mean_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ctx->stream,
                       d_mode, w.d_ids, w.d_window_n, w.d_counts, n, n_contigs, w.d_out);
    GNN_HIP(hipGetLastError());
    if (so) {
        const struct { float* host; const float* d_win; float* d_mean; float* win_host; } each[2] = {
            {so->contig_fwd, w.d_scores, w.d_out_strand, so->window_fwd},
            {so->contig_rev, w.d_scores_rev, w.d_out_strand + threads, so->window_rev}};
        for (const auto& e : each) {
            if (e.host) {
                hipLaunchKernelGGL(masked_segment_mean_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ctx->stream,
                                   e.d_win, w.d_ids, w.d_window_n, w.d_counts, n, n_contigs, e.d_mean);
                GNN_HIP(hipGetLastError());
                GNN_HIP(hipMemcpyAsync(e.host, e.d_mean, (size_t)threads * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
            }
            if (e.win_host)
                GNN_HIP(hipMemcpyAsync(e.win_host, e.d_win, (size_t)n * GNN_CLASSES * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        }
    }
    w.counts.resize((size_t)n);
    if (contig_scores_host)
        GNN_HIP(hipMemcpyAsync(contig_scores_host, w.d_out, (size_t)threads * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    GNN_HIP(hipMemcpyAsync(w.counts.data(), w.d_counts, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (scan) {
        GNN_HIP(hipMemcpyAsync(scan->window_scores, d_mode, (size_t)n * GNN_CLASSES * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        if (fold) {
            const size_t off_bytes = (size_t)(n_contigs + 1) * sizeof(int64_t);
            GNN_HIP(hipMemcpyAsync(w.d_win_off, w.win_off.data(), off_bytes, hipMemcpyHostToDevice, ctx->stream));
            GNN_HIP(hipMemcpyAsync(w.d_bin_off, w.bin_off.data(), off_bytes, hipMemcpyHostToDevice, ctx->stream));
            const int64_t cells = n_bins * GNN_CLASSES;
            hipLaunchKernelGGL(scan_track_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, ctx->stream, d_mode, w.d_lens,
                               w.d_counts, w.d_win_off, w.d_bin_off, n_contigs, n_bins, (int)stride, w.d_track, w.d_cover);
            GNN_HIP(hipGetLastError());
            if (scan->track)
                GNN_HIP(hipMemcpyAsync(scan->track, w.d_track, (size_t)cells * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
            if (scan->cover)
                GNN_HIP(hipMemcpyAsync(scan->cover, w.d_cover, (size_t)n_bins * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        }
    }
    GNN_HIP(hipStreamSynchronize(ctx->stream));
    int64_t kept = 0;
    for (int64_t i = 0; i < n; ++i) {
        const bool keep = w.window_n[i] == 0 || w.counts[i] <= MAX_N;
        if (scan) {
            if (scan->window_kept) scan->window_kept[i] = keep ? 1 : 0;
            kept += keep;
        } else if (keep) {
            window_ids_host[kept++] = w.ids[i];
        }
    }
    *n_windows_out = kept;
    return GNN_OK;
}

extern "C" int gnn_classify_contigs(gnn_ctx* ctx, const uint8_t* seq, int seq_on_host, int64_t seq_bytes,
                                    const int64_t* offsets_host, int64_t n_contigs, int single_window, int precision,
                                    float* contig_scores_host, int64_t* window_ids_host, int64_t ids_capacity,
                                    int64_t* n_windows_out) {
    return classify_contigs(ctx, seq, seq_on_host, seq_bytes, offsets_host, n_contigs, single_window, precision, contig_scores_host,
                            window_ids_host, ids_capacity, n_windows_out, nullptr);
}

extern "C" int gnn_classify_contigs_embed(gnn_ctx* ctx, const uint8_t* seq, int seq_on_host, int64_t seq_bytes,
                                          const int64_t* offsets_host, int64_t n_contigs, int single_window, int precision,
                                          float* contig_scores_host, int64_t* window_ids_host, int64_t ids_capacity,
                                          int64_t* n_windows_out, float* contig_emb_host) {
    if (n_contigs > 0 && !contig_emb_host) {
        set_error("bad argument to gnn_classify_contigs_embed: contig_emb_host is NULL");
        return GNN_ERR_ARG;
    }
    if (precision == GNN_PREC_F16C6) {
        set_error("gnn_classify_contigs_embed: GNN_PREC_F16C6 has no embedding path (the frozen mode's dense head runs on the matrix "
                  "pipe and is outside the tolerance); use f16x3tc, f16x3tk, f16x3, bf16x3 or f32");
        return GNN_ERR_ARG;
    }
    return classify_contigs(ctx, seq, seq_on_host, seq_bytes, offsets_host, n_contigs, single_window, precision, contig_scores_host,
                            window_ids_host, ids_capacity, n_windows_out, n_contigs > 0 ? contig_emb_host : nullptr);
}

static int check_stride(int stride, const char* fn) {
    if (stride >= 1 && stride <= W) return GNN_OK;
    set_error(std::string(fn) + ": stride " + std::to_string(stride) + " is outside [1, " + std::to_string(W) + "]");
    return GNN_ERR_ARG;
}

extern "C" int gnn_scan_plan(const int64_t* offsets_host, int64_t n_contigs, int stride, int single_window, int64_t* n_windows_out,
                             int64_t* n_bins_out, int64_t* win_offsets_or_null, int64_t* bin_offsets_or_null, int64_t* starts_or_null,
                             int32_t* lens_or_null) {
    if (!offsets_host || n_contigs < 0 || !n_windows_out || !n_bins_out) {
        set_error("bad argument to gnn_scan_plan");
        return GNN_ERR_ARG;
    }
    if (int rc = check_stride(stride, "gnn_scan_plan")) return rc;
    for (int64_t c = 0; c < n_contigs; ++c)
        if (offsets_host[c + 1] < offsets_host[c]) {
            set_error("contig offsets are not non-decreasing");
            return GNN_ERR_ARG;
        }
    int64_t n = 0, bins = 0;
    if (win_offsets_or_null) win_offsets_or_null[0] = 0;
    if (bin_offsets_or_null) bin_offsets_or_null[0] = 0;
    for (int64_t c = 0; c < n_contigs; ++c) {
        const int64_t len = offsets_host[c + 1] - offsets_host[c];
        for_each_window(len, stride, single_window, [&](int64_t k, int64_t l) {
            if (starts_or_null) starts_or_null[n] = k * stride;
            if (lens_or_null) lens_or_null[n] = (int32_t)l;
            ++n;
        });
        bins += (len + stride - 1) / stride;
        if (win_offsets_or_null) win_offsets_or_null[c + 1] = n;
        if (bin_offsets_or_null) bin_offsets_or_null[c + 1] = bins;
    }
    *n_windows_out = n;
    *n_bins_out = bins;
    return GNN_OK;
}

extern "C" int gnn_scan_contigs(gnn_ctx* ctx, const uint8_t* seq, int seq_on_host, int64_t seq_bytes, const int64_t* offsets_host,
                                int64_t n_contigs, int stride, int single_window, int precision, float* window_scores_host,
                                uint8_t* window_kept_host_or_null, int64_t windows_capacity, float* track_host_or_null,
                                int32_t* cover_host_or_null, int64_t bins_capacity, float* contig_scores_host_or_null) {
    if (int rc = check_stride(stride, "gnn_scan_contigs")) return rc;
    const ScanOut scan{window_scores_host, window_kept_host_or_null, windows_capacity, track_host_or_null, cover_host_or_null,
                       bins_capacity};
    int64_t kept = 0;
    return classify_contigs(ctx, seq, seq_on_host, seq_bytes, offsets_host, n_contigs, single_window, precision,
                            contig_scores_host_or_null, nullptr, 0, &kept, nullptr, stride, &scan);
}

static int check_strand(int strand, const char* fn) {
    if (strand == GNN_STRAND_FORWARD || strand == GNN_STRAND_REVERSE || strand == GNN_STRAND_BOTH) return GNN_OK;
    set_error(std::string(fn) + ": strand " + std::to_string(strand) + " is not a gnn_strand (0 forward, 1 reverse, 2 both)");
    return GNN_ERR_ARG;
}

extern "C" int gnn_classify_contigs_strand(gnn_ctx* ctx, const uint8_t* seq, int seq_on_host, int64_t seq_bytes,
                                           const int64_t* offsets_host, int64_t n_contigs, int single_window, int precision,
                                           float* contig_scores_host, int64_t* window_ids_host, int64_t ids_capacity,
                                           int64_t* n_windows_out, float* contig_emb_host_or_null, int strand,
                                           float* contig_scores_fwd_host_or_null, float* contig_scores_rev_host_or_null) {
    if (int rc = check_strand(strand, "gnn_classify_contigs_strand")) return rc;
    if (contig_emb_host_or_null && precision == GNN_PREC_F16C6) {
        set_error("gnn_classify_contigs_strand: GNN_PREC_F16C6 has no embedding path (the frozen mode's dense head runs on the matrix "
                  "pipe and is outside the tolerance); use f16x3tc, f16x3tk, f16x3, bf16x3 or f32");
        return GNN_ERR_ARG;
    }
    const StrandOut so{strand, contig_scores_fwd_host_or_null, contig_scores_rev_host_or_null, nullptr, nullptr};
    return classify_contigs(ctx, seq, seq_on_host, seq_bytes, offsets_host, n_contigs, single_window, precision, contig_scores_host,
                            window_ids_host, ids_capacity, n_windows_out, n_contigs > 0 ? contig_emb_host_or_null : nullptr, W, nullptr,
                            &so);
}

extern "C" int gnn_scan_contigs_strand(gnn_ctx* ctx, const uint8_t* seq, int seq_on_host, int64_t seq_bytes, const int64_t* offsets_host,
                                       int64_t n_contigs, int stride, int single_window, int precision, float* window_scores_host,
                                       uint8_t* window_kept_host_or_null, int64_t windows_capacity, float* track_host_or_null,
                                       int32_t* cover_host_or_null, int64_t bins_capacity, float* contig_scores_host_or_null, int strand,
                                       float* window_scores_fwd_host_or_null, float* window_scores_rev_host_or_null) {
    if (int rc = check_stride(stride, "gnn_scan_contigs_strand")) return rc;
    if (int rc = check_strand(strand, "gnn_scan_contigs_strand")) return rc;
    const ScanOut scan{window_scores_host, window_kept_host_or_null, windows_capacity, track_host_or_null, cover_host_or_null,
                       bins_capacity};
    const StrandOut so{strand, nullptr, nullptr, window_scores_fwd_host_or_null, window_scores_rev_host_or_null};
    int64_t kept = 0;
    return classify_contigs(ctx, seq, seq_on_host, seq_bytes, offsets_host, n_contigs, single_window, precision,
                            contig_scores_host_or_null, nullptr, 0, &kept, nullptr, stride, &scan, &so);
}
