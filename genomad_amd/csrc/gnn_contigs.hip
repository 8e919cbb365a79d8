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
    int strand = GNN_STRAND_FORWARD;
    float* contig_fwd = nullptr;          // [n_contigs][3]: each strand's own masked mean
    float* contig_rev = nullptr;
    float* window_fwd = nullptr;          // scans only: [n_windows][3]
    float* window_rev = nullptr;
};

// What a contig call hands back per contig (any may be NULL where the entry point allows it): the mode's scores, the contig ids
// of the kept windows with their count (gnn_classify_contigs*; a scan reports kept per window instead) and the embeddings.
struct ContigOut {
    float* scores = nullptr;            // [n_contigs][3]
    int64_t* window_ids = nullptr;
    int64_t ids_capacity = 0;
    int64_t* n_windows = nullptr;
    float* emb = nullptr;               // [n_contigs][HID]
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
        if (window_kept(window_n[k], counts[k])) {
            s += scores[k * GNN_CLASSES + cl];
            ++kept;
        }
    out[i] = kept ? s / (float)kept : 0.f;
}

int launch_masked_segment_mean(gnn_ctx* ctx, const float* scores, const int64_t* ids, const int32_t* window_n, const int32_t* counts,
                               int64_t n, int64_t n_seg, float* out) {
    return launch_1d(masked_segment_mean_kernel, n_seg * GNN_CLASSES, ctx->stream, scores, ids, window_n, counts, n, n_seg, out);
}

// Per-contig embedding fold of one slab [a, a + m) of the window table: one block per contig the slab touches (ids are sorted, so
// contigs ids[a] .. ids[a+m-1]), 128 lanes x 4 columns = one 2 KB row per step, read as float4s (coalesced: a row is contiguous).
// The contig's kept windows of this slab are added to its running sum in window order, starting from what the slabs before left
// there, so the sum is ((0 + e_0) + e_1) + ... whatever the slab and launch sizes.  FOLD_THREADS: gnn_common.h.
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
        if (window_kept(window_n[i], counts[i])) {
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
// order is part of the contract: no atomics), divided once.  Kept = window_kept.  A bin without a kept
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
        if (b * stride < k * stride + lens[j] && window_kept((int32_t)k, counts[j])) {      // k, the index within the contig, IS window_n[j]
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

// ---- the steps every contig call is made of (declared in gnn_common.h) ----

int contig_begin(const ContigIn& in, const char* fn, bool outputs_ok, ContigWorkspace** w) {
    if (int rc = check_ctx(in.ctx)) return rc;
    if (in.n_contigs < 0 || in.seq_bytes < 0 || !in.offsets || !outputs_ok || (in.seq_bytes > 0 && !in.seq)) {
        set_error(std::string("bad argument to ") + fn);
        return GNN_ERR_ARG;
    }
    if (in.offsets[0] < 0 || in.offsets[in.n_contigs] > in.seq_bytes) {
        set_error("contig offsets outside the sequence buffer");
        return GNN_ERR_ARG;
    }
    if (!in.ctx->contig_ws) in.ctx->contig_ws = new ContigWorkspace();
    *w = in.ctx->contig_ws;
    return GNN_OK;
}

// candidate windows: seq_windows(seq, 6000, 2500, max_windows) for every contig (sequence.py:150-167), at in.stride
int plan_windows(const ContigIn& in, ContigWorkspace& w, bool csr, int block) {
    w.starts.clear(), w.lens.clear(), w.ids.clear(), w.window_n.clear();
    w.blk_off.assign(1, 0);
    WindowWalk walk;
    if (csr) {
        w.win_off.resize((size_t)in.n_contigs + 1), w.bin_off.resize((size_t)in.n_contigs + 1);
        walk.win_off = w.win_off.data(), walk.bin_off = w.bin_off.data();
    }
    return walk_windows(in.offsets, in.n_contigs, in.stride, in.single_window, walk, [&](int64_t c, int64_t k, int64_t l) {
        w.starts.push_back(in.offsets[c] + k * in.stride);
        w.lens.push_back((int32_t)l);
        w.ids.push_back(c);
        w.window_n.push_back((int32_t)k);
        if (block) w.blk_off.push_back(w.blk_off.back() + (l + block - 1) / block);
    });
}

int upload_span_table(gnn_ctx* ctx, ContigWorkspace& w) {
    const size_t n = w.starts.size();
    if (w.span_cap() < n) {
        GNN_HIP(hipStreamSynchronize(ctx->stream));      // a buffer that grows is freed first: nothing may still read it
        reset_all(w.d_starts, w.d_ids, w.d_lens, w.d_window_n, w.d_counts, w.d_scores);      // empty, not half-grown, on failure
        int rc = reserve_roomy(w.d_starts, n);
        if (!rc) rc = reserve_roomy(w.d_ids, n);
        if (!rc) rc = reserve_roomy(w.d_lens, n);
        if (!rc) rc = reserve_roomy(w.d_window_n, n);
        if (!rc) rc = reserve_roomy(w.d_counts, n);
        if (!rc) rc = reserve_roomy(w.d_scores, n * GNN_CLASSES);
        if (rc) return rc;
    }
    GNN_HIP(hipMemcpyAsync(w.d_starts, w.starts.data(), n * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    GNN_HIP(hipMemcpyAsync(w.d_lens, w.lens.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    GNN_HIP(hipMemcpyAsync(w.d_ids, w.ids.data(), n * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    GNN_HIP(hipMemcpyAsync(w.d_window_n, w.window_n.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    return GNN_OK;
}

int SeqFeed::begin(const ContigIn& in, ContigWorkspace& w) {
    ctx_ = in.ctx, w_ = &w, dev_ = in.seq;
    if (!in.seq_on_host) return GNN_OK;
    if (w.seq.capacity() < (size_t)in.seq_bytes) {      // freed before it grows: neither stream may still touch it
        GNN_HIP(hipStreamSynchronize(ctx_->stream));
        if (w.copy_stream) GNN_HIP(hipStreamSynchronize(w.copy_stream));
    }
    if (int rc = reserve_roomy(w.seq, (size_t)in.seq_bytes)) return rc;
    host_ = in.seq, dev_ = w.seq, bytes_ = in.seq_bytes;
    if (!w.copy_stream) GNN_HIP(hipStreamCreateWithFlags(&w.copy_stream, hipStreamNonBlocking));
    n_pieces_ = (bytes_ + PIECE - 1) / PIECE;
    while ((int64_t)w.piece_done.size() < n_pieces_) {
        hipEvent_t e = nullptr;
        GNN_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        w.piece_done.push_back(e);
    }
    // the previous call's kernels may still read w.seq: order the copies behind them
    hipEvent_t& first = w.piece_done[0];
    GNN_HIP(hipEventRecord(first, ctx_->stream));
    GNN_HIP(hipStreamWaitEvent(w.copy_stream, first, 0));
    return GNN_OK;
}

int SeqFeed::upto(int64_t end) {
    if (!host_) return GNN_OK;
    const int64_t upto = std::min<int64_t>(n_pieces_, (end + PIECE - 1) / PIECE);
    for (; uploaded_ < upto; ++uploaded_) {
        const int64_t off = uploaded_ * PIECE, len = std::min(PIECE, bytes_ - off);
        GNN_HIP(hipMemcpyAsync(w_->seq + off, host_ + off, (size_t)len, hipMemcpyHostToDevice, w_->copy_stream));
        GNN_HIP(hipEventRecord(w_->piece_done[uploaded_], w_->copy_stream));
    }
    if (upto > 0) GNN_HIP(hipStreamWaitEvent(ctx_->stream, w_->piece_done[upto - 1], 0));
    return GNN_OK;
}

int slab_pass(const ContigIn& in, ContigWorkspace& w, SeqFeed& feed, int64_t a, int64_t m, bool fwd, bool rev, float* scores,
              float* emb, const AttribOut* attr) {
    int rc = feed.upto(w.starts[a + m - 1] + w.lens[a + m - 1]);       // spans are in buffer order: the slab's last byte
    if (rc) return rc;
    const int64_t* const starts = w.d_starts + a;
    const int32_t* const lens = w.d_lens + a;
    if ((rc = launch_span_count(in.ctx, feed.dev(), starts, lens, m, 'N', w.d_counts + a))) return rc;      // serves both strands
    if (fwd && (rc = launch_materialize(in.ctx, feed.dev(), starts, lens, m, w.d_bases))) return rc;
    if (rev && (rc = launch_revcomp(in.ctx, feed.dev(), starts, lens, m, w.d_bases + (fwd ? m : 0) * W))) return rc;
    return classify_chunks(in.ctx, w.d_bases, m * (fwd + rev), in.precision, scores, false, emb, GNN_EMB_F32, attr);
}

int64_t kept_windows(const ContigWorkspace& w, uint8_t* mask_or_null, int64_t* ids_or_null) {
    int64_t kept = 0;
    for (size_t i = 0; i < w.starts.size(); ++i) {
        const bool keep = window_kept(w.window_n[i], w.counts[i]);
        if (mask_or_null) mask_or_null[i] = keep ? 1 : 0;
        if (keep && ids_or_null) ids_or_null[kept] = w.ids[i];
        kept += keep;
    }
    return kept;
}

}  // namespace gnn

using namespace gnn;

// ---- gnn_classify_contigs, gnn_scan_contigs and their *_embed / *_strand forms: one call, in five steps ----

// What the steps of one call share: the table's size, which strands run, the slab, what is folded.
struct ContigCall {
    const ContigIn& in;
    ContigWorkspace& w;
    const StrandOut& so;
    const ScanOut* scan;
    float* contig_scores_host;
    float* emb_host;            // NULL: no embeddings
    int64_t n, n_bins;          // candidate windows, bins (scans)
    bool need_f, need_r;        // which strands run: what the mode averages, and what the caller asked to see on its own
    int64_t ns, slab;           // strands that run; windows per slab
    bool fold;                  // a scan with a track
    // the window scores of the mode: what the contig mean, the track and window_scores_host carry
    const float* d_mode() const {
        return so.strand == GNN_STRAND_BOTH ? w.d_scores_mix : (so.strand == GNN_STRAND_REVERSE ? w.d_scores_rev : w.d_scores);
    }
};

// ---- reserve: everything but the span table and the sequence
static int reserve_buffers(const ContigCall& c) {
    gnn_ctx* const ctx = c.in.ctx;
    ContigWorkspace& w = c.w;
    const size_t n = (size_t)c.n, n_contigs = (size_t)c.in.n_contigs, batch = (size_t)(c.slab * c.ns);
    int rc = GNN_OK;
    if (c.need_r && w.strand_cap() < n) {      // 24 B per window more, and only for a caller of the *_strand entry points
        GNN_HIP(hipStreamSynchronize(ctx->stream));
        reset_all(w.d_scores_rev, w.d_scores_mix);
        if (!rc) rc = reserve_roomy(w.d_scores_rev, n * GNN_CLASSES);
        if (!rc) rc = reserve_roomy(w.d_scores_mix, n * GNN_CLASSES);
        if (rc) return rc;
    }
    if ((rc = reserve_roomy(w.d_bases, batch * W))) return rc;
    if ((rc = reserve_roomy(w.d_out, n_contigs * GNN_CLASSES))) return rc;
    if (c.ns == 2 && (rc = reserve_roomy(w.d_slab_scores, batch * GNN_CLASSES))) return rc;
    if ((c.so.contig_fwd || c.so.contig_rev) && (rc = reserve_roomy(w.d_out_strand, n_contigs * 2 * GNN_CLASSES))) return rc;
    if (c.fold) {        // 16 B per contig and 16 B per bin (hipFree of a buffer that grows waits for the kernels that read it)
        if (w.off_cap() < n_contigs + 1) {
            reset_all(w.d_win_off, w.d_bin_off);
            if (!rc) rc = reserve_roomy(w.d_win_off, n_contigs + 1);
            if (!rc) rc = reserve_roomy(w.d_bin_off, n_contigs + 1);
        }
        if (!rc && w.bin_cap() < (size_t)c.n_bins) {
            reset_all(w.d_track, w.d_cover);
            if (!rc) rc = reserve_roomy(w.d_track, (size_t)c.n_bins * GNN_CLASSES);
            if (!rc) rc = reserve_roomy(w.d_cover, (size_t)c.n_bins);
        }
        if (rc) return rc;
    }
    if (!c.emb_host) return GNN_OK;
    // a slab's window embeddings (2 KB each) and the per-contig sums: never every window's row (10 M windows would be 20 GB)
    const bool rev_sum = c.so.strand != GNN_STRAND_FORWARD;
    if (w.d_emb.capacity() < batch * HID || w.d_emb_sum.capacity() < n_contigs * HID || w.d_emb_kept.capacity() < n_contigs ||
        (rev_sum && (w.d_emb_sum_rev.capacity() < n_contigs * HID || w.d_emb_kept_rev.capacity() < n_contigs)))
        GNN_HIP(hipStreamSynchronize(ctx->stream));
    if ((rc = reserve_roomy(w.d_emb, batch * HID))) return rc;
    if (rev_sum) {       // the reverse strand folds into a sum of its own: two independent sums, whatever the slab size
        if ((rc = reserve_roomy(w.d_emb_sum_rev, n_contigs * HID))) return rc;
        if ((rc = reserve_roomy(w.d_emb_kept_rev, n_contigs))) return rc;
        GNN_HIP(hipMemsetAsync(w.d_emb_sum_rev, 0, n_contigs * HID * sizeof(float), ctx->stream));
        GNN_HIP(hipMemsetAsync(w.d_emb_kept_rev, 0, n_contigs * sizeof(int32_t), ctx->stream));
    }
    if ((rc = reserve_roomy(w.d_emb_sum, n_contigs * HID))) return rc;
    if ((rc = reserve_roomy(w.d_emb_kept, n_contigs))) return rc;
    GNN_HIP(hipMemsetAsync(w.d_emb_sum, 0, n_contigs * HID * sizeof(float), ctx->stream));
    GNN_HIP(hipMemsetAsync(w.d_emb_kept, 0, n_contigs * sizeof(int32_t), ctx->stream));
    return GNN_OK;
}

// ---- pass: slabs of windows through the front end; both strands' scores are split, the embeddings folded, slab by slab
static int run_slabs(const ContigCall& c, SeqFeed& feed) {
    hipStream_t const stream = c.in.ctx->stream;
    ContigWorkspace& w = c.w;
    const int strand = c.so.strand;
    int rc = GNN_OK;
    for (int64_t a = 0; a < c.n; a += c.slab) {
        const int64_t m = std::min(c.slab, c.n - a), row = a * GNN_CLASSES;
        float* const batch_scores = c.ns == 2 ? w.d_slab_scores.get() : (c.need_f ? w.d_scores : w.d_scores_rev) + row;
        if ((rc = slab_pass(c.in, w, feed, a, m, c.need_f, c.need_r, batch_scores, c.emb_host ? w.d_emb.get() : nullptr))) return rc;
        if (c.ns == 2 && (rc = launch_1d(strand_split_kernel, m * GNN_CLASSES, stream, w.d_slab_scores, m * GNN_CLASSES, w.d_scores + row,
                                         w.d_scores_rev + row, w.d_scores_mix + row)))
            return rc;
        if (c.emb_host) {     // classify_chunks has ordered its back ends before ctx->stream: the slab's rows are complete
            const int64_t touched = w.ids[a + m - 1] - w.ids[a] + 1;
            const int64_t r0 = c.need_f ? m : 0;      // the batch's first reverse window
            if (strand != GNN_STRAND_REVERSE)
                hipLaunchKernelGGL(emb_fold_kernel, dim3((unsigned)touched), dim3(FOLD_THREADS), 0, stream, w.d_emb, w.d_ids,
                                   w.d_window_n, w.d_counts, a, m, w.d_emb_sum, w.d_emb_kept);
            if (strand != GNN_STRAND_FORWARD)
                hipLaunchKernelGGL(emb_fold_kernel, dim3((unsigned)touched), dim3(FOLD_THREADS), 0, stream, w.d_emb + r0 * HID, w.d_ids,
                                   w.d_window_n, w.d_counts, a, m, w.d_emb_sum_rev, w.d_emb_kept_rev);
            GNN_HIP(hipGetLastError());
        }
    }
    return GNN_OK;
}

// ---- folds and copies back: embedding means, the masked means per contig, the track; everything the host asked for
static int fold_and_copy_back(const ContigCall& c) {
    hipStream_t const stream = c.in.ctx->stream;
    ContigWorkspace& w = c.w;
    const int strand = c.so.strand;
    const int64_t n = c.n, n_contigs = c.in.n_contigs, threads = n_contigs * GNN_CLASSES;
    const size_t window_bytes = (size_t)n * GNN_CLASSES * sizeof(float), contig_bytes = (size_t)threads * sizeof(float);
    int rc = GNN_OK;
    if (c.emb_host) {
        const int64_t cells = n_contigs * HID;
        float* const d_mean = strand == GNN_STRAND_REVERSE ? w.d_emb_sum_rev : w.d_emb_sum;
        rc = strand == GNN_STRAND_BOTH
                 ? launch_1d(emb_both_mean_kernel, cells, stream, w.d_emb_sum, w.d_emb_sum_rev, w.d_emb_kept, n_contigs)
                 : launch_1d(emb_mean_kernel, cells, stream, d_mean, strand == GNN_STRAND_REVERSE ? w.d_emb_kept_rev : w.d_emb_kept,
                             n_contigs);
        if (rc) return rc;
        GNN_HIP(hipMemcpyAsync(c.emb_host, d_mean, (size_t)cells * sizeof(float), hipMemcpyDeviceToHost, stream));
    }
    if ((rc = launch_masked_segment_mean(c.in.ctx, c.d_mode(), w.d_ids, w.d_window_n, w.d_counts, n, n_contigs, w.d_out))) return rc;
    const struct { float* host; const float* d_win; float* d_mean; float* win_host; } each[2] = {
        {c.so.contig_fwd, w.d_scores, w.d_out_strand, c.so.window_fwd},
        {c.so.contig_rev, w.d_scores_rev, w.d_out_strand + threads, c.so.window_rev}};
    for (const auto& e : each) {
        if (e.host) {
            if ((rc = launch_masked_segment_mean(c.in.ctx, e.d_win, w.d_ids, w.d_window_n, w.d_counts, n, n_contigs, e.d_mean))) return rc;
            GNN_HIP(hipMemcpyAsync(e.host, e.d_mean, contig_bytes, hipMemcpyDeviceToHost, stream));
        }
        if (e.win_host) GNN_HIP(hipMemcpyAsync(e.win_host, e.d_win, window_bytes, hipMemcpyDeviceToHost, stream));
    }
    w.counts.resize((size_t)n);
    if (c.contig_scores_host) GNN_HIP(hipMemcpyAsync(c.contig_scores_host, w.d_out, contig_bytes, hipMemcpyDeviceToHost, stream));
    GNN_HIP(hipMemcpyAsync(w.counts.data(), w.d_counts, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    if (!c.scan) return GNN_OK;
    GNN_HIP(hipMemcpyAsync(c.scan->window_scores, c.d_mode(), window_bytes, hipMemcpyDeviceToHost, stream));
    if (!c.fold) return GNN_OK;
    const size_t off_bytes = (size_t)(n_contigs + 1) * sizeof(int64_t);
    GNN_HIP(hipMemcpyAsync(w.d_win_off, w.win_off.data(), off_bytes, hipMemcpyHostToDevice, stream));
    GNN_HIP(hipMemcpyAsync(w.d_bin_off, w.bin_off.data(), off_bytes, hipMemcpyHostToDevice, stream));
    const int64_t cells = c.n_bins * GNN_CLASSES;
    if ((rc = launch_1d(scan_track_kernel, cells, stream, c.d_mode(), w.d_lens, w.d_counts, w.d_win_off, w.d_bin_off, n_contigs, c.n_bins,
                        (int)c.in.stride, w.d_track, w.d_cover)))
        return rc;
    if (c.scan->track) GNN_HIP(hipMemcpyAsync(c.scan->track, w.d_track, (size_t)cells * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (c.scan->cover)
        GNN_HIP(hipMemcpyAsync(c.scan->cover, w.d_cover, (size_t)c.n_bins * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    return GNN_OK;
}

static int classify_contigs(const ContigIn& in, const ContigOut& out, const StrandOut& so = {}, const ScanOut* scan = nullptr) {
    const char* const fn = scan ? "gnn_scan_contigs" : "gnn_classify_contigs";
    ContigWorkspace* wp = nullptr;
    int rc = contig_begin(in, fn, scan || (out.n_windows && (in.n_contigs == 0 || out.scores)), &wp);
    if (rc) return rc;
    // ---- plan: the window table, the outputs zeroed, the caller's capacities
    if ((rc = plan_windows(in, *wp, scan != nullptr, 0))) return rc;
    const bool need_f = so.strand != GNN_STRAND_REVERSE || so.contig_fwd || so.window_fwd;
    const bool need_r = so.strand != GNN_STRAND_FORWARD || so.contig_rev || so.window_rev;
    const int64_t n = (int64_t)wp->starts.size(), ns = (need_f ? 1 : 0) + (need_r ? 1 : 0);
    // a slab is what d_bases holds: 4 launches of windows, of one strand or - forward windows, then reverse windows - of both
    const int64_t slab = std::min<int64_t>(n, std::max<int64_t>(4 * std::max<int64_t>(in.ctx->chunk_fused, 1) / ns, 1));
    const ContigCall c{in, *wp, so, scan, out.scores, in.n_contigs > 0 ? out.emb : nullptr, n, scan ? wp->bin_off.back() : 0,
                       need_f, need_r, ns, slab, scan && (scan->track || scan->cover)};
    if (out.n_windows) *out.n_windows = 0;
    for (float* p : {out.scores, so.contig_fwd, so.contig_rev})
        if (in.n_contigs && p) std::memset(p, 0, (size_t)in.n_contigs * GNN_CLASSES * sizeof(float));
    if (c.emb_host) std::memset(c.emb_host, 0, (size_t)in.n_contigs * HID * sizeof(float));
    if (n == 0) return GNN_OK;
    if (scan) {
        if (!scan->window_scores || scan->windows_capacity < n) {
            set_error("window_scores_host holds " + std::to_string(scan->windows_capacity) + " windows, the scan has " + std::to_string(n));
            return GNN_ERR_ARG;
        }
        if (c.fold && scan->bins_capacity < c.n_bins) {
            set_error("track_host / cover_host hold " + std::to_string(scan->bins_capacity) + " bins, the scan has " + std::to_string(c.n_bins));
            return GNN_ERR_ARG;
        }
    } else if (!out.window_ids || out.ids_capacity < n) {
        set_error("window_ids_host holds " + std::to_string(out.ids_capacity) + " entries, " + std::to_string(n) + " candidate windows");
        return GNN_ERR_ARG;
    }
    // ---- reserve, pass, folds, copies back
    SeqFeed feed;
    if ((rc = upload_span_table(in.ctx, c.w))) return rc;
    if ((rc = reserve_buffers(c))) return rc;
    if ((rc = feed.begin(in, c.w))) return rc;
    if ((rc = run_slabs(c, feed))) return rc;
    if ((rc = fold_and_copy_back(c))) return rc;
    GNN_HIP(hipStreamSynchronize(in.ctx->stream));
    const int64_t kept = kept_windows(c.w, scan ? scan->window_kept : nullptr, scan ? nullptr : out.window_ids);
    if (out.n_windows) *out.n_windows = kept;
    return GNN_OK;
}

extern "C" int gnn_classify_contigs(gnn_ctx* ctx, const uint8_t* seq, int seq_on_host, int64_t seq_bytes,
                                    const int64_t* offsets_host, int64_t n_contigs, int single_window, int precision,
                                    float* contig_scores_host, int64_t* window_ids_host, int64_t ids_capacity,
                                    int64_t* n_windows_out) {
    return classify_contigs({ctx, seq, seq_on_host, seq_bytes, offsets_host, n_contigs, single_window, precision, W},
                            {contig_scores_host, window_ids_host, ids_capacity, n_windows_out});
}

extern "C" int gnn_classify_contigs_embed(gnn_ctx* ctx, const uint8_t* seq, int seq_on_host, int64_t seq_bytes,
                                          const int64_t* offsets_host, int64_t n_contigs, int single_window, int precision,
                                          float* contig_scores_host, int64_t* window_ids_host, int64_t ids_capacity,
                                          int64_t* n_windows_out, float* contig_emb_host) {
    if (n_contigs > 0 && !contig_emb_host) {
        set_error("bad argument to gnn_classify_contigs_embed: contig_emb_host is NULL");
        return GNN_ERR_ARG;
    }
    if (int rc = check_embed_precision(precision, "gnn_classify_contigs_embed")) return rc;
    return classify_contigs({ctx, seq, seq_on_host, seq_bytes, offsets_host, n_contigs, single_window, precision, W},
                            {contig_scores_host, window_ids_host, ids_capacity, n_windows_out, contig_emb_host});
}

int gnn::check_stride(int stride, const char* fn) {
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
    WindowWalk walk{win_offsets_or_null, bin_offsets_or_null};
    const int rc = walk_windows(offsets_host, n_contigs, stride, single_window, walk, [&](int64_t, int64_t k, int64_t l) {
        if (starts_or_null) starts_or_null[walk.windows] = k * stride;
        if (lens_or_null) lens_or_null[walk.windows] = (int32_t)l;
    });
    if (rc) return rc;
    *n_windows_out = walk.windows;
    *n_bins_out = walk.bins;
    return GNN_OK;
}

extern "C" int gnn_scan_contigs(gnn_ctx* ctx, const uint8_t* seq, int seq_on_host, int64_t seq_bytes, const int64_t* offsets_host,
                                int64_t n_contigs, int stride, int single_window, int precision, float* window_scores_host,
                                uint8_t* window_kept_host_or_null, int64_t windows_capacity, float* track_host_or_null,
                                int32_t* cover_host_or_null, int64_t bins_capacity, float* contig_scores_host_or_null) {
    if (int rc = check_stride(stride, "gnn_scan_contigs")) return rc;
    const ScanOut scan{window_scores_host, window_kept_host_or_null, windows_capacity, track_host_or_null, cover_host_or_null,
                       bins_capacity};
    return classify_contigs({ctx, seq, seq_on_host, seq_bytes, offsets_host, n_contigs, single_window, precision, stride},
                            {contig_scores_host_or_null}, StrandOut{GNN_STRAND_FORWARD}, &scan);
}

int gnn::check_strand(int strand, const char* fn) {
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
    if (contig_emb_host_or_null)
        if (int rc = check_embed_precision(precision, "gnn_classify_contigs_strand")) return rc;
    return classify_contigs({ctx, seq, seq_on_host, seq_bytes, offsets_host, n_contigs, single_window, precision, W},
                            {contig_scores_host, window_ids_host, ids_capacity, n_windows_out, contig_emb_host_or_null},
                            StrandOut{strand, contig_scores_fwd_host_or_null, contig_scores_rev_host_or_null});
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
    StrandOut so{strand};
    so.window_fwd = window_scores_fwd_host_or_null, so.window_rev = window_scores_rev_host_or_null;
    return classify_contigs({ctx, seq, seq_on_host, seq_bytes, offsets_host, n_contigs, single_window, precision, stride},
                            {contig_scores_host_or_null}, so, &scan);
}
