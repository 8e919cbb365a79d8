// Occlusion maps ("Occlusion maps"): which bases a window's score rests on, answered with the forward pass alone.  Every
// window of gnn_classify_contigs' table is scored once as it is (base) and once per block of `block` bases with that block set to
// 'N' (occ); delta = base - occ, one f32 subtraction per (pair, class).
//
//   block     B, 1 <= B <= 6000.
//   windows   the table of gnn_classify_contigs: seq_windows(seq, 6000, 2500, max_windows) per contig, honouring single_window.
//             Window ids, the N rule and the kept mask are unchanged.  Every window is occluded; kept is a mask, as in the scan.
//   blocks    window i of length len_i has nb_i = ceil(len_i / B) blocks; block j is the window-relative interval
//             [j B, min((j + 1) B, len_i)).  The pad is never a block.
//   pairs     all (window, block) pairs in window order, then block order: P = sum nb_i, indexed through the CSR
//             blk_offsets[n_windows + 1].
//   occluded  window: the forward window as materialize_kernel writes it (upper-cased, right-padded with 'N') with the block's bytes
//             set to 'N' (occlude_kernel, gnn_encode.hip).
//   delta     delta[p][c] = base[i][c] - occ[p][c].  Positive: the block supports class c.  A block without an ACGT byte yields
//             exactly +0.0 - its tokens are the window's own, and every arithmetic is batch-invariant.
//
// The base windows go first, in the slabs of gnn_classify_contigs; the contig scores are their masked mean.  Then the pairs, in
// slabs of at most what d_bases holds (4 launches): a slab is materialised by occlude_kernel, scored by classify_chunks, differenced
// in place by occlusion_delta_kernel and copied to delta_host.  Device memory does not grow with P: 6000 B + 12 B per pair of ONE
// slab, the per-window tables of gnn_classify_contigs and 8 B per window of blk_offsets.  Entry, plan, span table, sequence feed and
// the base windows' slabs are the steps of gnn_classify_contigs (gnn_common.h), run forward-only.
#include <cstring>

#include "gnn_common.h"

namespace gnn {

// One thread per (pair, class) of the slab [pair0, pair0 + m): occ[r][c] <- base[window of pair0 + r][c] - occ[r][c].  The window is
// found by bisection of blk_off, as in occlude_kernel.  In place: a thread reads and writes its own element only.
__global__ void occlusion_delta_kernel(const float* __restrict__ base, const int64_t* __restrict__ blk_off, int64_t n_windows,
                                       int64_t pair0, int64_t m, float* __restrict__ occ) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m * GNN_CLASSES) return;
    const int64_t p = pair0 + i / GNN_CLASSES;
    const int cl = (int)(i % GNN_CLASSES);
    int64_t a = 0, b = n_windows - 1;
    while (a < b) {
        const int64_t mid = (a + b) >> 1;
        if (blk_off[mid + 1] <= p) a = mid + 1; else b = mid;
    }
    occ[i] = base[a * GNN_CLASSES + cl] - occ[i];
}

static int check_block(int block, const char* fn) {
    if (block >= 1 && block <= W) return GNN_OK;
    set_error(std::string(fn) + ": block " + std::to_string(block) + " is outside [1, " + std::to_string(W) + "]");
    return GNN_ERR_ARG;
}

}  // namespace gnn

using namespace gnn;

extern "C" int gnn_occlusion_plan(const int64_t* offsets_host, int64_t n_contigs, int block, int single_window, int64_t* n_windows_out,
                                  int64_t* n_pairs_out, int64_t* win_offsets_or_null, int64_t* starts_or_null, int32_t* lens_or_null,
                                  int64_t* blk_offsets_or_null) {
    if (!offsets_host || n_contigs < 0 || !n_windows_out || !n_pairs_out) {
        set_error("bad argument to gnn_occlusion_plan");
        return GNN_ERR_ARG;
    }
    if (int rc = check_block(block, "gnn_occlusion_plan")) return rc;
    int64_t pairs = 0;
    WindowWalk walk{win_offsets_or_null};
    const int rc = walk_windows(offsets_host, n_contigs, W, single_window, walk, [&](int64_t, int64_t k, int64_t l) {
        if (starts_or_null) starts_or_null[walk.windows] = k * W;
        if (lens_or_null) lens_or_null[walk.windows] = (int32_t)l;
        pairs += (l + block - 1) / block;
        if (blk_offsets_or_null) blk_offsets_or_null[walk.windows + 1] = pairs;
    });
    if (rc) return rc;
    if (blk_offsets_or_null) blk_offsets_or_null[0] = 0;
    *n_windows_out = walk.windows;
    *n_pairs_out = pairs;
    return GNN_OK;
}

extern "C" int gnn_occlude_spans_dev(gnn_ctx* ctx, const uint8_t* seq_dev, const int64_t* starts_host, const int32_t* lens_host,
                                     const int32_t* lo_host, const int32_t* hi_host, int64_t n, uint8_t* bases_dev_out) {
    if (int rc = check_ctx(ctx)) return rc;
    if (n < 0 || (n > 0 && (!seq_dev || !starts_host || !lens_host || !lo_host || !hi_host || !bases_dev_out))) {
        set_error("bad argument to gnn_occlude_spans_dev");
        return GNN_ERR_ARG;
    }
    if ((uintptr_t)bases_dev_out & 3) {
        set_error("gnn_occlude_spans_dev: bases_dev_out is not 4-byte aligned");
        return GNN_ERR_ARG;
    }
    for (int64_t i = 0; i < n; ++i) {
        if (starts_host[i] < 0 || lens_host[i] < 0 || lens_host[i] > W) {
            set_error("gnn_occlude_spans_dev: span " + std::to_string(i) + " has start " + std::to_string(starts_host[i]) + " and length " +
                      std::to_string(lens_host[i]) + ": a negative start or a length outside [0, 6000]");
            return GNN_ERR_ARG;
        }
        if (lo_host[i] < 0 || lo_host[i] > hi_host[i] || hi_host[i] > W) {
            set_error("gnn_occlude_spans_dev: span " + std::to_string(i) + " has the interval [" + std::to_string(lo_host[i]) + ", " +
                      std::to_string(hi_host[i]) + "): 0 <= lo <= hi <= 6000 is required");
            return GNN_ERR_ARG;
        }
    }
    if (n == 0) return GNN_OK;
    DevBuf<int64_t> ds;
    DevBuf<int32_t> dl, dlo, dhi;
    int rc = ds.reserve((size_t)n);
    if (!rc) rc = dl.reserve((size_t)n);
    if (!rc) rc = dlo.reserve((size_t)n);
    if (!rc) rc = dhi.reserve((size_t)n);
    if (rc) return rc;
    GNN_HIP(hipMemcpyAsync(ds, starts_host, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    GNN_HIP(hipMemcpyAsync(dl, lens_host, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    GNN_HIP(hipMemcpyAsync(dlo, lo_host, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    GNN_HIP(hipMemcpyAsync(dhi, hi_host, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    rc = launch_occlude(ctx, seq_dev, ds, dl, nullptr, n, 0, 0, dlo, dhi, n, bases_dev_out);
    const hipError_t e = hipStreamSynchronize(ctx->stream);      // the span table goes with this call
    if (rc) return rc;
    GNN_HIP(e);
    return GNN_OK;
}

extern "C" int gnn_occlude_contigs(gnn_ctx* ctx, const uint8_t* seq, int seq_on_host, int64_t seq_bytes, const int64_t* offsets_host,
                                   int64_t n_contigs, int block, int single_window, int precision, float* window_scores_host,
                                   uint8_t* window_kept_host_or_null, int64_t windows_capacity, float* delta_host,
                                   int64_t pairs_capacity, float* contig_scores_host_or_null) {
    const char* const fn = "gnn_occlude_contigs";
    if (int rc = check_block(block, fn)) return rc;
    const ContigIn in{ctx, seq, seq_on_host, seq_bytes, offsets_host, n_contigs, single_window, precision, W};
    ContigWorkspace* wp = nullptr;
    int rc = contig_begin(in, fn, true, &wp);
    if (rc) return rc;
    ContigWorkspace& w = *wp;

    // ---- plan: the windows (the table of gnn_classify_contigs) and the CSR of their blocks
    if ((rc = plan_windows(in, w, false, block))) return rc;
    const int64_t n = (int64_t)w.starts.size();
    const int64_t n_pairs = w.blk_off.back();
    if (n_contigs && contig_scores_host_or_null) std::memset(contig_scores_host_or_null, 0, (size_t)n_contigs * GNN_CLASSES * sizeof(float));
    if (n == 0) return GNN_OK;
    if (!window_scores_host || windows_capacity < n) {
        set_error("window_scores_host holds " + std::to_string(windows_capacity) + " windows, the occlusion has " + std::to_string(n));
        return GNN_ERR_ARG;
    }
    if (!delta_host || pairs_capacity < n_pairs) {
        set_error("delta_host holds " + std::to_string(pairs_capacity) + " pairs, the occlusion has " + std::to_string(n_pairs));
        return GNN_ERR_ARG;
    }

    // ---- reserve: the span table, blk_offsets, one slab of windows / of pairs, the sequence
    if ((rc = upload_span_table(ctx, w))) return rc;
    const int64_t launches4 = std::max<int64_t>(4 * std::max<int64_t>(ctx->chunk_fused, 1), 1);     // what d_bases holds today
    const int64_t slab_w = std::min(n, launches4), slab_p = std::min(n_pairs, launches4);
    if (w.d_blk_off.capacity() < (size_t)n + 1 || w.d_bases.capacity() < (size_t)std::max(slab_w, slab_p) * W ||
        w.d_occ.capacity() < (size_t)slab_p * GNN_CLASSES || w.d_out.capacity() < (size_t)n_contigs * GNN_CLASSES)
        GNN_HIP(hipStreamSynchronize(ctx->stream));      // a buffer that grows is freed first: nothing may still read it
    if ((rc = reserve_roomy(w.d_blk_off, (size_t)n + 1))) return rc;
    if ((rc = reserve_roomy(w.d_bases, (size_t)std::max(slab_w, slab_p) * W))) return rc;
    if ((rc = reserve_roomy(w.d_occ, (size_t)slab_p * GNN_CLASSES))) return rc;
    if ((rc = reserve_roomy(w.d_out, (size_t)n_contigs * GNN_CLASSES))) return rc;
    SeqFeed feed;
    if ((rc = feed.begin(in, w))) return rc;
    GNN_HIP(hipMemcpyAsync(w.d_blk_off, w.blk_off.data(), (size_t)(n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));

    // ---- the base windows, forward only: N counts, windows, scores; the contig scores are their masked mean
    for (int64_t a = 0; a < n; a += slab_w)
        if ((rc = slab_pass(in, w, feed, a, std::min(slab_w, n - a), true, false, w.d_scores + a * GNN_CLASSES, nullptr))) return rc;
    if ((rc = launch_masked_segment_mean(ctx, w.d_scores, w.d_ids, w.d_window_n, w.d_counts, n, n_contigs, w.d_out))) return rc;
    w.counts.resize((size_t)n);
    if (contig_scores_host_or_null)
        GNN_HIP(hipMemcpyAsync(contig_scores_host_or_null, w.d_out, (size_t)n_contigs * GNN_CLASSES * sizeof(float), hipMemcpyDeviceToHost,
                               ctx->stream));
    GNN_HIP(hipMemcpyAsync(w.counts.data(), w.d_counts, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    GNN_HIP(hipMemcpyAsync(window_scores_host, w.d_scores, (size_t)n * GNN_CLASSES * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));

    // ---- the pairs, a slab at a time: occluded windows, their scores, base - occ in place, out.  A pair reads the bytes of its
    // window and nothing else, and the base pass's last slab named the last byte any window reads (spans are in buffer order): the
    // feed has nothing left to upload, and the ctx stream already waits for all of it.
    for (int64_t p0 = 0; p0 < n_pairs; p0 += slab_p) {
        const int64_t m = std::min(slab_p, n_pairs - p0);
        if ((rc = launch_occlude(ctx, feed.dev(), w.d_starts, w.d_lens, w.d_blk_off, n, p0, block, nullptr, nullptr, m, w.d_bases))) return rc;
        if ((rc = classify_chunks(ctx, w.d_bases, m, precision, w.d_occ))) return rc;
        if ((rc = launch_1d(occlusion_delta_kernel, m * GNN_CLASSES, ctx->stream, w.d_scores, w.d_blk_off, n, p0, m, w.d_occ))) return rc;
        GNN_HIP(hipMemcpyAsync(delta_host + p0 * GNN_CLASSES, w.d_occ, (size_t)m * GNN_CLASSES * sizeof(float), hipMemcpyDeviceToHost,
                               ctx->stream));
    }
    GNN_HIP(hipStreamSynchronize(ctx->stream));
    kept_windows(w, window_kept_host_or_null, nullptr);
    return GNN_OK;
}
