// Attention contribution maps ("Attention contribution maps"): each pooled position's share of a logit, from what the back
// end already holds when a window is scored.  The encoder ends in two attention sums, feat[h*128 + ch] = sum_q alpha[h][q] yp[h][q][ch]
// (igloo.py:208-214), and the dense head behind them is piecewise linear: for the window's own ReLU pattern
//   logit_c = g_c . feat + bias_c,    g_c = d logit_c / d feat (256 values),  bias_c = the three bias terms along the active units,
// so   contrib[h][q][c] = alpha[h][q] * sum_ch yp[h][q][ch] g_c[h*128 + ch]   and   sum_h sum_q contrib + bias_c = logit_c.
// Gradient x input at the attention layer with alpha held fixed: exact, signed, per class - and no statement about what an edit of
// the window would do (alpha depends on the whole window; gnn_occlude_contigs answers that).
//
//   attrib_head_kernel     dense_kernel's forward pass (the same f32 FMAs in the same order: the scores are bit-identical) and the
//                          backward pass of the three logits through the window's ReLU masks -> g[w][256][3], bias, logits, scores
//   attrib_contrib_kernel  one workgroup per (window, head): every yp row once, three dot products with g, times alpha[q], binned
//
// Both run on the stream and the workspace of the launch whose alpha, yp and feat they read (classify_chunks), before that
// workspace can be handed to the next chunk.
#include <cstring>

#include "gnn_common.h"

namespace gnn {

constexpr int AW = 4;                    // windows per workgroup of the head kernel
constexpr int TR = 128, TK = 32;         // tile of a backward product: rows x contraction length

// acc[c] (c < 3) of thread (r = tid & 127, w = tid >> 7) for the rows r0 .. r0 + 127 of out[w][r][c] = sum_k M[r][k] rhs(w, k)[c]:
// M is row-major [.][ld] in global memory ([in][out] of a dense layer: the backward pass contracts ALONG a row).  No thread
// walks its 2 KB row in global memory: tiles of 128 rows x 32 k are fetched as float4s (a row's 128 B segment per 8 lanes) into LDS
// rows of 33 words, and a thread walks its row there.  Banks (32 for ds_read_b32 and ds_write_b32, per 32-lane half): the read
// tile[r][kk] of 32 consecutive r is at words 33 r + kk, banks r + kk: all different.  The fill's four scalar stores: a half holds
// rows 4a .. 4a + 3 (tid >> 3) and kq = 0, 4 .. 28, word 33 row + kq + e, bank row + kq + e - 32 different values: no conflict.  The right-hand side of
// the tile's 32 k is formed once per tile (rhs(w, k) -> float4, .w unused) and read as a broadcast: a wave holds one w.  k ascends
// across and inside the tiles, one fmaf per term: the order is fixed and knows nothing of the batch.
template <typename Rhs>
__device__ __forceinline__ void backward_rows(const float* __restrict__ M, int ld, int r0, int K, float (*tile)[TK + 1],
                                              float4 (*rt)[TK], Rhs&& rhs, float (&acc)[3]) {
    const int tid = threadIdx.x, r = tid & (TR - 1), w = tid >> 7;
    acc[0] = acc[1] = acc[2] = 0.f;
    for (int k0 = 0; k0 < K; k0 += TK) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int row = (tid >> 3) + 64 * p, kq = (tid & 7) * 4;
            const float4 v = *reinterpret_cast<const float4*>(M + (size_t)(r0 + row) * ld + k0 + kq);
            tile[row][kq] = v.x;
            tile[row][kq + 1] = v.y;
            tile[row][kq + 2] = v.z;
            tile[row][kq + 3] = v.w;
        }
        if (tid < AW * TK) rt[tid / TK][tid % TK] = rhs(tid / TK, k0 + tid % TK);
        __syncthreads();
#pragma unroll 8
        for (int kk = 0; kk < TK; ++kk) {
            const float m = tile[r][kk];
            const float4 v = rt[w][kk];
            acc[0] = fmaf(m, v.x, acc[0]);
            acc[1] = fmaf(m, v.y, acc[1]);
            acc[2] = fmaf(m, v.z, acc[2]);
        }
        __syncthreads();
    }
}

// Forward: dense_kernel<0> of gnn_backend.hip for AW windows per workgroup - thread j owns hidden unit j, every sum runs over k in
// ascending order with one fmaf per term, the NaN-preserving ReLU, one wave per (window, class) for the output layer - so h1, h2,
// the logits and the scores carry the bits gnn_classify computes (a window's arithmetic never depended on how many windows share
// its workgroup).  Backward, BN already folded into d1_* / d2_*, masks = what the forward pass stored is > 0:
//   v2[k][c] = (h2[k] > 0) d3k[k][c]
//   v1[j][c] = (h1[j] > 0) sum_k d2k[j][k] v2[k][c]
//   g[i][c]  = sum_j d1k[i][j] v1[j][c]
//   bias[c]  = d3b[c] + sum_k d2b[k] v2[k][c] + sum_j d1b[j] v1[j][c]
// A masked unit contributes an exact 0 (a select, not a product).  scores / bias_out / logits_out may be NULL.
__global__ __launch_bounds__(512) void attrib_head_kernel(const float* __restrict__ feat,
                                                          const float* __restrict__ d1k, const float* __restrict__ d1b,
                                                          const float* __restrict__ d2k, const float* __restrict__ d2b,
                                                          const float* __restrict__ d3k, const float* __restrict__ d3b,
                                                          int n, float* __restrict__ scores, float* __restrict__ g_out,
                                                          float* __restrict__ bias_out, float* __restrict__ logits_out) {
    __shared__ float f[AW][FEAT];
    __shared__ float h1[AW][HID];
    __shared__ float h2[AW][HID];
    __shared__ float lg[AW][4];
    __shared__ float v1[AW][HID][GNN_CLASSES];
    __shared__ float tile[TR][TK + 1];
    __shared__ __attribute__((aligned(16))) float4 rt[AW][TK];
    static_assert(AW * TR == 512 && AW * TK <= 512 && TR * TK == 2 * 512 * 4, "backward_rows' thread mapping");
    static_assert(HID % TR == 0 && FEAT % TR == 0 && HID % TK == 0, "backward_rows' tiling");
    const int w0 = blockIdx.x * AW;
    const int j = threadIdx.x;
    for (int i = j; i < AW * FEAT; i += 512) {
        const int w = i / FEAT, k = i % FEAT;
        f[w][k] = (w0 + w < n) ? feat[(size_t)(w0 + w) * FEAT + k] : 0.f;
    }
    __syncthreads();
    float acc[AW];
#pragma unroll
    for (int w = 0; w < AW; ++w) acc[w] = d1b[j];
    for (int k = 0; k < FEAT; ++k) {
        const float wv = d1k[(size_t)k * HID + j];
#pragma unroll
        for (int w = 0; w < AW; ++w) acc[w] = fmaf(f[w][k], wv, acc[w]);
    }
#pragma unroll
    for (int w = 0; w < AW; ++w) h1[w][j] = acc[w] < 0.f ? 0.f : acc[w];      // NaN stays NaN (dense_kernel)
    __syncthreads();
#pragma unroll
    for (int w = 0; w < AW; ++w) acc[w] = d2b[j];
    for (int k = 0; k < HID; ++k) {
        const float wv = d2k[(size_t)k * HID + j];
#pragma unroll
        for (int w = 0; w < AW; ++w) acc[w] = fmaf(h1[w][k], wv, acc[w]);
    }
#pragma unroll
    for (int w = 0; w < AW; ++w) h2[w][j] = acc[w] < 0.f ? 0.f : acc[w];
    __syncthreads();
    const int wave = j >> 6, lane = j & 63;
    for (int o = wave; o < AW * GNN_CLASSES; o += 8) {
        const int w = o / GNN_CLASSES, cl = o % GNN_CLASSES;
        float s = 0.f;
        for (int k = lane; k < HID; k += 64) s = fmaf(h2[w][k], d3k[(size_t)k * GNN_CLASSES + cl], s);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
        if (lane == 0) lg[w][cl] = s + d3b[cl];
    }
    __syncthreads();
    if (j < AW && w0 + j < n) {
        const float a = lg[j][0], b = lg[j][1], c = lg[j][2];
        if (logits_out) {
            float* o = logits_out + (size_t)(w0 + j) * GNN_CLASSES;
            o[0] = a;
            o[1] = b;
            o[2] = c;
        }
        if (scores) {
            const float mx = fmaxf(a, fmaxf(b, c));
            const float ea = expf(a - mx), eb = expf(b - mx), ec = expf(c - mx);
            const float inv = 1.f / (ea + eb + ec);
            float* o = scores + (size_t)(w0 + j) * GNN_CLASSES;
            o[0] = ea * inv;
            o[1] = eb * inv;
            o[2] = ec * inv;
        }
    }
    // ---- backward
    const int r = j & (TR - 1), w = j >> 7;
    float a3[3];
    auto v2 = [&](int ww, int k) {
        const bool on = h2[ww][k] > 0.f;
        return make_float4(on ? d3k[k * GNN_CLASSES] : 0.f, on ? d3k[k * GNN_CLASSES + 1] : 0.f, on ? d3k[k * GNN_CLASSES + 2] : 0.f, 0.f);
    };
    for (int j0 = 0; j0 < HID; j0 += TR) {
        backward_rows(d2k, HID, j0, HID, tile, rt, v2, a3);
        const bool on = h1[w][j0 + r] > 0.f;
#pragma unroll
        for (int c = 0; c < GNN_CLASSES; ++c) v1[w][j0 + r][c] = on ? a3[c] : 0.f;
    }
    __syncthreads();
    auto v1_of = [&](int ww, int k) { return make_float4(v1[ww][k][0], v1[ww][k][1], v1[ww][k][2], 0.f); };
    for (int i0 = 0; i0 < FEAT; i0 += TR) {
        backward_rows(d1k, HID, i0, HID, tile, rt, v1_of, a3);
        if (w0 + w < n) {
            float* o = g_out + ((size_t)(w0 + w) * FEAT + i0 + r) * GNN_CLASSES;
            o[0] = a3[0];
            o[1] = a3[1];
            o[2] = a3[2];
        }
    }
    if (!bias_out) return;
    // bias: one wave per (window, class), lanes stride the 512 + 512 terms, then the butterfly of the output layer - a fixed order
    for (int o = wave; o < AW * GNN_CLASSES; o += 8) {
        const int ww = o / GNN_CLASSES, cl = o % GNN_CLASSES;
        float s = 0.f;
        for (int k = lane; k < HID; k += 64) s = fmaf(d2b[k], h2[ww][k] > 0.f ? d3k[(size_t)k * GNN_CLASSES + cl] : 0.f, s);
        for (int k = lane; k < HID; k += 64) s = fmaf(d1b[k], v1[ww][k][cl], s);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
        if (lane == 0 && w0 + ww < n) bias_out[(size_t)(w0 + ww) * GNN_CLASSES + cl] = s + d3b[cl];
    }
}

// One workgroup per (window, head), shaped like attn_kernel: 256 threads = 8 row groups x 32 channel quads.  A yp row (512 B) is
// read once, one float4 per lane of a 32-lane group (non-temporal: nothing reads it again), four rows in flight per thread; its
// three dot products with g_c run over the lane's four channels in order, then across the group by the xor butterfly 16, 8, 4, 2, 1
// - a fixed order.  pos[q][c] = alpha[q] * dot is staged in LDS for all 749 positions, whatever the bin; then one thread per (bin,
// class) adds its positions in increasing q in f32: the map at bin = k is, bit for bit, the sequential f32 sums of the bin = 1 map.
__global__ __launch_bounds__(256) void attrib_contrib_kernel(const float* __restrict__ alpha, const float* __restrict__ yp,
                                                             const float* __restrict__ g, int bin, int nb,
                                                             float* __restrict__ contrib) {
    __shared__ float a[POOLED + 3];
    __shared__ float gs[C * GNN_CLASSES];
    __shared__ float pos[POOLED][GNN_CLASSES];
    const int wi = blockIdx.x, h = blockIdx.y;
    for (int q = threadIdx.x; q < POOLED; q += 256) a[q] = alpha[((size_t)wi * 2 + h) * POOLED + q];
    for (int i = threadIdx.x; i < C * GNN_CLASSES; i += 256) gs[i] = g[((size_t)wi * FEAT + h * C) * GNN_CLASSES + i];
    __syncthreads();
    const int cq = threadIdx.x & 31, grp = threadIdx.x >> 5;
    float gc[GNN_CLASSES][4];
#pragma unroll
    for (int c = 0; c < GNN_CLASSES; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) gc[c][e] = gs[(cq * 4 + e) * GNN_CLASSES + c];
    typedef float ntf4 __attribute__((ext_vector_type(4)));
    const ntf4* y = reinterpret_cast<const ntf4*>(yp + ((size_t)wi * 2 + h) * POOLED * C) + cq;
    auto row = [&](int q, const ntf4 v) {
        float p[GNN_CLASSES];
#pragma unroll
        for (int c = 0; c < GNN_CLASSES; ++c) {
            p[c] = fmaf(v.w, gc[c][3], fmaf(v.z, gc[c][2], fmaf(v.y, gc[c][1], v.x * gc[c][0])));
#pragma unroll
            for (int off = 16; off >= 1; off >>= 1) p[c] += __shfl_xor(p[c], off, 32);
        }
        if (cq == 0) {
            const float aq = a[q];
#pragma unroll
            for (int c = 0; c < GNN_CLASSES; ++c) pos[q][c] = aq * p[c];
        }
    };
    int q = grp;
    for (; q + 24 < POOLED; q += 32) {
        const ntf4 u0 = __builtin_nontemporal_load(y + (size_t)q * (C / 4)), u1 = __builtin_nontemporal_load(y + (size_t)(q + 8) * (C / 4)),
                   u2 = __builtin_nontemporal_load(y + (size_t)(q + 16) * (C / 4)), u3 = __builtin_nontemporal_load(y + (size_t)(q + 24) * (C / 4));
        row(q, u0);
        row(q + 8, u1);
        row(q + 16, u2);
        row(q + 24, u3);
    }
    for (; q < POOLED; q += 8) row(q, __builtin_nontemporal_load(y + (size_t)q * (C / 4)));
    __syncthreads();
    float* out = contrib + ((size_t)wi * 2 + h) * nb * GNN_CLASSES;
    for (int t = threadIdx.x; t < nb * GNN_CLASSES; t += 256) {
        const int b = t / GNN_CLASSES, c = t % GNN_CLASSES;
        const int q0 = b * bin, q1 = min(q0 + bin, POOLED);
        float s = pos[q0][c];
        for (int k = q0 + 1; k < q1; ++k) s += pos[k][c];
        out[t] = s;
    }
}

int check_attrib_args(int precision, int bin, const char* fn) {
    if (precision == GNN_PREC_F16C6 || precision == GNN_PREC_F16C8) {
        set_error(std::string(fn) + ": " + (precision == GNN_PREC_F16C6 ? "GNN_PREC_F16C6 (f16c6)" : "GNN_PREC_F16C8 (f16c8)") +
                  " has no attribution path (its dense head runs on the matrix pipe, and the map is the gradient of the exact f32 "
                  "head); use f16x3tc, f16x3tk, f16x3, bf16x3 or f32");
        return GNN_ERR_ARG;
    }
    if (bin < 1 || bin > POOLED) {
        set_error(std::string(fn) + ": bin " + std::to_string(bin) + " is outside [1, " + std::to_string(POOLED) + "]");
        return GNN_ERR_ARG;
    }
    return GNN_OK;
}

int launch_attrib_head(gnn_ctx* ctx, int64_t n, float* scores_dev, const AttribOut& at, int64_t row0) {
    const DeviceWeights& d = ctx->w;
    hipLaunchKernelGGL(attrib_head_kernel, dim3((unsigned)((n + AW - 1) / AW)), dim3(512), 0, ctx->stream, ctx->ws.feat.get(), d.d1_k,
                       d.d1_b, d.d2_k, d.d2_b, d.d3_k, d.d3_b, (int)n, scores_dev, ctx->attr_g.get(),
                       at.bias ? at.bias + row0 * GNN_CLASSES : nullptr, at.logits ? at.logits + row0 * GNN_CLASSES : nullptr);
    GNN_HIP(hipGetLastError());
    return GNN_OK;
}

int launch_attrib_contrib(gnn_ctx* ctx, int64_t n, const AttribOut& at, int64_t row0) {
    const int nb = attrib_bins(at.bin);
    hipLaunchKernelGGL(attrib_contrib_kernel, dim3((unsigned)n, 2), dim3(256), 0, ctx->stream, ctx->ws.alpha.get(), ctx->ws.yp.get(),
                       ctx->attr_g.get(), at.bin, nb, at.contrib + (size_t)row0 * 2 * nb * GNN_CLASSES);
    GNN_HIP(hipGetLastError());
    return GNN_OK;
}

}  // namespace gnn

using namespace gnn;

extern "C" int gnn_attribute_contigs(gnn_ctx* ctx, const uint8_t* seq, int seq_on_host, int64_t seq_bytes, const int64_t* offsets_host,
                                     int64_t n_contigs, int bin, int single_window, int precision, float* contrib_host,
                                     int64_t windows_capacity, float* bias_host_or_null, float* logits_host_or_null,
                                     float* window_scores_host_or_null, uint8_t* window_kept_host_or_null,
                                     float* contig_scores_host_or_null) {
    const char* const fn = "gnn_attribute_contigs";
    if (int rc = check_attrib_args(precision, bin, fn)) return rc;
    const ContigIn in{ctx, seq, seq_on_host, seq_bytes, offsets_host, n_contigs, single_window, precision, W};
    ContigWorkspace* wp = nullptr;
    int rc = contig_begin(in, fn, true, &wp);
    if (rc) return rc;
    ContigWorkspace& w = *wp;

    // ---- plan: the window table of gnn_classify_contigs
    if ((rc = plan_windows(in, w, false, 0))) return rc;
    const int64_t n = (int64_t)w.starts.size();
    if (n_contigs && contig_scores_host_or_null) std::memset(contig_scores_host_or_null, 0, (size_t)n_contigs * GNN_CLASSES * sizeof(float));
    if (n == 0) return GNN_OK;
    if (!contrib_host || windows_capacity < n) {
        set_error("contrib_host holds " + std::to_string(windows_capacity) + " windows, the attribution has " + std::to_string(n));
        return GNN_ERR_ARG;
    }

    // ---- reserve: the span table, one slab of windows and of their maps (24 nb + 24 B per window), the sequence
    if ((rc = upload_span_table(ctx, w))) return rc;
    const size_t map = (size_t)2 * attrib_bins(bin) * GNN_CLASSES;                            // floats of one window's map
    const int64_t slab = std::min(n, std::max<int64_t>(4 * std::max<int64_t>(ctx->chunk_fused, 1), 1));     // what d_bases holds today
    if (w.d_bases.capacity() < (size_t)slab * W || w.d_attr.capacity() < (size_t)slab * (map + 2 * GNN_CLASSES) ||
        w.d_out.capacity() < (size_t)n_contigs * GNN_CLASSES)
        GNN_HIP(hipStreamSynchronize(ctx->stream));      // a buffer that grows is freed first: nothing may still read it
    if ((rc = reserve_roomy(w.d_bases, (size_t)slab * W))) return rc;
    if ((rc = reserve_roomy(w.d_attr, (size_t)slab * (map + 2 * GNN_CLASSES)))) return rc;
    if ((rc = reserve_roomy(w.d_out, (size_t)n_contigs * GNN_CLASSES))) return rc;
    SeqFeed feed;
    if ((rc = feed.begin(in, w))) return rc;

    // ---- the windows, a slab at a time: N counts, windows, scores and maps; the maps leave with their slab
    float* const d_contrib = w.d_attr;
    float* const d_bias = d_contrib + (size_t)slab * map;
    float* const d_logits = d_bias + (size_t)slab * GNN_CLASSES;
    const AttribOut at{bin, d_contrib, d_bias, d_logits};
    for (int64_t a = 0; a < n; a += slab) {
        const int64_t m = std::min(slab, n - a);
        if ((rc = slab_pass(in, w, feed, a, m, true, false, w.d_scores + a * GNN_CLASSES, nullptr, &at))) return rc;
        GNN_HIP(hipMemcpyAsync(contrib_host + (size_t)a * map, d_contrib, (size_t)m * map * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        if (bias_host_or_null)
            GNN_HIP(hipMemcpyAsync(bias_host_or_null + a * GNN_CLASSES, d_bias, (size_t)m * GNN_CLASSES * sizeof(float), hipMemcpyDeviceToHost,
                                   ctx->stream));
        if (logits_host_or_null)
            GNN_HIP(hipMemcpyAsync(logits_host_or_null + a * GNN_CLASSES, d_logits, (size_t)m * GNN_CLASSES * sizeof(float),
                                   hipMemcpyDeviceToHost, ctx->stream));
    }

    // ---- the contig scores (the masked mean of gnn_classify_contigs), the N counts and the window scores
    if ((rc = launch_masked_segment_mean(ctx, w.d_scores, w.d_ids, w.d_window_n, w.d_counts, n, n_contigs, w.d_out))) return rc;
    w.counts.resize((size_t)n);
    if (contig_scores_host_or_null)
        GNN_HIP(hipMemcpyAsync(contig_scores_host_or_null, w.d_out, (size_t)n_contigs * GNN_CLASSES * sizeof(float), hipMemcpyDeviceToHost,
                               ctx->stream));
    GNN_HIP(hipMemcpyAsync(w.counts.data(), w.d_counts, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (window_scores_host_or_null)
        GNN_HIP(hipMemcpyAsync(window_scores_host_or_null, w.d_scores, (size_t)n * GNN_CLASSES * sizeof(float), hipMemcpyDeviceToHost,
                               ctx->stream));
    GNN_HIP(hipStreamSynchronize(ctx->stream));
    kept_windows(w, window_kept_host_or_null, nullptr);
    return GNN_OK;
}
