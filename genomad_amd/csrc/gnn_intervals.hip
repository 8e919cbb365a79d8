// Interval embeddings: the window embeddings of a scan folded into caller-given intervals of contigs, on the device.
//
// Definitions (include/genomad_nn.h has them in full).
//   - Windows are those of gnn_scan_plan at `stride`; window k of a contig has the centre base m_k = k * stride + len_k / 2 and
//     belongs to the interval [start, end) of its contig with start <= m_k < end, or to none.  m_k is strictly increasing in k (only
//     a contig's last window is shorter than 6000, by less than 2 * its advance), so the members of an interval are one range
//     [w_lo, w_hi) of the global window order; the ranges of sorted, disjoint intervals are disjoint and ordered.
//   - Per interval, over its KEPT members e_0, e_1, ... in window order: S = ((0 + e_0) + e_1) + ..., the same for the window scores,
//     and U = ((0 + u_0) + u_1) + ... with u_i = e_i * rsqrt(sum_j e_i[j]^2) (a zero row when e_i has a non-finite element or is
//     all zeros - the rows gnn_neighbours calls invalid under cosine; every other row has a unit row, whatever its scale).
//     embedding = S / count, coherence = |U| / count; under GNN_STRAND_BOTH (S_f + S_r) / (2 count) and |U_f + U_r| / (2 count).
//
// Scheme.  A pass walks the window table in slabs, as every contig call does.  interval_fold_kernel runs one workgroup per interval
// the slab [a, a + m) touches - the host finds them by bisection of the monotone ranges - and walks [max(w_lo, a), min(w_hi, a + m))
// in window order from the running sums the slabs before left in global memory: the result does not depend on the slab.  One
// workgroup owns an interval within a launch and launches are ordered on the stream: plain loads and stores, no atomics.
// The walk is serial per interval (one 2 Mbp interval at stride 1000 is 2000 dependent steps per pass) but only its ADDITIONS are:
// the rows of IV_BATCH consecutive windows are loaded and their squared norms reduced together, then added one after the other,
// while the loads of the next batch are in flight.
#include <cfloat>
#include <cstring>
#include <type_traits>

#include "gnn_common.h"

namespace gnn {

constexpr int IV_BATCH = 8;                      // rows in flight per step of a workgroup: 8 x 16 B per lane

// The plain f32 squared norm of a row serves as it is when it lies in [IV_PLAIN_MIN, FLT_MAX].  Finite: no element is inf or NaN
// and no partial sum has overflowed (the terms are non-negative, so every partial sum is at most the total).  At least 2^-116: a
// product below FLT_MIN = 2^-126 is rounded to a multiple of 2^-149, off by at most 2^-150; 512 of them cost at most
// 512 * 2^-150 = 2^-141 absolute (sums of such values are exact), which is 2^-25 of 2^-116 - half a rounding error, a quarter of
// an ulp, beside the 11 roundings of the sum itself.  Every other row - a non-finite element, all zeros, squares that overflow
// or vanish - goes the slow way of unit_scale below.
constexpr float IV_PLAIN_MIN = 0x1p-116f;

// f over the FOLD_THREADS values x of a workgroup, in every lane: a butterfly inside each wave, one exchange through `slot`, wave 0's
// part first.  Every lane of the workgroup calls it (two barriers: the readers of the call before are done, the parts are written).
template <class F>
__device__ __forceinline__ float over_workgroup(float x, float* slot, int wave, int lane, F f) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) x = f(x, __shfl_xor(x, off));
    __syncthreads();
    if (lane == 0) slot[wave] = x;
    __syncthreads();
    return f(slot[0], slot[1]);
}

// The slow way to a unit row, the rule of nn_prepare_kernel (gnn_neighbours.hip): a row is valid iff every element is finite and
// one is not zero.  v <- v * 2^-ex, which brings the largest |element| into [0.5, 1) - exact but for elements that fall below
// 2^-149 of it, and those weigh nothing in a unit row - so the squared norm lies in [0.25, 512): it neither overflows nor vanishes.
// Returns whether the row is valid and, if so, 1 / |v| of the scaled row in r.  Every lane of the workgroup calls it.
__device__ __forceinline__ bool unit_scale(float4& v, float& r, float* slot, int wave, int lane) {
    const float a = fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));      // fmaxf drops a NaN: ask each element
    const bool finite = fabsf(v.x) <= FLT_MAX && fabsf(v.y) <= FLT_MAX && fabsf(v.z) <= FLT_MAX && fabsf(v.w) <= FLT_MAX;
    const float amax = over_workgroup(finite ? a : INFINITY, slot, wave, lane, [](float p, float q) { return fmaxf(p, q); });
    if (!(amax > 0.f && amax <= FLT_MAX)) return false;      // uniform: amax is the same in every lane
    int ex;
    (void)frexpf(amax, &ex);
    v.x = ldexpf(v.x, -ex), v.y = ldexpf(v.y, -ex), v.z = ldexpf(v.z, -ex), v.w = ldexpf(v.w, -ex);
    const float ss = ((v.x * v.x + v.y * v.y) + v.z * v.z) + v.w * v.w;
    r = rsqrtf(over_workgroup(ss, slot, wave, lane, [](float p, float q) { return p + q; }));
    return true;
}

// The kept windows of slab rows [lo, hi) of interval iv0 + blockIdx.x -> its running sums.  Every pointer but the sums is relative
// to the slab's first window: rows[m][HID], scores[m][3] (SCORES), and the N rule's inputs window_n[m] / counts[m] (RULE) or
// kept[m].  FOLD_THREADS lanes x float4 = one row per load instruction.  The squared norm of a row: each lane sums its 4
// squares, a butterfly over the 64 lanes of each wave (__shfl_xor, offsets 1 .. 32), one exchange through LDS between the two
// waves, wave 0's part first - the same order every time, in every lane.  A kept row whose sum is not in [IV_PLAIN_MIN, FLT_MAX]
// is scaled by a power of two first (unit_scale) - a decision about the row alone, so no result depends on the slab.
// No other branch inside a step: a row beyond the range is read as the range's last row and, like a masked one, enters as zeros (a sum
// is never -0, so adding +0 leaves its bits alone) - the loads of a batch are independent and all in flight together.
template <bool RULE, bool SCORES>
__global__ __launch_bounds__(FOLD_THREADS) void interval_fold_kernel(const float* __restrict__ rows, const float* __restrict__ scores,
                                                                     const uint8_t* __restrict__ kept, const int32_t* __restrict__ window_n,
                                                                     const int32_t* __restrict__ counts, int64_t a, int64_t m,
                                                                     const int64_t* __restrict__ w_lo, const int64_t* __restrict__ w_hi,
                                                                     int64_t iv0, float* __restrict__ sum, float* __restrict__ unit,
                                                                     float* __restrict__ score_sum, int32_t* __restrict__ count) {
    __shared__ float part[2][2][IV_BATCH];       // [parity of the step][wave][row of the batch]
    __shared__ float wide[2];                    // unit_scale's exchange, one value per wave
    const int64_t iv = iv0 + blockIdx.x;
    const int64_t lo = (w_lo[iv] > a ? w_lo[iv] : a) - a, hi = (w_hi[iv] < a + m ? w_hi[iv] : a + m) - a;
    if (lo >= hi) return;                        // an empty range between two touched ones: the whole workgroup leaves
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int cls = tid < GNN_CLASSES ? tid : GNN_CLASSES - 1;       // every lane reads a score; lanes 0 .. 2 keep theirs
    float4* const srow = reinterpret_cast<float4*>(sum + (size_t)iv * HID) + tid;
    float4* const urow = reinterpret_cast<float4*>(unit + (size_t)iv * HID) + tid;
    float4 s = *srow, u = *urow;
    float sc = SCORES ? score_sum[iv * GNN_CLASSES + cls] : 0.f;
    int k = 0, par = 0;
    struct Batch {
        float4 v[IV_BATCH];
        float score[IV_BATCH];
        bool keep[IV_BATCH];
    };
    auto fetch = [&](int64_t i, Batch& b) {
#pragma unroll
        for (int j = 0; j < IV_BATCH; ++j) {     // uniform over the workgroup: every lane decides alike
            const int64_t r = i + j < hi ? i + j : hi - 1;
            b.v[j] = reinterpret_cast<const float4*>(rows + (size_t)r * HID)[tid];
            b.score[j] = SCORES ? scores[r * GNN_CLASSES + cls] : 0.f;
            b.keep[j] = (i + j < hi) & (RULE ? window_kept(window_n[r], counts[r]) : kept[r] != 0);
        }
    };
    Batch next;
    fetch(lo, next);
    for (int64_t i = lo; i < hi; i += IV_BATCH, par ^= 1) {
        const Batch cur = next;
        fetch(i + IV_BATCH, next);               // in flight while this batch is reduced and added (beyond the range: its last row)
        float ss[IV_BATCH];
#pragma unroll
        for (int j = 0; j < IV_BATCH; ++j) {
            const float4 v = cur.v[j];
            ss[j] = ((v.x * v.x + v.y * v.y) + v.z * v.z) + v.w * v.w;
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1)
#pragma unroll
            for (int j = 0; j < IV_BATCH; ++j) ss[j] += __shfl_xor(ss[j], off);
        if (lane == 0)
#pragma unroll
            for (int j = 0; j < IV_BATCH; ++j) part[par][wave][j] = ss[j];
        __syncthreads();                         // one barrier per step: the next step writes the other parity
        float n2[IV_BATCH];
        bool odd = false;                        // a kept row of this batch needs the slow way (a NaN sum fails the comparison too)
#pragma unroll
        for (int j = 0; j < IV_BATCH; ++j) {
            n2[j] = part[par][0][j] + part[par][1][j];
            odd |= cur.keep[j] && !(n2[j] >= IV_PLAIN_MIN && n2[j] <= FLT_MAX);
        }
        // the batch, row after row; with_slow: the rows that need the slow way take it
        auto add = [&](auto with_slow) {
#pragma unroll
            for (int j = 0; j < IV_BATCH; ++j) {
                const bool keep = cur.keep[j];
                const float4 v = cur.v[j];
                float4 w = v;                                        // the row its unit row is made of
                float r = rsqrtf(n2[j]);
                bool ok = keep;
                if constexpr (decltype(with_slow)::value)
                    if (__builtin_amdgcn_readfirstlane(keep && !(n2[j] >= IV_PLAIN_MIN && n2[j] <= FLT_MAX)))
                        ok = unit_scale(w, r, wide, wave, lane);
                s.x += keep ? v.x : 0.f, s.y += keep ? v.y : 0.f, s.z += keep ? v.z : 0.f, s.w += keep ? v.w : 0.f;
                // scaled, then added: two roundings, no fused multiply-add
                u.x += ok ? __fmul_rn(w.x, r) : 0.f, u.y += ok ? __fmul_rn(w.y, r) : 0.f;
                u.z += ok ? __fmul_rn(w.z, r) : 0.f, u.w += ok ? __fmul_rn(w.w, r) : 0.f;
                sc += keep ? cur.score[j] : 0.f;
                k += keep;
            }
        };
        // keep and n2 are the same in every lane, and the compiler is told so: the whole workgroup takes a branch or none of it does,
        // and no barrier is split.  One branch per step on the way every ordinary batch goes.
        if (__builtin_amdgcn_readfirstlane(odd)) add(std::true_type{});
        else add(std::false_type{});
    }
    *srow = s;
    *urow = u;
    if (SCORES && tid < GNN_CLASSES) score_sum[iv * GNN_CLASSES + tid] = sc;
    if (tid == 0 && count) count[iv] += k;
}

// The sums -> the outputs, one workgroup per interval.  sum_rev / unit_rev (NULL, or both): the second strand of GNN_STRAND_BOTH.
// |U| by the reduction of the fold.  An output may alias its sum: a lane reads its own elements before it writes them.
__global__ __launch_bounds__(FOLD_THREADS) void interval_finish_kernel(const float* sum, const float* unit,
                                                                       const float* __restrict__ sum_rev, const float* __restrict__ unit_rev,
                                                                       const float* score_sum, const int32_t* __restrict__ count,
                                                                       float* emb, float* __restrict__ coherence, float* scores) {
    __shared__ float part[2];
    const int64_t iv = blockIdx.x;
    const int tid = threadIdx.x;
    const size_t cell = (size_t)iv * (HID / 4) + tid;
    const int k = count[iv];
    const float d = (float)(sum_rev ? 2 * k : k);
    float4 s = reinterpret_cast<const float4*>(sum)[cell], u = reinterpret_cast<const float4*>(unit)[cell];
    if (sum_rev) {
        const float4 sr = reinterpret_cast<const float4*>(sum_rev)[cell], ur = reinterpret_cast<const float4*>(unit_rev)[cell];
        s.x += sr.x, s.y += sr.y, s.z += sr.z, s.w += sr.w;
        u.x += ur.x, u.y += ur.y, u.z += ur.z, u.w += ur.w;
    }
    reinterpret_cast<float4*>(emb)[cell] = k ? make_float4(s.x / d, s.y / d, s.z / d, s.w / d) : make_float4(0.f, 0.f, 0.f, 0.f);
    if (scores && tid < GNN_CLASSES) {
        const float v = score_sum[iv * GNN_CLASSES + tid];
        scores[iv * GNN_CLASSES + tid] = k ? v / (float)k : 0.f;
    }
    if (!coherence) return;                      // uniform: no barrier is skipped by a part of the workgroup
    float ss = ((u.x * u.x + u.y * u.y) + u.z * u.z) + u.w * u.w;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) ss += __shfl_xor(ss, off);
    if ((tid & 63) == 0) part[tid >> 6] = ss;
    __syncthreads();
    if (tid == 0) coherence[iv] = k ? sqrtf(part[0] + part[1]) / d : 0.f;
}

// the combined window scores of one slab's batch [m forward | m reverse]: (f + r) * 0.5f, as strand_split_kernel files them
__global__ void interval_mix_kernel(const float* __restrict__ batch, int64_t cells, float* __restrict__ mix) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cells) mix[i] = (batch[i] + batch[cells + i]) * 0.5f;
}

// ---- host side ----

// The first window k of a contig (length len, nw windows at `stride`) whose centre is >= x.
static int64_t first_centre_at_least(int64_t len, int64_t nw, int64_t stride, int64_t x) {
    int64_t lo = 0, hi = nw;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int64_t centre = mid * stride + std::min<int64_t>(W, len - mid * stride) / 2;
        if (centre < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Validation and the member ranges: win_off is the window CSR of the contigs (walk_windows).
static int plan_intervals(const char* fn, const int64_t* offsets, int64_t n_contigs, int64_t stride, const int64_t* win_off,
                          const int64_t* iv_contig, const int64_t* iv_start, const int64_t* iv_end, int64_t n, int64_t* w_lo,
                          int64_t* w_hi) {
    auto bad = [&](int64_t i, const std::string& why) {
        set_error(std::string(fn) + ": interval " + std::to_string(i) + " (contig " + std::to_string(iv_contig[i]) + ", [" +
                  std::to_string(iv_start[i]) + ", " + std::to_string(iv_end[i]) + ")) " + why);
        return GNN_ERR_ARG;
    };
    for (int64_t i = 0; i < n; ++i) {
        const int64_t c = iv_contig[i], s = iv_start[i], e = iv_end[i];
        if (c < 0 || c >= n_contigs) return bad(i, "names a contig outside [0, " + std::to_string(n_contigs) + ")");
        const int64_t len = offsets[c + 1] - offsets[c];
        if (s < 0) return bad(i, "starts below 0");
        if (e < s) return bad(i, "ends before it starts");
        if (e > len) return bad(i, "ends beyond its contig of " + std::to_string(len) + " bases");
        if (i > 0 && (iv_contig[i - 1] > c || (iv_contig[i - 1] == c && iv_start[i - 1] > s)))
            return bad(i, "is not sorted by (contig, start): it follows contig " + std::to_string(iv_contig[i - 1]) + ", start " +
                              std::to_string(iv_start[i - 1]));
        if (i > 0 && iv_contig[i - 1] == c && iv_end[i - 1] > s)
            return bad(i, "overlaps interval " + std::to_string(i - 1) + ", which ends at " + std::to_string(iv_end[i - 1]));
        const int64_t nw = win_off[c + 1] - win_off[c];
        w_lo[i] = win_off[c] + first_centre_at_least(len, nw, stride, s);
        w_hi[i] = win_off[c] + first_centre_at_least(len, nw, stride, e);
    }
    return GNN_OK;
}

static IntervalWorkspace& interval_ws(gnn_ctx* ctx) {
    if (!ctx->contig_ws) ctx->contig_ws = new ContigWorkspace();
    return ctx->contig_ws->intervals;
}

// The member ranges (and, unless NULL, n_kept kept flags) reach the device through pinned images the previous upload has left.
static int upload_tables(gnn_ctx* ctx, IntervalWorkspace& w, const int64_t* w_lo, const int64_t* w_hi, int64_t n, const uint8_t* kept,
                         int64_t n_kept) {
    if (w.tables_read) GNN_HIP(hipEventSynchronize(w.tables_read));
    else GNN_HIP(hipEventCreateWithFlags(&w.tables_read, hipEventDisableTiming));
    int rc = w.h_range.reserve(2 * (size_t)n, (size_t)n / 2 + 64);
    if (!rc && kept) rc = w.h_kept.reserve((size_t)n_kept, (size_t)n_kept / 4 + 64);
    if (rc) return rc;
    if (w.d_range.capacity() < 2 * (size_t)n || (kept && w.d_kept.capacity() < (size_t)n_kept))
        GNN_HIP(hipStreamSynchronize(ctx->stream));      // a buffer that grows is freed first: nothing may still read it
    if ((rc = reserve_roomy(w.d_range, 2 * (size_t)n))) return rc;
    if (kept && (rc = reserve_roomy(w.d_kept, (size_t)n_kept))) return rc;
    std::memcpy(w.h_range.get(), w_lo, (size_t)n * sizeof(int64_t));
    std::memcpy(w.h_range.get() + n, w_hi, (size_t)n * sizeof(int64_t));
    GNN_HIP(hipMemcpyAsync(w.d_range, w.h_range, 2 * (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    if (kept) {
        std::memcpy(w.h_kept.get(), kept, (size_t)n_kept);
        GNN_HIP(hipMemcpyAsync(w.d_kept, w.h_kept, (size_t)n_kept, hipMemcpyHostToDevice, ctx->stream));
    }
    GNN_HIP(hipEventRecord(w.tables_read, ctx->stream));
    return GNN_OK;
}

// What one fold launch reads and writes beside the ranges; every input is relative to the slab's first window.
struct FoldArgs {
    const float* rows;
    const float* scores;         // may be NULL
    const uint8_t* kept;         // or NULL: the N rule on window_n / counts
    const int32_t* window_n;
    const int32_t* counts;
    float* sum;
    float* unit;
    float* score_sum;            // NULL with scores
    int32_t* count;              // may be NULL (the second strand of BOTH counts nothing)
};

// Slab [a, a + m) of the window order -> the intervals it touches: w_hi and w_lo are non-decreasing, so they are the intervals from
// the first with w_hi > a to the last with w_lo < a + m (empty ranges among them leave at once).
static int launch_fold(gnn_ctx* ctx, const int64_t* w_lo, const int64_t* w_hi, int64_t n, const int64_t* d_range, int64_t a, int64_t m,
                       const FoldArgs& f) {
    const int64_t first = std::upper_bound(w_hi, w_hi + n, a) - w_hi;
    const int64_t last = std::lower_bound(w_lo, w_lo + n, a + m) - w_lo;       // one past
    if (first >= last) return GNN_OK;
    const bool rule = !f.kept, with_scores = f.scores != nullptr;
    auto* const kernel = rule ? (with_scores ? interval_fold_kernel<true, true> : interval_fold_kernel<true, false>)
                              : (with_scores ? interval_fold_kernel<false, true> : interval_fold_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)(last - first)), dim3(FOLD_THREADS), 0, ctx->stream, f.rows, f.scores, f.kept, f.window_n,
                       f.counts, a, m, d_range, d_range + n, first, f.sum, f.unit, f.score_sum, f.count);
    GNN_HIP(hipGetLastError());
    return GNN_OK;
}

static int launch_finish(gnn_ctx* ctx, const float* sum, const float* unit, const float* sum_rev, const float* unit_rev,
                         const float* score_sum, const int32_t* count, int64_t n, float* emb, float* coherence, float* scores) {
    hipLaunchKernelGGL(interval_finish_kernel, dim3((unsigned)n), dim3(FOLD_THREADS), 0, ctx->stream, sum, unit, sum_rev, unit_rev, score_sum,
                       count, emb, coherence, scores);
    GNN_HIP(hipGetLastError());
    return GNN_OK;
}

}  // namespace gnn

using namespace gnn;

extern "C" int gnn_interval_plan(const int64_t* offsets_host, int64_t n_contigs, int stride, int single_window, const int64_t* iv_contig,
                                 const int64_t* iv_start, const int64_t* iv_end, int64_t n_intervals, int64_t* w_lo_out,
                                 int64_t* w_hi_out) {
    const char* const fn = "gnn_interval_plan";
    if (!offsets_host || n_contigs < 0 || n_intervals < 0 ||
        (n_intervals > 0 && (!iv_contig || !iv_start || !iv_end || !w_lo_out || !w_hi_out))) {
        set_error(std::string("bad argument to ") + fn);
        return GNN_ERR_ARG;
    }
    if (int rc = check_stride(stride, fn)) return rc;
    std::vector<int64_t> win_off((size_t)n_contigs + 1);
    WindowWalk walk{win_off.data(), nullptr};
    if (int rc = walk_windows(offsets_host, n_contigs, stride, single_window, walk, [](int64_t, int64_t, int64_t) {})) return rc;
    return plan_intervals(fn, offsets_host, n_contigs, stride, win_off.data(), iv_contig, iv_start, iv_end, n_intervals, w_lo_out, w_hi_out);
}

extern "C" int gnn_interval_fold_dev(gnn_ctx* ctx, const float* rows_dev, const float* scores_dev_or_null, int64_t first_window,
                                     int64_t n_rows, const uint8_t* kept_host, const int64_t* w_lo_host, const int64_t* w_hi_host,
                                     int64_t n_intervals, float* sum_dev, float* unit_dev, float* score_sum_dev_or_null,
                                     int32_t* count_dev) {
    const char* const fn = "gnn_interval_fold_dev";
    if (first_window < 0 || n_rows < 0 || n_intervals < 0) {
        set_error(std::string("bad argument to ") + fn);
        return GNN_ERR_ARG;
    }
    if (n_rows == 0 || n_intervals == 0) return check_ctx(ctx);
    if (!rows_dev || !kept_host || !w_lo_host || !w_hi_host || !sum_dev || !unit_dev || !count_dev ||
        (scores_dev_or_null && !score_sum_dev_or_null)) {
        set_error(std::string("bad argument to ") + fn + ": rows, kept, the ranges, sum, unit and count are required, and scores need score_sum");
        return GNN_ERR_ARG;
    }
    for (int64_t i = 0; i < n_intervals; ++i)
        if (w_lo_host[i] < 0 || w_hi_host[i] < w_lo_host[i] || (i > 0 && w_lo_host[i] < w_hi_host[i - 1])) {
            set_error(std::string(fn) + ": interval " + std::to_string(i) + " has the member range [" + std::to_string(w_lo_host[i]) + ", " +
                      std::to_string(w_hi_host[i]) + "): 0 <= w_lo <= w_hi and w_lo >= the range before it (" +
                      std::to_string(i > 0 ? w_hi_host[i - 1] : 0) + ") are required");
            return GNN_ERR_ARG;
        }
    if (int rc = check_ctx(ctx)) return rc;
    IntervalWorkspace& w = interval_ws(ctx);
    if (int rc = upload_tables(ctx, w, w_lo_host, w_hi_host, n_intervals, kept_host + first_window, n_rows)) return rc;
    ProfScope prof(ctx, GNN_K_REGIONS);
    const FoldArgs f{rows_dev + (size_t)first_window * HID,
                     scores_dev_or_null ? scores_dev_or_null + (size_t)first_window * GNN_CLASSES : nullptr,
                     w.d_kept, nullptr, nullptr, sum_dev, unit_dev, scores_dev_or_null ? score_sum_dev_or_null : nullptr, count_dev};
    return launch_fold(ctx, w_lo_host, w_hi_host, n_intervals, w.d_range, first_window, n_rows, f);
}

extern "C" int gnn_interval_finish_dev(gnn_ctx* ctx, const float* sum_dev, const float* unit_dev, const float* sum_rev_dev_or_null,
                                       const float* unit_rev_dev_or_null, const float* score_sum_dev_or_null, const int32_t* count_dev,
                                       int64_t n_intervals, float* emb_dev, float* coherence_dev_or_null, float* scores_dev_or_null) {
    const char* const fn = "gnn_interval_finish_dev";
    if (n_intervals < 0 || !sum_rev_dev_or_null != !unit_rev_dev_or_null) {
        set_error(std::string("bad argument to ") + fn + ": sum_rev and unit_rev are given or NULL together");
        return GNN_ERR_ARG;
    }
    if (int rc = check_ctx(ctx)) return rc;
    if (n_intervals == 0) return GNN_OK;
    if (!sum_dev || !unit_dev || !count_dev || !emb_dev || (scores_dev_or_null && !score_sum_dev_or_null)) {
        set_error(std::string("bad argument to ") + fn + ": sum, unit, count and emb are required, and scores need score_sum");
        return GNN_ERR_ARG;
    }
    ProfScope prof(ctx, GNN_K_REGIONS);
    return launch_finish(ctx, sum_dev, unit_dev, sum_rev_dev_or_null, unit_rev_dev_or_null, score_sum_dev_or_null, count_dev, n_intervals,
                         emb_dev, coherence_dev_or_null, scores_dev_or_null);
}

// ---- the pass: a sibling of classify_contigs' run_slabs (gnn_contigs.hip) over the same steps ----
extern "C" int gnn_embed_intervals(gnn_ctx* ctx, const uint8_t* seq, int seq_on_host, int64_t seq_bytes, const int64_t* offsets_host,
                                   int64_t n_contigs, int stride, int single_window, int precision, int strand, const int64_t* iv_contig,
                                   const int64_t* iv_start, const int64_t* iv_end, int64_t n_intervals, float* emb_host,
                                   int32_t* count_host, float* coherence_host_or_null, float* scores_host_or_null) {
    const char* const fn = "gnn_embed_intervals";
    if (int rc = check_stride(stride, fn)) return rc;
    if (int rc = check_strand(strand, fn)) return rc;
    if (int rc = check_embed_precision(precision, fn)) return rc;
    const ContigIn in{ctx, seq, seq_on_host, seq_bytes, offsets_host, n_contigs, single_window, precision, stride};
    const bool some = n_intervals > 0 && n_contigs > 0;
    ContigWorkspace* wp = nullptr;
    int rc = contig_begin(in, fn, n_intervals >= 0 && (!some || (iv_contig && iv_start && iv_end && emb_host && count_host)), &wp);
    if (rc) return rc;
    if (!some) return GNN_OK;        // nothing is written
    ContigWorkspace& w = *wp;
    IntervalWorkspace& iw = w.intervals;
    // ---- plan: the window table, the member ranges, the outputs zeroed
    if ((rc = plan_windows(in, w, true, 0))) return rc;
    const size_t ni = (size_t)n_intervals;
    iw.w_lo.resize(ni), iw.w_hi.resize(ni);
    if ((rc = plan_intervals(fn, offsets_host, n_contigs, stride, w.win_off.data(), iv_contig, iv_start, iv_end, n_intervals,
                             iw.w_lo.data(), iw.w_hi.data())))
        return rc;
    std::memset(emb_host, 0, ni * HID * sizeof(float));
    std::memset(count_host, 0, ni * sizeof(int32_t));
    if (coherence_host_or_null) std::memset(coherence_host_or_null, 0, ni * sizeof(float));
    if (scores_host_or_null) std::memset(scores_host_or_null, 0, ni * GNN_CLASSES * sizeof(float));
    const int64_t n = (int64_t)w.starts.size();
    if (n == 0) return GNN_OK;
    const bool need_f = strand != GNN_STRAND_REVERSE, need_r = strand != GNN_STRAND_FORWARD, both = need_f && need_r;
    const int64_t ns = both ? 2 : 1;
    // a slab is what d_bases holds: 4 launches of windows, of one strand or - forward windows, then reverse windows - of both
    const int64_t slab = std::min<int64_t>(n, std::max<int64_t>(4 * std::max<int64_t>(ctx->chunk_fused, 1) / ns, 1));
    const size_t batch = (size_t)(slab * ns);
    // ---- reserve: the span table, one slab of windows, scores and rows, the sums
    hipStream_t const stream = ctx->stream;
    if ((rc = upload_span_table(ctx, w))) return rc;
    if ((rc = upload_tables(ctx, iw, iw.w_lo.data(), iw.w_hi.data(), n_intervals, nullptr, 0))) return rc;
    if (w.d_emb.capacity() < batch * HID || w.d_slab_scores.capacity() < batch * GNN_CLASSES || iw.d_sum.capacity() < ni * HID ||
        iw.d_unit.capacity() < ni * HID || iw.d_score_sum.capacity() < ni * GNN_CLASSES || iw.d_coherence.capacity() < ni ||
        iw.d_count.capacity() < ni ||
        (both && (iw.d_sum_rev.capacity() < ni * HID || iw.d_unit_rev.capacity() < ni * HID || iw.d_mix.capacity() < (size_t)slab * GNN_CLASSES)))
        GNN_HIP(hipStreamSynchronize(stream));      // a buffer that grows is freed first: nothing may still read it
    if ((rc = reserve_roomy(w.d_bases, batch * W))) return rc;
    if ((rc = reserve_roomy(w.d_slab_scores, batch * GNN_CLASSES))) return rc;
    if ((rc = reserve_roomy(w.d_emb, batch * HID))) return rc;
    if ((rc = reserve_roomy(iw.d_sum, ni * HID))) return rc;
    if ((rc = reserve_roomy(iw.d_unit, ni * HID))) return rc;
    if ((rc = reserve_roomy(iw.d_score_sum, ni * GNN_CLASSES))) return rc;
    if ((rc = reserve_roomy(iw.d_coherence, ni))) return rc;
    if ((rc = reserve_roomy(iw.d_count, ni))) return rc;
    GNN_HIP(hipMemsetAsync(iw.d_sum, 0, ni * HID * sizeof(float), stream));
    GNN_HIP(hipMemsetAsync(iw.d_unit, 0, ni * HID * sizeof(float), stream));
    GNN_HIP(hipMemsetAsync(iw.d_score_sum, 0, ni * GNN_CLASSES * sizeof(float), stream));
    GNN_HIP(hipMemsetAsync(iw.d_count, 0, ni * sizeof(int32_t), stream));
    if (both) {          // the reverse strand folds into sums of its own: two independent sums, whatever the slab size
        if ((rc = reserve_roomy(iw.d_sum_rev, ni * HID))) return rc;
        if ((rc = reserve_roomy(iw.d_unit_rev, ni * HID))) return rc;
        if ((rc = reserve_roomy(iw.d_mix, (size_t)slab * GNN_CLASSES))) return rc;
        GNN_HIP(hipMemsetAsync(iw.d_sum_rev, 0, ni * HID * sizeof(float), stream));
        GNN_HIP(hipMemsetAsync(iw.d_unit_rev, 0, ni * HID * sizeof(float), stream));
    }
    // ---- pass: slabs of windows through the front end, each folded into the intervals it touches
    SeqFeed feed;
    if ((rc = feed.begin(in, w))) return rc;
    for (int64_t a = 0; a < n; a += slab) {
        const int64_t m = std::min(slab, n - a);
        if ((rc = slab_pass(in, w, feed, a, m, need_f, need_r, w.d_slab_scores, w.d_emb))) return rc;
        // classify_chunks has ordered its back ends before ctx->stream: the slab's rows and scores are complete
        const float* mode_scores = w.d_slab_scores;      // one strand: its scores are the mode's
        if (both) {
            if ((rc = launch_1d(interval_mix_kernel, m * GNN_CLASSES, stream, w.d_slab_scores, m * GNN_CLASSES, iw.d_mix))) return rc;
            mode_scores = iw.d_mix;
        }
        ProfScope prof(ctx, GNN_K_REGIONS);
        const FoldArgs f{w.d_emb, mode_scores, nullptr, w.d_window_n + a, w.d_counts + a, iw.d_sum, iw.d_unit, iw.d_score_sum, iw.d_count};
        if ((rc = launch_fold(ctx, iw.w_lo.data(), iw.w_hi.data(), n_intervals, iw.d_range, a, m, f))) return rc;
        if (both) {
            const FoldArgs r{w.d_emb + (size_t)m * HID, nullptr, nullptr, w.d_window_n + a, w.d_counts + a, iw.d_sum_rev, iw.d_unit_rev,
                             nullptr, nullptr};
            if ((rc = launch_fold(ctx, iw.w_lo.data(), iw.w_hi.data(), n_intervals, iw.d_range, a, m, r))) return rc;
        }
    }
    // ---- finish in place and copy back
    {
        ProfScope prof(ctx, GNN_K_REGIONS);
        if ((rc = launch_finish(ctx, iw.d_sum, iw.d_unit, both ? iw.d_sum_rev.get() : nullptr, both ? iw.d_unit_rev.get() : nullptr,
                                iw.d_score_sum, iw.d_count, n_intervals, iw.d_sum, iw.d_coherence, iw.d_score_sum)))
            return rc;
    }
    GNN_HIP(hipMemcpyAsync(emb_host, iw.d_sum, ni * HID * sizeof(float), hipMemcpyDeviceToHost, stream));
    GNN_HIP(hipMemcpyAsync(count_host, iw.d_count, ni * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    if (coherence_host_or_null)
        GNN_HIP(hipMemcpyAsync(coherence_host_or_null, iw.d_coherence, ni * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (scores_host_or_null)
        GNN_HIP(hipMemcpyAsync(scores_host_or_null, iw.d_score_sum, ni * GNN_CLASSES * sizeof(float), hipMemcpyDeviceToHost, stream));
    GNN_HIP(hipStreamSynchronize(stream));
    return GNN_OK;
}
