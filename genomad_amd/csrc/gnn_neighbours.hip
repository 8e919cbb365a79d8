// Nearest neighbours among encoder embeddings (include/genomad_nn.h, "nearest neighbours"): the k most similar
// base rows of every query row under cosine or dot similarity, exact search, three kernels.
//   prepare   per row: the validity flag, for cosine the f32 norm in a fixed order, the row normalised and scaled by 2^8, then the
//             split into f16 hi / lo limbs stored in MFMA fragment order (2 KB per row; queries and base rows share the layout).
//   tile      one workgroup = 64 query rows (their fragments in LDS, 128 KB) x one range of base rows, streamed in steps of 256
//             columns: three v_mfma_f32_32x32x16_f16 products per k-step into f32 accumulators in a fixed k order - a pair's value
//             depends on its two rows only - and the selection fused behind every step: the nq x nb matrix is never written.
//   merge     the partial lists of a query's ranges into its k best.
// The order everywhere is (f32 similarity descending, base index ascending) on the device's own values: total, so no result depends
// on how the base is split over workgroups or the queries over slabs.
#include "gnn_nn_frag.h"

namespace gnn {
namespace {

constexpr int KMAX = 64;                         // one list entry per lane of a wave
constexpr int64_t QSLAB = 16384;                 // query rows per launch: bounds the partial lists (8 k B per query and range)
constexpr int64_t SPLIT_MAX = 65280;             // base rows per workgroup at the most: a neighbour list entry holds its row as a 16-bit offset

// ---- prepare: grid = padded rows / 32, 256 threads; wave w of a block takes its rows 8 w .. 8 w + 7, lane l the elements
// 8 l .. 8 l + 7 = the 16-byte fragment chunk (k-step l >> 1, half l & 1).  Rows at or beyond n, and invalid rows, become zero
// fragments with flag 0.  Cosine: the row is first scaled by the power of two that brings its largest element into [0.5, 1) - exact,
// and the norm then neither overflows nor vanishes - the squares are summed per lane in element order and over the lanes by a fixed
// butterfly; y = x / norm * 2^8 (the low limbs of a unit row, about 3e-5, would be f16 subnormals; the tile kernel scales the f32
// result back by 2^-16, exactly).
__global__ __launch_bounds__(256) void nn_prepare_kernel(const float* __restrict__ rows, int64_t n, int cosine, uint4* __restrict__ frag,
                                                         uint8_t* __restrict__ valid) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t blk = blockIdx.x;
    for (int i = 0; i < 8; ++i) {
        const int rb = wave * 8 + i;
        const int64_t row = blk * 32 + rb;
        float x[8];
        bool finite = true;
        float amax = 0.f;
        if (row < n) {
            const float4* src = reinterpret_cast<const float4*>(rows + row * D) + lane * 2;
            const float4 a = src[0], b = src[1];
            x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                finite = finite && fabsf(x[e]) <= 3.4028234663852886e38f;      // false for Inf and for NaN
                amax = fmaxf(amax, fabsf(x[e]));
            }
        } else {
            finite = false;
        }
        bool ok = __all(finite);
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) amax = fmaxf(amax, __shfl_xor(amax, s));
        if (cosine) {
            ok = ok && amax > 0.f;
            if (ok) {
                int ex;
                (void)frexpf(amax, &ex);
                float ss = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    x[e] = ldexpf(x[e], -ex);
                    ss += x[e] * x[e];
                }
#pragma unroll
                for (int s = 32; s > 0; s >>= 1) ss += __shfl_xor(ss, s);
                const float norm = sqrtf(ss);
#pragma unroll
                for (int e = 0; e < 8; ++e) x[e] = x[e] / norm * 256.f;
            }
        }
        f16x8 hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = ok ? x[e] : 0.f;
            hi[e] = (_Float16)v;
            lo[e] = (_Float16)(v - (float)hi[e]);
        }
        uint4* dst = frag + (blk * NKS + (lane >> 1)) * 2 * 64 + (lane & 1) * 32 + rb;
        dst[0] = __builtin_bit_cast(uint4, hi);
        dst[64] = __builtin_bit_cast(uint4, lo);
        if (lane == 0) valid[row] = ok ? 1 : 0;
    }
}

struct TileArgs {
    const uint4* qfrag;        // the slab's query fragments: 2 * gridDim.x blocks
    const uint8_t* qvalid;     // [2 * 32 * gridDim.x]
    int nq;                    // query rows of the slab
    const uint4* bfrag;        // ceil(nb / 32) blocks
    const uint8_t* bvalid;
    int64_t nb;
    int64_t split_rows;        // base rows per workgroup: a multiple of 32, <= SPLIT_MAX
    int splits;                // = gridDim.y
    int k;
    float scale;               // 2^-16 for cosine, 1 for dot
    int64_t self_off;          // self-search: query row i of the slab is base row self_off + i and is no candidate; < 0: none
    float* psim;               // partial lists [nq][splits][k]: NaN / -1 behind a list's end
    int32_t* pidx;
};

// The whole wave files one candidate into a row's sorted list: lane j holds entry j, the entries that precede the candidate are a
// prefix, everything behind it moves down one place.  A list is touched by one wave at a time (the phases of the tile kernel), lane j
// reads and writes entry j only, and the LDS executes a wave's operations in order.
__device__ __forceinline__ void nn_insert(volatile float* sims, volatile uint16_t* offs, volatile int* cnt_p, int k, int lane, float s,
                                          unsigned off) {
    const int cnt = *cnt_p;
    const float es = sims[lane];
    const unsigned eo = offs[lane];
    const bool prec = lane < cnt && (es > s || (es == s && eo < off));
    const int p = __popcll(__ballot(prec));
    if (p >= k) return;                                   // the list has tightened since the candidate was picked
    const float ps = __shfl_up(es, 1);
    const unsigned po = __shfl_up(eo, 1);
    const int ncnt = min(cnt + 1, k);
    if (lane == p) {
        sims[lane] = s;
        offs[lane] = (uint16_t)off;
    } else if (lane > p && lane < ncnt) {
        sims[lane] = ps;
        offs[lane] = (uint16_t)po;
    }
    if (lane == 0) *cnt_p = ncnt;
}

// grid = (query tiles of the slab, base ranges), 256 threads.  LDS: the tile's fragments 128 KB, the lists 24 KB (f32 similarity and
// 16-bit offset into the workgroup's range per entry; lane j of an inserting wave touches entry j: consecutive banks), their lengths.
__global__ __launch_bounds__(256) void nn_tile_kernel(TileArgs a) {
    __shared__ uint4 qs[2 * BLK_U4];
    __shared__ float lsim[QT][KMAX];
    __shared__ uint16_t loff[QT][KMAX];
    __shared__ int lcnt[QT];
    __shared__ int lself[QT];              // the row's own offset in this range (self-search), or -1
    __shared__ uint8_t lok[QT];
    __shared__ int lany[2][4];             // per step parity and wave: does the wave hold a candidate
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = a.k;
    TileRange t;
    nn_tile_range(t, a.split_rows, a.nb, false);          // never empty: the host launches no empty range
    nn_copy_tile(qs, a.qfrag, tid);
    if (tid < QT) {
        const int q = blockIdx.x * QT + tid;
        lcnt[tid] = 0;
        lok[tid] = q < a.nq && a.qvalid[q];
        const int64_t own = a.self_off < 0 ? -1 : a.self_off + q - t.b0;
        lself[tid] = own >= 0 && own < a.split_rows ? (int)own : -1;
    }
    __syncthreads();
    const int64_t last_blk = t.last_blk();
    int par = 0;
    for (int64_t c0 = t.c0; c0 < t.b1; c0 += STEP, par ^= 1) {
        const uint4* bp[2];
        int coff[2];                       // the lane's column as an offset into the range, -1: no candidate
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const int64_t col = nn_step_column(a.bfrag, c0, wave, lane, nb, last_blk, bp[nb]);
            coff[nb] = col < t.b1 && a.bvalid[col] ? (int)(col - t.b0) : -1;
        }
        f32x16 acc[2][2];
        NN_PRODUCTS(qs, bp, lane, acc);
        // ---- candidates.  A value that does not reach the row's k-th best is dropped here; the others are re-examined when they are
        // filed
        unsigned long long pick = 0;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = nn_acc_row(mb, r, lane >> 5);
                const int cnt = lcnt[row];
                const float kth = lsim[row][k - 1];
                const int own = lself[row];
                const bool rok = lok[row];
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    const float s = acc[mb][nb][r] * a.scale;
                    acc[mb][nb][r] = s;
                    const bool take = rok && coff[nb] >= 0 && coff[nb] != own && s == s && (cnt < k || s >= kth);
                    pick |= (unsigned long long)take << ((mb * 2 + nb) * 16 + r);
                }
            }
        const bool wave_any = __ballot(pick != 0) != 0;
        if (lane == 0) lany[par][wave] = wave_any;
        __syncthreads();
        if (lany[par][0] | lany[par][1] | lany[par][2] | lany[par][3]) {
            // ---- one wave at a time files its candidates; the order cannot matter, the list is the k best of a total order
            for (int w = 0; w < 4; ++w) {
                if (w == wave && wave_any) {
#pragma unroll
                    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                            for (int r = 0; r < 16; ++r) {
                                unsigned long long bal = __ballot((pick >> ((mb * 2 + nb) * 16 + r)) & 1);
                                while (bal) {
                                    const int src = __ffsll((long long)bal) - 1;
                                    bal &= bal - 1;
                                    const int row = nn_acc_row(mb, r, src >> 5);
                                    const float s = __shfl(acc[mb][nb][r], src);
                                    const unsigned off = (unsigned)__shfl(coff[nb], src);
                                    nn_insert(lsim[row], loff[row], &lcnt[row], k, lane, s, off);
                                }
                            }
                }
                __syncthreads();
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < QT * k; i += 256) {
        const int row = i / k, j = i - row * k;
        const int q = blockIdx.x * QT + row;
        if (q >= a.nq) continue;
        const bool have = j < lcnt[row];
        const int64_t o = ((int64_t)q * a.splits + blockIdx.y) * k + j;
        a.psim[o] = have ? lsim[row][j] : NAN;
        a.pidx[o] = have ? (int32_t)(t.b0 + loff[row][j]) : -1;
    }
}

__device__ __forceinline__ bool nn_precedes(float s0, int i0, float s1, int i1) { return s0 > s1 || (s0 == s1 && i0 < i1); }

// grid = query rows of the slab, 64 threads = one wave: lane j holds entry j of the running list; every partial list is merged in
// by ranks - an entry's place is its own index plus the number of entries of the other list that precede it.  No range (nb == 0):
// the row is all -1 / NaN.
__global__ __launch_bounds__(64) void nn_merge_kernel(const float* __restrict__ psim, const int32_t* __restrict__ pidx, int splits, int k,
                                                      int64_t* __restrict__ idx, float* __restrict__ sim) {
    __shared__ float os[KMAX];
    __shared__ int oi[KMAX];
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    float rs = 0.f;
    int ri = -1, cnt = 0;
    for (int s = 0; s < splits; ++s) {
        const int64_t o = (q * splits + s) * k + lane;
        const float ns = lane < k ? psim[o] : 0.f;
        const int ni = lane < k ? pidx[o] : -1;
        const int ncnt = __popcll(__ballot(ni >= 0));
        if (ncnt == 0) continue;
        int rank_new = 0, rank_run = 0;
        for (int i = 0; i < cnt; ++i) rank_new += nn_precedes(__shfl(rs, i), __shfl(ri, i), ns, ni);
        for (int i = 0; i < ncnt; ++i) rank_run += nn_precedes(__shfl(ns, i), __shfl(ni, i), rs, ri);
        __syncthreads();
        if (lane < cnt && lane + rank_run < k) {
            os[lane + rank_run] = rs;
            oi[lane + rank_run] = ri;
        }
        if (ni >= 0 && lane + rank_new < k) {
            os[lane + rank_new] = ns;
            oi[lane + rank_new] = ni;
        }
        __syncthreads();
        cnt = min(cnt + ncnt, k);
        rs = os[lane];
        ri = oi[lane];
    }
    if (lane < k) {
        idx[q * k + lane] = lane < cnt ? ri : -1;
        sim[q * k + lane] = lane < cnt ? rs : NAN;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

int check_nn_args(const char* fn, const void* query, int64_t nq, int64_t nb, bool self, int k, int metric, const void* idx,
                  const void* sim) {
    const std::string f(fn);
    if (k < 1 || k > KMAX) {
        set_error(f + ": k " + std::to_string(k) + " is outside [1, " + std::to_string(KMAX) + "]");
        return GNN_ERR_ARG;
    }
    if (int rc = nn_check_metric(f, metric)) return rc;
    if (nq < 0) {
        set_error(f + ": n_query " + std::to_string(nq) + " is outside [0, 2^63)");
        return GNN_ERR_ARG;
    }
    if (int rc = nn_check_rows(f, self ? nq : nb, "base rows")) return rc;
    return nn_check_required(f, nq == 0 || (query && idx && sim), "the query and both outputs");
}

// m <= QSLAB prepared query rows against the prepared base: tile, then merge into idx_dev[m][k], sim_dev[m][k]
int nn_search_slab(gnn_ctx* ctx, const uint4* qfrag, const uint8_t* qvalid, int64_t m, int64_t nb, int k, int metric, int64_t self_off,
                   int64_t* idx_dev, float* sim_dev) {
    NeighbourWorkspace& w = ctx->nn;
    const int64_t tiles = (m + QT - 1) / QT;
    int64_t split_rows, splits;
    int rc = nn_tile_grid(ctx, "gnn_neighbours", "base rows", tiles, nb, &split_rows, &splits);
    if (rc) return rc;
    const size_t part = (size_t)m * splits * k;
    rc = nn_reserve(ctx, w.psim, part);
    if (!rc) rc = nn_reserve(ctx, w.pidx, part);
    if (rc) return rc;
    ProfScope prof(ctx, GNN_K_NEIGHBOURS);
    if (splits > 0) {
        TileArgs a;
        a.qfrag = qfrag;
        a.qvalid = qvalid;
        a.nq = (int)m;
        a.bfrag = w.bfrag.get();
        a.bvalid = w.bvalid.get();
        a.nb = nb;
        a.split_rows = split_rows;
        a.splits = (int)splits;
        a.k = k;
        a.scale = nn_metric_scale(metric);
        a.self_off = self_off;
        a.psim = w.psim.get();
        a.pidx = w.pidx.get();
        if ((rc = launch_tiles(nn_tile_kernel, tiles, splits, ctx->stream, a))) return rc;
    }
    hipLaunchKernelGGL(nn_merge_kernel, dim3((unsigned)m), dim3(64), 0, ctx->stream, w.psim.get(), w.pidx.get(), (int)splits, k, idx_dev,
                       sim_dev);
    GNN_HIP(hipGetLastError());
    return GNN_OK;
}

// The search over a base on the device, the queries in slabs of QSLAB rows.  self: the query fragments are the base's own.  Otherwise
// the query rows are on the device (query_dev) or go up slab by slab (query_host).  to_host: idx / sim are host pointers; every slab
// lands in the ctx's buffers, is copied out and waited for.
int nn_search(gnn_ctx* ctx, const float* query_dev, const float* query_host, int64_t nq, const float* base_dev, int64_t nb, bool self, int k,
              int metric, int64_t* idx, float* sim, bool to_host) {
    NeighbourWorkspace& w = ctx->nn;
    int rc = nn_prepare(ctx, base_dev, nb, metric, w.bfrag, w.bvalid);
    if (rc) return rc;
    for (int64_t q0 = 0; q0 < nq; q0 += QSLAB) {
        const int64_t m = std::min(QSLAB, nq - q0);
        const uint4* qfrag = w.bfrag.get() + q0 / 32 * BLK_U4;
        const uint8_t* qvalid = w.bvalid.get() + q0;
        if (!self) {
            const float* rows = query_dev ? query_dev + q0 * D : nullptr;
            if (query_host) {
                if ((rc = nn_reserve(ctx, w.d_query, (size_t)m * D))) return rc;
                GNN_HIP(hipMemcpyAsync(w.d_query, query_host + q0 * D, (size_t)m * D * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
                rows = w.d_query;
            }
            if ((rc = nn_prepare(ctx, rows, m, metric, w.qfrag, w.qvalid))) return rc;
            qfrag = w.qfrag;
            qvalid = w.qvalid;
        }
        int64_t* idx_dev = idx + q0 * k;
        float* sim_dev = sim + q0 * k;
        Landing land(w.d_out);
        if (to_host) {
            land.add(idx_dev, m * k);
            land.add(sim_dev, m * k);
            if ((rc = land.reserve(ctx))) return rc;
            idx_dev = land.dev<int64_t>(0);
            sim_dev = land.dev<float>(1);
        }
        if ((rc = nn_search_slab(ctx, qfrag, qvalid, m, nb, k, metric, self ? q0 : -1, idx_dev, sim_dev))) return rc;
        if (to_host && (rc = land.copy_out(ctx))) return rc;      // synchronised: the landing buffer and d_query serve the next slab
    }
    return GNN_OK;
}

}  // namespace

// ---- the prologue of every search over encoder embeddings (declared in gnn_common.h) ------------------------------------------------

int nn_check_metric(const std::string& fn, int metric) {
    if (metric == GNN_KNN_COSINE || metric == GNN_KNN_DOT) return GNN_OK;
    set_error(fn + ": metric " + std::to_string(metric) + " is outside [0, 1] (GNN_KNN_COSINE, GNN_KNN_DOT)");
    return GNN_ERR_ARG;
}

float nn_metric_scale(int metric) { return metric == GNN_KNN_COSINE ? 1.f / 65536.f : 1.f; }

int nn_prepare(gnn_ctx* ctx, const float* rows_dev, int64_t n, int metric, DevBuf<uint4>& frag, DevBuf<uint8_t>& valid) {
    const int64_t padded = round_up(n, QT);
    int rc = nn_reserve(ctx, frag, (size_t)(padded / 32 * BLK_U4));
    if (!rc) rc = nn_reserve(ctx, valid, (size_t)padded);
    if (rc) return rc;
    if (padded == 0) return GNN_OK;
    ProfScope prof(ctx, GNN_K_NEIGHBOURS);
    hipLaunchKernelGGL(nn_prepare_kernel, dim3((unsigned)(padded / 32)), dim3(256), 0, ctx->stream, rows_dev, n, metric == GNN_KNN_COSINE,
                       frag.get(), valid.get());
    GNN_HIP(hipGetLastError());
    return GNN_OK;
}

int nn_tile_grid(const gnn_ctx* ctx, const std::string& fn, const char* noun, int64_t tiles, int64_t nb, int64_t* split_rows, int64_t* splits) {
    int64_t rows = ctx->nn.split;
    if (rows <= 0) {
        const int64_t want = std::max<int64_t>(1, (2 * std::max(ctx->cu_count, 1) + tiles - 1) / tiles);
        rows = std::max<int64_t>(STEP, (nb + want - 1) / want);
    }
    *split_rows = std::min(round_up(rows, 32), SPLIT_MAX);
    *splits = (nb + *split_rows - 1) / *split_rows;
    if (*splits <= 65535) return GNN_OK;
    set_error(fn + ": " + std::to_string(nb) + " " + noun + " in ranges of " + std::to_string(*split_rows) + " are more than 65535 ranges");
    return GNN_ERR_ARG;
}

int nn_upload_rows(gnn_ctx* ctx, const float* rows_host, int64_t n) {
    DevBuf<float>& d_base = ctx->nn.d_base;
    ctx->gr.host_rows = false;             // gnn_graph_fill / gnn_match_fill read the rows their count uploaded here: these replace them
    if (int rc = nn_reserve(ctx, d_base, (size_t)std::max<int64_t>(n, 1) * D)) return rc;
    if (n > 0) GNN_HIP(hipMemcpyAsync(d_base, rows_host, (size_t)n * D * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    return GNN_OK;
}

// ---- the scan (nn_scan): ONE block, thread t owns a run of counters, thread 0 scans the 1024 run sums between two barriers.  Every
// loop ends: i grows towards e, or towards SCAN_THREADS.
constexpr int SCAN_THREADS = 1024;
__global__ __launch_bounds__(SCAN_THREADS) void nn_scan_kernel(const int32_t* __restrict__ cnt, int64_t m, int64_t* __restrict__ off,
                                                               unsigned long long* __restrict__ cursor) {
    __shared__ int64_t run[SCAN_THREADS];
    const int64_t per = (m + SCAN_THREADS - 1) / SCAN_THREADS;
    const int64_t a = min(m, (int64_t)threadIdx.x * per), e = min(m, a + per);
    int64_t s = 0;
    for (int64_t i = a; i < e; ++i) s += cnt[i];
    run[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t acc = 0;
        for (int i = 0; i < SCAN_THREADS; ++i) {
            const int64_t v = run[i];
            run[i] = acc;
            acc += v;
        }
        off[m] = acc;
    }
    __syncthreads();
    s = run[threadIdx.x];
    for (int64_t i = a; i < e; ++i) {
        off[i] = s;
        if (cursor) cursor[i] = (unsigned long long)s;
        s += cnt[i];
    }
}

int nn_scan(hipStream_t stream, const int32_t* cnt, int64_t m, int64_t* off, unsigned long long* cursor) {
    hipLaunchKernelGGL(nn_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, cnt, m, off, cursor);
    GNN_HIP(hipGetLastError());
    return GNN_OK;
}

// ---- PassLog, HostCounters, Landing (gnn_nn_host.h) ----------------------------------------------------------------------------------

void PassLog::settle() {
    for (const auto& pr : pending_) {
        float ms = 0.f;                    // profiling only: the pair's events have completed with the synchronise before this
        if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) ms_.push_back(ms);
    }
    pending_.clear();
}

int PassLog::out(gnn_ctx* ctx, const char* fn, double* ms_out, int64_t capacity, int64_t* n_out) {
    if (!pending_.empty()) {
        GNN_HIP(hipStreamSynchronize(ctx->stream));
        settle();
    }
    if (capacity < 0 || (capacity > 0 && !ms_out) || !n_out) {
        set_error(std::string("bad argument to ") + fn + ": a capacity >= 0, its array and n_out are required");
        return GNN_ERR_ARG;
    }
    *n_out = (int64_t)ms_.size();
    for (int64_t i = 0; i < std::min<int64_t>(capacity, (int64_t)ms_.size()); ++i) ms_out[i] = ms_[i];
    return GNN_OK;
}

int HostCounters::reserve(gnn_ctx* ctx, size_t words) { return nn_reserve(ctx, dev_, words); }

int HostCounters::zero(gnn_ctx* ctx, size_t first, size_t words) {
    GNN_HIP(hipMemsetAsync(dev_.get() + first, 0, words * sizeof(unsigned long long), ctx->stream));
    return GNN_OK;
}

int HostCounters::read(gnn_ctx* ctx, size_t first, size_t words, unsigned long long* out) {
    if (int rc = host_.reserve(words)) return rc;             // no copy into it is in flight: every read ends with a synchronise
    GNN_HIP(hipMemcpyAsync(host_.get(), dev_.get() + first, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    GNN_HIP(hipStreamSynchronize(ctx->stream));
    std::copy(host_.get(), host_.get() + words, out);
    return GNN_OK;
}

int Landing::reserve(gnn_ctx* ctx) {
    if (!ok()) {
        set_error("a Landing holds at most " + std::to_string(LANDING_SLICES) + " slices");
        return GNN_ERR_STATE;
    }
    return nn_reserve(ctx, buf_, std::max<size_t>(total_ / sizeof(int64_t), 1));
}

int Landing::copy_out(gnn_ctx* ctx) const {
    for (int i = 0; i < n_; ++i)
        if (s_[i].host && s_[i].bytes)
            GNN_HIP(hipMemcpyAsync(s_[i].host, reinterpret_cast<char*>(buf_.get()) + s_[i].at, s_[i].bytes, hipMemcpyDeviceToHost, ctx->stream));
    GNN_HIP(hipStreamSynchronize(ctx->stream));
    return GNN_OK;
}

}  // namespace gnn

using namespace gnn;

extern "C" int gnn_debug_set_neighbour_split(gnn_ctx* ctx, int64_t base_rows_per_workgroup) {
    if (int rc = check_ctx(ctx)) return rc;
    if (base_rows_per_workgroup < 0) {
        set_error("gnn_debug_set_neighbour_split: " + std::to_string(base_rows_per_workgroup) +
                  " base rows per workgroup is outside [0, 2^63) (0 = the library's choice)");
        return GNN_ERR_ARG;
    }
    ctx->nn.split = base_rows_per_workgroup;
    return GNN_OK;
}

extern "C" int gnn_neighbours_dev(gnn_ctx* ctx, const float* query_dev, int64_t n_query, const float* base_dev_or_null, int64_t n_base, int k,
                                  int metric, int64_t* idx_dev, float* sim_dev) {
    const char* const fn = "gnn_neighbours_dev";
    const bool self = !base_dev_or_null;
    if (int rc = check_nn_args(fn, query_dev, n_query, n_base, self, k, metric, idx_dev, sim_dev)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (n_query == 0) return GNN_OK;
    return nn_search(ctx, query_dev, nullptr, n_query, self ? query_dev : base_dev_or_null, self ? n_query : n_base, self, k, metric, idx_dev,
                     sim_dev, false);
}

extern "C" int gnn_neighbours(gnn_ctx* ctx, const float* query_host, int64_t n_query, const float* base_host_or_null, int64_t n_base, int k,
                              int metric, int64_t* idx_host, float* sim_host) {
    const char* const fn = "gnn_neighbours";
    const bool self = !base_host_or_null;
    if (int rc = check_nn_args(fn, query_host, n_query, n_base, self, k, metric, idx_host, sim_host)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (n_query == 0) return GNN_OK;
    const int64_t nb = self ? n_query : n_base;
    // the base goes up once; the queries follow slab by slab
    if (int rc = nn_upload_rows(ctx, self ? query_host : base_host_or_null, nb)) return rc;
    return nn_search(ctx, nullptr, self ? nullptr : query_host, n_query, ctx->nn.d_base, nb, self, k, metric, idx_host, sim_host, true);
}
