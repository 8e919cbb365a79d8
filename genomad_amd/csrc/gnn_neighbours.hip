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
constexpr int64_t NB_MAX = (int64_t)1 << 31;     // base indices are int32 in the partial lists

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
    const int64_t b0 = (int64_t)blockIdx.y * a.split_rows, b1 = min(a.nb, b0 + a.split_rows);
    {
        const uint4* src = a.qfrag + (int64_t)blockIdx.x * 2 * BLK_U4;
        for (int i = tid; i < 2 * BLK_U4; i += 256) qs[i] = src[i];
        if (tid < QT) {
            const int q = blockIdx.x * QT + tid;
            lcnt[tid] = 0;
            lok[tid] = q < a.nq && a.qvalid[q];
            const int64_t own = a.self_off < 0 ? -1 : a.self_off + q - b0;
            lself[tid] = own >= 0 && own < a.split_rows ? (int)own : -1;
        }
    }
    __syncthreads();
    const int64_t last_blk = (b1 - 1) / 32;               // b1 > b0: the host launches no empty range
    int par = 0;
    for (int64_t c0 = b0; c0 < b1; c0 += STEP, par ^= 1) {
        // ---- this wave's two column blocks; one beyond the range reads the range's last block and is masked below
        const uint4* bp[2];
        int coff[2];                       // the lane's column as an offset into the range, -1: no candidate
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const int64_t blk = c0 / 32 + wave * 2 + nb;
            bp[nb] = a.bfrag + min(blk, last_blk) * BLK_U4 + lane;
            const int64_t col = blk * 32 + (lane & 31);
            coff[nb] = col < b1 && a.bvalid[col] ? (int)(col - b0) : -1;
        }
        f32x16 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        BFrag f0, f1;
        nn_load_b(f0, bp, 0);
#pragma unroll 1
        for (int ks = 0; ks < NKS; ks += 2) {              // k-step ks + 1 is fetched under the MFMAs of ks
            nn_load_b(f1, bp, ks + 1);
            nn_mfma(qs, ks, lane, f0, acc);
            nn_load_b(f0, bp, min(ks + 2, NKS - 1));
            nn_mfma(qs, ks + 1, lane, f1, acc);
        }
        // ---- candidates: C/D layout column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  A value that does not reach
        // the row's k-th best is dropped here; the others are re-examined when they are filed
        unsigned long long pick = 0;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
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
                                    const int row = mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * (src >> 5);
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
        a.pidx[o] = have ? (int32_t)(b0 + loff[row][j]) : -1;
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
    if (metric != GNN_KNN_COSINE && metric != GNN_KNN_DOT) {
        set_error(f + ": metric " + std::to_string(metric) + " is outside [0, 1] (GNN_KNN_COSINE, GNN_KNN_DOT)");
        return GNN_ERR_ARG;
    }
    if (nq < 0) {
        set_error(f + ": n_query " + std::to_string(nq) + " is outside [0, 2^63)");
        return GNN_ERR_ARG;
    }
    const int64_t rows = self ? nq : nb;
    if (rows < 0 || rows >= NB_MAX) {
        set_error(f + ": " + std::to_string(rows) + " base rows is outside [0, 2^31)");
        return GNN_ERR_ARG;
    }
    if (nq > 0 && (!query || !idx || !sim)) {
        set_error("bad argument to " + f + ": the query and both outputs are required");
        return GNN_ERR_ARG;
    }
    return GNN_OK;
}

// m <= QSLAB prepared query rows against the prepared base: tile, then merge into idx_dev[m][k], sim_dev[m][k]
int nn_search_slab(gnn_ctx* ctx, const uint4* qfrag, const uint8_t* qvalid, int64_t m, int64_t nb, int k, int metric, int64_t self_off,
                   int64_t* idx_dev, float* sim_dev) {
    NeighbourWorkspace& w = ctx->nn;
    const int64_t tiles = (m + QT - 1) / QT;
    const int64_t split_rows = nn_split_rows(ctx, tiles, nb);
    const int64_t splits = (nb + split_rows - 1) / split_rows;
    if (splits > 65535) {
        set_error("gnn_neighbours: " + std::to_string(nb) + " base rows in ranges of " + std::to_string(split_rows) + " are more than 65535 ranges");
        return GNN_ERR_ARG;
    }
    const size_t part = (size_t)m * splits * k;
    int rc = nn_reserve(ctx, w.psim, part);
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
        a.scale = metric == GNN_KNN_COSINE ? 1.f / 65536.f : 1.f;
        a.self_off = self_off;
        a.psim = w.psim.get();
        a.pidx = w.pidx.get();
        hipLaunchKernelGGL(nn_tile_kernel, dim3((unsigned)tiles, (unsigned)splits), dim3(256), 0, ctx->stream, a);
        GNN_HIP(hipGetLastError());
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
        if (to_host) {
            if ((rc = nn_reserve(ctx, w.d_idx, (size_t)m * k))) return rc;
            if ((rc = nn_reserve(ctx, w.d_sim, (size_t)m * k))) return rc;
            idx_dev = w.d_idx;
            sim_dev = w.d_sim;
        }
        if ((rc = nn_search_slab(ctx, qfrag, qvalid, m, nb, k, metric, self ? q0 : -1, idx_dev, sim_dev))) return rc;
        if (to_host) {
            GNN_HIP(hipMemcpyAsync(idx + q0 * k, w.d_idx, (size_t)m * k * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
            GNN_HIP(hipMemcpyAsync(sim + q0 * k, w.d_sim, (size_t)m * k * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
            GNN_HIP(hipStreamSynchronize(ctx->stream));      // the landing buffers and d_query serve the next slab
        }
    }
    return GNN_OK;
}

}  // namespace
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
    NeighbourWorkspace& w = ctx->nn;
    // the base goes up once; the queries follow slab by slab
    if (int rc = nn_reserve(ctx, w.d_base, (size_t)std::max<int64_t>(nb, 1) * D)) return rc;
    if (nb > 0)
        GNN_HIP(hipMemcpyAsync(w.d_base, self ? query_host : base_host_or_null, (size_t)nb * D * sizeof(float), hipMemcpyHostToDevice,
                               ctx->stream));
    return nn_search(ctx, nullptr, self ? nullptr : query_host, n_query, w.d_base, nb, self, k, metric, idx_host, sim_host, true);
}
