// Label transfer among encoder embeddings (include/genomad_nn.h, "label transfer"): per valid query row and per
// class of a labelled base, the voters - the valid base rows of that class whose cosine similarity reaches the threshold - counted,
// their similarities summed and the most similar one named.  Exact, over the plain rectangle query x base:
//   prepare    nn_prepare (gnn_neighbours.hip), as it is: the base's fragments and flags in the neighbour search's buffers, the
//              queries' slab by slab in its query buffers (the self form: the base's own).
//   labels     one thread per padded base column: the int64 label becomes an int32, -1 at an unlabelled, an invalid and a padded
//              column alike - one read masks all three in the tile kernel - and a value outside [-1, n_classes) raises a flag.  The
//              host reads the flag: the one synchronise of a call, before any tile kernel runs and before an output is touched.
//   votes      the tile parts of gnn_nn_frag.h: the tile is 64 query rows in LDS, the columns are base fragments, the value of
//              (query i, base row j) IS the f32 gnn_neighbours and gnn_match_* return for that pair.  A value with `rok && lab >= 0 &&
//              s >= threshold` (the self form: and j != i) does three things at (tile row, class): an integer add of 1, an integer add
//              of llrint((double)s * 2^32) and a 64-bit maximum of nn_key(nn_image(s), j).  A step without such a value costs a ballot.
//              Up to 16 classes the three arrays [64 rows][16 classes] live in LDS beside the tile (20 KB) and a workgroup flushes
//              them once, one global add / add / max per non-empty cell (gnn_debug_set_vote_lds); beyond, every value goes straight
//              to memory with the same three atomics.
//   finish     key -> nearest / nearest_sim (nn_key_index, nn_unimage): -1 / NaN where no key was written.
// Atomics are integer add / max only, stores are vector stores, nothing depends on the order the workgroups run in, on the split of
// the base (gnn_debug_set_neighbour_split) or on the path.  No loop here waits for another workgroup: every loop's termination
// argument stands next to it.  Memory beyond the fragments: 4 B per padded base column, the outputs and 8 B of keys per (query row of
// a slab, class); nothing is n_query x n_base.
#include <cmath>

#include "gnn_nn_frag.h"

namespace gnn {
namespace {

constexpr int64_t N_MAX = (int64_t)1 << 30;      // |rint(s * 2^32)| <= 2^32 + 2^10 per voter: the int64 sums of 2^30 base rows stay below 2^63
constexpr int C_MAX = 1024;
constexpr int LDS_C = 16;                        // classes whose cells a workgroup holds in LDS: 64 x 16 x (4 + 8 + 8) B = 20 KB
constexpr int64_t QSLAB = 262144;                // query rows per launch: bounds the query fragments (512 MB) and the keys (8 B per class and row)

// one thread per padded base column.  Every writer of *bad writes the same value.
__global__ __launch_bounds__(256) void vt_label_kernel(int64_t n, int64_t padded, int n_classes, const int64_t* __restrict__ label,
                                                       const uint8_t* __restrict__ valid, int32_t* __restrict__ out,
                                                       unsigned long long* __restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= padded) return;
    int32_t l = -1;
    if (i < n) {
        const int64_t v = label[i];
        if (v < -1 || v >= n_classes)
            *bad = 1;
        else if (valid[i])
            l = (int32_t)v;
    }
    out[i] = l;
}

struct VoteArgs {
    const uint4* qfrag;        // the slab's query fragments: 2 * gridDim.x blocks
    const uint8_t* qvalid;     // [64 * gridDim.x]
    int64_t nq;                // query rows of the slab
    const uint4* bfrag;        // round_up(nb, 64) / 32 blocks
    const int32_t* blabel;     // [round_up(nb, 64)]: the column's class, -1: no voter
    int64_t nb;
    int64_t split_rows;        // base rows per workgroup: a multiple of 32
    int n_classes;
    float scale;               // 2^-16: cosine
    float threshold;
    int64_t self_off;          // self form: query row i of the slab is base row self_off + i and does not vote for itself; < 0: none
    unsigned long long* cnt;   // [nq][n_classes], cleared before the launch: voters
    unsigned long long* wgt;   // the same: int64 sums of llrint(s * 2^32), two's complement
    unsigned long long* key;   // the same: max of (image of the similarity << 32) | (2^32 - 1 - base row), 0: none
};

// grid = (query tiles of the slab, base ranges), 256 threads.  LDS: the tile's fragments 128 KB, its rows' flags and,
// on the LDS path, the cells [64 rows][16 classes] - the lanes of a half hold one row and their columns' classes: one class, one
// address (the atomic unit serialises them); other classes, other banks.
// SELF false: the rectangle.  SELF true: the rows vote among themselves, and a column's own row is masked.
template <bool LDS, bool SELF>
__global__ __launch_bounds__(256) void vt_tile_kernel(VoteArgs a) {
    __shared__ uint4 qs[2 * BLK_U4];
    __shared__ unsigned long long lw[LDS ? QT * LDS_C : 1];
    __shared__ unsigned long long lk[LDS ? QT * LDS_C : 1];
    __shared__ unsigned lc[LDS ? QT * LDS_C : 1];
    __shared__ uint8_t lok[QT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
    TileRange t;
    nn_tile_range(t, a.split_rows, a.nb, false);          // never empty: the host launches no empty range
    const int64_t r0 = t.r0;
    nn_copy_tile(qs, a.qfrag, tid);
    if (LDS)
        for (int i = tid; i < QT * LDS_C; i += 256) {     // Ends: i grows by 256 towards 1024
            lc[i] = 0;
            lw[i] = 0;
            lk[i] = 0;
        }
    if (tid < QT) {
        const int64_t q = r0 + tid;
        lok[tid] = q < a.nq && a.qvalid[q];
    }
    __syncthreads();
    // self form: base row self0 + nn_acc_row(mb, r, 0) is the lane's tile row (mb, r) itself - nn_acc_row(mb, r, half) =
    // nn_acc_row(mb, r, 0) + 4 half -, so a column's own row is known without a read of LDS
    const int64_t self0 = a.self_off + r0 + 4 * half;
    const int64_t last_blk = t.last_blk();
    // Ends: c0 grows by STEP towards b1.
    for (int64_t c0 = t.c0; c0 < t.b1; c0 += STEP) {
        const uint4* bp[2];
        int cg[2], lab[2];                 // the lane's column and its class; -1: nobody votes there (beyond the range, padded, invalid, unlabelled)
        int own[2];                        // nn_acc_row(mb, r, 0) of the lane's tile row whose own column this is (self form), or -1
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const int64_t col = nn_step_column(a.bfrag, c0, wave, lane, nb, last_blk, bp[nb]);
            cg[nb] = (int)col;
            lab[nb] = col < t.b1 ? a.blabel[col] : -1;
            const int64_t rel = col - self0;
            own[nb] = SELF && rel >= 0 && rel < QT ? (int)rel : -1;
        }
        f32x16 acc[2][2];
        NN_PRODUCTS(qs, bp, lane, acc);
        // ---- votes: bit (mb * 2 + nb) * 16 + reg
        unsigned long long vote = 0;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                // The row's flag is read here, in every step, and the terms short-circuit: the compiler makes a branch and a wait for
                // LDS per row of it, 9 % of a pass without a vote (profiles/votes/README.md).  The forms without them - the flags in
                // a register, `&` for `&&` - were built and measured: the same compiler then sinks NN_PRODUCTS' loads of k-step
                // ks + 1 behind the MFMAs of ks, and the pass takes 50 % longer.
                const bool rok = lok[nn_acc_row(mb, r, half)];
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    const float s = acc[mb][nb][r] * a.scale;
                    // lab = -1 fails >= 0; a NaN fails >=
                    const bool v = rok && lab[nb] >= 0 && (!SELF || own[nb] != nn_acc_row(mb, r, 0)) && s >= a.threshold;
                    vote |= (unsigned long long)v << ((mb * 2 + nb) * 16 + r);
                }
            }
        if (__ballot(vote != 0) == 0) continue;                // wave-uniform, and no barrier follows in the loop
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = nn_acc_row(mb, r, half);
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    if (!((vote >> ((mb * 2 + nb) * 16 + r)) & 1)) continue;
                    const float s = acc[mb][nb][r] * a.scale;
                    const unsigned long long w = (unsigned long long)llrint((double)s * 4294967296.0);
                    const unsigned long long key = nn_key(nn_image(s), (unsigned)cg[nb]);
                    if (LDS) {
                        const int o = row * LDS_C + lab[nb];
                        atomicAdd(&lc[o], 1u);
                        atomicAdd(&lw[o], w);
                        atomicMax(&lk[o], key);
                    } else {
                        const int64_t o = (r0 + row) * a.n_classes + lab[nb];
                        atomicAdd(a.cnt + o, 1ull);
                        atomicAdd(a.wgt + o, w);
                        atomicMax(a.key + o, key);
                    }
                }
            }
    }
    if (LDS) {
        __syncthreads();
        // a cell is not empty only at a valid row < nq and a class < n_classes.  Ends: i grows by 256 towards 1024.
        for (int i = tid; i < QT * LDS_C; i += 256) {
            if (!lc[i]) continue;
            const int64_t o = (r0 + i / LDS_C) * a.n_classes + i % LDS_C;
            atomicAdd(a.cnt + o, (unsigned long long)lc[i]);
            atomicAdd(a.wgt + o, lw[i]);
            atomicMax(a.key + o, lk[i]);
        }
    }
}

__global__ __launch_bounds__(256) void vt_finish_kernel(int64_t cells, const unsigned long long* __restrict__ key, int64_t* __restrict__ nearest,
                                                        float* __restrict__ nearest_sim) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= cells) return;
    const unsigned long long b = key[i];
    nearest[i] = b ? (int64_t)nn_key_index(b) : -1;
    nearest_sim[i] = b ? nn_unimage((unsigned)(b >> 32)) : __builtin_nanf("");
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

int check_vote_args(const char* fn, const void* query, int64_t nq, const void* base, int64_t nb, const void* label, int n_classes,
                    float threshold, const void* count, const void* weight, const void* nearest, const void* nearest_sim) {
    const std::string f(fn);
    const bool self = !base;
    if (int rc = nn_check_rows(f, nq, "n_query")) return rc;
    const int64_t rows = self ? nq : nb;
    if (rows < 0 || rows > N_MAX) {
        set_error(f + ": " + std::to_string(rows) + " base rows is outside [0, 2^30]: the int64 sums of more rows could overflow");
        return GNN_ERR_ARG;
    }
    if (n_classes < 1 || n_classes > C_MAX) {
        set_error(f + ": n_classes " + std::to_string(n_classes) + " is outside [1, " + std::to_string(C_MAX) + "]");
        return GNN_ERR_ARG;
    }
    if (int rc = nn_check_threshold(f, threshold)) return rc;
    return nn_check_required(f, (rows == 0 || label) && (nq == 0 || (query && count && weight && nearest && nearest_sim)),
                             "the query, the labels and the four outputs");
}

// The votes over a base on the device, the queries in slabs of QSLAB rows.  self: the query fragments are the base's own.  Otherwise
// the query rows are on the device (query_dev) or go up slab by slab (query_host).  to_host: the four outputs are host pointers; every
// slab lands in the ctx's buffer, is copied out and waited for.  The ctx's stream is synchronised once before the first slab: the
// labels' verdict.
int vt_run(gnn_ctx* ctx, const char* fn, const float* query_dev, const float* query_host, int64_t nq, const float* base_dev, int64_t nb,
           bool self, const int64_t* label_dev, int n_classes, float threshold, int64_t* count, int64_t* weight, int64_t* nearest,
           float* nearest_sim, bool to_host) {
    NeighbourWorkspace& w = ctx->nn;
    VoteWorkspace& v = ctx->vt;
    v.passes.begin();
    const int64_t padded = round_up(nb, QT);
    int rc = nn_prepare(ctx, base_dev, nb, GNN_KNN_COSINE, w.bfrag, w.bvalid);
    if (!rc) rc = nn_reserve(ctx, v.blabel, (size_t)std::max<int64_t>(padded, 1));
    if (!rc) rc = v.flag.reserve(ctx, 1);
    if (rc) return rc;
    if (nb > 0) {
        {
            PassLog::Scope pass(ctx, v.passes);
            if ((rc = v.flag.zero(ctx, 0, 1))) return rc;
            if ((rc = launch_1d(vt_label_kernel, padded, ctx->stream, nb, padded, n_classes, label_dev, w.bvalid.get(), v.blabel.get(),
                                v.flag.dev())))
                return rc;
        }
        unsigned long long bad = 0;
        if ((rc = v.flag.read(ctx, 0, 1, &bad))) return rc;
        v.passes.settle();
        if (bad) {
            set_error(std::string(fn) + ": a label is outside [-1, " + std::to_string(n_classes) + ")");
            return GNN_ERR_ARG;
        }
    }
    // Ends: q0 grows by QSLAB towards nq.
    for (int64_t q0 = 0; q0 < nq; q0 += QSLAB) {
        const int64_t m = std::min(QSLAB, nq - q0);
        const int64_t cells = m * n_classes;
        const uint4* qfrag = w.bfrag.get() + q0 / 32 * BLK_U4;
        const uint8_t* qvalid = w.bvalid.get() + q0;
        if (!self) {
            const float* rows = query_dev ? query_dev + q0 * D : nullptr;
            if (query_host) {
                if ((rc = nn_reserve(ctx, w.d_query, (size_t)m * D))) return rc;
                GNN_HIP(hipMemcpyAsync(w.d_query, query_host + q0 * D, (size_t)m * D * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
                rows = w.d_query;
            }
            if ((rc = nn_prepare(ctx, rows, m, GNN_KNN_COSINE, w.qfrag, w.qvalid))) return rc;
            qfrag = w.qfrag;
            qvalid = w.qvalid;
        }
        if ((rc = nn_reserve(ctx, v.key, (size_t)cells))) return rc;
        unsigned long long* cnt_dev = reinterpret_cast<unsigned long long*>(count + q0 * n_classes);
        unsigned long long* wgt_dev = reinterpret_cast<unsigned long long*>(weight + q0 * n_classes);
        int64_t* near_dev = nearest + q0 * n_classes;
        float* nsim_dev = nearest_sim + q0 * n_classes;
        Landing land(v.d_out);
        if (to_host) {
            const int c = land.add(count + q0 * n_classes, cells), g = land.add(weight + q0 * n_classes, cells), nr = land.add(near_dev, cells),
                      ns = land.add(nsim_dev, cells);
            if ((rc = land.reserve(ctx))) return rc;
            cnt_dev = land.dev<unsigned long long>(c);
            wgt_dev = land.dev<unsigned long long>(g);
            near_dev = land.dev<int64_t>(nr);
            nsim_dev = land.dev<float>(ns);
        }
        const int64_t tiles = (m + QT - 1) / QT;
        int64_t split_rows, splits;
        if ((rc = nn_tile_grid(ctx, fn, "base rows", tiles, nb, &split_rows, &splits))) return rc;
        {
            PassLog::Scope pass(ctx, v.passes);
            GNN_HIP(hipMemsetAsync(cnt_dev, 0, (size_t)cells * sizeof(unsigned long long), ctx->stream));
            GNN_HIP(hipMemsetAsync(wgt_dev, 0, (size_t)cells * sizeof(unsigned long long), ctx->stream));
            GNN_HIP(hipMemsetAsync(v.key.get(), 0, (size_t)cells * sizeof(unsigned long long), ctx->stream));
            if (splits > 0) {
                VoteArgs a;
                a.qfrag = qfrag;
                a.qvalid = qvalid;
                a.nq = m;
                a.bfrag = w.bfrag.get();
                a.blabel = v.blabel.get();
                a.nb = nb;
                a.split_rows = split_rows;
                a.n_classes = n_classes;
                a.scale = nn_metric_scale(GNN_KNN_COSINE);
                a.threshold = threshold;
                a.self_off = self ? q0 : -1;
                a.cnt = cnt_dev;
                a.wgt = wgt_dev;
                a.key = v.key.get();
                void (*const kernel)(VoteArgs) = n_classes <= v.lds_c ? (self ? vt_tile_kernel<true, true> : vt_tile_kernel<true, false>)
                                                                       : (self ? vt_tile_kernel<false, true> : vt_tile_kernel<false, false>);
                if ((rc = launch_tiles(kernel, tiles, splits, ctx->stream, a))) return rc;
            }
        }
        {
            PassLog::Scope pass(ctx, v.passes);
            if ((rc = launch_1d(vt_finish_kernel, cells, ctx->stream, cells, v.key.get(), near_dev, nsim_dev))) return rc;
        }
        if (to_host) {
            if ((rc = land.copy_out(ctx))) return rc;         // synchronised: the landing buffer and d_query serve the next slab
            v.passes.settle();
        }
    }
    return GNN_OK;
}

}  // namespace
}  // namespace gnn

using namespace gnn;

extern "C" int gnn_vote_dev(gnn_ctx* ctx, const float* query_dev, int64_t n_query, const float* base_dev_or_null, int64_t n_base,
                            const int64_t* label_dev, int n_classes, float threshold, int64_t* count_dev, int64_t* weight_dev,
                            int64_t* nearest_dev, float* nearest_sim_dev) {
    const char* const fn = "gnn_vote_dev";
    const bool self = !base_dev_or_null;
    if (int rc = check_vote_args(fn, query_dev, n_query, base_dev_or_null, n_base, label_dev, n_classes, threshold, count_dev, weight_dev,
                                 nearest_dev, nearest_sim_dev))
        return rc;
    if (int rc = check_ctx(ctx)) return rc;
    return vt_run(ctx, fn, query_dev, nullptr, n_query, self ? query_dev : base_dev_or_null, self ? n_query : n_base, self, label_dev, n_classes,
                  threshold, count_dev, weight_dev, nearest_dev, nearest_sim_dev, false);
}

extern "C" int gnn_vote(gnn_ctx* ctx, const float* query_host, int64_t n_query, const float* base_host_or_null, int64_t n_base,
                        const int64_t* label_host, int n_classes, float threshold, int64_t* count_host, int64_t* weight_host,
                        int64_t* nearest_host, float* nearest_sim_host) {
    const char* const fn = "gnn_vote";
    const bool self = !base_host_or_null;
    if (int rc = check_vote_args(fn, query_host, n_query, base_host_or_null, n_base, label_host, n_classes, threshold, count_host, weight_host,
                                 nearest_host, nearest_sim_host))
        return rc;
    if (int rc = check_ctx(ctx)) return rc;
    const int64_t nb = self ? n_query : n_base;
    // every buffer stands before a copy is enqueued.  The base goes up once, with its labels; the queries follow slab by slab
    int rc = nn_reserve(ctx, ctx->vt.d_label, (size_t)std::max<int64_t>(nb, 1));
    if (!rc) rc = nn_upload_rows(ctx, self ? query_host : base_host_or_null, nb);
    if (rc) return rc;
    if (nb > 0)
        GNN_HIP(hipMemcpyAsync(ctx->vt.d_label.get(), label_host, (size_t)nb * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    return vt_run(ctx, fn, nullptr, self ? nullptr : query_host, n_query, ctx->nn.d_base, nb, self, ctx->vt.d_label.get(), n_classes, threshold,
                  count_host, weight_host, nearest_host, nearest_sim_host, true);
}

extern "C" int gnn_debug_set_vote_lds(gnn_ctx* ctx, int max_classes) {
    if (int rc = check_ctx(ctx)) return rc;
    if (max_classes < 0 || max_classes > LDS_C) {
        set_error("gnn_debug_set_vote_lds: " + std::to_string(max_classes) + " classes is outside [0, " + std::to_string(LDS_C) +
                  "] (0 = every vote straight to memory)");
        return GNN_ERR_ARG;
    }
    ctx->vt.lds_c = max_classes;
    return GNN_OK;
}

extern "C" int gnn_debug_vote_pass_ms(gnn_ctx* ctx, double* ms_out, int64_t capacity, int64_t* n_out) {
    if (int rc = check_ctx(ctx)) return rc;
    return ctx->vt.passes.out(ctx, "gnn_debug_vote_pass_ms", ms_out, capacity, n_out);
}
