// Density clusters among encoder embeddings (include/genomad_nn.h, "density clusters"): DBSCAN at one
// (threshold, min_points) on the graph of gnn_clusters.hip - an edge {i, j} iff both rows are valid and sim(i, j) >= threshold.  A valid
// row is CORE when its degree + 1 >= min_points; clusters are the components of the core rows under core-core edges; a valid row that
// is not core but has a core neighbour is a BORDER row of the most similar one (ties to the smaller index); the rest is NOISE.
//   prepare    nn_prepare (gnn_neighbours.hip), as it is: the neighbour search's fragments and flags, in its buffers.
//   init       parent[i] = i, degree = size = key = 0, the (tile, range) flags cleared.
//   count      the tile parts of gnn_nn_frag.h over the UPPER TRIANGLE, the edge mask and the ballot degree counts of cl_tile_kernel,
//              without its joins.  A workgroup that saw an edge says so in its own flag[tile * splits + range]: one owner, a plain
//              store.  A workgroup that leaves early stores nothing.
//   mark       core[i] = valid[i] && degree[i] + 1 >= min_points, one byte per row, padded to the 64-row tile like `valid`.
//   link       a workgroup whose flag is clear leaves before it loads its tile.  Otherwise: the same products, the same edge mask - the
//              value of the pair i < j is the f32 that gnn_neighbours returns for query i and base row j, (j, i) is never computed.
//              Both ends core: cl_join.  One end core: the other row's key takes nn_key(nn_image(s), the core row) by a 64-bit
//              maximum - the largest similarity, among equals the smallest core row.  No end core: nothing.
//   flatten    a launch of its own behind the link pass.  Core: label = its root.  A row with a key: anchor = the key's row, label =
//              the anchor's root, sim = the key's similarity.  Noise and invalid rows: -1.  Every labelled row counts at size[label].
//   summarise  every labelled row takes size[label]; degree goes out.
// Only integer adds, integer maxima and cl_join's compare-and-swap: nothing depends on the order the workgroups run in or on the split
// of the base.  The border rule looks at ALL core neighbours of a row, not at the first cluster that reaches it: unlike textbook
// DBSCAN there is no visiting order to depend on.  No loop here waits for another workgroup: every loop's termination argument stands
// next to it.  Memory: 21 B per row and one byte per (row tile, base range); nothing is n x n and no edge list is kept.
#include <cmath>

#include "gnn_nn_frag.h"

namespace gnn {
namespace {

constexpr int64_t N_MAX = (int64_t)1 << 31;      // rows are int32 in parent[]

enum : uint8_t { KIND_INVALID = 0, KIND_NOISE = 1, KIND_BORDER = 2, KIND_CORE = 3 };

__global__ __launch_bounds__(256) void dn_init_kernel(int64_t n, int64_t flags, int32_t* __restrict__ parent, int32_t* __restrict__ degree,
                                                      int32_t* __restrict__ size, unsigned long long* __restrict__ key,
                                                      uint8_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < flags) flag[i] = 0;
    if (i >= n) return;
    parent[i] = (int32_t)i;
    degree[i] = 0;
    size[i] = 0;
    key[i] = 0;
}

struct DensityArgs {
    const uint4* frag;         // round_up(n, 64) / 32 blocks: rows and columns alike
    const uint8_t* valid;      // [round_up(n, 64)]
    const uint8_t* core;       // [round_up(n, 64)]; the link pass
    int64_t n;
    int64_t split_rows;        // base rows per workgroup: a multiple of 32
    int64_t splits;
    float scale;               // 2^-16 for cosine, 1 for dot
    float threshold;
    int32_t* parent;
    int32_t* degree;
    unsigned long long* key;   // at a row that is not core: max of (image of the similarity << 32) | (2^32 - 1 - core neighbour), 0: none
    uint8_t* flag;             // [tiles * splits]: the workgroup saw an edge
};

// The edges of a step, bit (mb * 2 + nb) * 16 + reg: both rows valid, row < col < b1, s >= threshold.  cg = -1 fails rg < cg; a NaN
// fails >=.  A macro for NN_PRODUCTS' reason: the loop is compiled where it stands, in both kernels alike.
#define DN_EDGES(acc, lok, r0, cg, lane, a, edge)                                                                              \
    do {                                                                                                                       \
        _Pragma("unroll") for (int mb_ = 0; mb_ < 2; ++mb_)                                                                    \
            _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) {                                                                \
                const int row_ = nn_acc_row(mb_, r_, lane >> 5);                                                               \
                const int rg_ = (int)r0 + row_;                                                                                \
                const bool rok_ = lok[row_];                                                                                   \
                _Pragma("unroll") for (int nb_ = 0; nb_ < 2; ++nb_) {                                                          \
                    const float s_ = acc[mb_][nb_][r_] * a.scale;                                                              \
                    const bool e_ = rok_ && rg_ < cg[nb_] && s_ >= a.threshold;                                                \
                    edge |= (unsigned long long)e_ << ((mb_ * 2 + nb_) * 16 + r_);                                             \
                }                                                                                                              \
            }                                                                                                                  \
    } while (0)

// grid = (row tiles, base ranges), 256 threads.  LDS: the tile's fragments 128 KB, its rows' edge counts and flags.
__global__ __launch_bounds__(256) void dn_count_kernel(DensityArgs a) {
    __shared__ uint4 qs[2 * BLK_U4];
    __shared__ int ldeg[QT];               // edges of this workgroup's columns at the tile's rows: flushed once
    __shared__ uint8_t lok[QT];
    __shared__ int lany;                   // a wave of this workgroup saw an edge
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    TileRange t;
    if (!nn_tile_range(t, a.split_rows, a.n, true)) return;
    const int64_t r0 = t.r0;
    nn_copy_tile(qs, a.frag, tid);
    if (tid < QT) {
        ldeg[tid] = 0;
        lok[tid] = r0 + tid < a.n && a.valid[r0 + tid];
    }
    if (tid == 0) lany = 0;
    __syncthreads();
    const int64_t last_blk = t.last_blk();
    // Ends: c0 grows by STEP towards b1.
    for (int64_t c0 = t.c0; c0 < t.b1; c0 += STEP) {
        const uint4* bp[2];
        int cg[2];                         // the lane's column, -1: no edge can end there
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const int64_t col = nn_step_column(a.frag, c0, wave, lane, nb, last_blk, bp[nb]);
            cg[nb] = col < t.b1 && a.valid[col] ? (int)col : -1;
        }
        f32x16 acc[2][2];
        NN_PRODUCTS(qs, bp, lane, acc);
        unsigned long long edge = 0;
        DN_EDGES(acc, lok, r0, cg, lane, a, edge);
        if (__ballot(edge != 0) == 0) continue;            // wave-uniform, and no barrier follows in the loop
        if (lane == 0) lany = 1;                           // every writer writes the same value
        // ---- degrees, as cl_tile_kernel counts them: a ballot per register and half, one LDS add per row; one global add per column
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const unsigned long long e0 = __ballot((edge >> (mb * 32 + r)) & 1), e1 = __ballot((edge >> (mb * 32 + 16 + r)) & 1);
                const int half = lane >> 5;
                const int c = __popc((unsigned)(e0 >> (32 * half))) + __popc((unsigned)(e1 >> (32 * half)));
                if ((lane & 31) == 0 && c) atomicAdd(&ldeg[nn_acc_row(mb, r, half)], c);
            }
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            int c = __popc((unsigned)(edge >> (nb * 16)) & 0xffffu) + __popc((unsigned)(edge >> (32 + nb * 16)) & 0xffffu);
            c += __shfl_xor(c, 32);
            if (lane < 32 && c) atomicAdd(a.degree + cg[nb], c);               // c > 0 only where cg >= 0
        }
    }
    __syncthreads();
    if (tid < QT && ldeg[tid]) atomicAdd(a.degree + r0 + tid, ldeg[tid]);       // ldeg > 0 only at a valid row < n
    if (tid == 0 && lany) a.flag[(int64_t)blockIdx.x * a.splits + blockIdx.y] = 1;
}

// i < padded = round_up(n, 64)
__global__ __launch_bounds__(256) void dn_mark_kernel(int64_t n, int64_t padded, int64_t min_points, const uint8_t* __restrict__ valid,
                                                      const int32_t* __restrict__ degree, uint8_t* __restrict__ core) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= padded) return;
    core[i] = i < n && valid[i] && (int64_t)degree[i] + 1 >= min_points;
}

// grid = (row tiles, base ranges), 256 threads.  LDS: the tile's fragments 128 KB, its rows' flags and keys.
__global__ __launch_bounds__(256) void dn_link_kernel(DensityArgs a) {
    __shared__ uint4 qs[2 * BLK_U4];
    __shared__ unsigned long long lkey[QT];    // the best core neighbours of the tile's rows among this workgroup's columns: flushed once
    __shared__ uint8_t lok[QT], lcore[QT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
    TileRange t;
    if (!nn_tile_range(t, a.split_rows, a.n, true)) return;
    // the count pass saw no edge here (the same byte in every thread: the whole workgroup leaves, before it loads fragments)
    if (!a.flag[(int64_t)blockIdx.x * a.splits + blockIdx.y]) return;
    const int64_t r0 = t.r0;
    nn_copy_tile(qs, a.frag, tid);
    if (tid < QT) {
        lkey[tid] = 0;
        lok[tid] = r0 + tid < a.n && a.valid[r0 + tid];
        lcore[tid] = a.core[r0 + tid];                     // padded to the tile
    }
    __syncthreads();
    // the lane's core rows in the layout of the edge mask: bit (mb * 2 + nb) * 16 + reg
    unsigned long long rcore = 0;
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (lcore[nn_acc_row(mb, r, half)]) rcore |= 0x00010001ull << (mb * 32 + r);
    const int64_t last_blk = t.last_blk();
    // Ends: c0 grows by STEP towards b1.
    for (int64_t c0 = t.c0; c0 < t.b1; c0 += STEP) {
        const uint4* bp[2];
        int cg[2];                         // the lane's column, -1: no edge can end there
        unsigned long long ccore = 0;      // the lane's core columns in the layout of the edge mask
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const int64_t col = nn_step_column(a.frag, c0, wave, lane, nb, last_blk, bp[nb]);
            cg[nb] = col < t.b1 && a.valid[col] ? (int)col : -1;
            if (cg[nb] >= 0 && a.core[col]) ccore |= 0x0000ffff0000ffffull << (nb * 16);
        }
        f32x16 acc[2][2];
        NN_PRODUCTS(qs, bp, lane, acc);
        unsigned long long edge = 0;
        DN_EDGES(acc, lok, r0, cg, lane, a, edge);
        if (__ballot(edge != 0) == 0) continue;            // wave-uniform, and no barrier follows in the loop
        unsigned long long join = edge & rcore & ccore;    // both ends core
        const unsigned long long to_row = edge & ~rcore & ccore, to_col = edge & rcore & ~ccore;      // exactly one end core
        // ---- a row that is not core, its core columns: a row's candidates lie in one register of the 32 lanes of a half
        if (__ballot(to_row != 0)) {
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    unsigned long long key = 0;
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb)
                        if ((to_row >> ((mb * 2 + nb) * 16 + r)) & 1) {
                            const unsigned long long k = nn_key(nn_image(acc[mb][nb][r] * a.scale), (unsigned)cg[nb]);
                            key = k > key ? k : key;
                        }
                    if (__ballot(key != 0) == 0) continue;         // wave-uniform: the shuffles below run in every lane
#pragma unroll
                    for (int s = 16; s > 0; s >>= 1) {
                        const unsigned long long other = __shfl_xor(key, s);
                        key = other > key ? other : key;
                    }
                    if ((lane & 31) == 0 && key) atomicMax(&lkey[nn_acc_row(mb, r, half)], key);
                }
        }
        // ---- a column that is not core, its core rows: a column is one lane's in all its registers and the other half's
        if (__ballot(to_col != 0)) {
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                unsigned long long key = 0;
#pragma unroll
                for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if ((to_col >> ((mb * 2 + nb) * 16 + r)) & 1) {
                            const unsigned long long k =
                                nn_key(nn_image(acc[mb][nb][r] * a.scale), (unsigned)((int)r0 + nn_acc_row(mb, r, half)));
                            key = k > key ? k : key;
                        }
                const unsigned long long other = __shfl_xor(key, 32);
                key = other > key ? other : key;
                if (lane < 32 && key) atomicMax(a.key + cg[nb], key);          // key > 0 only where cg >= 0
            }
        }
        // ---- joins, edge by edge.  Ends: every pass clears the lowest set bit of `join`; cl_join ends by its own argument
        int top[2] = {cg[0], cg[1]};       // a member of the column's tree, as low as this lane has seen
        while (join) {
            const int b = __ffsll((long long)join) - 1;
            join &= join - 1;
            const int r = b & 15, nb = (b >> 4) & 1, mb = b >> 5;
            const int rg = (int)r0 + nn_acc_row(mb, r, half);
            const int j = cl_join(a.parent, rg, nb ? top[1] : top[0]);
            if (nb) top[1] = j; else top[0] = j;
        }
    }
    __syncthreads();
    if (tid < QT && lkey[tid]) atomicMax(a.key + r0 + tid, lkey[tid]);          // lkey > 0 only at a valid row < n that is not core
}

// A launch of its own behind the link pass: nn_root's plain loads see every link, and every key is final.
__global__ __launch_bounds__(256) void dn_flatten_kernel(int64_t n, const uint8_t* __restrict__ valid, const uint8_t* __restrict__ core,
                                                         const int32_t* __restrict__ parent, const unsigned long long* __restrict__ key,
                                                         int32_t* __restrict__ size, int64_t* __restrict__ label,
                                                         int64_t* __restrict__ anchor, float* __restrict__ sim, uint8_t* __restrict__ kind) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int64_t l = -1, an = -1;
    float s = __builtin_nanf("");
    uint8_t k = KIND_INVALID;
    if (valid[i]) {
        const unsigned long long best = key[i];
        if (core[i]) {
            k = KIND_CORE;
            an = i;
            l = nn_root(parent, (int)i);
        } else if (best) {
            k = KIND_BORDER;
            an = (int64_t)nn_key_index(best);
            l = nn_root(parent, (int)an);
            s = nn_unimage((unsigned)(best >> 32));
        } else {
            k = KIND_NOISE;
        }
    }
    label[i] = l;
    anchor[i] = an;
    sim[i] = s;
    kind[i] = k;
    if (l >= 0) atomicAdd(size + l, 1);
}

__global__ __launch_bounds__(256) void dn_summarise_kernel(int64_t n, const uint8_t* __restrict__ valid, const int32_t* __restrict__ degree,
                                                           const int32_t* __restrict__ size, const int64_t* __restrict__ label,
                                                           int64_t* __restrict__ degree_out, int64_t* __restrict__ size_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t l = label[i];
    degree_out[i] = valid[i] ? degree[i] : 0;
    size_out[i] = l >= 0 ? size[l] : 0;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

int check_density_args(const char* fn, const void* rows, int64_t n, float threshold, int64_t min_points, int metric, const void* label,
                       const void* degree, const void* size, const void* anchor, const void* sim, const void* kind) {
    const std::string f(fn);
    if (int rc = nn_check_rows(f, n, "rows")) return rc;
    if (int rc = nn_check_threshold(f, threshold)) return rc;
    if (min_points < 1 || min_points >= N_MAX) {
        set_error(f + ": min_points " + std::to_string(min_points) + " is outside [1, 2^31)");
        return GNN_ERR_ARG;
    }
    if (int rc = nn_check_metric(f, metric)) return rc;
    return nn_check_required(f, n == 0 || (rows && label && degree && size && anchor && sim && kind), "the rows and the six outputs");
}

// n > 0 rows on the device -> the six arrays on the device, enqueued on the ctx's stream
int dn_run(gnn_ctx* ctx, const char* fn, const float* rows_dev, int64_t n, float threshold, int64_t min_points, int metric, int64_t* label,
           int64_t* degree, int64_t* size, int64_t* anchor, float* sim, uint8_t* kind) {
    NeighbourWorkspace& w = ctx->nn;
    DensityWorkspace& d = ctx->dn;
    const int64_t tiles = (n + QT - 1) / QT, padded = tiles * QT;
    int rc = nn_prepare(ctx, rows_dev, n, metric, w.bfrag, w.bvalid);
    if (!rc) rc = nn_reserve(ctx, d.parent, (size_t)n);
    if (!rc) rc = nn_reserve(ctx, d.degree, (size_t)n);
    if (!rc) rc = nn_reserve(ctx, d.size, (size_t)n);
    if (!rc) rc = nn_reserve(ctx, d.key, (size_t)n);
    if (!rc) rc = nn_reserve(ctx, d.core, (size_t)padded);
    int64_t split_rows, splits;
    if (!rc) rc = nn_tile_grid(ctx, fn, "rows", tiles, n, &split_rows, &splits);
    const int64_t flags = rc ? 0 : tiles * splits;
    if (!rc) rc = nn_reserve(ctx, d.flag, (size_t)flags);
    if (rc) return rc;
    ProfScope prof(ctx, GNN_K_NEIGHBOURS);
    if ((rc = launch_1d(dn_init_kernel, std::max(n, flags), ctx->stream, n, flags, d.parent, d.degree, d.size, d.key, d.flag))) return rc;
    DensityArgs a;
    a.frag = w.bfrag.get();
    a.valid = w.bvalid.get();
    a.core = d.core.get();
    a.n = n;
    a.split_rows = split_rows;
    a.splits = splits;
    a.scale = nn_metric_scale(metric);
    a.threshold = threshold;
    a.parent = d.parent.get();
    a.degree = d.degree.get();
    a.key = d.key.get();
    a.flag = d.flag.get();
    if ((rc = launch_tiles(dn_count_kernel, tiles, splits, ctx->stream, a))) return rc;
    if ((rc = launch_1d(dn_mark_kernel, padded, ctx->stream, n, padded, min_points, w.bvalid, d.degree, d.core))) return rc;
    if ((rc = launch_tiles(dn_link_kernel, tiles, splits, ctx->stream, a))) return rc;
    if ((rc = launch_1d(dn_flatten_kernel, n, ctx->stream, n, w.bvalid, d.core, d.parent, d.key, d.size, label, anchor, sim, kind))) return rc;
    return launch_1d(dn_summarise_kernel, n, ctx->stream, n, w.bvalid, d.degree, d.size, label, degree, size);
}

}  // namespace
}  // namespace gnn

using namespace gnn;

extern "C" int gnn_density_dev(gnn_ctx* ctx, const float* rows_dev, int64_t n, float threshold, int64_t min_points, int metric,
                               int64_t* label_dev, int64_t* degree_dev, int64_t* size_dev, int64_t* anchor_dev, float* sim_dev,
                               uint8_t* kind_dev) {
    if (int rc = check_density_args("gnn_density_dev", rows_dev, n, threshold, min_points, metric, label_dev, degree_dev, size_dev, anchor_dev,
                                    sim_dev, kind_dev))
        return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (n == 0) return GNN_OK;
    return dn_run(ctx, "gnn_density_dev", rows_dev, n, threshold, min_points, metric, label_dev, degree_dev, size_dev, anchor_dev, sim_dev,
                  kind_dev);
}

extern "C" int gnn_density(gnn_ctx* ctx, const float* rows_host, int64_t n, float threshold, int64_t min_points, int metric,
                           int64_t* label_host, int64_t* degree_host, int64_t* size_host, int64_t* anchor_host, float* sim_host,
                           uint8_t* kind_host) {
    if (int rc = check_density_args("gnn_density", rows_host, n, threshold, min_points, metric, label_host, degree_host, size_host, anchor_host,
                                    sim_host, kind_host))
        return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (n == 0) return GNN_OK;
    NeighbourWorkspace& w = ctx->nn;
    DensityWorkspace& d = ctx->dn;
    Landing land(d.d_out);
    const int label = land.add(label_host, n), degree = land.add(degree_host, n), size = land.add(size_host, n), anchor = land.add(anchor_host, n),
              sim = land.add(sim_host, n), kind = land.add(kind_host, n);
    int rc = land.reserve(ctx);                               // both buffers stand before the copy is enqueued
    if (!rc) rc = nn_upload_rows(ctx, rows_host, n);
    if (!rc)
        rc = dn_run(ctx, "gnn_density", w.d_base, n, threshold, min_points, metric, land.dev<int64_t>(label), land.dev<int64_t>(degree),
                    land.dev<int64_t>(size), land.dev<int64_t>(anchor), land.dev<float>(sim), land.dev<uint8_t>(kind));
    return rc ? rc : land.copy_out(ctx);
}
