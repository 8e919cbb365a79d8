// Clusters among encoder embeddings (include/genomad_nn.h, "clusters"): the connected components of the graph
// with an edge {i, j} iff both rows are valid and sim(i, j) >= threshold - single linkage at the threshold, exact, five kernels.
//   prepare    nn_prepare (gnn_neighbours.hip), as it is: the neighbour search's fragments and flags, in its buffers.
//   init       parent[i] = i, degree = size = key = 0.
//   tile       the tile parts of gnn_nn_frag.h - 64 rows' fragments in LDS, the base streamed in steps of 256 columns, NN_PRODUCTS'
//              three products per k-step in their order, the same scale - over the UPPER TRIANGLE only.  The value of the pair {i, j},
//              i < j, is the f32 that gnn_neighbours returns for query i and base row j; (j, i) is never computed: hi.lo then lo.hi is
//              not symmetric in the last bit.  Behind every step, for every value with row < col, both rows valid and s >= threshold
//              (false for a NaN): the edge is counted at both ends and the two rows are joined.  No lists, no barrier per step.
//   flatten    label = the root of the row's tree; the root gathers the tree's size and the key of its representative.
//   summarise  every valid row takes its root's size and representative; an invalid row is -1 / 0 / 0 / -1.
// Union-find (cl_peek and cl_join of gnn_nn_frag.h, shared with gnn_linkage.hip): parent[] is int32 in global memory and a link
// always points to the SMALLER index, so a tree's root is its smallest member and the label needs no tie rule.  parent[x] is x until
// one compare-and-swap replaces it by something smaller, and never changes again.  Degrees and sizes are integer adds, the key an
// integer max: nothing depends on the order the workgroups run in or on the split of the base.  No loop here waits for another
// workgroup: every loop's termination argument stands next to it.
#include <cmath>

#include "gnn_nn_frag.h"

namespace gnn {
namespace {


__global__ __launch_bounds__(256) void cl_init_kernel(int64_t n, int32_t* __restrict__ parent, int32_t* __restrict__ degree,
                                                      int32_t* __restrict__ size, unsigned long long* __restrict__ key) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    parent[i] = (int32_t)i;
    degree[i] = 0;
    size[i] = 0;
    key[i] = 0;
}

struct ClusterArgs {
    const uint4* frag;         // round_up(n, 64) / 32 blocks: rows and columns alike
    const uint8_t* valid;      // [round_up(n, 64)]
    int64_t n;
    int64_t split_rows;        // base rows per workgroup: a multiple of 32
    float scale;               // 2^-16 for cosine, 1 for dot
    float threshold;
    int32_t* parent;
    int32_t* degree;
};

// grid = (row tiles, base ranges), 256 threads.  LDS: the tile's fragments 128 KB, its rows' edge counts and flags.
__global__ __launch_bounds__(256) void cl_tile_kernel(ClusterArgs a) {
    __shared__ uint4 qs[2 * BLK_U4];
    __shared__ int ldeg[QT];               // edges of this workgroup's columns at the tile's rows: flushed once
    __shared__ uint8_t lok[QT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    TileRange t;
    if (!nn_tile_range(t, a.split_rows, a.n, true)) return;
    const int64_t r0 = t.r0;
    nn_copy_tile(qs, a.frag, tid);
    if (tid < QT) {
        ldeg[tid] = 0;
        lok[tid] = r0 + tid < a.n && a.valid[r0 + tid];
    }
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
        // ---- edges: bit (mb * 2 + nb) * 16 + reg
        unsigned long long edge = 0;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = nn_acc_row(mb, r, lane >> 5);
                const int rg = (int)r0 + row;
                const bool rok = lok[row];
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    const float s = acc[mb][nb][r] * a.scale;
                    const bool e = rok && rg < cg[nb] && s >= a.threshold;          // cg = -1 fails rg < cg; a NaN fails >=
                    edge |= (unsigned long long)e << ((mb * 2 + nb) * 16 + r);
                }
            }
        if (__ballot(edge != 0) == 0) continue;            // wave-uniform, and no barrier follows in the loop
        // ---- degrees.  A row's edges of this step lie in one register of 32 lanes per column block: a ballot counts them, one lane
        // per half adds them in LDS.  A column is one lane's in all its registers and the other half's: one add per column and step
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
        // ---- joins, edge by edge.  Ends: every pass clears the lowest set bit of `edge`; cl_join ends by its own argument
        int top[2] = {cg[0], cg[1]};       // a member of the column's tree, as low as this lane has seen
        while (edge) {
            const int b = __ffsll((long long)edge) - 1;
            edge &= edge - 1;
            const int r = b & 15, nb = (b >> 4) & 1, mb = b >> 5;
            const int rg = (int)r0 + nn_acc_row(mb, r, lane >> 5);
            const int t = cl_join(a.parent, rg, nb ? top[1] : top[0]);
            if (nb) top[1] = t; else top[0] = t;
        }
    }
    __syncthreads();
    if (tid < QT && ldeg[tid]) atomicAdd(a.degree + r0 + tid, ldeg[tid]);       // ldeg > 0 only at a valid row < n
}

// A launch of its own behind the tile kernel: nn_root's plain loads see every link.
__global__ __launch_bounds__(256) void cl_flatten_kernel(int64_t n, const uint8_t* __restrict__ valid, const int32_t* __restrict__ parent,
                                                         const int32_t* __restrict__ degree, int32_t* __restrict__ size,
                                                         unsigned long long* __restrict__ key, int64_t* __restrict__ label) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (!valid[i]) {
        label[i] = -1;
        return;
    }
    const int r = nn_root(parent, (int)i);
    label[i] = r;
    atomicAdd(size + r, 1);
    // the largest degree wins, among equals the smallest row
    atomicMax(key + r, nn_key((unsigned)degree[i], (unsigned)i));
}

__global__ __launch_bounds__(256) void cl_summarise_kernel(int64_t n, const uint8_t* __restrict__ valid, const int32_t* __restrict__ degree,
                                                           const int32_t* __restrict__ size, const unsigned long long* __restrict__ key,
                                                           const int64_t* __restrict__ label, int64_t* __restrict__ degree_out,
                                                           int64_t* __restrict__ size_out, int64_t* __restrict__ rep_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (!valid[i]) {
        degree_out[i] = 0;
        size_out[i] = 0;
        rep_out[i] = -1;
        return;
    }
    const int64_t r = label[i];
    degree_out[i] = degree[i];
    size_out[i] = size[r];
    rep_out[i] = (int64_t)nn_key_index(key[r]);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

int check_cluster_args(const char* fn, const void* rows, int64_t n, float threshold, int metric, const void* label, const void* degree,
                       const void* size, const void* rep) {
    const std::string f(fn);
    if (int rc = nn_check_rows(f, n, "rows")) return rc;
    if (int rc = nn_check_threshold(f, threshold)) return rc;
    if (int rc = nn_check_metric(f, metric)) return rc;
    return nn_check_required(f, n == 0 || (rows && label && degree && size && rep), "the rows and the four outputs");
}

// n > 0 rows on the device -> the four arrays on the device, enqueued on the ctx's stream
int cl_run(gnn_ctx* ctx, const float* rows_dev, int64_t n, float threshold, int metric, int64_t* label, int64_t* degree, int64_t* size,
           int64_t* rep) {
    NeighbourWorkspace& w = ctx->nn;
    ClusterWorkspace& c = ctx->cl;
    int rc = nn_prepare(ctx, rows_dev, n, metric, w.bfrag, w.bvalid);
    if (!rc) rc = nn_reserve(ctx, c.parent, (size_t)n);
    if (!rc) rc = nn_reserve(ctx, c.degree, (size_t)n);
    if (!rc) rc = nn_reserve(ctx, c.size, (size_t)n);
    if (!rc) rc = nn_reserve(ctx, c.key, (size_t)n);
    const int64_t tiles = (n + QT - 1) / QT;
    int64_t split_rows, splits;
    if (!rc) rc = nn_tile_grid(ctx, "gnn_cluster", "rows", tiles, n, &split_rows, &splits);
    if (rc) return rc;
    ProfScope prof(ctx, GNN_K_NEIGHBOURS);
    if ((rc = launch_1d(cl_init_kernel, n, ctx->stream, n, c.parent, c.degree, c.size, c.key))) return rc;
    ClusterArgs a;
    a.frag = w.bfrag.get();
    a.valid = w.bvalid.get();
    a.n = n;
    a.split_rows = split_rows;
    a.scale = nn_metric_scale(metric);
    a.threshold = threshold;
    a.parent = c.parent.get();
    a.degree = c.degree.get();
    if ((rc = launch_tiles(cl_tile_kernel, tiles, splits, ctx->stream, a))) return rc;
    if ((rc = launch_1d(cl_flatten_kernel, n, ctx->stream, n, w.bvalid, c.parent, c.degree, c.size, c.key, label))) return rc;
    return launch_1d(cl_summarise_kernel, n, ctx->stream, n, w.bvalid, c.degree, c.size, c.key, label, degree, size, rep);
}

}  // namespace
}  // namespace gnn

using namespace gnn;

extern "C" int gnn_cluster_dev(gnn_ctx* ctx, const float* rows_dev, int64_t n, float threshold, int metric, int64_t* label_dev,
                               int64_t* degree_dev, int64_t* size_dev, int64_t* rep_dev) {
    if (int rc = check_cluster_args("gnn_cluster_dev", rows_dev, n, threshold, metric, label_dev, degree_dev, size_dev, rep_dev)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (n == 0) return GNN_OK;
    return cl_run(ctx, rows_dev, n, threshold, metric, label_dev, degree_dev, size_dev, rep_dev);
}

extern "C" int gnn_cluster(gnn_ctx* ctx, const float* rows_host, int64_t n, float threshold, int metric, int64_t* label_host,
                           int64_t* degree_host, int64_t* size_host, int64_t* rep_host) {
    if (int rc = check_cluster_args("gnn_cluster", rows_host, n, threshold, metric, label_host, degree_host, size_host, rep_host)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (n == 0) return GNN_OK;
    NeighbourWorkspace& w = ctx->nn;
    ClusterWorkspace& c = ctx->cl;
    Landing land(c.d_out);
    const int label = land.add(label_host, n), degree = land.add(degree_host, n), size = land.add(size_host, n), rep = land.add(rep_host, n);
    int rc = land.reserve(ctx);                               // both buffers stand before the copy is enqueued
    if (!rc) rc = nn_upload_rows(ctx, rows_host, n);
    if (!rc)
        rc = cl_run(ctx, w.d_base, n, threshold, metric, land.dev<int64_t>(label), land.dev<int64_t>(degree), land.dev<int64_t>(size),
                    land.dev<int64_t>(rep));
    return rc ? rc : land.copy_out(ctx);
}
