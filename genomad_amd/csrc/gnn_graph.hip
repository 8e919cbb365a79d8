// Similarity graph among encoder embeddings (include/genomad_nn.h, "similarity graph"): every pair i < j of valid
// rows with sim(i, j) >= threshold and its f32 similarity, as a CSR over the upper triangle - rows in order, a row's columns
// ascending.  The edge set is the one gnn_cluster acts on; here it is kept.  Exact, two passes of one tile kernel and a scan:
//   prepare    nn_prepare (gnn_neighbours.hip), as it is: the neighbour search's fragments and flags, in its buffers.
//   count      gr_tile_kernel<false>: gnn_clusters.hip's tile kernel up to and including its `edge` mask - the tile parts of
//              gnn_nn_frag.h, NN_PRODUCTS' three products per k-step in their order, the same scale, the UPPER TRIANGLE only: the
//              value of the pair i < j is the f32 that gnn_neighbours returns for query i and base row j.  An edge belongs to its
//              smaller row: each of the tile's rows counts its edges among the workgroup's columns (ballots, one LDS add per row
//              and step) and stores the count at cnt[row * splits + part] - one owner workgroup per counter, a plain store.  A
//              workgroup that leaves early stores nothing: the array is cleared first.
//   scan       exclusive int64 prefix sums over the n * splits counters in the order (row, part), the total behind them; integer
//              sums, so the shape of the scan changes nothing.  indptr[i] = off[i * splits].  The host reads the 8-byte total.
//   fill       gr_tile_kernel<true>: the same products in the same steps.  A workgroup whose 64 (row, part) segments are all empty
//              leaves before it loads fragments.  Otherwise lpos[row] starts at the segment's offset; in a step with an edge every
//              wave files its rows' counts, and an edge's place is lpos[row] + the counts of the lower waves + its own wave's
//              column block 0 if it sits in block 1 + the edges at lower lanes of its half of the ballot: ascending in (wave,
//              column block, lane & 31), which is ascending in the column.  Steps ascend and the parts follow each other in the scan:
//              a row's columns come out sorted.  Every store is guarded by the segment's end: rows that change between count and
//              fill give garbage, never an overrun.
// No atomics in global memory, no position that depends on the order workgroups or waves run in: bit-identical for every split of the
// base.  No loop here waits for another workgroup: every loop's termination argument stands next to it.
//
// The match (include/genomad_nn.h, "matches against a reference") is the same kernel over the RECTANGLE query x
// base (gr_tile_kernel<., true>): the tile's fragments and flags are the query's (NeighbourWorkspace's qfrag / qvalid), the columns the
// base's, the ranges those of nn_tile_range(..., upper = false), the edge rule `rok && cg >= 0 && s >= threshold` - no pair is left
// out, the value of (i, j) is the f32 gnn_neighbours returns for query i and base row j - and the counters sit at cnt[row * splits +
// part] for row < n_query.  Products, scale, ballots, placement, segment guard, early exit, scan and indptr are the lines above.
// Memory: all query rows are prepared at once, with no slabs - 2 KB of fragments + 1 B per query row - and 12 B per (query row, base
// range) of counters and offsets; the workspace is the graph's, so a fill belongs to the ctx's last count of either kind.
#include <cmath>
#include <cstring>

#include "gnn_nn_frag.h"

namespace gnn {
namespace {


struct GraphArgs {
    const uint4* frag;         // round_up(n, 64) / 32 blocks: rows and columns alike; rectangle: the query's, the tile's rows only
    const uint8_t* valid;      // [round_up(n, 64)]
    int64_t n;                 // rows; rectangle: n_query
    int64_t split_rows;        // base rows per workgroup: a multiple of 32
    int64_t splits;            // = gridDim.y
    float scale;               // 2^-16 for cosine, 1 for dot
    float threshold;
    int32_t* cnt;              // count: [n * splits], cleared before the launch
    const int64_t* off;        // fill: [n * splits + 1]
    int32_t* col;              // fill: [off[n * splits]]
    float* sim;
    // the rectangle alone, behind everything the upper triangle reads: the columns' fragments, flags and number
    const uint4* bfrag;        // round_up(nb, 64) / 32 blocks
    const uint8_t* bvalid;     // [round_up(nb, 64)]
    int64_t nb;                // n_base
};

// grid = (row tiles, base ranges), 256 threads.  LDS: the tile's fragments 128 KB, its rows' flags and counts or positions.
// FILL false: the count pass.  FILL true: the fill pass - there every thread reaches the same barriers: the step loop's bounds and
// the vote behind the products are the same in the whole workgroup.
// RECT false: the upper triangle among one set of rows (the graph).  RECT true: the rectangle (the match) - the tile's rows are the
// query's, the columns the base's, every pair of valid rows is a candidate; the ranges run over the base, none is empty.
template <bool FILL, bool RECT>
__global__ __launch_bounds__(256) void gr_tile_kernel(GraphArgs a) {
    __shared__ uint4 qs[2 * BLK_U4];
    __shared__ uint8_t lok[QT];
    __shared__ int lcnt[QT];               // count: edges of this workgroup's columns at the tile's rows, stored once
    __shared__ int64_t lpos[QT], lend[QT]; // fill: where the row's next edge goes, and the end of its (row, part) segment
    __shared__ int wcnt[4][QT];            // fill: the step's edges per wave and row
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
    TileRange t;
    const uint4* const cfrag = RECT ? a.bfrag : a.frag;        // where the columns come from
    const uint8_t* const cvalid = RECT ? a.bvalid : a.valid;
    if (!nn_tile_range(t, a.split_rows, RECT ? a.nb : a.n, !RECT)) return;
    const int64_t r0 = t.r0;
    if (FILL) {
        int64_t p = 0, e = 0;
        if (tid < QT && r0 + tid < a.n) {
            const int64_t i = (r0 + tid) * a.splits + blockIdx.y;
            p = a.off[i];
            e = a.off[i + 1];
        }
        if (!__syncthreads_or(e > p)) return;                  // no edge in the 64 segments (uniform: the whole workgroup leaves)
        if (tid < QT) {
            lpos[tid] = p;
            lend[tid] = e;
        }
    }
    nn_copy_tile(qs, a.frag, tid);
    if (tid < QT) {
        lcnt[tid] = 0;
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
            const int64_t col = nn_step_column(cfrag, c0, wave, lane, nb, last_blk, bp[nb]);
            cg[nb] = col < t.b1 && cvalid[col] ? (int)col : -1;
        }
        f32x16 acc[2][2];
        NN_PRODUCTS(qs, bp, lane, acc);
        // ---- edges: bit (mb * 2 + nb) * 16 + reg
        unsigned long long edge = 0;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = nn_acc_row(mb, r, half);
                const int rg = (int)r0 + row;
                const bool rok = lok[row];
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    const float s = acc[mb][nb][r] * a.scale;
                    // cg = -1 fails rg < cg; a NaN fails >=.  The rectangle has no row < col: (i, i) and both orientations count
                    const bool e = rok && (RECT ? cg[nb] >= 0 : rg < cg[nb]) && s >= a.threshold;
                    edge |= (unsigned long long)e << ((mb * 2 + nb) * 16 + r);
                }
            }
        if (!FILL) {
            if (__ballot(edge != 0) == 0) continue;            // wave-uniform, and no barrier follows in the loop
            // A row's edges of this step lie in one register of 32 lanes per column block: a ballot counts them, one lane per half
            // adds them in LDS.
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const unsigned long long e0 = __ballot((edge >> (mb * 32 + r)) & 1), e1 = __ballot((edge >> (mb * 32 + 16 + r)) & 1);
                    const int c = __popc((unsigned)(e0 >> (32 * half))) + __popc((unsigned)(e1 >> (32 * half)));
                    if ((lane & 31) == 0 && c) atomicAdd(&lcnt[nn_acc_row(mb, r, half)], c);
                }
        } else {
            if (!__syncthreads_or(edge != 0)) continue;        // workgroup-uniform: an edge-free step costs this one vote
            // ---- the wave's edges per row: row (mb, r, half) is one lane's to file, and every wave files all 64 of its rows
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const unsigned long long e0 = __ballot((edge >> (mb * 32 + r)) & 1), e1 = __ballot((edge >> (mb * 32 + 16 + r)) & 1);
                    const int c = __popc((unsigned)(e0 >> (32 * half))) + __popc((unsigned)(e1 >> (32 * half)));
                    if ((lane & 31) == 0) wcnt[wave][nn_acc_row(mb, r, half)] = c;
                }
            __syncthreads();
            // ---- places: ascending in (wave, column block, lane & 31)
            const unsigned below = (1u << (lane & 31)) - 1u;
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const unsigned h0 = (unsigned)(__ballot((edge >> (mb * 32 + r)) & 1) >> (32 * half));
                    const unsigned h1 = (unsigned)(__ballot((edge >> (mb * 32 + 16 + r)) & 1) >> (32 * half));
                    if (((edge >> (mb * 32 + r)) | (edge >> (mb * 32 + 16 + r))) & 1) {
                        const int row = nn_acc_row(mb, r, half);
                        int64_t base = lpos[row];
                        for (int w = 0; w < wave; ++w) base += wcnt[w][row];       // Ends: w grows towards wave <= 3
                        const int64_t end = lend[row];
#pragma unroll
                        for (int nb = 0; nb < 2; ++nb)
                            if ((edge >> ((mb * 2 + nb) * 16 + r)) & 1) {
                                const int64_t at = base + (nb ? __popc(h0) : 0) + __popc((nb ? h1 : h0) & below);
                                if (at < end) {            // always, unless the rows changed since the count: never an overrun
                                    a.col[at] = cg[nb];
                                    a.sim[at] = acc[mb][nb][r] * a.scale;
                                }
                            }
                    }
                }
            __syncthreads();
            if (tid < QT) lpos[tid] += wcnt[0][tid] + wcnt[1][tid] + wcnt[2][tid] + wcnt[3][tid];
            __syncthreads();
        }
    }
    if (!FILL) {
        __syncthreads();
        if (tid < QT && r0 + tid < a.n) a.cnt[(r0 + tid) * a.splits + blockIdx.y] = lcnt[tid];
    }
}

// indptr[i] = off[i * splits] for i <= n: a row's first part, and the total at n
__global__ __launch_bounds__(256) void gr_indptr_kernel(int64_t n, int64_t splits, const int64_t* __restrict__ off, int64_t* __restrict__ indptr) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    indptr[i] = off[i * splits];
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

int check_graph_args(const std::string& f, int64_t n, float threshold, int metric) {
    if (int rc = nn_check_rows(f, n, "rows")) return rc;
    if (int rc = nn_check_threshold(f, threshold)) return rc;
    return nn_check_metric(f, metric);
}

int check_match_args(const std::string& f, int64_t nq, int64_t nb, float threshold, int metric) {
    if (int rc = nn_check_rows(f, nq, "n_query")) return rc;
    if (int rc = nn_check_rows(f, nb, "n_base")) return rc;
    if (int rc = nn_check_threshold(f, threshold)) return rc;
    return nn_check_metric(f, metric);
}

uint32_t bits_of(float x) {
    uint32_t u;
    std::memcpy(&u, &x, sizeof u);
    return u;
}

// what both passes of the counted search run with; g.rect: the rectangle (n = n_query rows against g.nb base rows)
GraphArgs gr_args(gnn_ctx* ctx, float threshold, int metric) {
    const NeighbourWorkspace& w = ctx->nn;
    const GraphWorkspace& g = ctx->gr;
    GraphArgs a;
    a.frag = g.rect ? w.qfrag.get() : w.bfrag.get();
    a.valid = g.rect ? w.qvalid.get() : w.bvalid.get();
    a.n = g.n;
    a.split_rows = g.split_rows;
    a.splits = g.splits;
    a.scale = nn_metric_scale(metric);
    a.threshold = threshold;
    a.cnt = g.cnt.get();
    a.off = g.off.get();
    a.col = nullptr;
    a.sim = nullptr;
    a.bfrag = w.bfrag.get();
    a.bvalid = w.bvalid.get();
    a.nb = g.nb;
    return a;
}

// The fragments and flags of the counted search, for either pass.  The graph: its rows in the base's buffers.  The match: the base
// there, and ALL query rows at once in the query's buffers (no slabs: 2 KB + 1 B per query row).
int gr_prepare(gnn_ctx* ctx, const float* rows_dev, const float* base_dev, int metric) {
    NeighbourWorkspace& w = ctx->nn;
    const GraphWorkspace& g = ctx->gr;
    if (!g.rect) return nn_prepare(ctx, rows_dev, g.n, metric, w.bfrag, w.bvalid);
    if (int rc = nn_prepare(ctx, base_dev, g.nb, metric, w.bfrag, w.bvalid)) return rc;
    return nn_prepare(ctx, rows_dev, g.n, metric, w.qfrag, w.qvalid);
}

// n >= 0 rows on the device -> indptr[n + 1] on the device and the total on the host; the ctx's stream is synchronised once.  The
// workspace then remembers what the fill needs.  rect: the n rows are queries against the nb rows of base_dev (the match); otherwise
// the upper triangle among the n rows (the graph; base_dev and nb are not looked at).
int gr_count(gnn_ctx* ctx, const char* fn, const float* rows_dev, int64_t n, const float* base_dev, int64_t nb, bool rect, float threshold,
             int metric, int64_t* indptr_dev, int64_t* nnz_host) {
    GraphWorkspace& g = ctx->gr;
    g.counted = false;
    g.host_rows = false;
    g.passes.begin();
    g.rect = rect;
    g.n = n;
    g.nb = rect ? nb : n;
    int64_t total = 0;
    if (n == 0 || g.nb == 0) {             // an empty side launches nothing
        g.split_rows = g.splits = 0;
        GNN_HIP(hipMemsetAsync(indptr_dev, 0, (size_t)(n + 1) * sizeof(int64_t), ctx->stream));
    } else {
        int rc = gr_prepare(ctx, rows_dev, base_dev, metric);
        const int64_t tiles = (n + QT - 1) / QT;
        if (!rc) rc = nn_tile_grid(ctx, fn, rect ? "base rows" : "rows", tiles, g.nb, &g.split_rows, &g.splits);
        const int64_t m = n * g.splits;
        if (!rc) rc = nn_reserve(ctx, g.cnt, (size_t)m);
        if (!rc) rc = nn_reserve(ctx, g.off, (size_t)m + 1);
        if (rc) return rc;
        {
            PassLog::Scope pass(ctx, g.passes);
            GNN_HIP(hipMemsetAsync(g.cnt.get(), 0, (size_t)m * sizeof(int32_t), ctx->stream));
            if ((rc = launch_tiles(rect ? gr_tile_kernel<false, true> : gr_tile_kernel<false, false>, tiles, g.splits, ctx->stream,
                                   gr_args(ctx, threshold, metric))))
                return rc;
        }
        {
            PassLog::Scope pass(ctx, g.passes);
            if ((rc = nn_scan(ctx->stream, g.cnt, m, g.off, nullptr))) return rc;
            if ((rc = launch_1d(gr_indptr_kernel, n + 1, ctx->stream, n, g.splits, g.off, indptr_dev))) return rc;
        }
        GNN_HIP(hipMemcpyAsync(&total, g.off.get() + m, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    GNN_HIP(hipStreamSynchronize(ctx->stream));
    g.passes.settle();
    g.threshold_bits = bits_of(threshold);
    g.metric = metric;
    g.total = total;
    g.counted = true;
    *nnz_host = total;
    return GNN_OK;
}

// GNN_OK when the fill may run (or has nothing to do), with the total in the workspace.  A fill belongs to the ctx's last count, of
// its own kind: rect - a gnn_match_count* of the same (n, nb, ...); otherwise a gnn_graph_count* of the same (n, ...).
int gr_check_fill(gnn_ctx* ctx, const std::string& f, int64_t n, int64_t nb, bool rect, float threshold, int metric, int64_t capacity,
                  bool host_rows) {
    const GraphWorkspace& g = ctx->gr;
    if (!g.counted || g.rect != rect || g.n != n || (rect && g.nb != nb) || g.threshold_bits != bits_of(threshold) || g.metric != metric ||
        (host_rows && !g.host_rows)) {
        const std::string count = std::string(rect ? "gnn_match_count" : "gnn_graph_count") + (host_rows ? "" : "*");
        const std::string what = rect ? "(n_query, n_base, threshold, metric) = (" + std::to_string(n) + ", " + std::to_string(nb) + ", "
                                      : "(n, threshold, metric) = (" + std::to_string(n) + ", ";
        set_error(f + ": no " + count + " of the same " + what + std::to_string(threshold) + ", " + std::to_string(metric) +
                  ") came before it" + (host_rows ? ", or another search has replaced the rows it uploaded" : ""));
        return GNN_ERR_STATE;
    }
    if (capacity < g.total) {
        set_error(f + ": capacity " + std::to_string(capacity) + " is below the " + std::to_string(g.total) + " edges the count found");
        return GNN_ERR_ARG;
    }
    return GNN_OK;
}

// total > 0 edges of the counted search -> col and sim on the device, enqueued on the ctx's stream.  The prepare runs again: another
// search may have used the shared fragment buffers since the count, and it is deterministic.
int gr_fill(gnn_ctx* ctx, const float* rows_dev, const float* base_dev, float threshold, int metric, int32_t* col_dev, float* sim_dev) {
    const GraphWorkspace& g = ctx->gr;
    if (int rc = gr_prepare(ctx, rows_dev, base_dev, metric)) return rc;
    ProfScope prof(ctx, GNN_K_NEIGHBOURS);
    GraphArgs a = gr_args(ctx, threshold, metric);
    a.col = col_dev;
    a.sim = sim_dev;
    return launch_tiles(g.rect ? gr_tile_kernel<true, true> : gr_tile_kernel<true, false>, (g.n + QT - 1) / QT, g.splits, ctx->stream, a);
}

// the host fill of either kind, behind its checks: the edges land in the ctx's buffers, are copied out and waited for
int gr_fill_host(gnn_ctx* ctx, const char* fn, float threshold, int metric, int32_t* col_host, float* sim_host) {
    GraphWorkspace& g = ctx->gr;
    const int64_t total = g.total;
    if (total == 0) return GNN_OK;
    if (int rc = nn_check_required(fn, col_host && sim_host, "col and sim")) return rc;
    Landing land(g.d_out);
    const int col = land.add(col_host, total), sim = land.add(sim_host, total);
    int rc = land.reserve(ctx);
    if (!rc)
        rc = gr_fill(ctx, g.rect ? g.d_query.get() : ctx->nn.d_base.get(), ctx->nn.d_base, threshold, metric, land.dev<int32_t>(col),
                     land.dev<float>(sim));
    return rc ? rc : land.copy_out(ctx);
}

}  // namespace
}  // namespace gnn

using namespace gnn;

extern "C" int gnn_graph_count_dev(gnn_ctx* ctx, const float* rows_dev, int64_t n, float threshold, int metric, int64_t* indptr_dev,
                                   int64_t* nnz_host) {
    const char* const fn = "gnn_graph_count_dev";
    if (int rc = check_graph_args(fn, n, threshold, metric)) return rc;
    if (int rc = nn_check_required(fn, (n == 0 || rows_dev) && indptr_dev && nnz_host, "the rows, indptr and nnz")) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    return gr_count(ctx, fn, rows_dev, n, nullptr, 0, false, threshold, metric, indptr_dev, nnz_host);
}

extern "C" int gnn_graph_fill_dev(gnn_ctx* ctx, const float* rows_dev, int64_t n, float threshold, int metric, int32_t* col_dev, float* sim_dev,
                                  int64_t capacity) {
    const char* const fn = "gnn_graph_fill_dev";
    if (int rc = check_graph_args(fn, n, threshold, metric)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (int rc = gr_check_fill(ctx, fn, n, 0, false, threshold, metric, capacity, false)) return rc;
    if (ctx->gr.total == 0) return GNN_OK;
    if (int rc = nn_check_required(fn, rows_dev && col_dev && sim_dev, "the rows, col and sim")) return rc;
    return gr_fill(ctx, rows_dev, nullptr, threshold, metric, col_dev, sim_dev);
}

extern "C" int gnn_graph_count(gnn_ctx* ctx, const float* rows_host, int64_t n, float threshold, int metric, int64_t* indptr_host,
                               int64_t* nnz_host) {
    const char* const fn = "gnn_graph_count";
    if (int rc = check_graph_args(fn, n, threshold, metric)) return rc;
    if (int rc = nn_check_required(fn, (n == 0 || rows_host) && indptr_host && nnz_host, "the rows, indptr and nnz")) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    GraphWorkspace& g = ctx->gr;
    g.counted = false;
    Landing land(g.d_out);
    land.add(indptr_host, n + 1);
    int rc = land.reserve(ctx);                               // both buffers stand before the copy is enqueued
    if (!rc) rc = nn_upload_rows(ctx, rows_host, n);
    if (!rc) rc = gr_count(ctx, fn, ctx->nn.d_base, n, nullptr, 0, false, threshold, metric, land.dev<int64_t>(0), nnz_host);
    if (!rc) rc = land.copy_out(ctx);
    if (rc) return rc;
    g.host_rows = true;
    return GNN_OK;
}

extern "C" int gnn_debug_graph_pass_ms(gnn_ctx* ctx, double* ms_out, int64_t capacity, int64_t* n_out) {
    if (int rc = check_ctx(ctx)) return rc;
    return ctx->gr.passes.out(ctx, "gnn_debug_graph_pass_ms", ms_out, capacity, n_out);
}

extern "C" int gnn_graph_fill(gnn_ctx* ctx, int64_t n, float threshold, int metric, int32_t* col_host, float* sim_host, int64_t capacity) {
    const char* const fn = "gnn_graph_fill";
    if (int rc = check_graph_args(fn, n, threshold, metric)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (int rc = gr_check_fill(ctx, fn, n, 0, false, threshold, metric, capacity, true)) return rc;
    return gr_fill_host(ctx, fn, threshold, metric, col_host, sim_host);
}

// ---- the match: the same passes over the rectangle query x base ----------------------------------------------------------------------

extern "C" int gnn_match_count_dev(gnn_ctx* ctx, const float* query_dev, int64_t n_query, const float* base_dev, int64_t n_base,
                                   float threshold, int metric, int64_t* indptr_dev, int64_t* nnz_host) {
    const char* const fn = "gnn_match_count_dev";
    if (int rc = check_match_args(fn, n_query, n_base, threshold, metric)) return rc;
    if (int rc = nn_check_required(fn, (n_query == 0 || query_dev) && (n_base == 0 || base_dev) && indptr_dev && nnz_host,
                                   "the query, the base, indptr and nnz"))
        return rc;
    if (int rc = check_ctx(ctx)) return rc;
    return gr_count(ctx, fn, query_dev, n_query, base_dev, n_base, true, threshold, metric, indptr_dev, nnz_host);
}

extern "C" int gnn_match_fill_dev(gnn_ctx* ctx, const float* query_dev, int64_t n_query, const float* base_dev, int64_t n_base,
                                  float threshold, int metric, int32_t* col_dev, float* sim_dev, int64_t capacity) {
    const char* const fn = "gnn_match_fill_dev";
    if (int rc = check_match_args(fn, n_query, n_base, threshold, metric)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (int rc = gr_check_fill(ctx, fn, n_query, n_base, true, threshold, metric, capacity, false)) return rc;
    if (ctx->gr.total == 0) return GNN_OK;
    if (int rc = nn_check_required(fn, query_dev && base_dev && col_dev && sim_dev, "the query, the base, col and sim")) return rc;
    return gr_fill(ctx, query_dev, base_dev, threshold, metric, col_dev, sim_dev);
}

extern "C" int gnn_match_count(gnn_ctx* ctx, const float* query_host, int64_t n_query, const float* base_host, int64_t n_base,
                               float threshold, int metric, int64_t* indptr_host, int64_t* nnz_host) {
    const char* const fn = "gnn_match_count";
    if (int rc = check_match_args(fn, n_query, n_base, threshold, metric)) return rc;
    if (int rc = nn_check_required(fn, (n_query == 0 || query_host) && (n_base == 0 || base_host) && indptr_host && nnz_host,
                                   "the query, the base, indptr and nnz"))
        return rc;
    if (int rc = check_ctx(ctx)) return rc;
    GraphWorkspace& g = ctx->gr;
    g.counted = false;
    // every buffer stands before a copy is enqueued.  The query rows go into a buffer of the match's own: no other search writes it
    Landing land(g.d_out);
    land.add(indptr_host, n_query + 1);
    int rc = land.reserve(ctx);
    if (!rc) rc = nn_reserve(ctx, g.d_query, (size_t)std::max<int64_t>(n_query, 1) * D);
    if (!rc) rc = nn_upload_rows(ctx, base_host, n_base);
    if (rc) return rc;
    if (n_query > 0)
        GNN_HIP(hipMemcpyAsync(g.d_query.get(), query_host, (size_t)n_query * D * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    rc = gr_count(ctx, fn, g.d_query, n_query, ctx->nn.d_base, n_base, true, threshold, metric, land.dev<int64_t>(0), nnz_host);
    if (!rc) rc = land.copy_out(ctx);
    if (rc) return rc;
    g.host_rows = true;
    return GNN_OK;
}

extern "C" int gnn_match_fill(gnn_ctx* ctx, int64_t n_query, int64_t n_base, float threshold, int metric, int32_t* col_host, float* sim_host,
                              int64_t capacity) {
    const char* const fn = "gnn_match_fill";
    if (int rc = check_match_args(fn, n_query, n_base, threshold, metric)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (int rc = gr_check_fill(ctx, fn, n_query, n_base, true, threshold, metric, capacity, true)) return rc;
    return gr_fill_host(ctx, fn, threshold, metric, col_host, sim_host);
}

extern "C" int gnn_debug_match_pass_ms(gnn_ctx* ctx, double* ms_out, int64_t capacity, int64_t* n_out) {
    if (int rc = check_ctx(ctx)) return rc;
    return ctx->gr.passes.out(ctx, "gnn_debug_match_pass_ms", ms_out, capacity, n_out);
}
