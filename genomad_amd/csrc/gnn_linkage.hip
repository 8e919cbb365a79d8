// Single-linkage tree among encoder embeddings (include/genomad_nn.h, "single-linkage tree"): the
// maximum-similarity spanning tree (a forest where NaN pairs split it) of the complete graph over the valid rows, under the strict
// order (value descending, lo ascending, hi ascending) - what Kruskal takes.  Boruvka rounds; a round is six launches:
//   reset      best = cbest = 0, chi = INT_MAX, parent = comp (the trees of the last round, compressed to depth one; comp[i] is -1
//              for an invalid row, which stays a tree of its own that nothing joins).
//   tile       the tile parts of gnn_nn_frag.h - 64 rows' fragments in LDS, the base streamed in steps of 256 columns, NN_PRODUCTS'
//              three products per k-step in their order, the same scale - over the UPPER TRIANGLE only.  Every value with row < col,
//              both rows valid, comp[row] != comp[col] and not NaN is a candidate AT BOTH ENDS: best[x] = max of nn_key(nn_image(s),
//              partner) = (image << 32) | (2^32 - 1 - partner) over the candidates at x, 0: none.  A lane keeps a running best per accumulator
//              register over the workgroup's steps (the row side: one LDS max per row and wave at the end, one global max per row and
//              workgroup) and takes one max per column and step (the column side).  A wave whose rows and columns share one component
//              skips its k-loop.
//   pick       cbest[root] = max of (image << 32) | (2^32 - 1 - lo) over the best keys of the component's rows; then chi[root] = min
//              of hi among the rows that match: the component's best outgoing edge in the strict order.
//   link       per root with a chosen edge: the edge is recorded - not when the other component chose the same edge and has the
//              smaller root - in a slot taken by an integer add, and the two trees are joined (cl_join of gnn_nn_frag.h).
//   flatten    comp[i] = the root of i's tree.
// The host reads 8 bytes per round - the edges recorded so far - and stops after a round that adds none; it then sorts the records.
// Every best, cbest and chi is an integer max or min of values that depend on the pair alone, the slots' order is sorted away: nothing
// depends on the order the workgroups run in or on the split of the base.  No loop here waits for another workgroup: every loop's
// termination argument stands next to it.
// The density-aware linkage tree (gnn_density_tree*; "density-aware linkage tree" in the header) is the same rounds
// over the mutual-reachability values min(v, core[row], core[col]): the tile kernel and its candidates are templates on a bool, the
// cores come from the self-search of gnn_neighbours.hip (lk_core_kernel), and reset, pick, link, flatten and lk_run are shared.
#include <algorithm>
#include <climits>
#include <cmath>
#include <numeric>
#include <vector>

#include "gnn_nn_frag.h"

namespace gnn {
namespace {

constexpr int ROUNDS_MAX = 32;                   // components at least halve per round: n < 2^31 needs at most 31

__device__ __forceinline__ unsigned long long lk_peek(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void lk_init_kernel(int64_t n, const uint8_t* __restrict__ valid, int32_t* __restrict__ comp) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) comp[i] = valid[i] ? (int32_t)i : -1;
}

__global__ __launch_bounds__(256) void lk_reset_kernel(int64_t n, const int32_t* __restrict__ comp, int32_t* __restrict__ parent,
                                                       unsigned long long* __restrict__ best, unsigned long long* __restrict__ cbest,
                                                       int32_t* __restrict__ chi) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    parent[i] = comp[i] < 0 ? (int32_t)i : comp[i];
    best[i] = 0;
    cbest[i] = 0;
    chi[i] = INT_MAX;
}

struct LinkageArgs {
    const uint4* frag;         // round_up(n, 64) / 32 blocks: rows and columns alike
    const int32_t* comp;       // [n] the root of the row's component, flat; -1: the row is invalid
    int64_t n;
    int64_t split_rows;        // base rows per workgroup: a multiple of 32
    float scale;               // 2^-16 for cosine, 1 for dot
    unsigned long long* best;  // [n]
    const float* core;         // [n] the density tree's core similarities, NaN at an invalid row; unread by the plain tree
};

// The candidates of one step.  The registers are walked by ascending row (nn_acc_row) and a lane's columns ascend with nb and with the
// steps, and `!(s <= best so far)` is false for an equal value (-0 equals +0) and true while the best is still NaN (none): the
// smallest partner among equals is kept.  An invalid column has scale = NaN, so its values fail s == s like a NaN pair.  DIAG: the
// step overlaps the tile's own rows, and only then is row < col a test.  MR (the density tree): the candidate's value is the pair's
// mutual-reachability value min(s, core[row], core[col]) - taken behind the s == s test, since fminf drops a NaN operand and would
// turn a NaN pair into an edge; a valid row's core is a number wherever it has a candidate.
template <bool DIAG, bool MR>
__device__ __forceinline__ void lk_candidates(const f32x16 (&acc)[2][2], const int* lcomp, const float* lcore, int r0, int lane,
                                              const float (&scale)[2], const int (&col)[2], const int (&cc)[2], const float (&ccore)[2],
                                              float (&bval)[2][16], int (&bcol)[2][16], float (&cval)[2], int (&crow)[2]) {
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = nn_acc_row(mb, r, lane >> 5);
            const int rg = r0 + row;
            const int rc = lcomp[row];
            float rcore = 0.f;
            if constexpr (MR) rcore = lcore[row];
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                float s = acc[mb][nb][r] * scale[nb];
                const bool e = rc >= 0 && rc != cc[nb] && s == s && (!DIAG || rg < col[nb]);
                if constexpr (MR) s = fminf(fminf(s, rcore), ccore[nb]);
                if (e && !(s <= bval[mb][r])) {
                    bval[mb][r] = s;
                    bcol[mb][r] = col[nb];
                }
                if (e && !(s <= cval[nb])) {
                    cval[nb] = s;
                    crow[nb] = rg;
                }
            }
        }
}

// grid = (row tiles, base ranges), 256 threads.  LDS: the tile's fragments 128 KB - one workgroup per CU, a wave has its SIMD's whole
// register file: 64 VGPRs of running bests beside the 64 of acc -, its rows' components and bests.  MR: the density tree's values
// (lk_candidates), the rows' cores in LDS and a column's fetched with its component; the skip rule and the key > pk shortcut only ever
// skip a maximum that cannot win, whatever the value is made of.
template <bool MR>
__global__ __launch_bounds__(256) void lk_tile_kernel(LinkageArgs a) {
    __shared__ uint4 qs[2 * BLK_U4];
    __shared__ unsigned long long lbest[QT];   // the rows' best partners among this workgroup's columns: flushed once
    __shared__ int lcomp[QT];                  // the row's component, -1: the row is invalid or beyond n
    __shared__ float lcore[MR ? QT : 1];       // MR: the row's core similarity
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    TileRange t;
    if (!nn_tile_range(t, a.split_rows, a.n, true)) return;
    const int64_t r0 = t.r0, b1 = t.b1;
    nn_copy_tile(qs, a.frag, tid);
    if (tid < QT) {
        lbest[tid] = 0;
        lcomp[tid] = r0 + tid < a.n ? a.comp[r0 + tid] : -1;
        if constexpr (MR) lcore[tid] = r0 + tid < a.n ? a.core[r0 + tid] : NAN;
    }
    __syncthreads();
    // the component all valid rows of the tile share; -1: they do not.  The same in every wave: a tile without a valid row leaves whole
    int tc;
    {
        const int c = lcomp[lane];
        const unsigned long long okm = __ballot(c >= 0);
        if (okm == 0) return;
        const int first = __shfl(c, __ffsll((long long)okm) - 1);
        tc = __all(c < 0 || c == first) ? first : -1;
    }
    float bval[2][16];                     // per accumulator register: the best value at its row in this lane's columns, NaN: none
    int bcol[2][16];                       // and its column, -1: none
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            bval[mb][r] = NAN;
            bcol[mb][r] = -1;
        }
    const int64_t last_blk = t.last_blk();
    // what a step needs of its columns, fetched one step ahead - with one wave per SIMD nothing else hides a load in front of the
    // fragment loads: the column's component (-1: no column, or an invalid one) and what best[] holds for it now.  The latter may be
    // older than another workgroup's maximum by the time it is used: then a maximum is merely not skipped.
    int ncc[2];
    unsigned long long npk[2];
    float ncore[2] = {NAN, NAN};           // MR: the column's core similarity
    auto fetch = [&](int64_t c0) {
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const int64_t col = nn_blk_col(nn_step_blk(c0, wave, nb), lane);
            ncc[nb] = col < b1 ? a.comp[col] : -1;
            npk[nb] = col < b1 ? lk_peek(a.best + col) : ~0ull;
            if constexpr (MR) ncore[nb] = col < b1 ? a.core[col] : NAN;
        }
    };
    fetch(t.c0);
    // Ends: c0 grows by STEP towards b1.
    for (int64_t c0 = t.c0; c0 < b1; c0 += STEP) {
        const uint4* bp[2];
        int col[2], cc[2];                 // the lane's column and its component, -1: no edge can end there
        unsigned long long pk[2];
        float scale[2], ccore[2];
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            col[nb] = (int)nn_step_column(a.frag, c0, wave, lane, nb, last_blk, bp[nb]);    // read only where cc >= 0: there it is < b1 < 2^31
            cc[nb] = ncc[nb];
            pk[nb] = npk[nb];
            ccore[nb] = ncore[nb];
            scale[nb] = cc[nb] >= 0 ? a.scale : NAN;
        }
        fetch(c0 + STEP);
        // the skip rule: every column of the wave is no column or in the tile's one component (tc = -1 equals no column's).
        // Wave-uniform, and no barrier follows in the loop
        if (__all((cc[0] < 0 || cc[0] == tc) && (cc[1] < 0 || cc[1] == tc))) continue;
        f32x16 acc[2][2];
        NN_PRODUCTS(qs, bp, lane, acc);
        float cval[2] = {NAN, NAN};        // per column of the lane: the best value in this step's rows, and its row
        int crow[2] = {-1, -1};
        if (c0 < r0 + QT)                  // wave-uniform
            lk_candidates<true, MR>(acc, lcomp, lcore, (int)r0, lane, scale, col, cc, ccore, bval, bcol, cval, crow);
        else
            lk_candidates<false, MR>(acc, lcomp, lcore, (int)r0, lane, scale, col, cc, ccore, bval, bcol, cval, crow);
        // ---- the column side: a column is one lane's in all its registers and the other half's - one max per column and step, and
        // only where it can raise what the load of a step ago saw
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            unsigned long long key = crow[nb] >= 0 ? nn_key(nn_image(cval[nb]), (unsigned)crow[nb]) : 0ull;
            const unsigned long long other = __shfl_xor(key, 32);
            key = other > key ? other : key;
            if (lane < 32 && key > pk[nb]) atomicMax(a.best + col[nb], key);     // key > 0 only where cc >= 0: col < b1
        }
    }
    // ---- the row side, once: a row's candidates lie in one register of the 32 lanes of a half
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            unsigned long long key = bcol[mb][r] >= 0 ? nn_key(nn_image(bval[mb][r]), (unsigned)bcol[mb][r]) : 0ull;
#pragma unroll
            for (int s = 16; s > 0; s >>= 1) {
                const unsigned long long other = __shfl_xor(key, s);
                key = other > key ? other : key;
            }
            if ((lane & 31) == 0 && key) atomicMax(&lbest[nn_acc_row(mb, r, lane >> 5)], key);
        }
    __syncthreads();
    if (tid < QT && lbest[tid]) atomicMax(a.best + r0 + tid, lbest[tid]);       // lbest > 0 only at a valid row < n
}

// best[i] names i's best partner; the component's key names the smaller end of the pair
__global__ __launch_bounds__(256) void lk_pick_lo_kernel(int64_t n, const int32_t* __restrict__ comp, const unsigned long long* __restrict__ best,
                                                         unsigned long long* __restrict__ cbest) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || best[i] == 0) return;
    const unsigned partner = nn_key_index(best[i]);
    const unsigned lo = min((unsigned)i, partner);
    atomicMax(cbest + comp[i], nn_key((unsigned)(best[i] >> 32), lo));
}

__global__ __launch_bounds__(256) void lk_pick_hi_kernel(int64_t n, const int32_t* __restrict__ comp, const unsigned long long* __restrict__ best,
                                                         const unsigned long long* __restrict__ cbest, int32_t* __restrict__ chi) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || best[i] == 0) return;
    const unsigned partner = nn_key_index(best[i]);
    const unsigned lo = min((unsigned)i, partner), hi = max((unsigned)i, partner);
    if (nn_key((unsigned)(best[i] >> 32), lo) == cbest[comp[i]]) atomicMin(chi + comp[i], (int32_t)hi);
}

// One thread per root with a chosen edge.  comp, cbest and chi are the round's and constant here; only parent[] changes.
__global__ __launch_bounds__(256) void lk_link_kernel(int64_t n, int64_t capacity, const int32_t* __restrict__ comp,
                                                      const unsigned long long* __restrict__ cbest, const int32_t* __restrict__ chi,
                                                      int32_t* parent, int32_t* __restrict__ ea, int32_t* __restrict__ eb,
                                                      unsigned* __restrict__ es, unsigned long long* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || comp[i] != (int32_t)i || cbest[i] == 0) return;
    const int lo = (int)nn_key_index(cbest[i]), hi = chi[i];
    if ((int64_t)hi >= n) return;          // never: the row that set cbest[i] matches it and has set chi[i]
    const int other = comp[lo] == (int32_t)i ? comp[hi] : comp[lo];
    // a mutual pick is recorded once, by the smaller root; any other pair of components chose two different edges
    const bool mutual = cbest[other] == cbest[i] && chi[other] == hi;
    if (!(mutual && other < (int)i)) {
        const unsigned long long slot = atomicAdd(count, 1ull);
        if ((int64_t)slot < capacity) {    // a forest has at most n - 1 edges: always
            ea[slot] = lo;
            eb[slot] = hi;
            es[slot] = (unsigned)(cbest[i] >> 32);
        }
    }
    (void)cl_join(parent, (int)i, other);
}

// A launch of its own behind the links: nn_root's plain loads see every link.
__global__ __launch_bounds__(256) void lk_flatten_kernel(int64_t n, const int32_t* __restrict__ parent, int32_t* comp) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || comp[i] < 0) return;     // an invalid row stays -1
    comp[i] = nn_root(parent, (int)i);
}

// The density tree's core similarities from the self-search's lists (gnn_neighbours_dev, k = min_points - 1): the last entry of the
// row's list that is a number - the lists are NaN-padded behind their last partner -, NaN for a row without one.  k == 0
// (min_points 1): +inf at a valid row, which leaves every pair value as it is.
__global__ __launch_bounds__(256) void lk_core_kernel(int64_t n, int k, const uint8_t* __restrict__ valid, const float* __restrict__ nsim,
                                                      float* __restrict__ core) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float c = k == 0 && valid[i] ? INFINITY : NAN;
    for (int j = 0; j < k; ++j) {          // Ends: j counts to k <= 64
        const float s = nsim[i * k + j];
        if (s == s) c = s;
    }
    core[i] = c;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

int check_linkage_args(const char* fn, const void* rows, int64_t n, int metric, const void* a, const void* b, const void* sim, const void* valid,
                       const void* n_edges, const void* rounds) {
    const std::string f(fn);
    if (int rc = nn_check_rows(f, n, "rows")) return rc;
    if (int rc = nn_check_metric(f, metric)) return rc;
    return nn_check_required(f, n_edges && rounds && (n == 0 || (rows && valid)) && (n <= 1 || (a && b && sim)),
                             "the rows, the four arrays, n_edges and rounds");
}

// n > 0 rows on the device -> the sorted tree, the flags and the two counts on the host.  The ctx's stream is synchronised once per
// round (the host reads the number of edges) and once for the records.  min_points > 0: the density tree - the pair values are the
// mutual-reachability values under the core similarities, which go to core_host [n] as well; min_points >= 2 runs the self-search
// first, whose prepare leaves the same fragments and flags as nn_prepare would.
int lk_run(gnn_ctx* ctx, const char* fn, const float* rows_dev, int64_t n, int metric, int min_points, int64_t* a_host, int64_t* b_host,
           float* sim_host, float* core_host, uint8_t* valid_host, int64_t* n_edges_host, int64_t* rounds_host) {
    NeighbourWorkspace& w = ctx->nn;
    LinkageWorkspace& k = ctx->lk;
    const int64_t capacity = n - 1;
    const bool mr = min_points > 0;
    const int nk = mr ? min_points - 1 : 0;
    PassLog& log = mr ? k.tree_rounds : k.rounds;
    int rc = GNN_OK;
    if (nk > 0) {
        rc = nn_reserve(ctx, k.nidx, (size_t)n * nk);
        if (!rc) rc = nn_reserve(ctx, k.nsim, (size_t)n * nk);
        if (!rc) rc = gnn_neighbours_dev(ctx, rows_dev, n, nullptr, n, nk, metric, k.nidx.get(), k.nsim.get());
    } else {
        rc = nn_prepare(ctx, rows_dev, n, metric, w.bfrag, w.bvalid);
    }
    if (!rc && mr) rc = nn_reserve(ctx, k.core, (size_t)n);
    if (!rc) rc = nn_reserve(ctx, k.parent, (size_t)n);
    if (!rc) rc = nn_reserve(ctx, k.comp, (size_t)n);
    if (!rc) rc = nn_reserve(ctx, k.chi, (size_t)n);
    if (!rc) rc = nn_reserve(ctx, k.best, (size_t)n);
    if (!rc) rc = nn_reserve(ctx, k.cbest, (size_t)n);
    if (!rc) rc = nn_reserve(ctx, k.ea, (size_t)n);
    if (!rc) rc = nn_reserve(ctx, k.eb, (size_t)n);
    if (!rc) rc = nn_reserve(ctx, k.es, (size_t)n);
    if (!rc) rc = k.count.reserve(ctx, 1);
    const int64_t tiles = (n + QT - 1) / QT;
    int64_t split_rows, splits;
    if (!rc) rc = nn_tile_grid(ctx, fn, "rows", tiles, n, &split_rows, &splits);
    if (rc) return rc;
    LinkageArgs a;
    a.frag = w.bfrag.get();
    a.comp = k.comp.get();
    a.n = n;
    a.split_rows = split_rows;
    a.scale = nn_metric_scale(metric);
    a.best = k.best.get();
    a.core = mr ? k.core.get() : nullptr;
    log.begin();
    {
        ProfScope prof(ctx, GNN_K_NEIGHBOURS);
        if ((rc = k.count.zero(ctx, 0, 1))) return rc;
        if ((rc = launch_1d(lk_init_kernel, n, ctx->stream, n, w.bvalid, k.comp))) return rc;
        if (mr && (rc = launch_1d(lk_core_kernel, n, ctx->stream, n, nk, w.bvalid, k.nsim, k.core))) return rc;
    }
    // One Boruvka round per pass.  Every component with an outgoing edge is joined to another one, so the components that are not
    // yet final at least halve: at most 31 rounds add an edge for n < 2^31, and one more adds none.  Ends: the loop is bounded by
    // ROUNDS_MAX whatever the device answers; it leaves early after a round that adds no edge or completes a spanning tree.
    unsigned long long edges = 0;
    int64_t rounds = 0;
    for (int pass = 0;; ++pass) {
        if (pass == ROUNDS_MAX) {
            set_error(std::string(fn) + ": round " + std::to_string(pass + 1) + " would be needed for " + std::to_string(n) + " rows (" +
                      std::to_string(edges) + " edges so far): at most " + std::to_string(ROUNDS_MAX) + " rounds can be");
            return GNN_ERR_STATE;
        }
        {
            PassLog::Scope round(ctx, log);
            if ((rc = launch_1d(lk_reset_kernel, n, ctx->stream, n, k.comp, k.parent, k.best, k.cbest, k.chi))) return rc;
            if ((rc = launch_tiles(mr ? lk_tile_kernel<true> : lk_tile_kernel<false>, tiles, splits, ctx->stream, a))) return rc;
            if ((rc = launch_1d(lk_pick_lo_kernel, n, ctx->stream, n, k.comp, k.best, k.cbest))) return rc;
            if ((rc = launch_1d(lk_pick_hi_kernel, n, ctx->stream, n, k.comp, k.best, k.cbest, k.chi))) return rc;
            if ((rc = launch_1d(lk_link_kernel, n, ctx->stream, n, capacity, k.comp, k.cbest, k.chi, k.parent, k.ea, k.eb, k.es, k.count.dev())))
                return rc;
            if ((rc = launch_1d(lk_flatten_kernel, n, ctx->stream, n, k.parent, k.comp))) return rc;
        }
        unsigned long long now = 0;
        if ((rc = k.count.read(ctx, 0, 1, &now))) return rc;
        log.settle();
        if (now > (unsigned long long)capacity) {
            set_error(std::string(fn) + ": round " + std::to_string(pass + 1) + " recorded " + std::to_string(now) + " edges among " +
                      std::to_string(n) + " rows: a forest has at most n - 1");
            return GNN_ERR_STATE;
        }
        if (now == edges) break;
        edges = now;
        ++rounds;
        if (edges == (unsigned long long)capacity) break;
    }
    const size_t m = (size_t)edges;
    std::vector<int32_t> ea(m), eb(m);
    std::vector<unsigned> es(m);
    if (m) {
        GNN_HIP(hipMemcpyAsync(ea.data(), k.ea.get(), m * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        GNN_HIP(hipMemcpyAsync(eb.data(), k.eb.get(), m * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        GNN_HIP(hipMemcpyAsync(es.data(), k.es.get(), m * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    }
    GNN_HIP(hipMemcpyAsync(valid_host, w.bvalid.get(), (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (mr) GNN_HIP(hipMemcpyAsync(core_host, k.core.get(), (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    GNN_HIP(hipStreamSynchronize(ctx->stream));
    std::vector<int64_t> order(m);
    std::iota(order.begin(), order.end(), (int64_t)0);
    std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
        if (es[x] != es[y]) return es[x] > es[y];
        if (ea[x] != ea[y]) return ea[x] < ea[y];
        return eb[x] < eb[y];
    });
    for (int64_t i = 0; i < capacity; ++i) {
        const bool edge = i < (int64_t)m;
        a_host[i] = edge ? ea[order[i]] : -1;
        b_host[i] = edge ? eb[order[i]] : -1;
        sim_host[i] = edge ? nn_unimage(es[order[i]]) : NAN;
    }
    *n_edges_host = (int64_t)m;
    *rounds_host = rounds;
    return GNN_OK;
}

}  // namespace
}  // namespace gnn

using namespace gnn;

extern "C" int gnn_linkage_dev(gnn_ctx* ctx, const float* rows_dev, int64_t n, int metric, int64_t* a_host, int64_t* b_host, float* sim_host,
                               uint8_t* valid_host, int64_t* n_edges_host, int64_t* rounds_host) {
    const char* const fn = "gnn_linkage_dev";
    if (int rc = check_linkage_args(fn, rows_dev, n, metric, a_host, b_host, sim_host, valid_host, n_edges_host, rounds_host)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    *n_edges_host = 0;
    *rounds_host = 0;
    if (n == 0) return GNN_OK;
    return lk_run(ctx, fn, rows_dev, n, metric, 0, a_host, b_host, sim_host, nullptr, valid_host, n_edges_host, rounds_host);
}

extern "C" int gnn_linkage(gnn_ctx* ctx, const float* rows_host, int64_t n, int metric, int64_t* a_host, int64_t* b_host, float* sim_host,
                           uint8_t* valid_host, int64_t* n_edges_host, int64_t* rounds_host) {
    const char* const fn = "gnn_linkage";
    if (int rc = check_linkage_args(fn, rows_host, n, metric, a_host, b_host, sim_host, valid_host, n_edges_host, rounds_host)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    *n_edges_host = 0;
    *rounds_host = 0;
    if (n == 0) return GNN_OK;
    if (int rc = nn_upload_rows(ctx, rows_host, n)) return rc;
    return lk_run(ctx, fn, ctx->nn.d_base, n, metric, 0, a_host, b_host, sim_host, nullptr, valid_host, n_edges_host, rounds_host);
}

extern "C" int gnn_debug_linkage_round_ms(gnn_ctx* ctx, double* ms_out, int64_t capacity, int64_t* n_out) {
    if (int rc = check_ctx(ctx)) return rc;
    return ctx->lk.rounds.out(ctx, "gnn_debug_linkage_round_ms", ms_out, capacity, n_out);
}

// ---- the density tree: the same rounds over the mutual-reachability values (include/genomad_nn.h, "density-aware linkage tree") ----

namespace gnn {
namespace {

constexpr int MIN_POINTS_MAX = 65;               // the row itself and the neighbour search's 64

int check_density_tree_args(const char* fn, const void* rows, int64_t n, int min_points, int metric, const void* a, const void* b, const void* sim,
                            const void* core, const void* valid, const void* n_edges, const void* rounds) {
    if (min_points < 1 || min_points > MIN_POINTS_MAX) {
        set_error(std::string(fn) + ": min_points " + std::to_string(min_points) + " is outside [1, " + std::to_string(MIN_POINTS_MAX) + "]");
        return GNN_ERR_ARG;
    }
    if (int rc = check_linkage_args(fn, rows, n, metric, a, b, sim, valid, n_edges, rounds)) return rc;
    if (n > 0 && !core) {
        set_error(std::string("bad argument to ") + fn + ": core is required");      // "is", not nn_check_required's "are"
        return GNN_ERR_ARG;
    }
    return GNN_OK;
}

}  // namespace
}  // namespace gnn

extern "C" int gnn_density_tree_dev(gnn_ctx* ctx, const float* rows_dev, int64_t n, int min_points, int metric, int64_t* a_host, int64_t* b_host,
                                    float* sim_host, float* core_host, uint8_t* valid_host, int64_t* n_edges_host, int64_t* rounds_host) {
    const char* const fn = "gnn_density_tree_dev";
    if (int rc = check_density_tree_args(fn, rows_dev, n, min_points, metric, a_host, b_host, sim_host, core_host, valid_host, n_edges_host,
                                         rounds_host))
        return rc;
    if (int rc = check_ctx(ctx)) return rc;
    *n_edges_host = 0;
    *rounds_host = 0;
    if (n == 0) return GNN_OK;
    return lk_run(ctx, fn, rows_dev, n, metric, min_points, a_host, b_host, sim_host, core_host, valid_host, n_edges_host, rounds_host);
}

extern "C" int gnn_density_tree(gnn_ctx* ctx, const float* rows_host, int64_t n, int min_points, int metric, int64_t* a_host, int64_t* b_host,
                                float* sim_host, float* core_host, uint8_t* valid_host, int64_t* n_edges_host, int64_t* rounds_host) {
    const char* const fn = "gnn_density_tree";
    if (int rc = check_density_tree_args(fn, rows_host, n, min_points, metric, a_host, b_host, sim_host, core_host, valid_host, n_edges_host,
                                         rounds_host))
        return rc;
    if (int rc = check_ctx(ctx)) return rc;
    *n_edges_host = 0;
    *rounds_host = 0;
    if (n == 0) return GNN_OK;
    if (int rc = nn_upload_rows(ctx, rows_host, n)) return rc;
    return lk_run(ctx, fn, ctx->nn.d_base, n, metric, min_points, a_host, b_host, sim_host, core_host, valid_host, n_edges_host, rounds_host);
}

extern "C" int gnn_debug_density_tree_round_ms(gnn_ctx* ctx, double* ms_out, int64_t capacity, int64_t* n_out) {
    if (int rc = check_ctx(ctx)) return rc;
    return ctx->lk.tree_rounds.out(ctx, "gnn_debug_density_tree_round_ms", ms_out, capacity, n_out);
}
