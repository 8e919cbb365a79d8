// What the consumers of the similarity graph's CSR share (gnn_mcl.hip, gnn_spread.hip, gnn_avglink.hip, gnn_communities.hip): the
// verdict on the graph, its symmetric form and the host-side prologue of their entry points.  Included behind gnn_nn_frag.h
// (nn_reserve, launch_1d, nn_scan); everything here has internal linkage.
//   validate     one thread per row: indptr rises within [0, nnz], every col lies in (row, n), every sim is finite and < 64.  The host
//                reads one flag; GNN_ERR_ARG before anything else runs, the outputs untouched.  It also writes the rows' validity.
//   symmetrise   the edges that exist (q = rint(sim * W) > 0, both ends valid) are counted at both ends (integer adds), the counts
//                scanned by one block, the edges filed through per-row cursors.  A row's entries stand in arrival order: nothing
//                downstream may depend on it.  Parallel entries are all filed.
//   prologue     graph_check (n and nnz), graph_reserve / graph_upload (a host-pointer entry point's graph into GraphStaging),
//                graph_validate (the launch, the one read and the one error text; in two halves for gnn_spread.hip).
#pragma once

namespace gnn {
namespace {

constexpr double CSR_W = 16777216.0;             // 2^24: a similarity of 1 as an integer weight

__device__ __forceinline__ int64_t mc_weight(float sim) { return (int64_t)rint((double)sim * CSR_W); }      // exact product, ties to even

// one thread per row; flag: a CSR that is none.  ok[i] = the row takes part
__global__ __launch_bounds__(256) void mc_validate_kernel(int64_t n, int64_t nnz, const int64_t* __restrict__ indptr, const int32_t* __restrict__ col,
                                                          const float* __restrict__ sim, const uint8_t* __restrict__ valid,
                                                          uint8_t* __restrict__ ok, unsigned long long* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    ok[i] = valid ? valid[i] != 0 : 1;
    const int64_t b = indptr[i], e = indptr[i + 1];
    bool bad = b < 0 || e < b || e > nnz || (i == 0 && b != 0) || (i == n - 1 && e != nnz);
    if (!bad)
        for (int64_t x = b; x < e; ++x) {                     // Ends: x grows towards e <= nnz
            const int32_t c = col[x];
            const float s = sim[x];
            bad |= c <= i || c >= n || !(fabsf(s) < INFINITY) || !(s < 64.0f);
        }
    if (bad) atomicOr(flag, 1ull);
}

// one thread per row: its existing edges are counted at both ends (FILL false) or filed there (FILL true) through the cursors, every
// store below the end of its row's segment
template <bool FILL>
__global__ __launch_bounds__(256) void mc_edges_kernel(int64_t n, const int64_t* __restrict__ indptr, const int32_t* __restrict__ col,
                                                       const float* __restrict__ sim, const uint8_t* __restrict__ ok, int32_t* __restrict__ deg,
                                                       const int64_t* __restrict__ soff, unsigned long long* __restrict__ cursor,
                                                       int32_t* __restrict__ sidx, uint32_t* __restrict__ sq) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !ok[i]) return;
    for (int64_t x = indptr[i]; x < indptr[i + 1]; ++x) {     // Ends: x grows towards the row's end
        const int64_t c = col[x];
        const int64_t q = mc_weight(sim[x]);
        if (q <= 0 || !ok[c]) continue;
        if (!FILL) {
            atomicAdd(deg + i, 1);
            atomicAdd(deg + c, 1);
        } else {
            const int64_t at = (int64_t)atomicAdd(cursor + i, 1ull), bt = (int64_t)atomicAdd(cursor + c, 1ull);
            if (at < soff[i + 1]) {
                sidx[at] = (int32_t)c;
                sq[at] = (uint32_t)q;
            }
            if (bt < soff[c + 1]) {
                sidx[bt] = (int32_t)i;
                sq[bt] = (uint32_t)q;
            }
        }
    }
}

// The symmetric graph of a validated CSR, enqueued on `stream`: deg[n] (zeroed here), soff[n + 1], cursor[n] and the entries sidx / sq,
// which hold 2 * nnz elements at the least.
inline int csr_symmetrise(hipStream_t stream, int64_t n, const int64_t* indptr, const int32_t* col, const float* sim, const uint8_t* ok,
                          int32_t* deg, int64_t* soff, unsigned long long* cursor, int32_t* sidx, uint32_t* sq) {
    GNN_HIP(hipMemsetAsync(deg, 0, (size_t)n * sizeof(int32_t), stream));
    if (int rc = launch_1d(mc_edges_kernel<false>, n, stream, n, indptr, col, sim, ok, deg, soff, cursor, sidx, sq)) return rc;
    if (int rc = nn_scan(stream, deg, n, soff, cursor)) return rc;
    return launch_1d(mc_edges_kernel<true>, n, stream, n, indptr, col, sim, ok, deg, soff, cursor, sidx, sq);
}

// ---- the graph prologue of every entry point ------------------------------------------------------------------------------------

constexpr int64_t CSR_N_MAX = (int64_t)1 << 24;  // a row index has 24 bits in gnn_mcl's selection key; every consumer keeps the limit

// what every consumer's arguments begin with
struct CsrGraph {
    const int64_t* indptr;     // [n + 1]
    const int32_t* col;        // [nnz]
    const float* sim;
    const uint8_t* valid;      // [n], or NULL: every row
    int64_t n, nnz;
};

// n in [0, 2^24] and nnz in [0, nnz_end), which the text calls `nnz_range`
inline int graph_check(const std::string& f, int64_t n, int64_t nnz, int64_t nnz_end, const char* nnz_range) {
    const auto bad = [&](const char* what, int64_t v, const char* range) {
        set_error(f + ": " + what + " " + std::to_string(v) + " is outside " + range);
        return GNN_ERR_ARG;
    };
    if (n < 0 || n > CSR_N_MAX) return bad("n", n, "[0, 2^24]");
    if (nnz < 0 || nnz >= nnz_end) return bad("nnz", nnz, nnz_range);
    return GNN_OK;
}
inline int graph_check(const std::string& f, int64_t n, int64_t nnz) { return graph_check(f, n, nnz, INT64_MAX, "[0, 2^63)"); }

// A host-pointer entry point's graph on the device: graph_reserve with every other reserve of the call, graph_upload behind them all -
// every buffer stands before a copy is enqueued.  g then names the copies.
inline int graph_reserve(gnn_ctx* ctx, GraphStaging& s, int64_t n, int64_t nnz) {
    int rc = nn_reserve(ctx, s.d_indptr, (size_t)n + 1);
    if (!rc) rc = nn_reserve(ctx, s.d_col, (size_t)std::max<int64_t>(nnz, 1));
    if (!rc) rc = nn_reserve(ctx, s.d_sim, (size_t)std::max<int64_t>(nnz, 1));
    if (!rc) rc = nn_reserve(ctx, s.d_valid, (size_t)n);
    return rc;
}

inline int graph_upload(gnn_ctx* ctx, GraphStaging& s, CsrGraph& g) {
    GNN_HIP(hipMemcpyAsync(s.d_indptr.get(), g.indptr, (size_t)(g.n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    if (g.nnz > 0) {
        GNN_HIP(hipMemcpyAsync(s.d_col.get(), g.col, (size_t)g.nnz * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        GNN_HIP(hipMemcpyAsync(s.d_sim.get(), g.sim, (size_t)g.nnz * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    }
    if (g.valid) GNN_HIP(hipMemcpyAsync(s.d_valid.get(), g.valid, (size_t)g.n, hipMemcpyHostToDevice, ctx->stream));
    g.indptr = s.d_indptr.get();
    g.col = s.d_col.get();
    g.sim = s.d_sim.get();
    g.valid = g.valid ? s.d_valid.get() : nullptr;
    return GNN_OK;
}

// The verdict on the graph (on the device) in two halves, so that a caller can have further launches set further bits of the same word
// (gnn_spread.hip: a label out of range) before the one read.  ok[n] receives the rows' validity; counters[flag] is zero before.
inline int graph_validate_launch(gnn_ctx* ctx, const CsrGraph& g, uint8_t* ok, HostCounters& counters, size_t flag) {
    return launch_1d(mc_validate_kernel, g.n, ctx->stream, g.n, g.nnz, g.indptr, g.col, g.sim, g.valid, ok, counters.dev() + flag);
}

// one synchronise; GNN_ERR_ARG where bit 0 stands.  word (or NULL) receives what was read
inline int graph_verdict(gnn_ctx* ctx, const char* fn, const CsrGraph& g, HostCounters& counters, size_t flag, unsigned long long* word = nullptr) {
    unsigned long long bad = 0;
    if (int rc = counters.read(ctx, flag, 1, &bad)) return rc;
    if (word) *word = bad;
    if (bad & 1) {
        set_error(std::string(fn) + ": the graph is no upper-triangle CSR of " + std::to_string(g.n) + " rows and " + std::to_string(g.nnz) +
                  " entries with similarities below 64: indptr must rise from 0 to nnz, a row's col lie in (row, n), sim be finite");
        return GNN_ERR_ARG;
    }
    return GNN_OK;
}

inline int graph_validate(gnn_ctx* ctx, const char* fn, const CsrGraph& g, uint8_t* ok, HostCounters& counters, size_t flag) {
    if (int rc = graph_validate_launch(ctx, g, ok, counters, flag)) return rc;
    return graph_verdict(ctx, fn, g, counters, flag);
}

}  // namespace
}  // namespace gnn
