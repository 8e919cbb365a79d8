// What the consumers of the similarity graph's CSR share on the device (gnn_mcl.hip, gnn_spread.hip): the verdict on the graph and
// its symmetric form.  Included behind gnn_nn_frag.h (nn_reserve, launch_1d, nn_scan); everything here has internal linkage.
//   validate     one thread per row: indptr rises within [0, nnz], every col lies in (row, n), every sim is finite and < 64.  The host
//                reads one flag; GNN_ERR_ARG before anything else runs, the outputs untouched.  It also writes the rows' validity.
//   symmetrise   the edges that exist (q = rint(sim * W) > 0, both ends valid) are counted at both ends (integer adds), the counts
//                scanned by one block, the edges filed through per-row cursors.  A row's entries stand in arrival order: nothing
//                downstream may depend on it.  Parallel entries are all filed.
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

}  // namespace
}  // namespace gnn
