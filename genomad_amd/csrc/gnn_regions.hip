// Region calls along contigs: a 3-state Viterbi path over a score track, bit-exact, on the device.
//
// Inputs.
//   - track[n_bins][3] f32 and bin_offsets[n_contigs + 1], the CSR of gnn_scan_plan / gnn_scan_contigs.
//   - A switch penalty `penalty`, a double, 0 <= penalty <= 4096, in units of score x bins.
// Emissions (exact, no transcendental on either side).
//   - Bin b is an *evidence* bin iff all three values of track[b] are finite.
//   - For an evidence bin, q[b][s] = rint(min(max(track[b][s], 0), 1) * 2^20) as an integer.  The f32 product with a power of two
//     is exact, and the rounding is to nearest, ties to even.
//   - For any other bin q[b][.] = 0.  This covers an uncovered bin (NaN by construction) and a NaN from an f16 overflow.
//   - P = rint(penalty * 2^20) as int64, computed once on the host in double.
//   - Linear scores rather than log scores make the objective the expected number of correctly labelled bins minus `penalty` per
//     switch.  They also make every quantity an integer: max and + on int64 are associative, so a parallel scan and the
//     sequential definition give identical results.
// Path, per contig with n > 0 bins, K = 3 states in class order.
//   - d[0][s] = q[0][s].
//   - d[b][s] = q[b][s] + max(d[b-1][s], max_{s' != s} d[b-1][s'] - P).
//   - Back pointer psi[b][s] = s if d[b-1][s] >= max_{s' != s}(d[b-1][s'] - P).  A tie stays.  Otherwise it is the lowest s'
//     attaining the maximum.
//   - The last bin's state is the lowest s with maximal d[n-1][s], and the path follows psi backwards.
//   - All DP values are int64.
//   - Consequences, which are also tests:
//       - At P = 0, every evidence bin gets its lowest-index argmax.
//       - At penalty = 4096, on contigs of fewer than 4096 bins, every contig is one region.
//       - A contig without any evidence bin is one region of state 0 with evidence = 0.
//       - An interior uncovered run takes a state from its neighbours and never forces a switch.
// Regions.
//   - A region is a maximal run of equal states within one contig.
//   - Regions are ordered by contig, then by position.
//   - An empty contig has no region.
//   - Each region has these fields: contig (int64); lo, hi (int64, contig-relative bins, half-open); state (uint8); evidence
//     (int64, the number of evidence bins in the region); qsum[3] (int64, the sum of q over the region).
//   - The sums are integer, so they are exact and independent of order.
//   - The Python layer derives these from the fields above: base coordinates lo * stride, min(hi * stride, L);
//     mean = qsum / (evidence * 2^20), NaN where evidence == 0; margin = (qsum[state] - max other) / 2^20.
//
// Scheme: a chunked max-plus scan.  Each contig's bins are cut into tiles of `tile` consecutive bins (default 256; the last tile
// of a contig may be short, a tile never spans contigs).  d of the bin before a tile is the tile's ENTRY vector; a contig's first
// tile enters with (0, 0, 0), which gives d[0][s] = q[0][s] + max(0, 0 - P) = q[0][s] and psi[0][s] = s: no special case.
//   1 tile transfer  one thread per tile: the tile's 3 x 3 max-plus matrix, [s'][s] = best value from s' before the tile to s at its end.
//   2 carry          one thread per contig: entry vector of every tile, in tile order; the contig's last state.
//   3 back pointers  one thread per tile: d inside the tile from its entry vector; psi per bin (3 x 2 bits in a byte) and the tile's
//                    composed map from exit state to entry state (3 x 2 bits).
//   4 carry back     one thread per contig: the path's state at every tile's exit, from the last tile to the first.
//   5 states         one thread per tile: back through its psi bytes, state[b] (uint8).
//   6 regions        flag[b] = b is a contig's first bin or state[b] != state[b - 1]; the flags' exclusive prefix sum as a count per
//                    block of 256 bins, a scan of the counts by one block, and a scan inside each block - fixed order, integers; the
//                    total is the region count.  The thread of a region's first bin writes contig, lo, state; evidence and qsum are
//                    summed per block and run in shared memory and added with one integer atomic set per (block, run); hi is the
//                    next start, or the contig's end.
// The longest sequential chain of a thread is max(tile, tiles of one contig) (phase 6: 256, and blocks / 1024 in the scan of the
// counts).  The track is read once in phase 1 and once in phase 3 (and once more by the sums of phase 6).  Tile -> contig is a
// bisection of a tile CSR built on the host from bin_offsets, as scan_track_kernel does for bins.
//
// Device memory, persistent in the ctx and grow-only (RegionWorkspace, gnn_common.h): 16 B per contig, 98 B per tile (transfer
// matrix 72, entry vector 24, composed back pointers 1, exit state 1), 1 B per bin (psi) for gnn_region_states_dev; gnn_call_regions
// adds 14 B per bin (track 12, state 1, flag 1), 12 B per 256 bins (block count and offset) and 65 B per region.
#include <cmath>
#include <cstring>

#include "gnn_common.h"

namespace gnn {

constexpr int NS = GNN_CLASSES;                  // states = classes
constexpr float Q_ONE = 1048576.f;               // 2^20
constexpr double PENALTY_MAX = 4096.0;
constexpr int TILE_MAX = 4096;
constexpr int RB = 256;                          // bins per block of the region kernels

typedef long long i64;
__host__ __device__ inline i64 imin(i64 a, i64 b) { return a < b ? a : b; }
__host__ __device__ inline i64 imax(i64 a, i64 b) { return a > b ? a : b; }

// q of one bin; returns whether it is an evidence bin
__device__ inline bool load_q(const float* __restrict__ track, int64_t b, i64 q[NS]) {
    const float v0 = track[b * NS], v1 = track[b * NS + 1], v2 = track[b * NS + 2];
    const bool ev = isfinite(v0) && isfinite(v1) && isfinite(v2);
    q[0] = ev ? (i64)rintf(fminf(fmaxf(v0, 0.f), 1.f) * Q_ONE) : 0;
    q[1] = ev ? (i64)rintf(fminf(fmaxf(v1, 0.f), 1.f) * Q_ONE) : 0;
    q[2] = ev ? (i64)rintf(fminf(fmaxf(v2, 0.f), 1.f) * Q_ONE) : 0;
    return ev;
}

// One state of one step: the lower other state first, so that `arg` is the lowest s' attaining the maximum; a tie stays.
template <int S>
__device__ inline i64 dp_state(const i64 d[NS], i64 q, i64 P, unsigned& psi) {
    constexpr int A = S == 0 ? 1 : 0, B = S == 2 ? 1 : 2;
    const bool second = d[B] > d[A];
    const i64 other = (second ? d[B] : d[A]) - P;
    const bool stay = d[S] >= other;
    psi |= (unsigned)(stay ? S : (second ? B : A)) << (2 * S);
    return q + (stay ? d[S] : other);
}

// d[b-1] -> d[b] in place; returns psi[b] as 3 x 2 bits
__device__ inline unsigned dp_step(i64 d[NS], const i64 q[NS], i64 P) {
    unsigned psi = 0;
    const i64 n0 = dp_state<0>(d, q[0], P, psi), n1 = dp_state<1>(d, q[1], P, psi), n2 = dp_state<2>(d, q[2], P, psi);
    d[0] = n0, d[1] = n1, d[2] = n2;
    return psi;
}

// the contig c with off[c] <= i < off[c + 1] (empty contigs own nothing), as scan_track_kernel
__device__ inline int64_t owner_of(const int64_t* __restrict__ off, int64_t n_contigs, int64_t i) {
    int64_t lo = 0, hi = n_contigs - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid + 1] <= i) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// tile t: its first bin and its length
__device__ inline int64_t tile_span(const int64_t* __restrict__ bin_off, const int64_t* __restrict__ tile_off, int64_t n_contigs,
                                    int64_t t, int tile, int& len) {
    const int64_t c = owner_of(tile_off, n_contigs, t);
    const int64_t first = bin_off[c] + (t - tile_off[c]) * tile;
    len = (int)imin(tile, bin_off[c + 1] - first);
    return first;
}

// ---- 1: transfer[t][s'][s]
__global__ void tile_transfer_kernel(const float* __restrict__ track, const int64_t* __restrict__ bin_off,
                                     const int64_t* __restrict__ tile_off, int64_t n_contigs, int64_t n_tiles, int tile, i64 P,
                                     i64* __restrict__ transfer) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tiles) return;
    int len;
    const int64_t first = tile_span(bin_off, tile_off, n_contigs, t, tile, len);
    i64 m[NS][NS], q[NS];
    load_q(track, first, q);
    for (int sp = 0; sp < NS; ++sp)
        for (int s = 0; s < NS; ++s) m[sp][s] = q[s] - (sp != s ? P : 0);
    for (int i = 1; i < len; ++i) {
        load_q(track, first + i, q);
        for (int sp = 0; sp < NS; ++sp) dp_step(m[sp], q, P);
    }
    for (int sp = 0; sp < NS; ++sp)
        for (int s = 0; s < NS; ++s) transfer[t * (NS * NS) + sp * NS + s] = m[sp][s];
}

// ---- 2: entry[t] = d of the bin before tile t; exit_state of the contig's last tile = the lowest s with maximal d[n - 1][s]
__global__ void carry_kernel(const i64* __restrict__ transfer, const int64_t* __restrict__ tile_off, int64_t n_contigs,
                             i64* __restrict__ entry, uint8_t* __restrict__ exit_state) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_contigs) return;
    const int64_t t0 = tile_off[c], t1 = tile_off[c + 1];
    if (t0 == t1) return;
    i64 e[NS] = {0, 0, 0};
    for (int64_t t = t0; t < t1; ++t) {
        const i64* const m = transfer + t * (NS * NS);
        i64 n[NS];
        for (int s = 0; s < NS; ++s) {
            entry[t * NS + s] = e[s];
            n[s] = imax(e[0] + m[s], imax(e[1] + m[NS + s], e[2] + m[2 * NS + s]));
        }
        for (int s = 0; s < NS; ++s) e[s] = n[s];
    }
    exit_state[t1 - 1] = e[1] > e[0] ? (e[2] > e[1] ? 2 : 1) : (e[2] > e[0] ? 2 : 0);
}

// ---- 3: psi[b], comp[t]
__global__ void backptr_kernel(const float* __restrict__ track, const int64_t* __restrict__ bin_off,
                               const int64_t* __restrict__ tile_off, int64_t n_contigs, int64_t n_tiles, int tile, i64 P,
                               const i64* __restrict__ entry, uint8_t* __restrict__ psi, uint8_t* __restrict__ comp) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tiles) return;
    int len;
    const int64_t first = tile_span(bin_off, tile_off, n_contigs, t, tile, len);
    i64 d[NS] = {entry[t * NS], entry[t * NS + 1], entry[t * NS + 2]}, q[NS];
    unsigned map = 0 | 1 << 2 | 2 << 4;          // state of the current bin -> state before the tile; the identity before bin 0
    for (int i = 0; i < len; ++i) {
        load_q(track, first + i, q);
        const unsigned p = dp_step(d, q, P);
        psi[first + i] = (uint8_t)p;
        unsigned next = 0;
        for (int s = 0; s < NS; ++s) next |= ((map >> (2 * ((p >> (2 * s)) & 3))) & 3) << (2 * s);
        map = next;
    }
    comp[t] = (uint8_t)map;
}

// ---- 4: exit_state[t - 1] = comp[t][exit_state[t]]
__global__ void carry_back_kernel(const uint8_t* __restrict__ comp, const int64_t* __restrict__ tile_off, int64_t n_contigs,
                                  uint8_t* __restrict__ exit_state) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_contigs) return;
    const int64_t t0 = tile_off[c], t1 = tile_off[c + 1];
    if (t0 == t1) return;
    unsigned s = exit_state[t1 - 1];
    for (int64_t t = t1 - 1; t > t0; --t) {
        s = (comp[t] >> (2 * s)) & 3;
        exit_state[t - 1] = (uint8_t)s;
    }
}

// ---- 5: state[b]
__global__ void states_kernel(const uint8_t* __restrict__ psi, const uint8_t* __restrict__ exit_state,
                              const int64_t* __restrict__ bin_off, const int64_t* __restrict__ tile_off, int64_t n_contigs,
                              int64_t n_tiles, int tile, uint8_t* __restrict__ state) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tiles) return;
    int len;
    const int64_t first = tile_span(bin_off, tile_off, n_contigs, t, tile, len);
    unsigned s = exit_state[t];
    for (int i = len - 1; i >= 0; --i) {
        state[first + i] = (uint8_t)s;
        s = (psi[first + i] >> (2 * s)) & 3;
    }
}

// ---- 6a: flag[b], and the flags of every block of RB bins
__global__ __launch_bounds__(RB) void region_flag_kernel(const uint8_t* __restrict__ state, const int64_t* __restrict__ bin_off,
                                                         int64_t n_contigs, int64_t n_bins, uint8_t* __restrict__ flag,
                                                         int32_t* __restrict__ blk_count) {
    const int64_t b = (int64_t)blockIdx.x * RB + threadIdx.x;
    int f = 0;
    if (b < n_bins) {
        f = b == bin_off[owner_of(bin_off, n_contigs, b)] || state[b] != state[b - 1];       // a contig's first bin never reads b - 1
        flag[b] = (uint8_t)f;
    }
    const int n = __syncthreads_count(f);
    if (threadIdx.x == 0) blk_count[blockIdx.x] = n;
}

// ---- 6b: exclusive prefix sums of the block counts, and their total behind them: nn_scan (gnn_nn_host.h)

// ---- 6c: region r of bin b = (flags before b, itself included) - 1.  The thread of a region's first bin writes contig, lo, state;
// the first thread of every run of one region inside the block sums the run's q and evidence and adds them to the region.
__global__ __launch_bounds__(RB) void region_emit_kernel(const float* __restrict__ track, const uint8_t* __restrict__ state,
                                                         const uint8_t* __restrict__ flag, const int64_t* __restrict__ bin_off,
                                                         int64_t n_contigs, int64_t n_bins, const int64_t* __restrict__ blk_off,
                                                         int64_t* __restrict__ r_contig, int64_t* __restrict__ r_lo,
                                                         uint8_t* __restrict__ r_state, int64_t* __restrict__ r_evidence,
                                                         int64_t* __restrict__ r_qsum) {
    __shared__ int scan[RB];
    __shared__ int sq[NS][RB];               // q <= 2^20
    __shared__ uint8_t sf[RB], sev[RB];
    const int tid = threadIdx.x;
    const int64_t b = (int64_t)blockIdx.x * RB + tid;
    const bool valid = b < n_bins;
    const int f = valid ? flag[b] : 0;
    i64 q[NS] = {0, 0, 0};
    const bool ev = valid && load_q(track, b, q);
    scan[tid] = f, sf[tid] = (uint8_t)f, sev[tid] = ev;
    for (int s = 0; s < NS; ++s) sq[s][tid] = (int)q[s];
    __syncthreads();
    for (int off = 1; off < RB; off <<= 1) {          // inclusive scan of the flags
        const int v = tid >= off ? scan[tid - off] : 0;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    if (!valid) return;                               // no barrier below
    const int64_t r = blk_off[blockIdx.x] + scan[tid] - 1;       // bin 0 is flagged: r >= 0
    if (f) {
        const int64_t c = owner_of(bin_off, n_contigs, b);
        r_contig[r] = c;
        r_lo[r] = b - bin_off[c];
        r_state[r] = state[b];
    }
    if (f || tid == 0) {
        const int end = (int)imin(RB, n_bins - (int64_t)blockIdx.x * RB);
        i64 sum[NS] = {0, 0, 0}, n_ev = 0;
        for (int j = tid; j < end && (j == tid || !sf[j]); ++j) {
            for (int s = 0; s < NS; ++s) sum[s] += sq[s][j];
            n_ev += sev[j];
        }
        atomicAdd(reinterpret_cast<unsigned long long*>(r_evidence + r), (unsigned long long)n_ev);
        for (int s = 0; s < NS; ++s) atomicAdd(reinterpret_cast<unsigned long long*>(r_qsum + r * NS + s), (unsigned long long)sum[s]);
    }
}

// ---- 6d: hi = the next region's lo in the same contig, or the contig's number of bins
__global__ void region_hi_kernel(const int64_t* __restrict__ r_contig, const int64_t* __restrict__ r_lo,
                                 const int64_t* __restrict__ bin_off, int64_t n_regions, int64_t* __restrict__ r_hi) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_regions) return;
    const int64_t c = r_contig[r];
    r_hi[r] = r + 1 < n_regions && r_contig[r + 1] == c ? r_lo[r + 1] : bin_off[c + 1] - bin_off[c];
}

// What both entry points check before the ctx is looked at: the penalty and the offsets.  n_bins counts from bin_offsets[0].
static int check_region_args(const char* fn, const int64_t* bin_offsets, int64_t n_contigs, double penalty) {
    if (!(penalty >= 0.0 && penalty <= PENALTY_MAX)) {       // a NaN fails both comparisons
        set_error(std::string(fn) + ": penalty " + std::to_string(penalty) + " is outside [0, 4096]");
        return GNN_ERR_ARG;
    }
    if (!bin_offsets || n_contigs < 0) {
        set_error(std::string("bad argument to ") + fn);
        return GNN_ERR_ARG;
    }
    if (bin_offsets[0] < 0) {
        set_error(std::string(fn) + ": the first bin offset " + std::to_string(bin_offsets[0]) + " is outside [0, 2^63)");
        return GNN_ERR_ARG;
    }
    for (int64_t c = 0; c < n_contigs; ++c)
        if (bin_offsets[c + 1] < bin_offsets[c]) {
            set_error(std::string(fn) + ": bin offsets are not non-decreasing: offset " + std::to_string(c + 1) + " is " +
                      std::to_string(bin_offsets[c + 1]) + ", below " + std::to_string(bin_offsets[c]) + "; each must lie in [previous, 2^63)");
            return GNN_ERR_ARG;
        }
    return GNN_OK;
}

static RegionWorkspace& region_ws(gnn_ctx* ctx) {
    if (!ctx->contig_ws) ctx->contig_ws = new ContigWorkspace();
    return ctx->contig_ws->regions;
}

// Phases 1 - 5 on ctx->stream: track and state are device pointers to the contigs' first bin (bin_offsets[0]); n_bins > 0.
static int region_states(gnn_ctx* ctx, RegionWorkspace& w, const float* track, const int64_t* bin_offsets, int64_t n_contigs,
                         double penalty, uint8_t* state) {
    const int tile = w.tile;
    const int64_t base = bin_offsets[0];
    // ---- the bin CSR from its first bin and the tile CSR, in pinned memory the previous call's upload has left
    if (w.tables_read) GNN_HIP(hipEventSynchronize(w.tables_read));
    else GNN_HIP(hipEventCreateWithFlags(&w.tables_read, hipEventDisableTiming));
    const size_t no = (size_t)n_contigs + 1;
    int rc = w.h_off.reserve(2 * no, no / 2 + 64);
    if (rc) return rc;
    int64_t* const bin_off = w.h_off.get();
    int64_t* const tile_off = bin_off + no;
    tile_off[0] = 0;
    for (int64_t c = 0; c <= n_contigs; ++c) bin_off[c] = bin_offsets[c] - base;
    for (int64_t c = 0; c < n_contigs; ++c) tile_off[c + 1] = tile_off[c] + (bin_off[c + 1] - bin_off[c] + tile - 1) / tile;
    const int64_t n_bins = bin_off[n_contigs], n_tiles = tile_off[n_contigs];
    // ---- reserve: a buffer that grows is freed first, and nothing may still read it
    if (w.d_off.capacity() < 2 * no || w.d_transfer.capacity() < (size_t)n_tiles * NS * NS || w.d_entry.capacity() < (size_t)n_tiles * NS ||
        w.d_comp.capacity() < (size_t)n_tiles || w.d_exit.capacity() < (size_t)n_tiles || w.d_psi.capacity() < (size_t)n_bins)
        GNN_HIP(hipStreamSynchronize(ctx->stream));
    if ((rc = reserve_roomy(w.d_off, 2 * no))) return rc;
    if ((rc = reserve_roomy(w.d_transfer, (size_t)n_tiles * NS * NS))) return rc;
    if ((rc = reserve_roomy(w.d_entry, (size_t)n_tiles * NS))) return rc;
    if ((rc = reserve_roomy(w.d_comp, (size_t)n_tiles))) return rc;
    if ((rc = reserve_roomy(w.d_exit, (size_t)n_tiles))) return rc;
    if ((rc = reserve_roomy(w.d_psi, (size_t)n_bins))) return rc;
    GNN_HIP(hipMemcpyAsync(w.d_off, bin_off, 2 * no * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    GNN_HIP(hipEventRecord(w.tables_read, ctx->stream));
    const int64_t* const d_bin = w.d_off;
    const int64_t* const d_tile = w.d_off + no;
    const i64 P = std::llrint(penalty * (double)Q_ONE);
    i64* const transfer = reinterpret_cast<i64*>(w.d_transfer.get());
    i64* const entry = reinterpret_cast<i64*>(w.d_entry.get());
    ProfScope prof(ctx, GNN_K_REGIONS);
    if ((rc = launch_1d(tile_transfer_kernel, n_tiles, ctx->stream, track, d_bin, d_tile, n_contigs, n_tiles, tile, P, transfer))) return rc;
    if ((rc = launch_1d(carry_kernel, n_contigs, ctx->stream, transfer, d_tile, n_contigs, entry, w.d_exit))) return rc;
    if ((rc = launch_1d(backptr_kernel, n_tiles, ctx->stream, track, d_bin, d_tile, n_contigs, n_tiles, tile, P, entry, w.d_psi, w.d_comp)))
        return rc;
    if ((rc = launch_1d(carry_back_kernel, n_contigs, ctx->stream, w.d_comp, d_tile, n_contigs, w.d_exit))) return rc;
    return launch_1d(states_kernel, n_tiles, ctx->stream, w.d_psi, w.d_exit, d_bin, d_tile, n_contigs, n_tiles, tile, state);
}

}  // namespace gnn

using namespace gnn;

extern "C" int gnn_debug_set_region_tile(gnn_ctx* ctx, int bins) {
    if (int rc = check_ctx(ctx)) return rc;
    if (bins < 1 || bins > TILE_MAX) {
        set_error("gnn_debug_set_region_tile: " + std::to_string(bins) + " bins per tile is outside [1, " + std::to_string(TILE_MAX) + "]");
        return GNN_ERR_ARG;
    }
    region_ws(ctx).tile = bins;
    return GNN_OK;
}

extern "C" int gnn_region_states_dev(gnn_ctx* ctx, const float* track_dev, const int64_t* bin_offsets_host, int64_t n_contigs,
                                     double penalty, uint8_t* state_dev) {
    const char* const fn = "gnn_region_states_dev";
    if (int rc = check_region_args(fn, bin_offsets_host, n_contigs, penalty)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (bin_offsets_host[n_contigs] == bin_offsets_host[0]) return GNN_OK;
    if (!track_dev || !state_dev) {
        set_error(std::string("bad argument to ") + fn);
        return GNN_ERR_ARG;
    }
    const int64_t base = bin_offsets_host[0];
    return region_states(ctx, region_ws(ctx), track_dev + base * NS, bin_offsets_host, n_contigs, penalty, state_dev + base);
}

extern "C" int gnn_call_regions(gnn_ctx* ctx, const float* track_host, const int64_t* bin_offsets_host, int64_t n_contigs, double penalty,
                                uint8_t* state_host_or_null, int64_t* region_contig, int64_t* region_lo, int64_t* region_hi,
                                uint8_t* region_state, int64_t* region_evidence, int64_t* region_qsum, int64_t regions_capacity,
                                int64_t* n_regions_out) {
    const char* const fn = "gnn_call_regions";
    if (int rc = check_region_args(fn, bin_offsets_host, n_contigs, penalty)) return rc;
    const int given = !!region_contig + !!region_lo + !!region_hi + !!region_state + !!region_evidence + !!region_qsum;
    if (!n_regions_out || (given != 0 && given != 6) || regions_capacity < 0) {
        set_error(std::string("bad argument to ") + fn + ": n_regions_out is required, and the six region arrays are given or NULL together");
        return GNN_ERR_ARG;
    }
    if (int rc = check_ctx(ctx)) return rc;
    *n_regions_out = 0;
    const int64_t base = bin_offsets_host[0], n_bins = bin_offsets_host[n_contigs] - base;
    if (n_bins == 0) return GNN_OK;
    if (!track_host) {
        set_error(std::string("bad argument to ") + fn + ": track_host is NULL");
        return GNN_ERR_ARG;
    }
    RegionWorkspace& w = region_ws(ctx);
    hipStream_t const stream = ctx->stream;
    const int64_t n_blocks = (n_bins + RB - 1) / RB;
    int rc = GNN_OK;
    if (w.d_track.capacity() < (size_t)n_bins * NS || w.d_state.capacity() < (size_t)n_bins || w.d_flag.capacity() < (size_t)n_bins ||
        w.d_blk_count.capacity() < (size_t)n_blocks || w.d_blk_off.capacity() < (size_t)n_blocks + 1)
        GNN_HIP(hipStreamSynchronize(stream));      // a buffer that grows is freed first: nothing may still read it
    if ((rc = reserve_roomy(w.d_track, (size_t)n_bins * NS))) return rc;
    if ((rc = reserve_roomy(w.d_state, (size_t)n_bins))) return rc;
    if ((rc = reserve_roomy(w.d_flag, (size_t)n_bins))) return rc;
    if ((rc = reserve_roomy(w.d_blk_count, (size_t)n_blocks))) return rc;
    if ((rc = reserve_roomy(w.d_blk_off, (size_t)n_blocks + 1))) return rc;
    GNN_HIP(hipMemcpyAsync(w.d_track, track_host + base * NS, (size_t)n_bins * NS * sizeof(float), hipMemcpyHostToDevice, stream));
    if ((rc = region_states(ctx, w, w.d_track, bin_offsets_host, n_contigs, penalty, w.d_state))) return rc;
    const int64_t* const d_bin = w.d_off;        // region_states has uploaded the bin CSR, counted from the first bin
    // ---- the flags and their prefix sums; the total is the region count
    {
        ProfScope prof(ctx, GNN_K_REGIONS);
        hipLaunchKernelGGL(region_flag_kernel, dim3((unsigned)n_blocks), dim3(RB), 0, stream, w.d_state.get(), d_bin, n_contigs, n_bins,
                           w.d_flag.get(), w.d_blk_count.get());
        if ((rc = nn_scan(stream, w.d_blk_count, n_blocks, w.d_blk_off, nullptr))) return rc;
    }
    int64_t n_regions = 0;
    GNN_HIP(hipMemcpyAsync(&n_regions, w.d_blk_off + n_blocks, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    if (state_host_or_null)
        GNN_HIP(hipMemcpyAsync(state_host_or_null + base, w.d_state, (size_t)n_bins, hipMemcpyDeviceToHost, stream));
    GNN_HIP(hipStreamSynchronize(stream));
    *n_regions_out = n_regions;
    if (!given) return GNN_OK;
    if (regions_capacity < n_regions) {
        set_error("the region arrays hold " + std::to_string(regions_capacity) + " regions, the call has " + std::to_string(n_regions));
        return GNN_ERR_ARG;
    }
    // ---- the regions (the stream is idle: buffers may grow)
    const size_t nr = (size_t)n_regions;
    if ((rc = reserve_roomy(w.d_r_contig, nr))) return rc;
    if ((rc = reserve_roomy(w.d_r_lo, nr))) return rc;
    if ((rc = reserve_roomy(w.d_r_hi, nr))) return rc;
    if ((rc = reserve_roomy(w.d_r_state, nr))) return rc;
    if ((rc = reserve_roomy(w.d_r_evidence, nr))) return rc;
    if ((rc = reserve_roomy(w.d_r_qsum, nr * NS))) return rc;
    GNN_HIP(hipMemsetAsync(w.d_r_evidence, 0, nr * sizeof(int64_t), stream));
    GNN_HIP(hipMemsetAsync(w.d_r_qsum, 0, nr * NS * sizeof(int64_t), stream));
    {
        ProfScope prof(ctx, GNN_K_REGIONS);
        hipLaunchKernelGGL(region_emit_kernel, dim3((unsigned)n_blocks), dim3(RB), 0, stream, w.d_track.get(), w.d_state.get(), w.d_flag.get(),
                           d_bin, n_contigs, n_bins, w.d_blk_off.get(), w.d_r_contig.get(), w.d_r_lo.get(), w.d_r_state.get(),
                           w.d_r_evidence.get(), w.d_r_qsum.get());
        GNN_HIP(hipGetLastError());
        if ((rc = launch_1d(region_hi_kernel, n_regions, stream, w.d_r_contig, w.d_r_lo, d_bin, n_regions, w.d_r_hi))) return rc;
    }
    GNN_HIP(hipMemcpyAsync(region_contig, w.d_r_contig, nr * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    GNN_HIP(hipMemcpyAsync(region_lo, w.d_r_lo, nr * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    GNN_HIP(hipMemcpyAsync(region_hi, w.d_r_hi, nr * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    GNN_HIP(hipMemcpyAsync(region_state, w.d_r_state, nr, hipMemcpyDeviceToHost, stream));
    GNN_HIP(hipMemcpyAsync(region_evidence, w.d_r_evidence, nr * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    GNN_HIP(hipMemcpyAsync(region_qsum, w.d_r_qsum, nr * NS * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    GNN_HIP(hipStreamSynchronize(stream));
    return GNN_OK;
}
