// Spherical k-means among encoder embeddings (include/genomad_nn.h, "spherical k-means"): a partition of the
// valid rows into exactly k groups under cosine similarity and one unit centroid per group, the iteration on the device.
//   prepare    nn_prepare (gnn_neighbours.hip), as it is: the rows' fragments and flags in the neighbour search's buffers, the centroids'
//              (k f32 unit rows, after every update) in this search's own.
//   assign     the tile parts of gnn_nn_frag.h over the plain rectangle rows x centroids: the tile is 64 data rows in LDS, the columns
//              are centroid fragments, the value of (row i, centroid c) IS the f32 gnn_neighbours returns for query i and base row c.
//              A lane keeps nn_key(nn_image(s), c) per accumulator register, the row side is folded by shuffles and one LDS maximum,
//              and a workgroup ends with one 64-bit atomicMax per row: the largest similarity, among equals the smallest centroid.
//              Columns at or beyond k and invalid rows are masked (a padded column is a zero fragment: its 0 would beat every
//              negative similarity).
//   label      key -> label / sim, the changed labels counted by an integer add, the key cleared for the next assign.  The host reads
//              those 8 bytes: the one synchronise of an iteration.
//   update     S[c][d] += q_i[d] in int64, q_i = (hi + lo) * 2^24 of row i's own fragments: every f16 is a multiple of 2^-24, so q is
//              exact, a pure function of the row, and a 32-bit fixed-point image of its unit vector (the fragments hold unit * 2^8).
//              |q| < 2^33, so n <= 2^30 rows cannot overflow a sum (N_MAX).  Integer adds commute: any order gives the same bits.  Up
//              to 128 centroids a workgroup adds in LDS first, a window of 16 at a time, and flushes once per window (gnn_debug_set_kmeans_lds);
//              beyond, straight to memory.
//   finish     S -> unit f32 rows: the squares summed in float64 per lane in element order and over the lanes by a fixed butterfly,
//              v / norm rounded to f32 once.  A centroid without members or with a zero sum keeps its row bit for bit (gnn_centroids:
//              becomes a zero row).  Then nn_prepare on the k rows.
//   far / pick farthest-first init: a 64-bit minimum of (image of the best similarity so far, row) over the valid unpicked rows, the
//              row's fragments copied into a one-column base, assign against it with the pick's number as the column: keys merge by
//              maximum into the rows' running keys.  The values are gnn_neighbours' for (row, that row alone as the base).
// Atomics are integer add / max / min only, stores are vector stores, nothing depends on the order the workgroups run in or on the
// split of the centroids (gnn_debug_set_neighbour_split).  No loop here waits for another workgroup: every loop's termination argument
// stands next to it.  Memory: 8 B per row, 4 KB + 8 B per centroid, one 128 KB one-column base; nothing is n x k.
#include <cmath>

#include "gnn_nn_frag.h"

namespace gnn {
namespace {

constexpr int64_t N_MAX = (int64_t)1 << 30;      // |q| < 2^33 per element and row: the int64 sums of 2^30 rows stay below 2^63
constexpr int K_MAX = 65535;
constexpr int MAX_ITER_MAX = 1000;
constexpr int LDS_K = 16;                        // groups whose sums a workgroup holds in LDS at a time: 16 x 4 KB
constexpr int LDS_K_MAX = 128;                   // up to this many groups the update may go through LDS, in windows of LDS_K
constexpr unsigned long long NO_PICK = ~0ull;

struct AssignArgs {
    const uint4* frag;         // the rows: round_up(n, 64) / 32 blocks
    const uint8_t* valid;      // [round_up(n, 64)]
    int64_t n;
    const uint4* cfrag;        // the columns: round_up(k, 64) / 32 blocks
    const uint8_t* cvalid;     // [round_up(k, 64)]
    int64_t k;                 // columns of this launch
    unsigned col_off;          // what column 0 is called in the keys (farthest-first: the pick's number)
    int64_t split_rows;        // columns per workgroup: a multiple of 32
    float scale;               // 2^-16: cosine
    unsigned long long* key;   // at a row: max of (image of the similarity << 32) | (2^32 - 1 - centroid), 0: none
};

// grid = (row tiles, centroid ranges), 256 threads.  LDS: the tile's fragments 128 KB, its rows' keys and flags.
__global__ __launch_bounds__(256) void km_assign_kernel(AssignArgs a) {
    __shared__ uint4 qs[2 * BLK_U4];
    __shared__ unsigned long long lkey[QT];    // the best centroids of the tile's rows among this workgroup's columns: flushed once
    __shared__ uint8_t lok[QT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
    TileRange t;
    nn_tile_range(t, a.split_rows, a.k, false);            // never empty: the host launches no empty range
    const int64_t r0 = t.r0;
    nn_copy_tile(qs, a.frag, tid);
    if (tid < QT) {
        lkey[tid] = 0;
        lok[tid] = r0 + tid < a.n && a.valid[r0 + tid];
    }
    __syncthreads();
    unsigned long long best[2][16];            // per accumulator register: the lane's columns so far
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int r = 0; r < 16; ++r) best[mb][r] = 0;
    const int64_t last_blk = t.last_blk();
    // Ends: c0 grows by STEP towards b1.
    for (int64_t c0 = t.c0; c0 < t.b1; c0 += STEP) {
        const uint4* bp[2];
        int cg[2];                             // the lane's column, -1: masked (at or beyond k: a padded column is a zero fragment)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const int64_t col = nn_step_column(a.cfrag, c0, wave, lane, nb, last_blk, bp[nb]);
            cg[nb] = col < t.b1 && a.cvalid[col] ? (int)col : -1;
        }
        f32x16 acc[2][2];
        NN_PRODUCTS(qs, bp, lane, acc);
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            if (cg[nb] < 0) continue;
            const unsigned c = a.col_off + (unsigned)cg[nb];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const unsigned long long key = nn_key(nn_image(acc[mb][nb][r] * a.scale), c);
                    best[mb][r] = key > best[mb][r] ? key : best[mb][r];
                }
        }
    }
    // ---- the row side: a row's candidates lie in one register of the 32 lanes of a half.  An invalid row is masked here
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = nn_acc_row(mb, r, half);
            unsigned long long key = lok[row] ? best[mb][r] : 0;
#pragma unroll
            for (int s = 16; s > 0; s >>= 1) {
                const unsigned long long other = __shfl_xor(key, s);
                key = other > key ? other : key;
            }
            if ((lane & 31) == 0 && key) atomicMax(&lkey[row], key);
        }
    __syncthreads();
    if (tid < QT && lkey[tid]) atomicMax(a.key + r0 + tid, lkey[tid]);          // lkey > 0 only at a valid row < n
}

// Every thread reaches the ballot.  label = -1 and sim = NaN where no key was written: an invalid row.
__global__ __launch_bounds__(256) void km_label_kernel(int64_t n, unsigned long long* __restrict__ key, int64_t* __restrict__ label,
                                                       float* __restrict__ sim, unsigned long long* __restrict__ changed) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool moved = false;
    if (i < n) {
        const unsigned long long b = key[i];
        const int64_t l = b ? (int64_t)nn_key_index(b) : -1;
        moved = label[i] != l;
        label[i] = l;
        sim[i] = b ? nn_unimage((unsigned)(b >> 32)) : __builtin_nanf("");
        key[i] = 0;
    }
    const int c = __popcll(__ballot(moved));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(changed, (unsigned long long)c);
}

__global__ __launch_bounds__(256) void km_fill_kernel(int64_t n, int64_t value, int64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = value;
}

// census[0] += valid rows, census[1] += invalid init rows (n_init = 0: no init was given).  Every thread reaches the ballots.
__global__ __launch_bounds__(256) void km_census_kernel(int64_t n, const uint8_t* __restrict__ valid, int64_t n_init,
                                                        const uint8_t* __restrict__ ivalid, unsigned long long* __restrict__ census) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int ok = __popcll(__ballot(i < n && valid[i])), bad = __popcll(__ballot(i < n_init && !ivalid[i]));
    if ((threadIdx.x & 63) == 0) {
        if (ok) atomicAdd(census, (unsigned long long)ok);
        if (bad) atomicAdd(census + 1, (unsigned long long)bad);
    }
}

// gnn_centroids: a label outside [-1, k) raises the flag (every writer writes the same value)
__global__ __launch_bounds__(256) void km_check_kernel(int64_t n, int64_t k, const int64_t* __restrict__ label,
                                                       unsigned long long* __restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && (label[i] < -1 || label[i] >= k)) *bad = 1;
}

struct UpdateArgs {
    const uint4* frag;         // the items' rows live here
    const uint8_t* valid;
    int64_t items;
    const int64_t* pick;       // item i is row pick[i]; NULL: row i
    const int64_t* label;      // the row's group; NULL: item i is group i
    int64_t k;
    unsigned long long* S;     // [k][D] int64 sums, two's complement
    unsigned long long* cnt;   // [k] members
};

// grid = ceil(items / per_block), 256 threads: wave w takes the block's items w, w + 4, ...; lane l the row's elements 8 l .. 8 l + 7,
// the 16-byte chunk of its hi and of its lo fragment.  LDS: the sums of a window of LDS_K groups, element e of every lane side by side
// (no bank is hit twice by a wave), flushed once per window: k x 512 global adds per workgroup instead of 512 per row.
template <bool LDS>
__global__ __launch_bounds__(256) void km_update_kernel(UpdateArgs a, int64_t per_block) {
    __shared__ unsigned long long ls[LDS ? LDS_K * D : 1];
    __shared__ unsigned long long lc[LDS ? LDS_K : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * per_block, i1 = min(a.items, i0 + per_block);
    // LDS: one pass over the block's items per window of LDS_K groups - a row's fragments are read in its own group's window only.
    // Ends: w0 grows by LDS_K towards k; straight to memory: one pass.
    for (int64_t w0 = 0; w0 < (LDS ? a.k : 1); w0 += LDS_K) {
        if (LDS) {
            for (int i = tid; i < LDS_K * D; i += 256) ls[i] = 0;
            if (tid < LDS_K) lc[tid] = 0;
            __syncthreads();
        }
        // Ends: i grows by 4 towards i1.
        for (int64_t i = i0 + wave; i < i1; i += 4) {
            const int64_t row = a.pick ? a.pick[i] : i;
            const int64_t l = a.label ? a.label[row] : i;
            if (l < 0 || l >= a.k || !a.valid[row]) continue;      // wave-uniform
            if (LDS && (l < w0 || l >= w0 + LDS_K)) continue;      // another window's
            const uint4* p = a.frag + (row / 32 * NKS + (lane >> 1)) * 128 + (lane & 1) * 32 + (row & 31);
            const f16x8 hi = __builtin_bit_cast(f16x8, p[0]), lo = __builtin_bit_cast(f16x8, p[64]);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                // exact: an f16 times 2^24 is an integer below 2^41 in magnitude, and an f32 holds its 11 bits
                const long long q = (long long)((float)hi[e] * 16777216.f) + (long long)((float)lo[e] * 16777216.f);
                if (!q) continue;
                if (LDS)
                    atomicAdd(&ls[((l - w0) * 8 + e) * 64 + lane], (unsigned long long)q);
                else
                    atomicAdd(a.S + l * D + lane * 8 + e, (unsigned long long)q);
            }
            if (lane == 0) atomicAdd(LDS ? &lc[l - w0] : a.cnt + l, 1ull);
        }
        if (LDS) {
            __syncthreads();
            const int64_t m = min(a.k - w0, (int64_t)LDS_K) * D;
            for (int i = tid; i < m; i += 256) {
                const int l = i / D, e = (i >> 6) & 7, ln = i & 63;
                if (ls[i]) atomicAdd(a.S + (w0 + l) * D + ln * 8 + e, ls[i]);
            }
            if (w0 + tid < a.k && tid < LDS_K && lc[tid]) atomicAdd(a.cnt + w0 + tid, lc[tid]);
            __syncthreads();               // the next window clears what this one has flushed
        }
    }
}

// grid = k, 64 threads = one wave per centroid.  zero_empty: a group without members or with a zero sum becomes a zero row
// (gnn_centroids); otherwise its row stays as it is.
__global__ __launch_bounds__(64) void km_finish_kernel(const unsigned long long* __restrict__ S, const unsigned long long* __restrict__ cnt,
                                                       int zero_empty, float* __restrict__ cent) {
    const int lane = threadIdx.x;
    const int64_t c = blockIdx.x;
    double v[8], ss = 0.0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        v[e] = (double)(long long)S[c * D + lane * 8 + e];
        ss += v[e] * v[e];
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) ss += __shfl_xor(ss, s);
    const bool keep = cnt[c] == 0 || !(ss > 0.0);
    if (keep && !zero_empty) return;
    const double norm = sqrt(ss);
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = keep ? 0.f : (float)(v[e] / norm);
    float4* dst = reinterpret_cast<float4*>(cent + c * D) + lane * 2;
    dst[0] = make_float4(o[0], o[1], o[2], o[3]);
    dst[1] = make_float4(o[4], o[5], o[6], o[7]);
}

__global__ __launch_bounds__(256) void km_size_kernel(int64_t n, int64_t k, const int64_t* __restrict__ label,
                                                      unsigned long long* __restrict__ size) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && label[i] >= 0 && label[i] < k) atomicAdd(size + label[i], 1ull);
}

// farthest-first: the minimum of (image of the row's best similarity to the picks so far, row) over the valid unpicked rows.  A row
// without a key (before the first pick) has image 0: the first pick is the valid row of smallest index.  Every thread reaches the
// shuffles.
__global__ __launch_bounds__(256) void km_far_kernel(int64_t n, const uint8_t* __restrict__ valid, const uint8_t* __restrict__ picked,
                                                     const unsigned long long* __restrict__ key, unsigned long long* __restrict__ best) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long v = NO_PICK;
    if (i < n && valid[i] && !picked[i]) v = (key[i] & ~LOW32) | (unsigned long long)i;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const unsigned long long other = __shfl_xor(v, s);
        v = other < v ? other : v;
    }
    if ((threadIdx.x & 63) == 0 && v != NO_PICK) atomicMin(best, v);
}

// one wave: the chosen row becomes pick j - its fragments go to row 0 of the one-column base (the other 63 rows stay zero) - and the
// minimum is cleared for the next pick.  No candidate (k > valid rows; the host has refused that): nothing happens.
__global__ __launch_bounds__(64) void km_pick_kernel(const uint4* __restrict__ frag, unsigned long long* __restrict__ best, int64_t j,
                                                     int64_t* __restrict__ picks, uint8_t* __restrict__ picked, uint4* __restrict__ one) {
    const int lane = threadIdx.x;
    const unsigned long long b = *best;
    if (b == NO_PICK) return;
    const int64_t row = (int64_t)(b & LOW32);
    const uint4* src = frag + (row / 32 * NKS + (lane >> 1)) * 128 + (lane & 1) * 32 + (row & 31);
    uint4* dst = one + (lane >> 1) * 128 + (lane & 1) * 32;
    dst[0] = src[0];
    dst[64] = src[64];
    __syncthreads();                       // every lane has read *best
    if (lane == 0) {
        picks[j] = row;
        picked[row] = 1;
        *best = NO_PICK;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

int check_rows(const std::string& f, int64_t n) {
    if (n >= 0 && n <= N_MAX) return GNN_OK;
    set_error(f + ": " + std::to_string(n) + " rows is outside [0, 2^30]: the int64 sums of more rows could overflow");
    return GNN_ERR_ARG;
}

int check_k(const std::string& f, int64_t k) {
    if (k >= 1 && k <= K_MAX) return GNN_OK;
    set_error(f + ": k " + std::to_string(k) + " is outside [1, " + std::to_string(K_MAX) + "]");
    return GNN_ERR_ARG;
}

int check_kmeans_args(const char* fn, const void* rows, int64_t n, int k, int max_iter, const void* label, const void* sim, const void* cent,
                      const void* size, const void* init_rows, const void* iterations, const void* converged) {
    const std::string f(fn);
    if (int rc = check_rows(f, n)) return rc;
    if (int rc = check_k(f, k)) return rc;
    if (max_iter < 0 || max_iter > MAX_ITER_MAX) {
        set_error(f + ": max_iter " + std::to_string(max_iter) + " is outside [0, " + std::to_string(MAX_ITER_MAX) + "]");
        return GNN_ERR_ARG;
    }
    return nn_check_required(f, cent && size && init_rows && iterations && converged && (n == 0 || (rows && label && sim)),
                             "the rows, the five outputs, iterations and converged");
}

int check_centroid_args(const char* fn, const void* rows, int64_t n, const void* label, int k, const void* cent, const void* size) {
    const std::string f(fn);
    if (int rc = check_rows(f, n)) return rc;
    if (int rc = check_k(f, k)) return rc;
    return nn_check_required(f, cent && size && (n == 0 || (rows && label)), "the rows, the labels and both outputs");
}

enum { C_CHANGED = 0, C_VALID = 1, C_BAD_INIT = 2, C_BAD_LABEL = 3, C_BEST = 4, C_WORDS = 5 };

int km_reserve(gnn_ctx* ctx, int64_t n, int64_t k) {
    KMeansWorkspace& m = ctx->km;
    int rc = nn_reserve(ctx, m.key, (size_t)std::max<int64_t>(n, 1));
    if (!rc) rc = nn_reserve(ctx, m.S, (size_t)k * D);
    if (!rc) rc = nn_reserve(ctx, m.cnt, (size_t)k);
    if (!rc) rc = m.count.reserve(ctx, C_WORDS);
    return rc;
}

// The sums of `items` rows by group -> k rows of `cent`, enqueued.  The sums and counts are cleared here.  log: where the two passes
// (update, finish) are timed, or NULL.
int km_update(gnn_ctx* ctx, const uint4* frag, const uint8_t* valid, int64_t items, const int64_t* pick, const int64_t* label, int64_t k,
              int zero_empty, float* cent, PassLog* log) {
    KMeansWorkspace& m = ctx->km;
    {
        PassLog::Scope pass(ctx, log);
        GNN_HIP(hipMemsetAsync(m.S.get(), 0, (size_t)k * D * sizeof(unsigned long long), ctx->stream));
        GNN_HIP(hipMemsetAsync(m.cnt.get(), 0, (size_t)k * sizeof(unsigned long long), ctx->stream));
        if (items > 0) {
            UpdateArgs u;
            u.frag = frag;
            u.valid = valid;
            u.items = items;
            u.pick = pick;
            u.label = label;
            u.k = k;
            u.S = m.S.get();
            u.cnt = m.cnt.get();
            if (k <= m.lds_k) {
                // few groups: every add would land on k x 512 addresses, and a workgroup's rows are more than its groups.  A workgroup
                // per 1 / (2 x CUs) of the rows, 64 rows at the least
                const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((items + 63) / 64, 2 * std::max(ctx->cu_count, 1)));
                const int64_t per_block = (items + blocks - 1) / blocks;
                hipLaunchKernelGGL(km_update_kernel<true>, dim3((unsigned)((items + per_block - 1) / per_block)), dim3(256), 0, ctx->stream, u,
                                   per_block);
            } else {
                hipLaunchKernelGGL(km_update_kernel<false>, dim3((unsigned)((items + 63) / 64)), dim3(256), 0, ctx->stream, u, (int64_t)64);
            }
            GNN_HIP(hipGetLastError());
        }
    }
    PassLog::Scope pass(ctx, log);
    hipLaunchKernelGGL(km_finish_kernel, dim3((unsigned)k), dim3(64), 0, ctx->stream, m.S.get(), m.cnt.get(), zero_empty, cent);
    GNN_HIP(hipGetLastError());
    return GNN_OK;
}

int km_assign(gnn_ctx* ctx, const char* fn, int64_t n, const uint4* cfrag, const uint8_t* cvalid, int64_t k, unsigned col_off) {
    NeighbourWorkspace& w = ctx->nn;
    const int64_t tiles = (n + QT - 1) / QT;
    int64_t split_rows, splits;
    if (int rc = nn_tile_grid(ctx, fn, "centroids", tiles, k, &split_rows, &splits)) return rc;
    AssignArgs a;
    a.frag = w.bfrag.get();
    a.valid = w.bvalid.get();
    a.n = n;
    a.cfrag = cfrag;
    a.cvalid = cvalid;
    a.k = k;
    a.col_off = col_off;
    a.split_rows = split_rows;
    a.scale = nn_metric_scale(GNN_KNN_COSINE);
    a.key = ctx->km.key.get();
    return launch_tiles(km_assign_kernel, tiles, splits, ctx->stream, a);
}

// n >= 0 rows on the device -> the five arrays on the device, iterations and converged on the host.  The ctx's stream is synchronised
// once at the start (the valid rows and the init's verdict) and once per assignment (the changed labels).
int km_run(gnn_ctx* ctx, const char* fn, const float* rows_dev, int64_t n, int k, const float* init_dev, int max_iter, int64_t* label, float* sim,
           float* cent, int64_t* size, int64_t* init_rows, int64_t* iterations_out, int* converged_out) {
    const std::string f(fn);
    NeighbourWorkspace& w = ctx->nn;
    KMeansWorkspace& m = ctx->km;
    m.passes.begin();
    int rc = nn_prepare(ctx, rows_dev, n, GNN_KNN_COSINE, w.bfrag, w.bvalid);
    if (!rc) rc = km_reserve(ctx, n, k);
    if (!rc && init_dev) rc = nn_prepare(ctx, init_dev, k, GNN_KNN_COSINE, m.cfrag, m.cvalid);
    if (!rc) rc = m.count.zero(ctx, 0, C_WORDS);
    if (rc) return rc;
    const int64_t cells = std::max<int64_t>(n, init_dev ? k : 0);
    if (cells > 0)
        if ((rc = launch_1d(km_census_kernel, cells, ctx->stream, n, w.bvalid.get(), (int64_t)(init_dev ? k : 0), m.cvalid.get(),
                            m.count.dev() + C_VALID)))
            return rc;
    unsigned long long census[2] = {0, 0};
    if ((rc = m.count.read(ctx, C_VALID, 2, census))) return rc;
    if ((unsigned long long)k > census[0]) {
        set_error(f + ": k " + std::to_string(k) + " is more than the " + std::to_string(census[0]) + " valid rows of " + std::to_string(n));
        return GNN_ERR_ARG;
    }
    if (census[1]) {
        set_error(f + ": " + std::to_string(census[1]) + " of the " + std::to_string(k) + " init rows are not valid (finite, norm > 0)");
        return GNN_ERR_ARG;
    }
    // every pass is settled behind a later synchronise: the next assignment's read
    if (init_dev) {
        // the init's rows, each a group of its own: the centroids are their unit rows by the update's own arithmetic
        PassLog::Scope init(ctx, m.passes);
        if ((rc = launch_1d(km_fill_kernel, k, ctx->stream, (int64_t)k, (int64_t)-1, init_rows))) return rc;
        if ((rc = km_update(ctx, m.cfrag.get(), m.cvalid.get(), k, nullptr, nullptr, k, 0, cent, nullptr))) return rc;
    } else {
        if ((rc = nn_reserve(ctx, m.one, (size_t)(2 * BLK_U4)))) return rc;
        if ((rc = nn_reserve(ctx, m.one_valid, (size_t)QT))) return rc;
        if ((rc = nn_reserve(ctx, m.picked, (size_t)n))) return rc;
        PassLog::Scope init(ctx, m.passes);
        GNN_HIP(hipMemsetAsync(m.one.get(), 0, (size_t)(2 * BLK_U4) * sizeof(uint4), ctx->stream));
        GNN_HIP(hipMemsetAsync(m.one_valid.get(), 0, (size_t)QT, ctx->stream));
        GNN_HIP(hipMemsetAsync(m.one_valid.get(), 1, 1, ctx->stream));
        GNN_HIP(hipMemsetAsync(m.picked.get(), 0, (size_t)n, ctx->stream));
        GNN_HIP(hipMemsetAsync(m.key.get(), 0, (size_t)n * sizeof(unsigned long long), ctx->stream));
        GNN_HIP(hipMemsetAsync(m.count.dev() + C_BEST, 0xff, sizeof(unsigned long long), ctx->stream));
        // Ends: k picks.  No pick waits for the host: the chosen row's fragments move on the device.
        for (int64_t j = 0; j < k; ++j) {
            if ((rc = launch_1d(km_far_kernel, n, ctx->stream, n, w.bvalid.get(), m.picked.get(), m.key.get(), m.count.dev() + C_BEST))) return rc;
            hipLaunchKernelGGL(km_pick_kernel, dim3(1), dim3(64), 0, ctx->stream, w.bfrag.get(), m.count.dev() + C_BEST, j, init_rows,
                               m.picked.get(), m.one.get());
            GNN_HIP(hipGetLastError());
            if (j + 1 < k && (rc = km_assign(ctx, fn, n, m.one.get(), m.one_valid.get(), 1, (unsigned)j))) return rc;
        }
        if ((rc = km_update(ctx, w.bfrag.get(), w.bvalid.get(), k, init_rows, nullptr, k, 0, cent, nullptr))) return rc;
    }
    if ((rc = nn_prepare(ctx, cent, k, GNN_KNN_COSINE, m.cfrag, m.cvalid))) return rc;
    GNN_HIP(hipMemsetAsync(m.key.get(), 0, (size_t)n * sizeof(unsigned long long), ctx->stream));
    if ((rc = launch_1d(km_fill_kernel, n, ctx->stream, n, (int64_t)-2, label))) return rc;       // no row has the label -2: the first assignment changes all
    // One assignment per pass.  Ends: `iterations` grows by one per pass and the loop leaves at max_iter <= 1000 at the latest.
    int64_t iterations = 0;
    bool converged = false;
    for (;;) {
        {
            PassLog::Scope assign(ctx, m.passes);
            if ((rc = m.count.zero(ctx, C_CHANGED, 1))) return rc;
            if ((rc = km_assign(ctx, fn, n, m.cfrag.get(), m.cvalid.get(), k, 0))) return rc;
            if ((rc = launch_1d(km_label_kernel, n, ctx->stream, n, m.key.get(), label, sim, m.count.dev() + C_CHANGED))) return rc;
        }
        unsigned long long changed = 0;
        if ((rc = m.count.read(ctx, C_CHANGED, 1, &changed))) return rc;
        m.passes.settle();
        if (changed == 0) {
            converged = true;
            break;
        }
        if (iterations == max_iter) break;
        if ((rc = km_update(ctx, w.bfrag.get(), w.bvalid.get(), n, nullptr, label, k, 0, cent, &m.passes))) return rc;
        {
            PassLog::Scope prepare(ctx, m.passes);
            if ((rc = nn_prepare(ctx, cent, k, GNN_KNN_COSINE, m.cfrag, m.cvalid))) return rc;
        }
        ++iterations;
    }
    ProfScope prof(ctx, GNN_K_NEIGHBOURS);
    GNN_HIP(hipMemsetAsync(size, 0, (size_t)k * sizeof(int64_t), ctx->stream));
    if ((rc = launch_1d(km_size_kernel, n, ctx->stream, n, (int64_t)k, label, reinterpret_cast<unsigned long long*>(size)))) return rc;
    *iterations_out = iterations;
    *converged_out = converged ? 1 : 0;
    return GNN_OK;
}

// n >= 0 rows and their labels on the device -> k centroid rows and sizes on the device; the ctx's stream is synchronised once (the
// labels' verdict), before anything is written.
int km_centroids(gnn_ctx* ctx, const char* fn, const float* rows_dev, int64_t n, const int64_t* label, int k, float* cent, int64_t* size) {
    NeighbourWorkspace& w = ctx->nn;
    KMeansWorkspace& m = ctx->km;
    int rc = nn_prepare(ctx, rows_dev, n, GNN_KNN_COSINE, w.bfrag, w.bvalid);
    if (!rc) rc = km_reserve(ctx, n, k);
    if (rc) return rc;
    if ((rc = m.count.zero(ctx, 0, C_WORDS))) return rc;
    if (n > 0 && (rc = launch_1d(km_check_kernel, n, ctx->stream, n, (int64_t)k, label, m.count.dev() + C_BAD_LABEL))) return rc;
    unsigned long long bad = 0;
    if ((rc = m.count.read(ctx, C_BAD_LABEL, 1, &bad))) return rc;
    if (bad) {
        set_error(std::string(fn) + ": a label is outside [-1, " + std::to_string(k) + ")");
        return GNN_ERR_ARG;
    }
    if ((rc = km_update(ctx, w.bfrag.get(), w.bvalid.get(), n, nullptr, label, k, 1, cent, nullptr))) return rc;
    GNN_HIP(hipMemcpyAsync(size, m.cnt.get(), (size_t)k * sizeof(int64_t), hipMemcpyDeviceToDevice, ctx->stream));
    return GNN_OK;
}

}  // namespace
}  // namespace gnn

using namespace gnn;

extern "C" int gnn_kmeans_dev(gnn_ctx* ctx, const float* rows_dev, int64_t n, int k, const float* init_dev_or_null, int max_iter,
                              int64_t* label_dev, float* sim_dev, float* centroids_dev, int64_t* size_dev, int64_t* init_rows_dev,
                              int64_t* iterations_host, int* converged_host) {
    const char* const fn = "gnn_kmeans_dev";
    if (int rc = check_kmeans_args(fn, rows_dev, n, k, max_iter, label_dev, sim_dev, centroids_dev, size_dev, init_rows_dev, iterations_host,
                                   converged_host))
        return rc;
    if (int rc = check_ctx(ctx)) return rc;
    return km_run(ctx, fn, rows_dev, n, k, init_dev_or_null, max_iter, label_dev, sim_dev, centroids_dev, size_dev, init_rows_dev,
                  iterations_host, converged_host);
}

extern "C" int gnn_kmeans(gnn_ctx* ctx, const float* rows_host, int64_t n, int k, const float* init_host_or_null, int max_iter,
                          int64_t* label_host, float* sim_host, float* centroids_host, int64_t* size_host, int64_t* init_rows_host,
                          int64_t* iterations_host, int* converged_host) {
    const char* const fn = "gnn_kmeans";
    if (int rc = check_kmeans_args(fn, rows_host, n, k, max_iter, label_host, sim_host, centroids_host, size_host, init_rows_host,
                                   iterations_host, converged_host))
        return rc;
    if (int rc = check_ctx(ctx)) return rc;
    NeighbourWorkspace& w = ctx->nn;
    KMeansWorkspace& m = ctx->km;
    Landing land(m.d_out);
    const int label = land.add(label_host, n), sim = land.add(sim_host, n), size = land.add(size_host, k), init_rows = land.add(init_rows_host, k),
              cent = land.add(centroids_host, (int64_t)k * D);
    int rc = land.reserve(ctx);                               // every buffer stands before a copy is enqueued
    if (!rc && init_host_or_null) rc = nn_reserve(ctx, m.d_init, (size_t)k * D);
    if (!rc) rc = nn_upload_rows(ctx, rows_host, n);
    if (rc) return rc;
    if (init_host_or_null)
        GNN_HIP(hipMemcpyAsync(m.d_init.get(), init_host_or_null, (size_t)k * D * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    rc = km_run(ctx, fn, w.d_base, n, k, init_host_or_null ? m.d_init.get() : nullptr, max_iter, land.dev<int64_t>(label), land.dev<float>(sim),
                land.dev<float>(cent), land.dev<int64_t>(size), land.dev<int64_t>(init_rows), iterations_host, converged_host);
    return rc ? rc : land.copy_out(ctx);
}

extern "C" int gnn_centroids_dev(gnn_ctx* ctx, const float* rows_dev, int64_t n, const int64_t* label_dev, int k, float* centroids_dev,
                                 int64_t* size_dev) {
    const char* const fn = "gnn_centroids_dev";
    if (int rc = check_centroid_args(fn, rows_dev, n, label_dev, k, centroids_dev, size_dev)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    return km_centroids(ctx, fn, rows_dev, n, label_dev, k, centroids_dev, size_dev);
}

extern "C" int gnn_centroids(gnn_ctx* ctx, const float* rows_host, int64_t n, const int64_t* label_host, int k, float* centroids_host,
                             int64_t* size_host) {
    const char* const fn = "gnn_centroids";
    if (int rc = check_centroid_args(fn, rows_host, n, label_host, k, centroids_host, size_host)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    NeighbourWorkspace& w = ctx->nn;
    KMeansWorkspace& m = ctx->km;
    Landing land(m.d_out);
    const int label = land.add<int64_t>(nullptr, n), size = land.add(size_host, k), cent = land.add(centroids_host, (int64_t)k * D);
    int rc = land.reserve(ctx);                               // both buffers stand before the copy is enqueued
    if (!rc) rc = nn_upload_rows(ctx, rows_host, n);
    if (rc) return rc;
    int64_t* const label_dev = land.dev<int64_t>(label);      // the slice is the call's own: the labels go up, nothing comes back
    if (n > 0) GNN_HIP(hipMemcpyAsync(label_dev, label_host, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    rc = km_centroids(ctx, fn, w.d_base, n, label_dev, k, land.dev<float>(cent), land.dev<int64_t>(size));
    return rc ? rc : land.copy_out(ctx);
}

extern "C" int gnn_debug_set_kmeans_lds(gnn_ctx* ctx, int max_k) {
    if (int rc = check_ctx(ctx)) return rc;
    if (max_k < 0 || max_k > LDS_K_MAX) {
        set_error("gnn_debug_set_kmeans_lds: " + std::to_string(max_k) + " groups is outside [0, " + std::to_string(LDS_K_MAX) +
                  "] (0 = every sum straight to memory)");
        return GNN_ERR_ARG;
    }
    ctx->km.lds_k = max_k;
    return GNN_OK;
}

extern "C" int gnn_debug_kmeans_pass_ms(gnn_ctx* ctx, double* ms_out, int64_t capacity, int64_t* n_out) {
    if (int rc = check_ctx(ctx)) return rc;
    return ctx->km.passes.out(ctx, "gnn_debug_kmeans_pass_ms", ms_out, capacity, n_out);
}
