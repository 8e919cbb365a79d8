// Exact t-SNE layout of a similarity graph (include/genomad_nn.h, "t-SNE layout"): the definition is
// sequence.tsne_layout, and every output here equals it bit for bit.  The affinities are the graph's own weights (W = 2^24 a similarity
// of 1, p = q / M2); the repulsive term is the exact all-pairs pass over the 2-D points.
//   validate, symmetrise   gnn_csr_sym.h, shared with the other consumers of the graph.  A row's entries stand in arrival order: nothing
//                downstream depends on it - every sum over entries is a sum of integers.
//   affinities   M2 = the integer sum of the symmetric entries' weights (one 64-bit atomic per workgroup), p = (f32)((f64)q / (f64)M2)
//                per entry, and the list of the rows with more than WAVE_ENTRIES entries.
//   repel        ts_repel_kernel: a thread owns ROWS rows, a workgroup stages 256 columns (x, y, 1 or 0 for a column that takes part)
//                in LDS - every lane reads the same column, a broadcast - and runs the three f32 chains of the definition over them in
//                ascending column order.  At a granule's end the chains become integers (rint of the exact f64 product) and are added
//                in int64 registers; one 64-bit atomicAdd per row and workgroup for zi / rx / ry, one per workgroup for Z.  The columns
//                are split over blockIdx.y at granule boundaries: a granule's chain is the same whoever runs it, integers add in any
//                order - no bit depends on the split or the grid.
//   attract      a row's entries by one wave (ts_attract_wave_kernel) or, for a row of the long list, by a workgroup
//                (ts_attract_group_kernel): the integer images rint((f64)((p * q) * d) * 2^32) reduced by shuffles, one plain store per row.
//   update       ts_update_kernel, one thread per coordinate: the gradient in f64, rounded to f32 once, gains, momentum, Y += upd; it
//                clears the row's sums for the next pass.  Z of iterate `it` is accumulated in z_trace[it] itself.
// The file is compiled with -ffp-contract=off (build.sh) and says so itself below: every f32 and f64 operation is one IEEE operation,
// the division the correctly rounded one.  Only integer atomics, no inline assembly, no loop that waits for another workgroup; every
// loop's termination argument stands next to it and every store is guarded by its bound.  The whole loop is enqueued without a host
// read: the one synchronise is the verdict on the graph and the init, before anything is written.
#pragma clang fp contract(off)
#include <cmath>

#include "gnn_nn_frag.h"
#include "gnn_csr_sym.h"

namespace gnn {
namespace {

typedef unsigned long long ull;
typedef long long ll;

constexpr int THREADS = 256;
constexpr int GRANULE = 256;                     // columns of one f32 chain, aligned to the absolute column index
constexpr int ROWS = 2;                          // rows per thread of the repel pass: two independent chains per lane
constexpr int WAVE_ENTRIES = 256;                // the longest row one wave attracts; a longer one is a workgroup's
constexpr int LONG_GROUPS = 256;                 // workgroups that walk the long list
constexpr int64_t TSNE_N_MAX = (int64_t)1 << 21; // Z < 2^63
constexpr int TSNE_ITER_MAX = 100000;
constexpr double Z_UNIT = 1048576.0;             // 2^20
constexpr double F_UNIT = 4294967296.0;          // 2^32
// HostCounters words
constexpr size_t C_FLAG = 0, C_M2 = 1, C_LONG = 2, C_WORDS = 3;

__device__ __forceinline__ ll ts_image(float v, double unit) { return (ll)rint((double)v * unit); }      // exact product, ties to even

// 1 / (1 + |d|^2) with the definition's operations in its order; m = 1 or 0 (a column that does not take part)
__device__ __forceinline__ float ts_q(float dx, float dy, float m) {
    const float s = dx * dx + dy * dy;
    const float d2 = 1.0f + s;
    return m / d2;
}

// one thread per row: bit 1 of the flag for an init that is not finite at a row that takes part
__global__ __launch_bounds__(256) void ts_init_check_kernel(int64_t n, const float* __restrict__ init, const uint8_t* __restrict__ ok,
                                                            ull* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !ok[i]) return;
    if (!(fabsf(init[2 * i]) < INFINITY) || !(fabsf(init[2 * i + 1]) < INFINITY)) atomicOr(flag, 2ull);
}

// one thread per row: M2 += the row's weights (a workgroup's sum, one atomic), and the long list.  Every entry of soff's range was
// filed by csr_symmetrise.
__global__ __launch_bounds__(256) void ts_m2_kernel(int64_t n, const int64_t* __restrict__ soff, const uint32_t* __restrict__ sq,
                                                    ull* __restrict__ m2, ull* __restrict__ long_count, int32_t* __restrict__ long_list) {
    __shared__ ull red[4];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    ull s = 0;
    if (i < n) {
        const int64_t b = soff[i], e = soff[i + 1];
        for (int64_t x = b; x < e; ++x) s += sq[x];           // Ends: x grows towards e
        if (e - b > WAVE_ENTRIES) {
            const ull at = atomicAdd(long_count, 1ull);
            if (at < (ull)n) long_list[at] = (int32_t)i;      // always: a row is pushed once
        }
    }
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const ull t = red[0] + red[1] + red[2] + red[3];
        if (t) atomicAdd(m2, t);
    }
}

// one thread per symmetric entry: p = (f32)((f64)q / (f64)M2); an entry exists only where M2 > 0
__global__ __launch_bounds__(256) void ts_p_kernel(int64_t total, const uint32_t* __restrict__ sq, const ull* __restrict__ m2,
                                                   float* __restrict__ sp) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= total) return;
    sp[x] = (float)((double)sq[x] / (double)*m2);
}

// one thread per coordinate: Y = the init (NaN at a row that does not take part), gain = 1, upd = 0; the row's sums are cleared
__global__ __launch_bounds__(256) void ts_start_kernel(int64_t n, const float* __restrict__ init, const uint8_t* __restrict__ ok,
                                                       float* __restrict__ y, float* __restrict__ gain, float* __restrict__ upd,
                                                       ll* __restrict__ zi, ll* __restrict__ rx, ll* __restrict__ ry) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= 2 * n) return;
    const int64_t i = k >> 1;
    y[k] = ok[i] ? init[k] : NAN;
    gain[k] = 1.0f;
    upd[k] = 0.0f;
    if (k & 1) {
        ry[i] = 0;
    } else {
        rx[i] = 0;
        zi[i] = 0;
    }
}

// grid = (ceil(n / (256 * ROWS)), splits), 256 threads.  Thread t of workgroup b owns the rows b * 256 * ROWS + r * 256 + t; the
// workgroup's columns are the granules [blockIdx.y * per, (blockIdx.y + 1) * per) below `granules`.
__global__ __launch_bounds__(THREADS) void ts_repel_kernel(int64_t n, int64_t granules, int64_t per, const float* __restrict__ y,
                                                           const uint8_t* __restrict__ ok, ll* __restrict__ zi, ll* __restrict__ rx,
                                                           ll* __restrict__ ry, ull* __restrict__ z) {
    __shared__ float4 cols[2][GRANULE];          // x, y, 1 or 0, unused
    __shared__ ll red[4];
    const int tid = threadIdx.x;
    int64_t row[ROWS];
    float xi[ROWS], yi[ROWS];
    bool live[ROWS];
    ll az[ROWS], ax[ROWS], ay[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        row[r] = ((int64_t)blockIdx.x * ROWS + r) * THREADS + tid;
        live[r] = row[r] < n && ok[row[r]];
        xi[r] = live[r] ? y[2 * row[r]] : 0.0f;
        yi[r] = live[r] ? y[2 * row[r] + 1] : 0.0f;
        az[r] = ax[r] = ay[r] = 0;
    }
    const int64_t g0 = (int64_t)blockIdx.y * per, g1 = min(granules, g0 + per);
    for (int64_t g = g0; g < g1; ++g) {                       // Ends: g grows towards g1.  Uniform: every thread passes the barrier
        float4* const buf = cols[g & 1];
        const int64_t c = g * GRANULE + tid;
        const bool in = c < n && ok[c];
        buf[tid] = in ? make_float4(y[2 * c], y[2 * c + 1], 1.0f, 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        // one barrier per granule: the other buffer's last readers passed the barrier of the granule before
        __syncthreads();
        float cz[ROWS], cx[ROWS], cy[ROWS];
        int self[ROWS];                                       // the row's own column in this granule, or -1
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            cz[r] = cx[r] = cy[r] = 0.0f;
            self[r] = (row[r] >= g * GRANULE && row[r] < (g + 1) * GRANULE) ? (int)(row[r] - g * GRANULE) : -1;
        }
#pragma unroll 4
        for (int j = 0; j < GRANULE; ++j) {                   // ascending column order: the chains' order
            const float4 cj = buf[j];
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                const float dx = xi[r] - cj.x, dy = yi[r] - cj.y;
                float q = ts_q(dx, dy, cj.z);
                q = j == self[r] ? 0.0f : q;
                cz[r] = cz[r] + q;
                const float q2 = q * q;
                cx[r] = cx[r] + q2 * dx;
                cy[r] = cy[r] + q2 * dy;
            }
        }
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            az[r] += ts_image(cz[r], Z_UNIT);
            ax[r] += ts_image(cx[r], F_UNIT);
            ay[r] += ts_image(cy[r], F_UNIT);
        }
    }
    ll zsum = 0;
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
        if (live[r] && g1 > g0) {                             // live: row[r] < n
            atomicAdd((ull*)(zi + row[r]), (ull)az[r]);
            atomicAdd((ull*)(rx + row[r]), (ull)ax[r]);
            atomicAdd((ull*)(ry + row[r]), (ull)ay[r]);
            zsum += az[r];
        }
    for (int o = 32; o; o >>= 1) zsum += __shfl_xor(zsum, o);
    if ((tid & 63) == 0) red[tid >> 6] = zsum;
    __syncthreads();
    if (tid == 0) {
        const ll t = red[0] + red[1] + red[2] + red[3];
        if (t) atomicAdd(z, (ull)t);
    }
}

// the integer images of entry x of row i: (p * q) * d, q from the two points
__device__ __forceinline__ void ts_attract_entry(const float* __restrict__ y, float xi, float yi, int j, float p, ll& ax, ll& ay) {
    const float dx = xi - y[2 * (int64_t)j], dy = yi - y[2 * (int64_t)j + 1];
    const float pq = p * ts_q(dx, dy, 1.0f);
    ax += ts_image(pq * dx, F_UNIT);
    ay += ts_image(pq * dy, F_UNIT);
}

// one wave per row, four rows per workgroup: the rows of up to WAVE_ENTRIES entries; a longer row is left to the long list's kernel
__global__ __launch_bounds__(THREADS) void ts_attract_wave_kernel(int64_t n, const int64_t* __restrict__ soff, const int32_t* __restrict__ sidx,
                                                                  const float* __restrict__ sp, const uint8_t* __restrict__ ok,
                                                                  const float* __restrict__ y, ll* __restrict__ ax_out, ll* __restrict__ ay_out) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;                                       // the whole wave: no barrier follows
    const int64_t b = soff[i], e = soff[i + 1];
    if (e - b > WAVE_ENTRIES) return;
    ll ax = 0, ay = 0;
    if (ok[i]) {                                              // a row that does not take part has no entry; its Y is NaN
        const float xi = y[2 * i], yi = y[2 * i + 1];
        for (int64_t x = b + lane; x < e; x += 64) ts_attract_entry(y, xi, yi, sidx[x], sp[x], ax, ay);      // Ends: x grows towards e
    }
    for (int o = 32; o; o >>= 1) {
        ax += __shfl_xor(ax, o);
        ay += __shfl_xor(ay, o);
    }
    if (lane == 0) {
        ax_out[i] = ax;
        ay_out[i] = ay;
    }
}

// LONG_GROUPS workgroups walk the long list, one row each at a time
__global__ __launch_bounds__(THREADS) void ts_attract_group_kernel(int64_t n, const ull* __restrict__ long_count, const int32_t* __restrict__ long_list,
                                                                   const int64_t* __restrict__ soff, const int32_t* __restrict__ sidx,
                                                                   const float* __restrict__ sp, const float* __restrict__ y,
                                                                   ll* __restrict__ ax_out, ll* __restrict__ ay_out) {
    __shared__ ll red[2][4];
    const int tid = threadIdx.x;
    const int64_t total = (int64_t)min<ull>(*long_count, (ull)n);
    for (int64_t w = blockIdx.x; w < total; w += gridDim.x) { // Ends: w grows towards total.  Uniform: w is the workgroup's
        const int64_t i = long_list[w];
        if (i < 0 || i >= n) continue;                        // never: the list holds rows
        const int64_t b = soff[i], e = soff[i + 1];
        const float xi = y[2 * i], yi = y[2 * i + 1];         // a row with entries takes part
        ll ax = 0, ay = 0;
        for (int64_t x = b + tid; x < e; x += THREADS) ts_attract_entry(y, xi, yi, sidx[x], sp[x], ax, ay);  // Ends: x grows towards e
        for (int o = 32; o; o >>= 1) {
            ax += __shfl_xor(ax, o);
            ay += __shfl_xor(ay, o);
        }
        __syncthreads();                                      // red[] is free of the row before
        if ((tid & 63) == 0) {
            red[0][tid >> 6] = ax;
            red[1][tid >> 6] = ay;
        }
        __syncthreads();
        if (tid == 0) {
            ax_out[i] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
            ay_out[i] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        }
    }
}

// One thread per coordinate k = 2 i + c of iterate `it` (its Z stands in *z).  It clears the row's sums behind its read.
__global__ __launch_bounds__(256) void ts_update_kernel(int64_t n, const uint8_t* __restrict__ ok, const ull* __restrict__ z, ll* __restrict__ zi,
                                                        ll* __restrict__ rx, ll* __restrict__ ry, const ll* __restrict__ ax,
                                                        const ll* __restrict__ ay, double e, float mom, float lr, float* __restrict__ y,
                                                        float* __restrict__ gain, float* __restrict__ upd) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= 2 * n) return;
    const int64_t i = k >> 1;
    ll* const rsum = (k & 1) ? ry : rx;
    const ll R = rsum[i];
    rsum[i] = 0;
    if (!(k & 1)) zi[i] = 0;
    if (!ok[i]) return;
    const ll A = ((k & 1) ? ay : ax)[i];
    const ull Z = *z;
    const double att = e * ((double)A / F_UNIT);
    const double rep = Z ? ((double)R / F_UNIT) / ((double)Z / Z_UNIT) : 0.0;
    const float g = (float)(4.0 * (att - rep));
    const float u = upd[k];
    float gn = gain[k];
    gn = ((g > 0.0f && u < 0.0f) || (g < 0.0f && u > 0.0f)) ? gn + 0.2f : gn * 0.8f;
    gn = gn < 0.01f ? 0.01f : gn;
    const float t1 = mom * u, t2 = gn * g;
    const float nu = t1 - lr * t2;
    gain[k] = gn;
    upd[k] = nu;
    y[k] = y[k] + nu;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

int ts_bad(const std::string& f, const char* what, const std::string& v, const char* range) {
    set_error(f + ": " + what + " " + v + " is outside " + range);
    return GNN_ERR_ARG;
}

int ts_check_graph(const std::string& f, int64_t n, int64_t nnz) {
    if (n < 0 || n > TSNE_N_MAX) return ts_bad(f, "n", std::to_string(n), "[0, 2^21]");
    return graph_check(f, n, nnz);
}

int ts_check_params(const std::string& f, int n_iter, int exaggeration_iter, double exaggeration, float learning_rate) {
    if (n_iter < 0 || n_iter > TSNE_ITER_MAX) return ts_bad(f, "n_iter", std::to_string(n_iter), "[0, 100000]");
    if (exaggeration_iter < 0 || exaggeration_iter > TSNE_ITER_MAX)
        return ts_bad(f, "exaggeration_iter", std::to_string(exaggeration_iter), "[0, 100000]");
    if (!(exaggeration >= 1.0 && exaggeration <= 1024.0)) return ts_bad(f, "exaggeration", std::to_string(exaggeration), "[1, 1024]");
    if (!(learning_rate > 0.0f && learning_rate <= 1048576.0f)) return ts_bad(f, "learning_rate", std::to_string(learning_rate), "(0, 2^20]");
    return GNN_OK;
}

// the workgroups over the columns: the debug value, or what gives every CU two workgroups; never more than there are granules
int64_t ts_splits(const gnn_ctx* ctx, int64_t n, int64_t granules) {
    const int64_t row_groups = (n + THREADS * ROWS - 1) / (THREADS * ROWS);
    int64_t s = ctx->ts.split > 0 ? ctx->ts.split : (2 * std::max(ctx->cu_count, 1) + row_groups - 1) / row_groups;
    return std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(s, granules), 65535));
}

// Everything the passes need stands; the verdict on the graph and the init (y_dev; the one synchronise); the symmetric graph, M2, p
// and the long list are enqueued.  n > 0.
int ts_setup(gnn_ctx* ctx, const char* fn, const CsrGraph& g, const float* y_dev, int n_iter) {
    TsneWorkspace& w = ctx->ts;
    const int64_t n = g.n;
    const size_t entries = (size_t)std::max<int64_t>(2 * g.nnz, 1);
    int rc = nn_reserve(ctx, w.ok, (size_t)n);
    if (!rc) rc = w.count.reserve(ctx, C_WORDS);
    if (!rc) rc = nn_reserve(ctx, w.deg, (size_t)n);
    if (!rc) rc = nn_reserve(ctx, w.soff, (size_t)n + 1);
    if (!rc) rc = nn_reserve(ctx, w.cursor, (size_t)n);
    if (!rc) rc = nn_reserve(ctx, w.sidx, entries);
    if (!rc) rc = nn_reserve(ctx, w.sq, entries);
    if (!rc) rc = nn_reserve(ctx, w.sp, entries);
    if (!rc) rc = nn_reserve(ctx, w.long_list, (size_t)n);
    if (!rc) rc = nn_reserve(ctx, w.y, (size_t)2 * n);
    if (!rc) rc = nn_reserve(ctx, w.gain, (size_t)2 * n);
    if (!rc) rc = nn_reserve(ctx, w.upd, (size_t)2 * n);
    if (!rc) rc = nn_reserve(ctx, w.zi, (size_t)n);
    if (!rc) rc = nn_reserve(ctx, w.rx, (size_t)n);
    if (!rc) rc = nn_reserve(ctx, w.ry, (size_t)n);
    if (!rc) rc = nn_reserve(ctx, w.ax, (size_t)n);
    if (!rc) rc = nn_reserve(ctx, w.ay, (size_t)n);
    if (!rc) rc = nn_reserve(ctx, w.ztrace, (size_t)n_iter + 1);
    if (!rc) rc = w.count.zero(ctx, 0, C_WORDS);
    if (rc) return rc;
    if ((rc = graph_validate_launch(ctx, g, w.ok.get(), w.count, C_FLAG))) return rc;
    if ((rc = launch_1d(ts_init_check_kernel, n, ctx->stream, n, y_dev, w.ok.get(), w.count.dev() + C_FLAG))) return rc;
    ull word = 0;
    if ((rc = graph_verdict(ctx, fn, g, w.count, C_FLAG, &word))) return rc;
    if (word & 2) {
        set_error(std::string(fn) + ": the init is not finite at a row that takes part");
        return GNN_ERR_ARG;
    }
    if ((rc = csr_symmetrise(ctx->stream, n, g.indptr, g.col, g.sim, w.ok.get(), w.deg.get(), w.soff.get(), w.cursor.get(), w.sidx.get(),
                             w.sq.get())))
        return rc;
    if ((rc = launch_1d(ts_m2_kernel, n, ctx->stream, n, w.soff.get(), w.sq.get(), w.count.dev() + C_M2, w.count.dev() + C_LONG, w.long_list.get())))
        return rc;
    // an entry beyond soff[n] does not exist: ts_p_kernel covers the buffer's 2 nnz, the passes read below soff[i + 1] only
    if (g.nnz > 0 && (rc = launch_1d(ts_p_kernel, 2 * g.nnz, ctx->stream, 2 * g.nnz, w.sq.get(), w.count.dev() + C_M2, w.sp.get()))) return rc;
    GNN_HIP(hipMemsetAsync(w.ztrace.get(), 0, ((size_t)n_iter + 1) * sizeof(ull), ctx->stream));
    return launch_1d(ts_start_kernel, 2 * n, ctx->stream, n, y_dev, w.ok.get(), w.y.get(), w.gain.get(), w.upd.get(), w.zi.get(), w.rx.get(),
                     w.ry.get());
}

// the forces of the ctx's Y: zi / rx / ry accumulate (they are zero before), Z into *z, ax / ay are stored
int ts_forces(gnn_ctx* ctx, int64_t n, ull* z, bool attract) {
    TsneWorkspace& w = ctx->ts;
    const int64_t granules = (n + GRANULE - 1) / GRANULE, splits = ts_splits(ctx, n, granules), per = (granules + splits - 1) / splits;
    const int64_t row_groups = (n + THREADS * ROWS - 1) / (THREADS * ROWS);
    hipLaunchKernelGGL(ts_repel_kernel, dim3((unsigned)row_groups, (unsigned)((granules + per - 1) / per)), dim3(THREADS), 0, ctx->stream, n,
                       granules, per, w.y.get(), w.ok.get(), w.zi.get(), w.rx.get(), w.ry.get(), z);
    GNN_HIP(hipGetLastError());
    if (!attract) return GNN_OK;
    hipLaunchKernelGGL(ts_attract_wave_kernel, dim3((unsigned)((n + 3) / 4)), dim3(THREADS), 0, ctx->stream, n, w.soff.get(), w.sidx.get(),
                       w.sp.get(), w.ok.get(), w.y.get(), w.ax.get(), w.ay.get());
    GNN_HIP(hipGetLastError());
    hipLaunchKernelGGL(ts_attract_group_kernel, dim3(LONG_GROUPS), dim3(THREADS), 0, ctx->stream, n, w.count.dev() + C_LONG, w.long_list.get(),
                       w.soff.get(), w.sidx.get(), w.sp.get(), w.y.get(), w.ax.get(), w.ay.get());
    GNN_HIP(hipGetLastError());
    return GNN_OK;
}

struct TsneIn : CsrGraph {
    const float* init;         // [n][2], on the device
    int n_iter, exaggeration_iter;
    double exaggeration;
    float learning_rate;
};

// n > 0: the graph and the init on the device -> layout [n][2], z_trace [n_iter + 1] and valid [n] on the device
int ts_run(gnn_ctx* ctx, const char* fn, const TsneIn& in, float* layout, uint64_t* z_trace, uint8_t* valid) {
    TsneWorkspace& w = ctx->ts;
    w.passes.begin();
    const int64_t n = in.n;
    int rc;
    {
        PassLog::Scope setup(ctx, w.passes);                  // open across the read: nothing is settled there
        if ((rc = ts_setup(ctx, fn, in, in.init, in.n_iter))) return rc;
    }
    {
        PassLog::Scope loop(ctx, w.passes);
        for (int it = 0; it < in.n_iter; ++it) {              // Ends: it grows towards n_iter
            const bool early = it < in.exaggeration_iter;
            if ((rc = ts_forces(ctx, n, w.ztrace.get() + it, true))) return rc;
            if ((rc = launch_1d(ts_update_kernel, 2 * n, ctx->stream, n, w.ok.get(), w.ztrace.get() + it, w.zi.get(), w.rx.get(), w.ry.get(),
                                w.ax.get(), w.ay.get(), early ? in.exaggeration : 1.0, early ? 0.5f : 0.8f, in.learning_rate, w.y.get(),
                                w.gain.get(), w.upd.get())))
                return rc;
        }
    }
    {
        PassLog::Scope finish(ctx, w.passes);
        if ((rc = ts_forces(ctx, n, w.ztrace.get() + in.n_iter, false))) return rc;
        GNN_HIP(hipMemcpyAsync(layout, w.y.get(), (size_t)2 * n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
        GNN_HIP(hipMemcpyAsync(z_trace, w.ztrace.get(), ((size_t)in.n_iter + 1) * sizeof(ull), hipMemcpyDeviceToDevice, ctx->stream));
        GNN_HIP(hipMemcpyAsync(valid, w.ok.get(), (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
    }
    return GNN_OK;
}

int ts_check(const char* fn, const TsneIn& in, const void* layout, const void* z_trace, const void* valid) {
    const std::string f(fn);
    if (int rc = ts_check_graph(f, in.n, in.nnz)) return rc;
    if (int rc = ts_check_params(f, in.n_iter, in.exaggeration_iter, in.exaggeration, in.learning_rate)) return rc;
    return nn_check_required(f, in.indptr && (in.nnz == 0 || (in.col && in.sim)) && z_trace && (in.n == 0 || (in.init && layout && valid)),
                             "indptr, col, sim, init, layout, z_trace and valid");
}

// n > 0: the graph and Y on the device -> the six results on the device
int ts_forces_run(gnn_ctx* ctx, const char* fn, const CsrGraph& g, const float* y_dev, int64_t* zi, int64_t* rx, int64_t* ry, int64_t* ax,
                  int64_t* ay, int64_t* m2) {
    TsneWorkspace& w = ctx->ts;
    w.passes.begin();
    const size_t bytes = (size_t)g.n * sizeof(ll);
    if (int rc = ts_setup(ctx, fn, g, y_dev, 0)) return rc;
    if (int rc = ts_forces(ctx, g.n, w.ztrace.get(), true)) return rc;
    GNN_HIP(hipMemcpyAsync(zi, w.zi.get(), bytes, hipMemcpyDeviceToDevice, ctx->stream));
    GNN_HIP(hipMemcpyAsync(rx, w.rx.get(), bytes, hipMemcpyDeviceToDevice, ctx->stream));
    GNN_HIP(hipMemcpyAsync(ry, w.ry.get(), bytes, hipMemcpyDeviceToDevice, ctx->stream));
    GNN_HIP(hipMemcpyAsync(ax, w.ax.get(), bytes, hipMemcpyDeviceToDevice, ctx->stream));
    GNN_HIP(hipMemcpyAsync(ay, w.ay.get(), bytes, hipMemcpyDeviceToDevice, ctx->stream));
    GNN_HIP(hipMemcpyAsync(m2, w.count.dev() + C_M2, sizeof(ull), hipMemcpyDeviceToDevice, ctx->stream));
    return GNN_OK;
}

int ts_forces_check(const char* fn, const CsrGraph& g, const void* y, const void* zi, const void* rx, const void* ry, const void* ax,
                    const void* ay, const void* m2) {
    const std::string f(fn);
    if (int rc = ts_check_graph(f, g.n, g.nnz)) return rc;
    return nn_check_required(f, g.indptr && (g.nnz == 0 || (g.col && g.sim)) && m2 && (g.n == 0 || (y && zi && rx && ry && ax && ay)),
                             "indptr, col, sim, y, zi, rx, ry, ax, ay and m2");
}

}  // namespace
}  // namespace gnn

using namespace gnn;

extern "C" int gnn_tsne_dev(gnn_ctx* ctx, const int64_t* indptr_dev, const int32_t* col_dev, const float* sim_dev, const uint8_t* valid_dev_or_null,
                            int64_t n, int64_t nnz, const float* init_dev, int n_iter, int exaggeration_iter, double exaggeration,
                            float learning_rate, float* layout_dev, uint64_t* z_trace_dev, uint8_t* valid_out_dev) {
    const char* const fn = "gnn_tsne_dev";
    const TsneIn in = {{indptr_dev, col_dev, sim_dev, valid_dev_or_null, n, nnz}, init_dev, n_iter, exaggeration_iter, exaggeration, learning_rate};
    if (int rc = ts_check(fn, in, layout_dev, z_trace_dev, valid_out_dev)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (n == 0) {
        ctx->ts.passes.begin();
        GNN_HIP(hipMemsetAsync(z_trace_dev, 0, ((size_t)n_iter + 1) * sizeof(uint64_t), ctx->stream));
        return GNN_OK;
    }
    return ts_run(ctx, fn, in, layout_dev, z_trace_dev, valid_out_dev);
}

extern "C" int gnn_tsne(gnn_ctx* ctx, const int64_t* indptr_host, const int32_t* col_host, const float* sim_host, const uint8_t* valid_host_or_null,
                        int64_t n, int64_t nnz, const float* init_host, int n_iter, int exaggeration_iter, double exaggeration,
                        float learning_rate, float* layout_host, uint64_t* z_trace_host, uint8_t* valid_out_host) {
    const char* const fn = "gnn_tsne";
    TsneIn in = {{indptr_host, col_host, sim_host, valid_host_or_null, n, nnz}, init_host, n_iter, exaggeration_iter, exaggeration, learning_rate};
    if (int rc = ts_check(fn, in, layout_host, z_trace_host, valid_out_host)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (n == 0) {
        ctx->ts.passes.begin();
        for (int it = 0; it <= n_iter; ++it) z_trace_host[it] = 0;       // Ends: it grows towards n_iter
        return GNN_OK;
    }
    TsneWorkspace& w = ctx->ts;
    // every buffer stands before a copy is enqueued.  d_out: [layout (f32) | z_trace | valid (u8) | the init (f32)]
    int rc = graph_reserve(ctx, w.graph, n, nnz);
    Landing land(w.d_out);
    const int layout = land.add(layout_host, 2 * n), z_trace = land.add(z_trace_host, (int64_t)n_iter + 1), valid = land.add(valid_out_host, n),
              init = land.add((float*)nullptr, 2 * n);
    if (!rc) rc = land.reserve(ctx);
    if (rc) return rc;
    if ((rc = graph_upload(ctx, w.graph, in))) return rc;
    GNN_HIP(hipMemcpyAsync(land.dev<float>(init), init_host, (size_t)2 * n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    in.init = land.dev<float>(init);
    rc = ts_run(ctx, fn, in, land.dev<float>(layout), land.dev<uint64_t>(z_trace), land.dev<uint8_t>(valid));
    return rc ? rc : land.copy_out(ctx);
}

extern "C" int gnn_tsne_forces_dev(gnn_ctx* ctx, const int64_t* indptr_dev, const int32_t* col_dev, const float* sim_dev,
                                   const uint8_t* valid_dev_or_null, int64_t n, int64_t nnz, const float* y_dev, int64_t* zi_dev, int64_t* rx_dev,
                                   int64_t* ry_dev, int64_t* ax_dev, int64_t* ay_dev, int64_t* m2_dev) {
    const char* const fn = "gnn_tsne_forces_dev";
    const CsrGraph g = {indptr_dev, col_dev, sim_dev, valid_dev_or_null, n, nnz};
    if (int rc = ts_forces_check(fn, g, y_dev, zi_dev, rx_dev, ry_dev, ax_dev, ay_dev, m2_dev)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (n == 0) {
        GNN_HIP(hipMemsetAsync(m2_dev, 0, sizeof(int64_t), ctx->stream));
        return GNN_OK;
    }
    return ts_forces_run(ctx, fn, g, y_dev, zi_dev, rx_dev, ry_dev, ax_dev, ay_dev, m2_dev);
}

extern "C" int gnn_tsne_forces(gnn_ctx* ctx, const int64_t* indptr_host, const int32_t* col_host, const float* sim_host,
                               const uint8_t* valid_host_or_null, int64_t n, int64_t nnz, const float* y_host, int64_t* zi_host, int64_t* rx_host,
                               int64_t* ry_host, int64_t* ax_host, int64_t* ay_host, int64_t* m2_host) {
    const char* const fn = "gnn_tsne_forces";
    CsrGraph g = {indptr_host, col_host, sim_host, valid_host_or_null, n, nnz};
    if (int rc = ts_forces_check(fn, g, y_host, zi_host, rx_host, ry_host, ax_host, ay_host, m2_host)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (n == 0) {
        *m2_host = 0;
        return GNN_OK;
    }
    TsneWorkspace& w = ctx->ts;
    // d_out: [zi | rx | ry | ax | ay | m2 | Y (f32)]
    int rc = graph_reserve(ctx, w.graph, n, nnz);
    Landing land(w.d_out);
    const int zi = land.add(zi_host, n), rx = land.add(rx_host, n), ry = land.add(ry_host, n), ax = land.add(ax_host, n), ay = land.add(ay_host, n),
              m2 = land.add(m2_host, 1), y = land.add((float*)nullptr, 2 * n);
    if (!rc) rc = land.reserve(ctx);
    if (rc) return rc;
    if ((rc = graph_upload(ctx, w.graph, g))) return rc;
    GNN_HIP(hipMemcpyAsync(land.dev<float>(y), y_host, (size_t)2 * n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    rc = ts_forces_run(ctx, fn, g, land.dev<float>(y), land.dev<int64_t>(zi), land.dev<int64_t>(rx), land.dev<int64_t>(ry), land.dev<int64_t>(ax),
                       land.dev<int64_t>(ay), land.dev<int64_t>(m2));
    return rc ? rc : land.copy_out(ctx);
}

extern "C" int gnn_debug_tsne_split(gnn_ctx* ctx, int splits) {
    if (int rc = check_ctx(ctx)) return rc;
    if (splits < 0 || splits > 65535) {
        set_error("gnn_debug_tsne_split: " + std::to_string(splits) + " workgroups over the columns is outside [0, 65535]");
        return GNN_ERR_ARG;
    }
    ctx->ts.split = splits;
    return GNN_OK;
}

extern "C" int gnn_debug_tsne_ms(gnn_ctx* ctx, double* ms_out, int64_t capacity, int64_t* n_out) {
    if (int rc = check_ctx(ctx)) return rc;
    return ctx->ts.passes.out(ctx, "gnn_debug_tsne_ms", ms_out, capacity, n_out);
}
