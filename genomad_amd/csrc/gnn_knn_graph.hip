// k-nearest-neighbour graph of encoder embeddings (include/genomad_nn.h, "k-nearest-neighbour graph"): the
// neighbour lists of the self-search, joined into the upper-triangle CSR gnn_graph_* gives - a pair i < j of valid rows is an edge when
// j is in N(i) or i in N(j) (union), or both (mutual); its weight is the similarity the lists carry or the Jaccard overlap of the two
// neighbourhoods; a flag tells whether both ends list each other.  Sparse integer work behind one search, seven passes:
//   search   gnn_neighbours_dev, as it is: the self-search into the workspace's lists (int64 index, f32 similarity, -1 / NaN padded).
//   lists    one wave per row: the -1 entries go, an entry's place is the number of the row's entries with a smaller index (64
//            shuffles); int32 indices ascending, their similarities beside them, and the length.
//   count    one wave per row i, one lane per entry j.  j > i: the pair is row i's, and counts there (mutual: when i is in N(j)).
//            j < i: the pair is row j's, which counts it itself when i is in N(j); otherwise (union alone) this lane adds it to row j's
//            counter.  Membership is a binary search in the ordered list; the counters take integer atomic adds.
//   scan     nn_scan: indptr, the cursors and the 8-byte total; a row's class follows from its length (below) and the rows of the two
//            workgroup classes are listed.  The host reads the total and the two list lengths behind one synchronise.
//   fill     the count's walk again: an edge goes to the place an atomic add on its owner's cursor gives, as partner << 32 | the bits
//            of its similarity - the f32 of the listing row's own list; where both ends list each other, row i's (i < j), which is
//            the value gnn_graph gives the pair.  Every store is guarded by the segment's end.  Arrival order is arbitrary.
//   order    every row's segment ascending as uint64, which is ascending in the partner: partners are distinct within a row.  Up to
//            wave_rows (<= 64) entries one wave, an entry's place the number of smaller ones; up to group_rows (<= 4096) a workgroup,
//            a bitonic network in LDS; beyond, one workgroup and a stable LSD radix of 4-bit digits between the segment and the same
//            segment of a second buffer - thread t owns a run of the segment, counts its digits, the (digit, thread) counters are
//            scanned in that order, and it files its run in order: stable without a ballot.
//   finish   one lane per edge: its row by a binary search in indptr, the partner and the similarity unpacked, the flag from two
//            membership tests; Jaccard: the wave then takes its 64 edges in turn, lane l tests entry l of N(i) against N+(j), a ballot
//            counts the hits, i itself counts when i is in N(j), and the weight is __fdiv_rn(s, u) - one correctly rounded division.
// The edge set, an edge's owner and its payload depend on (i, j) and the lists only, the order within a row is a total order on
// distinct keys: no output bit depends on the arrival order, the grid or the class limits.  Only integer atomics; no loop waits for
// another workgroup, and every loop's end stands next to it.
// Memory: per row 20 k B of lists and 36 B of counters, offsets, cursors and class lists; per edge 16 B.  Nothing is n x n.
#include <cstring>

#include "gnn_nn_frag.h"

namespace gnn {
namespace {

typedef unsigned long long ull;

constexpr int KG_K_MAX = 64;                    // gnn_neighbours' KMAX: one entry per lane
constexpr int KG_WAVE_MAX = 64;                 // the wave class: one entry per lane
constexpr int KG_GROUP_MAX = 4096;              // the LDS class: 32 KB of uint64
constexpr int KG_RADIX_BITS = 4, KG_RADIX = 1 << KG_RADIX_BITS;
constexpr ull KG_PAD = ~0ull;                   // above every entry: a partner is below 2^31

// x is among the `len` ascending entries of `list`.  Ends: hi - lo shrinks in every round.
__device__ inline bool kg_has(const int32_t* __restrict__ list, int len, int32_t x) {
    int lo = 0, hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (list[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo < len && list[lo] == x;
}

// ---- lists: grid = ceil(n / 4) blocks of 4 waves, one wave per row
__global__ __launch_bounds__(256) void kg_lists_kernel(int64_t n, int k, const int64_t* __restrict__ nidx, const float* __restrict__ nsim,
                                                       int32_t* __restrict__ lidx, float* __restrict__ lsim, int32_t* __restrict__ len) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;                          // wave-uniform
    int64_t j = -1;
    float s = 0.f;
    if (lane < k) {
        j = nidx[i * k + lane];
        s = nsim[i * k + lane];
    }
    const bool ok = j >= 0 && j < n && j != i;   // the search gives nothing else; a list that did would lose the entry, never overrun
    const int32_t mine = ok ? (int32_t)j : 0x7fffffff;
    int rank = 0;
    for (int t = 0; t < k; ++t) {                // Ends: t grows towards k <= 64
        const int32_t other = __shfl(mine, t);
        rank += other < mine;
    }
    if (ok) {
        lidx[i * k + rank] = mine;               // rank < the number of valid entries <= k: distinct indices have distinct ranks
        lsim[i * k + rank] = s;
    }
    const int m = __popcll(__ballot(ok));
    if (lane == 0) len[i] = m;
}

struct KgArgs {
    int64_t n;
    int k;
    int mutual_only;                             // GNN_KNN_GRAPH_MUTUAL
    const int32_t* lidx;
    const float* lsim;
    const int32_t* len;
    int32_t* cnt;                                // count: [n], cleared before the launch
    ull* cursor;                                 // fill: [n], the segments' starts
    const int64_t* off;                          // fill, order, finish: [n + 1]
    ull* pairs;                                  // fill: [off[n]]
};

// ---- count (FILL false) and fill (FILL true): grid = ceil(n / 4) blocks of 4 waves, one wave per row, one lane per entry
template <bool FILL>
__global__ __launch_bounds__(256) void kg_walk_kernel(KgArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= a.n) return;                        // wave-uniform
    const int m = min(a.len[i], a.k);
    int32_t j = -1;
    float s = 0.f;
    if (lane < m) {
        j = a.lidx[i * a.k + lane];
        s = a.lsim[i * a.k + lane];
    }
    const bool ok = j >= 0 && j < a.n && j != (int32_t)i;
    bool back = false;                           // i is in N(j): looked up where the answer matters - union: j < i, mutual: j > i
    if (ok && (j > (int32_t)i) == (a.mutual_only != 0)) back = kg_has(a.lidx + (int64_t)j * a.k, min(a.len[j], a.k), (int32_t)i);
    const bool own = ok && j > (int32_t)i && (!a.mutual_only || back);          // row i's edge (i, j)
    const bool theirs = ok && j < (int32_t)i && !a.mutual_only && !back;        // row j's edge (j, i), which row j does not see
    if (!FILL) {
        const int c = __popcll(__ballot(own));
        if (lane == 0 && c) atomicAdd(&a.cnt[i], c);
        if (theirs) atomicAdd(&a.cnt[j], 1);
    } else if (own || theirs) {
        const int64_t owner = own ? i : (int64_t)j;
        const int32_t partner = own ? j : (int32_t)i;
        const ull at = atomicAdd(&a.cursor[owner], 1ull);
        if (at < (ull)a.off[owner + 1])          // always, unless the lists changed since the count: never an overrun
            a.pairs[at] = (ull)(uint32_t)partner << 32 | (ull)__float_as_uint(s);
    }
}

// ---- classes: one thread per row lists it where a workgroup orders it.  The lists' order is that of the atomic adds; no output depends
// on it.
__global__ __launch_bounds__(256) void kg_class_kernel(int64_t n, const int32_t* __restrict__ cnt, int wave_limit, int group_limit,
                                                       int32_t* __restrict__ rows, ull* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = cnt[i];
    if (c <= wave_limit) return;
    const int cls = c <= group_limit ? 0 : 1;
    const ull at = atomicAdd(&count[cls], 1ull);
    if (at < (ull)n) rows[(int64_t)cls * n + (int64_t)at] = (int32_t)i;
}

// ---- order, the wave class: grid = ceil(n / 4) blocks of 4 waves, one wave per row with 2 .. wave_limit entries
__global__ __launch_bounds__(256) void kg_order_wave_kernel(int64_t n, const int64_t* __restrict__ off, int wave_limit, ull* __restrict__ pairs) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;                          // wave-uniform
    const int64_t p = off[i], m = off[i + 1] - p;
    if (m < 2 || m > wave_limit || m > KG_WAVE_MAX) return;
    const ull mine = lane < m ? pairs[p + lane] : KG_PAD;
    int rank = 0;
    for (int t = 0; t < (int)m; ++t) {           // Ends: t grows towards m <= 64
        const ull other = __shfl(mine, t);
        rank += other < mine;
    }
    // equal entries (only where the lists changed behind the count) share a rank: some place keeps garbage, none is overrun
    if (lane < m && rank < m) pairs[p + rank] = mine;
}

// ---- order, the LDS class: one workgroup per listed row
__global__ __launch_bounds__(256) void kg_order_group_kernel(const int32_t* __restrict__ rows, const int64_t* __restrict__ off, ull* __restrict__ pairs) {
    __shared__ ull key[KG_GROUP_MAX];
    const int64_t i = rows[blockIdx.x];
    const int64_t p = off[i], m = off[i + 1] - p;
    if (m < 2 || m > KG_GROUP_MAX) return;       // workgroup-uniform
    int size = 2;
    while (size < m) size <<= 1;                 // Ends: size doubles towards m <= 4096
    for (int t = threadIdx.x; t < size; t += 256) key[t] = t < m ? pairs[p + t] : KG_PAD;      // Ends: t grows towards size
    __syncthreads();
    // the bitonic network: every loop's bounds are the workgroup's.  Ends: span doubles towards size, step halves towards 0
    for (int span = 2; span <= size; span <<= 1)
        for (int step = span >> 1; step > 0; step >>= 1) {
            for (int t = threadIdx.x; t < size; t += 256) {
                const int u = t ^ step;
                if (u > t) {
                    const ull x = key[t], y = key[u];
                    if ((x > y) == ((t & span) == 0)) {
                        key[t] = y;
                        key[u] = x;
                    }
                }
            }
            __syncthreads();
        }
    for (int t = threadIdx.x; t < m; t += 256) pairs[p + t] = key[t];       // the padding sorts behind every entry
}

// ---- order, the radix class: one workgroup per listed row; `passes` digits of 4 bits of the partner, an even number: the segment
// ends where it began.  Every barrier is reached by the whole workgroup: the loops' bounds are uniform.
__global__ __launch_bounds__(256) void kg_order_radix_kernel(const int32_t* __restrict__ rows, const int64_t* __restrict__ off, int passes,
                                                             ull* pairs, ull* other) {
    __shared__ int cell[KG_RADIX * 256];         // [digit][thread]
    __shared__ int run[256];
    const int tid = threadIdx.x;
    const int64_t i = rows[blockIdx.x];
    const int64_t p = off[i], m = off[i + 1] - p;
    if (m < 2) return;                           // workgroup-uniform
    const int64_t per = (m + 255) / 256;
    const int64_t b = min(m, (int64_t)tid * per), e = min(m, b + per);
    ull* src = pairs + p;
    ull* dst = other + p;
    for (int pass = 0; pass < passes; ++pass) {  // Ends: pass grows towards passes
        const int shift = 32 + KG_RADIX_BITS * pass;
        for (int d = 0; d < KG_RADIX; ++d) cell[d * 256 + tid] = 0;
        for (int64_t t = b; t < e; ++t) cell[(int)((src[t] >> shift) & (KG_RADIX - 1)) * 256 + tid] += 1;       // the thread's own cells
        __syncthreads();
        // exclusive sums over the 4096 cells in the order (digit, thread): thread t scans cells 16 t .. 16 t + 15, thread 0 the 256 sums
        int sum = 0;
        for (int c = 0; c < KG_RADIX; ++c) sum += cell[tid * KG_RADIX + c];
        run[tid] = sum;
        __syncthreads();
        if (tid == 0) {
            int acc = 0;
            for (int t = 0; t < 256; ++t) {
                const int v = run[t];
                run[t] = acc;
                acc += v;
            }
        }
        __syncthreads();
        sum = run[tid];
        for (int c = 0; c < KG_RADIX; ++c) {
            const int v = cell[tid * KG_RADIX + c];
            cell[tid * KG_RADIX + c] = sum;
            sum += v;
        }
        __syncthreads();
        for (int64_t t = b; t < e; ++t) {
            const ull x = src[t];
            const int64_t at = cell[(int)((x >> shift) & (KG_RADIX - 1)) * 256 + tid]++;
            if (at < m) dst[at] = x;             // always: the cells sum to m
        }
        __syncthreads();                         // the next pass reads what every thread wrote (a workgroup's global stores, behind its barrier)
        ull* const swap = src;
        src = dst;
        dst = swap;
    }
}

struct KgFinishArgs {
    int64_t n, total;
    int k;
    int jaccard;
    const int32_t* lidx;
    const int32_t* len;
    const int64_t* off;
    const ull* pairs;
    int32_t* col;
    float* sim;
    uint8_t* mutual;                             // or NULL
};

// ---- finish: grid = ceil(total / 256) blocks of 4 waves, one lane per edge
__global__ __launch_bounds__(256) void kg_finish_kernel(KgFinishArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = e < a.total;
    int32_t i = 0, j = 0;
    float w = 0.f;
    bool fwd = false, back = false, sane = false;
    if (live) {
        // the row whose segment holds e: the last i with off[i] <= e.  Ends: hi - lo shrinks in every round
        int64_t lo = 0, hi = a.n - 1;
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (a.off[mid] <= e) lo = mid;
            else hi = mid - 1;
        }
        i = (int32_t)lo;
        const ull x = a.pairs[e];
        j = (int32_t)(uint32_t)(x >> 32);
        w = __uint_as_float((uint32_t)x);
        sane = j >= 0 && j < a.n;                // always, unless the lists changed since the count: no list is read for such an entry
        if (sane) {
            fwd = kg_has(a.lidx + (int64_t)i * a.k, min(a.len[i], a.k), j);
            back = kg_has(a.lidx + (int64_t)j * a.k, min(a.len[j], a.k), i);
        }
    }
    if (a.jaccard) {
        // the wave's edges in turn (wave-uniform: t, and what the shuffles hand out).  Ends: t grows towards 64
        for (int t = 0; t < 64; ++t) {
            if (!__shfl((int)(live && sane), t)) continue;
            const int32_t ti = __shfl(i, t), tj = __shfl(j, t);
            const int tback = __shfl((int)back, t);
            const int mi = min(a.len[ti], a.k), mj = min(a.len[tj], a.k);
            bool hit = false;
            if (lane < mi) {
                const int32_t x = a.lidx[(int64_t)ti * a.k + lane];
                hit = x == tj || kg_has(a.lidx + (int64_t)tj * a.k, mj, x);
            }
            const int s = __popcll(__ballot(hit)) + tback;       // N(i)'s entries in N+(j), and i itself where j lists it
            const int u = mi + 1 + mj + 1 - s;
            if (lane == t) w = __fdiv_rn((float)s, (float)u);
        }
    }
    if (live) {
        a.col[e] = j;
        a.sim[e] = w;
        if (a.mutual) a.mutual[e] = fwd && back;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

int check_kg_args(const std::string& f, int64_t n, int k, int mode, int weight, int metric) {
    if (int rc = nn_check_rows(f, n, "rows")) return rc;
    if (k < 1 || k > KG_K_MAX) {
        set_error(f + ": k " + std::to_string(k) + " is outside [1, " + std::to_string(KG_K_MAX) + "]");
        return GNN_ERR_ARG;
    }
    if (mode != GNN_KNN_GRAPH_UNION && mode != GNN_KNN_GRAPH_MUTUAL) {
        set_error(f + ": mode " + std::to_string(mode) + " is outside [0, 1] (GNN_KNN_GRAPH_UNION, GNN_KNN_GRAPH_MUTUAL)");
        return GNN_ERR_ARG;
    }
    if (weight != GNN_KNN_GRAPH_SIMILARITY && weight != GNN_KNN_GRAPH_JACCARD) {
        set_error(f + ": weight " + std::to_string(weight) + " is outside [0, 1] (GNN_KNN_GRAPH_SIMILARITY, GNN_KNN_GRAPH_JACCARD)");
        return GNN_ERR_ARG;
    }
    return nn_check_metric(f, metric);
}

KgArgs kg_args(const gnn_ctx* ctx) {
    const KnnGraphWorkspace& w = ctx->kg;
    KgArgs a;
    a.n = w.n;
    a.k = w.k;
    a.mutual_only = w.mode == GNN_KNN_GRAPH_MUTUAL;
    a.lidx = w.lidx.get();
    a.lsim = w.lsim.get();
    a.len = w.len.get();
    a.cnt = w.cnt.get();
    a.cursor = w.cursor.get();
    a.off = w.off.get();
    a.pairs = w.pairs[0].get();
    return a;
}

// one wave per row, four to a block
template <typename... P, typename... A>
int launch_rows(void (*kernel)(P...), int64_t n, hipStream_t stream, A&&... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, static_cast<P>(args)...);
    GNN_HIP(hipGetLastError());
    return GNN_OK;
}

// n >= 0 rows on the device -> indptr[n + 1] on the device and the total on the host; the ctx's stream is synchronised.  The workspace
// then holds the ordered lists, the offsets and the classes: all the fill needs.
int kg_count(gnn_ctx* ctx, const float* rows_dev, int64_t n, int k, int mode, int weight, int metric, int64_t* indptr_dev, int64_t* nnz_host) {
    KnnGraphWorkspace& w = ctx->kg;
    w.counted = false;
    w.host_rows = false;
    w.passes.begin();
    w.n = n;
    w.k = k;
    w.mode = mode;
    w.weight = weight;
    w.metric = metric;
    w.wave_limit = std::min(w.wave_rows, KG_WAVE_MAX);
    w.group_limit = std::min(w.group_rows, KG_GROUP_MAX);
    w.class_rows[0] = w.class_rows[1] = 0;
    int64_t total = 0;
    if (n == 0) {
        GNN_HIP(hipMemsetAsync(indptr_dev, 0, sizeof(int64_t), ctx->stream));
        GNN_HIP(hipStreamSynchronize(ctx->stream));
    } else {
        const size_t cells = (size_t)n * k;
        int rc = nn_reserve(ctx, w.nidx, cells);
        if (!rc) rc = nn_reserve(ctx, w.nsim, cells);
        if (!rc) rc = nn_reserve(ctx, w.lidx, cells);
        if (!rc) rc = nn_reserve(ctx, w.lsim, cells);
        if (!rc) rc = nn_reserve(ctx, w.len, (size_t)n);
        if (!rc) rc = nn_reserve(ctx, w.cnt, (size_t)n);
        if (!rc) rc = nn_reserve(ctx, w.off, (size_t)n + 1);
        if (!rc) rc = nn_reserve(ctx, w.cursor, (size_t)n);
        if (!rc) rc = nn_reserve(ctx, w.rows, (size_t)2 * n);
        if (!rc) rc = w.count.reserve(ctx, 2);
        if (rc) return rc;
        {
            PassLog::Scope pass(ctx, w.passes);
            if ((rc = gnn_neighbours_dev(ctx, rows_dev, n, nullptr, 0, k, metric, w.nidx.get(), w.nsim.get()))) return rc;
        }
        {
            PassLog::Scope pass(ctx, w.passes);
            if ((rc = launch_rows(kg_lists_kernel, n, ctx->stream, n, k, w.nidx, w.nsim, w.lidx, w.lsim, w.len))) return rc;
        }
        {
            PassLog::Scope pass(ctx, w.passes);
            GNN_HIP(hipMemsetAsync(w.cnt.get(), 0, (size_t)n * sizeof(int32_t), ctx->stream));
            if ((rc = launch_rows(kg_walk_kernel<false>, n, ctx->stream, kg_args(ctx)))) return rc;
        }
        {
            PassLog::Scope pass(ctx, w.passes);
            if ((rc = nn_scan(ctx->stream, w.cnt, n, w.off, nullptr))) return rc;
            GNN_HIP(hipMemcpyAsync(indptr_dev, w.off.get(), (size_t)(n + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, ctx->stream));
            if ((rc = w.count.zero(ctx, 0, 2))) return rc;
            if ((rc = launch_1d(kg_class_kernel, n, ctx->stream, n, w.cnt, w.wave_limit, w.group_limit, w.rows, w.count.dev()))) return rc;
        }
        GNN_HIP(hipMemcpyAsync(&total, w.off.get() + n, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        ull classes[2] = {0, 0};
        if ((rc = w.count.read(ctx, 0, 2, classes))) return rc;             // synchronises: the total has landed too
        w.class_rows[0] = (int64_t)std::min<ull>(classes[0], (ull)n);
        w.class_rows[1] = (int64_t)std::min<ull>(classes[1], (ull)n);
        // the fill's buffers, while nothing is enqueued: the fill itself allocates nothing
        if ((rc = nn_reserve(ctx, w.pairs[0], (size_t)std::max<int64_t>(total, 1)))) return rc;
        if (w.class_rows[1] > 0 && (rc = nn_reserve(ctx, w.pairs[1], (size_t)total))) return rc;
    }
    w.passes.settle();
    w.total = total;
    w.counted = true;
    *nnz_host = total;
    return GNN_OK;
}

// GNN_OK when the fill may run (or has nothing to do).  A fill belongs to the ctx's last count of the same arguments.
int kg_check_fill(gnn_ctx* ctx, const std::string& f, int64_t n, int k, int mode, int weight, int metric, int64_t capacity, bool host_rows) {
    const KnnGraphWorkspace& w = ctx->kg;
    if (!w.counted || w.n != n || w.k != k || w.mode != mode || w.weight != weight || w.metric != metric || (host_rows && !w.host_rows)) {
        set_error(f + ": no gnn_knn_graph_count" + (host_rows ? "" : "*") + " of the same (n, k, mode, weight, metric) = (" + std::to_string(n) + ", " +
                  std::to_string(k) + ", " + std::to_string(mode) + ", " + std::to_string(weight) + ", " + std::to_string(metric) +
                  ") came before it");
        return GNN_ERR_STATE;
    }
    if (capacity < w.total) {
        set_error(f + ": capacity " + std::to_string(capacity) + " is below the " + std::to_string(w.total) + " edges the count found");
        return GNN_ERR_ARG;
    }
    return GNN_OK;
}

// the 4-bit digits the radix class walks: enough for the partners of n rows, and an even number
int kg_radix_passes(int64_t n) {
    int bits = 1;
    while (bits < 31 && ((int64_t)1 << bits) < n) ++bits;
    const int passes = (bits + KG_RADIX_BITS - 1) / KG_RADIX_BITS;
    return passes + (passes & 1);
}

// total > 0 edges of the counted lists -> col, sim and (unless NULL) mutual on the device, enqueued on the ctx's stream
int kg_fill(gnn_ctx* ctx, int32_t* col_dev, float* sim_dev, uint8_t* mutual_dev) {
    KnnGraphWorkspace& w = ctx->kg;
    const int64_t n = w.n;
    int rc = GNN_OK;
    {
        PassLog::Scope pass(ctx, w.passes);
        GNN_HIP(hipMemcpyAsync(w.cursor.get(), w.off.get(), (size_t)n * sizeof(int64_t), hipMemcpyDeviceToDevice, ctx->stream));
        if ((rc = launch_rows(kg_walk_kernel<true>, n, ctx->stream, kg_args(ctx)))) return rc;
    }
    {
        PassLog::Scope pass(ctx, w.passes);
        if ((rc = launch_rows(kg_order_wave_kernel, n, ctx->stream, n, w.off, w.wave_limit, w.pairs[0]))) return rc;
        if (w.class_rows[0] > 0) {
            hipLaunchKernelGGL(kg_order_group_kernel, dim3((unsigned)w.class_rows[0]), dim3(256), 0, ctx->stream, w.rows.get(), w.off.get(),
                               w.pairs[0].get());
            GNN_HIP(hipGetLastError());
        }
        if (w.class_rows[1] > 0) {
            hipLaunchKernelGGL(kg_order_radix_kernel, dim3((unsigned)w.class_rows[1]), dim3(256), 0, ctx->stream, w.rows.get() + n, w.off.get(),
                               kg_radix_passes(n), w.pairs[0].get(), w.pairs[1].get());
            GNN_HIP(hipGetLastError());
        }
    }
    PassLog::Scope pass(ctx, w.passes);
    KgFinishArgs a;
    a.n = n;
    a.total = w.total;
    a.k = w.k;
    a.jaccard = w.weight == GNN_KNN_GRAPH_JACCARD;
    a.lidx = w.lidx.get();
    a.len = w.len.get();
    a.off = w.off.get();
    a.pairs = w.pairs[0].get();
    a.col = col_dev;
    a.sim = sim_dev;
    a.mutual = mutual_dev;
    return launch_1d(kg_finish_kernel, w.total, ctx->stream, a);
}

int kg_knob(gnn_ctx* ctx, const char* fn, int* knob, int value, int hi) {
    if (int rc = check_ctx(ctx)) return rc;
    if (value < 1 || value > hi) {
        set_error(std::string(fn) + ": " + std::to_string(value) + " entries is outside [1, " + std::to_string(hi) + "]");
        return GNN_ERR_ARG;
    }
    *knob = value;
    return GNN_OK;
}

}  // namespace
}  // namespace gnn

using namespace gnn;

extern "C" int gnn_knn_graph_count_dev(gnn_ctx* ctx, const float* rows_dev, int64_t n, int k, int mode, int weight, int metric,
                                       int64_t* indptr_dev, int64_t* nnz_host) {
    const char* const fn = "gnn_knn_graph_count_dev";
    if (int rc = check_kg_args(fn, n, k, mode, weight, metric)) return rc;
    if (int rc = nn_check_required(fn, (n == 0 || rows_dev) && indptr_dev && nnz_host, "the rows, indptr and nnz")) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    return kg_count(ctx, rows_dev, n, k, mode, weight, metric, indptr_dev, nnz_host);
}

extern "C" int gnn_knn_graph_fill_dev(gnn_ctx* ctx, int64_t n, int k, int mode, int weight, int metric, int32_t* col_dev, float* sim_dev,
                                      uint8_t* mutual_dev_or_null, int64_t capacity) {
    const char* const fn = "gnn_knn_graph_fill_dev";
    if (int rc = check_kg_args(fn, n, k, mode, weight, metric)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (int rc = kg_check_fill(ctx, fn, n, k, mode, weight, metric, capacity, false)) return rc;
    if (ctx->kg.total == 0) return GNN_OK;
    if (int rc = nn_check_required(fn, col_dev && sim_dev, "col and sim")) return rc;
    return kg_fill(ctx, col_dev, sim_dev, mutual_dev_or_null);
}

extern "C" int gnn_knn_graph_count(gnn_ctx* ctx, const float* rows_host, int64_t n, int k, int mode, int weight, int metric,
                                   int64_t* indptr_host, int64_t* nnz_host) {
    const char* const fn = "gnn_knn_graph_count";
    if (int rc = check_kg_args(fn, n, k, mode, weight, metric)) return rc;
    if (int rc = nn_check_required(fn, (n == 0 || rows_host) && indptr_host && nnz_host, "the rows, indptr and nnz")) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    KnnGraphWorkspace& w = ctx->kg;
    w.counted = false;
    Landing land(w.d_out);
    land.add(indptr_host, n + 1);
    int rc = land.reserve(ctx);                               // both buffers stand before the copy is enqueued
    if (!rc) rc = nn_upload_rows(ctx, rows_host, n);
    if (!rc) rc = kg_count(ctx, ctx->nn.d_base, n, k, mode, weight, metric, land.dev<int64_t>(0), nnz_host);
    if (!rc) rc = land.copy_out(ctx);
    if (rc) return rc;
    w.host_rows = true;
    return GNN_OK;
}

extern "C" int gnn_knn_graph_fill(gnn_ctx* ctx, int64_t n, int k, int mode, int weight, int metric, int32_t* col_host, float* sim_host,
                                  uint8_t* mutual_host_or_null, int64_t capacity) {
    const char* const fn = "gnn_knn_graph_fill";
    if (int rc = check_kg_args(fn, n, k, mode, weight, metric)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (int rc = kg_check_fill(ctx, fn, n, k, mode, weight, metric, capacity, true)) return rc;
    KnnGraphWorkspace& w = ctx->kg;
    const int64_t total = w.total;
    if (total == 0) return GNN_OK;
    if (int rc = nn_check_required(fn, col_host && sim_host, "col and sim")) return rc;
    Landing land(w.d_out);
    const int col = land.add(col_host, total), sim = land.add(sim_host, total), mutual = land.add(mutual_host_or_null, total);
    int rc = land.reserve(ctx);
    if (!rc) rc = kg_fill(ctx, land.dev<int32_t>(col), land.dev<float>(sim), mutual_host_or_null ? land.dev<uint8_t>(mutual) : nullptr);
    return rc ? rc : land.copy_out(ctx);
}

extern "C" int gnn_debug_knn_graph_wave_rows(gnn_ctx* ctx, int entries) {
    return ctx ? kg_knob(ctx, "gnn_debug_knn_graph_wave_rows", &ctx->kg.wave_rows, entries, KG_WAVE_MAX) : check_ctx(ctx);
}

extern "C" int gnn_debug_knn_graph_group_rows(gnn_ctx* ctx, int entries) {
    return ctx ? kg_knob(ctx, "gnn_debug_knn_graph_group_rows", &ctx->kg.group_rows, entries, KG_GROUP_MAX) : check_ctx(ctx);
}

extern "C" int gnn_debug_knn_graph_classes(gnn_ctx* ctx, int64_t* rows_out) {
    if (int rc = check_ctx(ctx)) return rc;
    if (int rc = nn_check_required("gnn_debug_knn_graph_classes", rows_out != nullptr, "rows_out")) return rc;
    rows_out[0] = ctx->kg.class_rows[0];
    rows_out[1] = ctx->kg.class_rows[1];
    return GNN_OK;
}

extern "C" int gnn_debug_knn_graph_ms(gnn_ctx* ctx, double* ms_out, int64_t capacity, int64_t* n_out) {
    if (int rc = check_ctx(ctx)) return rc;
    return ctx->kg.passes.out(ctx, "gnn_debug_knn_graph_ms", ms_out, capacity, n_out);
}
