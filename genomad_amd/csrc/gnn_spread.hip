// Label spreading over a similarity graph (include/genomad_nn.h, "label spreading"): the labels of seed rows
// spread along the graph's edges until nothing changes, in integers throughout - the definition is sequence.label_spread, and every
// output here equals it bit for bit.  ONE = 2^30 is a score of 1, 2^31 a row's transition mass, W = 2^24 a similarity of 1.
//   validate, symmetrise   gnn_csr_sym.h, shared with the other consumers of the graph; a second flag bit is a label outside
//                [-1, n_classes).  The host reads one word; GNN_ERR_ARG before anything else runs, the outputs untouched.
//   convert      one wave per row: d = the sum of the row's q (integer adds, a shuffle reduction), then p = (q << 31) / d in place of
//                q - the one 64-bit division per entry.  The rows an iteration has to compute - valid, with entries, no clamped seed -
//                are pushed on one of two lists: a row of up to LONG_ROW entries is a wave's work, a longer one a workgroup's.  A row
//                without entries is on neither list: it costs nothing.
//   iteration 1  F^0 = 0, so F^1 is the seeds' own term: one thread per (row, class) writes it into both buffers.
//   iteration t  one launch, F double buffered.  The lanes of a wave stand as (neighbour slot x class): S = 64 / cw slots of cw =
//                2^ceil(log2(min(n_classes, 64))) classes; above 64 classes the wave walks chunks of 64.  A lane adds p_ij * F_j[c]
//                over its slot's entries (64-bit integer multiply-adds), the slots are added by shuffles, a workgroup's four waves
//                through LDS - integer sums, the same bits in any order.  The epilogue does the two shifts, compares with the old row,
//                counts a changed row in LDS - the workgroup adds its count to the iteration's `changed` counter once, since 26 000
//                adds to one address were a third of a narrow iteration - and sets `first`.  The host reads that counter, 8 bytes.
//   dirty rows   a row that changes stores 1 at mark[t & 1][j] of itself and of every neighbour j - plain stores of the same value.
//                A row whose mark[(t - 1) & 1] is 0 recomputes the value it has - neither it nor a neighbour changed, so both buffers
//                hold that value already - and is skipped; a row that reads a 1 clears it, for iteration t + 1 to write there.
//                Iteration 2 computes every listed row.  gnn_debug_spread_skip(ctx, 0) computes every listed row always and
//                writes no marks.
//   summarise    one launch: best, best_score, second_score, total.
// Only integer add atomics (the lists' and the iterations' counters; the degrees).  No float is added or compared, no inline assembly,
// no loop that waits for another workgroup: every loop's termination argument stands next to it.  Every store is guarded by its bound.
#include "gnn_nn_frag.h"
#include "gnn_csr_sym.h"

namespace gnn {
namespace {

typedef unsigned long long ull;

constexpr int CLASSES_MAX = 1024;                // gnn_vote's
constexpr int MAX_ITER_MAX = 10000;
constexpr int LONG_ROW = 1024;                   // a row of more entries is a workgroup's work
constexpr int THREADS = 256;
constexpr ull ONE = 1ull << 30;

struct SpArgs {
    int64_t n;
    int C, cw_log, a, it, mark, skip;   // mark: the dirty-row rule is on; skip: and this iteration may skip (it > 2)
    const int64_t* soff;       // the symmetric graph: [n + 1]
    const int32_t* sidx;
    const uint32_t* sp;        // p_ij
    const int32_t* seed;       // [n]
    const uint32_t* Fo;        // step t - 1
    uint32_t* Fn;              // step t
    uint8_t* mprev;            // the marks iteration t - 1 wrote
    uint8_t* mnext;            // the marks this iteration writes
    int32_t* first;            // [n]
    ull* changed;              // the iteration's counter
    const int32_t* rows;       // the lists
    const int32_t* long_rows;
    const ull* nrows;          // [rows, long rows]
};

// a label outside [-1, C): bit 1 of the flag.  seed[i] = the class of a valid labelled row, -1 of every other
__global__ __launch_bounds__(256) void sp_seed_kernel(int64_t n, int C, const int64_t* __restrict__ label, const uint8_t* __restrict__ ok,
                                                      int32_t* __restrict__ seed, ull* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t l = label[i];
    const bool in = l >= -1 && l < C;
    if (!in) atomicOr(flag, 2ull);
    seed[i] = in && l >= 0 && ok[i] ? (int32_t)l : -1;
}

// one wave per row, four rows per workgroup: q -> p, and the row's place on a list
__global__ __launch_bounds__(THREADS) void sp_convert_kernel(int64_t n, int clamp, const int64_t* __restrict__ soff, uint32_t* __restrict__ sp,
                                                             const uint8_t* __restrict__ ok, const int32_t* __restrict__ seed,
                                                             int32_t* __restrict__ rows, int32_t* __restrict__ long_rows, ull* __restrict__ nrows) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;                                       // uniform in the wave
    const int64_t b = soff[i], e = soff[i + 1];
    if (e <= b) return;
    ull d = 0;
    for (int64_t x = b + lane; x < e; x += 64) d += sp[x];    // Ends: x grows towards e
    for (int o = 32; o; o >>= 1) d += __shfl_xor(d, o);
    if (d)                                                    // always: every filed q is > 0
        for (int64_t x = b + lane; x < e; x += 64) sp[x] = (uint32_t)(((ull)sp[x] << 31) / d);      // Ends: x grows towards e.  p <= 2^31
    if (lane == 0 && ok[i] && !(clamp && seed[i] >= 0)) {
        const bool wide = e - b > LONG_ROW;
        const ull at = atomicAdd(nrows + (wide ? 1 : 0), 1ull);
        if (at < (ull)n) (wide ? long_rows : rows)[at] = (int32_t)i;      // always: a row is pushed once
    }
}

// iteration 1: one thread per (row, class).  Both buffers get F^1; a seed's one non-zero cell counts the row as changed
__global__ __launch_bounds__(256) void sp_init_kernel(int64_t n, int C, int a, int clamp, const int32_t* __restrict__ seed,
                                                      uint32_t* __restrict__ F0, uint32_t* __restrict__ F1, int32_t* __restrict__ first,
                                                      ull* __restrict__ changed) {
    const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (cell >= n * C) return;
    const int64_t i = cell / C;
    const int c = (int)(cell - i * C), sd = seed[i];
    const uint32_t v = sd == c ? (uint32_t)(clamp ? ONE : ((ull)(64 - a) * ONE) >> 6) : 0u;
    F0[cell] = v;
    F1[cell] = v;
    if (v) {
        first[i] = 1;
        atomicAdd(changed, 1ull);
    } else if (c == 0 && sd < 0) {
        first[i] = -1;
    }
}

// Row i of iteration a.it, by one wave (BLOCK false) or by the whole workgroup (BLOCK true: every thread calls it).
template <bool BLOCK>
__device__ __forceinline__ void sp_row(const SpArgs& a, int i, ull (*part)[64], int* word, unsigned* tally) {
    const int tid = threadIdx.x, lane = tid & 63, wave = BLOCK ? tid >> 6 : 0;
    const int cw = 1 << a.cw_log, S = 64 >> a.cw_log, cl = lane & (cw - 1), s = lane >> a.cw_log;
    const int me = BLOCK ? tid : lane, coop = BLOCK ? THREADS : 64, step = BLOCK ? 4 * S : S;
    const int64_t b = a.soff[i], e = a.soff[i + 1];
    // the row's mark: read and cleared by one thread, in that order
    if (a.mark) {                                             // uniform
        int dirty = 0;
        if (me == 0) {
            dirty = a.mprev[i];
            if (dirty) a.mprev[i] = 0;
        }
        if (BLOCK) {
            if (tid == 0) *word = dirty;
            __syncthreads();
            dirty = *word;
            __syncthreads();
        } else {
            dirty = __shfl(dirty, 0);
        }
        if (a.skip && !dirty) return;                         // uniform: the row is the wave's or the workgroup's
    }
    const int sd = a.seed[i];
    bool ch = false, nz = false;
    for (int cb = 0; cb < a.C; cb += 64) {                    // Ends: cb grows towards C
        const int c = cb + cl;
        ull acc = 0;
        if (c < a.C)
            for (int64_t x = b + wave * S + s; x < e; x += step)      // Ends: x grows towards e
                acc += (ull)a.sp[x] * (ull)a.Fo[(int64_t)a.sidx[x] * a.C + c];
        for (int o = cw; o < 64; o <<= 1) acc += __shfl_xor(acc, o);  // Ends: o doubles towards 64
        if (BLOCK) {
            if (s == 0) part[wave][cl] = acc;
            __syncthreads();
            if (wave == 0) acc = part[0][cl] + part[1][cl] + part[2][cl] + part[3][cl];
            __syncthreads();
        }
        if (wave == 0 && s == 0 && c < a.C) {
            const ull g = acc >> 31;
            const ull nv = ((ull)a.a * g + (sd == c ? (ull)(64 - a.a) * ONE : 0ull)) >> 6;
            const int64_t at = (int64_t)i * a.C + c;          // i < n, c < C
            ch |= (uint32_t)nv != a.Fo[at];
            nz |= nv != 0;
            a.Fn[at] = (uint32_t)nv;
        }
    }
    int any = (__ballot(ch) != 0 ? 1 : 0) | (__ballot(nz) != 0 ? 2 : 0);
    if (BLOCK) {
        if (tid == 0) *word = any;
        __syncthreads();
        any = *word;
        __syncthreads();
    }
    if (any & 1) {
        if (me == 0) atomicAdd(tally, 1u);                    // in LDS: the workgroup adds its rows to the counter once
        if (a.mark) {
            if (me == 0) a.mnext[i] = 1;
            for (int64_t x = b + me; x < e; x += coop) {      // Ends: x grows towards e
                const int j = a.sidx[x];
                if ((unsigned)j < (ull)a.n) a.mnext[j] = 1;   // always: the graph holds rows below n
            }
        }
    }
    if (me == 0 && (any & 2) && a.first[i] < 0) a.first[i] = a.it;
}

// grid = the groups, 256 threads: workgroup g takes the long rows g, g + groups, ..., then its waves the rows w, w + 4 * groups, ...
__global__ __launch_bounds__(THREADS) void sp_iterate_kernel(SpArgs a) {
    __shared__ ull part[4][64];
    __shared__ int word;
    __shared__ unsigned tally;                                // the rows of this workgroup that changed
    if (threadIdx.x == 0) tally = 0;
    __syncthreads();
    const int64_t nlong = (int64_t)min(a.nrows[1], (ull)a.n), nshort = (int64_t)min(a.nrows[0], (ull)a.n);
    for (int64_t w = blockIdx.x; w < nlong; w += gridDim.x) { // Ends: w grows towards nlong
        const int i = a.long_rows[w];
        if ((unsigned)i < (ull)a.n) sp_row<true>(a, i, part, &word, &tally);      // always; uniform: w is the workgroup's
    }
    for (int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < nshort; w += (int64_t)gridDim.x * 4) {      // Ends: w grows towards nshort
        const int i = a.rows[w];
        if ((unsigned)i < (ull)a.n) sp_row<false>(a, i, part, &word, &tally);      // always; no barrier on this path
    }
    __syncthreads();                                          // every thread arrives: the loops above end, and nothing returns inside them
    if (threadIdx.x == 0 && tally) atomicAdd(a.changed, (ull)tally);
}

// 64 >> cw_log rows per wave: the largest score with the smallest class, the largest among the other classes, the sum
__global__ __launch_bounds__(THREADS) void sp_summarise_kernel(int64_t n, int C, int cw_log, const uint32_t* __restrict__ F, int32_t* __restrict__ best,
                                                               uint32_t* __restrict__ best_score, uint32_t* __restrict__ second_score,
                                                               ull* __restrict__ total) {
    const int lane = threadIdx.x & 63, cw = 1 << cw_log, cl = lane & (cw - 1);
    const int64_t i = (((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) << (6 - cw_log)) + (lane >> cw_log);
    ull key = 0, sum = 0;                                     // key: (score << 32) | (2^32 - 1 - class); 0: none
    uint32_t m2 = 0;
    if (i < n)
        for (int c = cl; c < C; c += cw) {                    // Ends: c grows towards C
            const uint32_t v = F[i * C + c];
            const ull k = ((ull)v << 32) | (ull)(0xffffffffu - (uint32_t)c);
            sum += v;
            if (k > key) {
                m2 = max(m2, (uint32_t)(key >> 32));
                key = k;
            } else {
                m2 = max(m2, v);
            }
        }
    for (int o = 1; o < cw; o <<= 1) {                        // Ends: o doubles towards cw
        const ull k2 = __shfl_xor(key, o);
        const uint32_t s2 = __shfl_xor(m2, o);
        sum += __shfl_xor(sum, o);
        m2 = max(max(m2, s2), (uint32_t)(min(key, k2) >> 32));
        key = max(key, k2);
    }
    if (i < n && cl == 0) {
        const uint32_t top = (uint32_t)(key >> 32);
        best[i] = top ? (int32_t)(0xffffffffu - (uint32_t)key) : -1;
        best_score[i] = top;
        second_score[i] = m2;
        total[i] = sum;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

struct SpreadIn : CsrGraph {    // the graph on the device
    const int64_t* label;      // device
    int C, a, clamp, max_iter;
};

struct SpreadOut {             // device; score may be NULL
    uint32_t* score;
    int32_t* best;
    uint32_t* best_score;
    uint32_t* second_score;
    ull* total;
    int32_t* first;
};

int spread_check(const char* fn, const SpreadIn& in, const SpreadOut& out, const void* changed, const void* iterations, const void* converged) {
    const std::string f(fn);
    const auto bad = [&](const char* what, int64_t v, const char* range) {
        set_error(f + ": " + what + " " + std::to_string(v) + " is outside " + range);
        return GNN_ERR_ARG;
    };
    if (int rc = graph_check(f, in.n, in.nnz)) return rc;
    if (in.C < 1 || in.C > CLASSES_MAX) return bad("n_classes", in.C, "[1, 1024]");
    if (in.a < 1 || in.a > 63) return bad("alpha_64ths", in.a, "[1, 63]: alpha is a multiple of 1/64 in (0, 1)");
    if (in.max_iter < 1 || in.max_iter > MAX_ITER_MAX) return bad("max_iter", in.max_iter, "[1, 10000]");
    return nn_check_required(f,
                             in.indptr && (in.nnz == 0 || (in.col && in.sim)) && iterations && converged && changed &&
                                 (in.n == 0 || (in.label && out.best && out.best_score && out.second_score && out.total && out.first)),
                             "indptr, col, sim, label, the five per-row outputs, changed, iterations and converged");
}

int ceil_log2(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;                                 // Ends: l grows towards 6
    return l;
}

// n > 0 rows: the graph and the labels on the device -> the outputs on the device and iterations, converged, changed on the host.  The
// ctx's stream is synchronised once for the verdict on graph and labels and once per iteration.
int spread_run(gnn_ctx* ctx, const char* fn, const SpreadIn& in, const SpreadOut& out, int64_t* changed_host, int64_t* iterations_host,
               int* converged_host) {
    SpreadWorkspace& w = ctx->sprd;
    w.passes.begin();
    const int64_t n = in.n;
    const size_t cells = (size_t)n * in.C, tail = (size_t)in.max_iter;       // the counters behind the iterations': [rows, long rows, verdict]
    const int cw_log = ceil_log2(std::min(in.C, 64));
    int rc = nn_reserve(ctx, w.ok, (size_t)n);
    if (!rc) rc = nn_reserve(ctx, w.seed, (size_t)n);
    if (!rc) rc = w.count.reserve(ctx, tail + 3);
    if (!rc) rc = w.count.zero(ctx, 0, tail + 3);
    if (rc) return rc;
    {
        PassLog::Scope setup(ctx, w.passes);                  // open across the read below: nothing is settled there
        if ((rc = graph_validate_launch(ctx, in, w.ok.get(), w.count, tail + 2))) return rc;
        if ((rc = launch_1d(sp_seed_kernel, n, ctx->stream, n, in.C, in.label, w.ok.get(), w.seed.get(), w.count.dev() + tail + 2))) return rc;
        ull bad = 0;
        if ((rc = graph_verdict(ctx, fn, in, w.count, tail + 2, &bad))) return rc;
        if (bad) {
            set_error(std::string(fn) + ": a label is outside [-1, " + std::to_string(in.C) + ")");
            return GNN_ERR_ARG;
        }
        const size_t entries = (size_t)std::max<int64_t>(2 * in.nnz, 1);
        rc = nn_reserve(ctx, w.deg, (size_t)n);
        if (!rc) rc = nn_reserve(ctx, w.soff, (size_t)n + 1);
        if (!rc) rc = nn_reserve(ctx, w.cursor, (size_t)n);
        if (!rc) rc = nn_reserve(ctx, w.sidx, entries);
        if (!rc) rc = nn_reserve(ctx, w.sp, entries);
        if (!rc) rc = nn_reserve(ctx, w.rows, (size_t)n);
        if (!rc) rc = nn_reserve(ctx, w.long_rows, (size_t)n);
        for (int b = 0; b < 2 && !rc; ++b) {
            rc = nn_reserve(ctx, w.F[b], cells);
            if (!rc) rc = nn_reserve(ctx, w.mark[b], (size_t)n);
        }
        if (rc) return rc;
        for (int b = 0; b < 2; ++b) GNN_HIP(hipMemsetAsync(w.mark[b].get(), 0, (size_t)n, ctx->stream));
        if ((rc = csr_symmetrise(ctx->stream, n, in.indptr, in.col, in.sim, w.ok.get(), w.deg.get(), w.soff.get(), w.cursor.get(), w.sidx.get(),
                                 w.sp.get())))
            return rc;
        hipLaunchKernelGGL(sp_convert_kernel, dim3((unsigned)((n + 3) / 4)), dim3(THREADS), 0, ctx->stream, n, in.clamp, w.soff.get(), w.sp.get(),
                           w.ok.get(), w.seed.get(), w.rows.get(), w.long_rows.get(), w.count.dev() + tail);
        GNN_HIP(hipGetLastError());
    }
    SpArgs a;
    a.n = n;
    a.C = in.C;
    a.cw_log = cw_log;
    a.a = in.a;
    a.soff = w.soff.get();
    a.sidx = w.sidx.get();
    a.sp = w.sp.get();
    a.seed = w.seed.get();
    a.first = out.first;
    a.rows = w.rows.get();
    a.long_rows = w.long_rows.get();
    a.nrows = w.count.dev() + tail;
    const int groups = w.groups > 0 ? w.groups : (int)std::min<int64_t>((n + 3) / 4, 8 * (int64_t)std::max(ctx->cu_count, 1));
    int it = 0;
    bool converged = false;
    while (it < in.max_iter && !converged) {                  // Ends: it grows towards max_iter
        ++it;
        {
            PassLog::Scope iteration(ctx, w.passes);
            if (it == 1) {
                if ((rc = launch_1d(sp_init_kernel, (int64_t)cells, ctx->stream, n, in.C, in.a, in.clamp, w.seed.get(), w.F[0].get(), w.F[1].get(),
                                    out.first, w.count.dev())))
                    return rc;
            } else {                                          // from buffer (it - 1) & 1 into buffer it & 1; the marks likewise
                a.it = it;
                a.mark = w.skip;
                a.skip = w.skip && it > 2;
                a.Fo = w.F[(it - 1) & 1].get();
                a.Fn = w.F[it & 1].get();
                a.mprev = w.mark[(it - 1) & 1].get();
                a.mnext = w.mark[it & 1].get();
                a.changed = w.count.dev() + (it - 1);
                hipLaunchKernelGGL(sp_iterate_kernel, dim3((unsigned)groups), dim3(THREADS), 0, ctx->stream, a);
                GNN_HIP(hipGetLastError());
            }
        }
        ull changed = 0;
        if ((rc = w.count.read(ctx, (size_t)it - 1, 1, &changed))) return rc;
        w.passes.settle();
        changed_host[it - 1] = (int64_t)changed;
        converged = changed == 0;
    }
    const uint32_t* F = w.F[it & 1].get();
    {
        ProfScope prof(ctx, GNN_K_NEIGHBOURS);
        const int64_t per_block = (int64_t)4 << (6 - cw_log);
        hipLaunchKernelGGL(sp_summarise_kernel, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(THREADS), 0, ctx->stream, n, in.C, cw_log, F,
                           out.best, out.best_score, out.second_score, out.total);
        GNN_HIP(hipGetLastError());
    }
    *iterations_host = it;
    *converged_host = converged;
    return GNN_OK;
}

// n == 0: the definition's answer - one iteration that changes nothing
void spread_empty(gnn_ctx* ctx, int64_t* changed_host, int64_t* iterations_host, int* converged_host) {
    ctx->sprd.passes.begin();
    changed_host[0] = 0;
    *iterations_host = 1;
    *converged_host = 1;
}

}  // namespace
}  // namespace gnn

using namespace gnn;

extern "C" int gnn_spread_dev(gnn_ctx* ctx, const int64_t* indptr_dev, const int32_t* col_dev, const float* sim_dev, const uint8_t* valid_dev_or_null,
                              const int64_t* label_dev, int64_t n, int64_t nnz, int n_classes, int alpha_64ths, int clamp, int max_iter,
                              uint32_t* score_dev_or_null, int32_t* best_dev, uint32_t* best_score_dev, uint32_t* second_score_dev,
                              uint64_t* total_dev, int32_t* first_dev, int64_t* changed_host, int64_t* iterations_host, int* converged_host) {
    const char* const fn = "gnn_spread_dev";
    const SpreadIn in = {{indptr_dev, col_dev, sim_dev, valid_dev_or_null, n, nnz}, label_dev, n_classes, alpha_64ths, clamp != 0, max_iter};
    const SpreadOut out = {score_dev_or_null, best_dev, best_score_dev, second_score_dev, reinterpret_cast<ull*>(total_dev), first_dev};
    if (int rc = spread_check(fn, in, out, changed_host, iterations_host, converged_host)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (n == 0) {
        spread_empty(ctx, changed_host, iterations_host, converged_host);
        return GNN_OK;
    }
    if (int rc = spread_run(ctx, fn, in, out, changed_host, iterations_host, converged_host)) return rc;
    if (score_dev_or_null)
        GNN_HIP(hipMemcpyAsync(score_dev_or_null, ctx->sprd.F[*iterations_host & 1].get(), (size_t)n * n_classes * sizeof(uint32_t),
                               hipMemcpyDeviceToDevice, ctx->stream));
    return GNN_OK;
}

extern "C" int gnn_spread(gnn_ctx* ctx, const int64_t* indptr_host, const int32_t* col_host, const float* sim_host, const uint8_t* valid_host_or_null,
                          const int64_t* label_host, int64_t n, int64_t nnz, int n_classes, int alpha_64ths, int clamp, int max_iter,
                          uint32_t* score_host_or_null, int32_t* best_host, uint32_t* best_score_host, uint32_t* second_score_host,
                          uint64_t* total_host, int32_t* first_host, int64_t* changed_host, int64_t* iterations_host, int* converged_host) {
    const char* const fn = "gnn_spread";
    SpreadIn in = {{indptr_host, col_host, sim_host, valid_host_or_null, n, nnz}, label_host, n_classes, alpha_64ths, clamp != 0, max_iter};
    const SpreadOut host = {score_host_or_null, best_host, best_score_host, second_score_host, reinterpret_cast<ull*>(total_host), first_host};
    if (int rc = spread_check(fn, in, host, changed_host, iterations_host, converged_host)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (n == 0) {
        spread_empty(ctx, changed_host, iterations_host, converged_host);
        return GNN_OK;
    }
    SpreadWorkspace& w = ctx->sprd;
    // every buffer stands before a copy is enqueued.  d_out: [best (i32) | best_score (u32) | second_score (u32) | total (u64) | first (i32)]
    int rc = graph_reserve(ctx, w.graph, n, nnz);
    if (!rc) rc = nn_reserve(ctx, w.d_label, (size_t)n);
    Landing land(w.d_out);
    const int best = land.add(best_host, n), best_score = land.add(best_score_host, n), second_score = land.add(second_score_host, n),
              total = land.add(host.total, n), first = land.add(first_host, n);
    if (!rc) rc = land.reserve(ctx);
    if (rc) return rc;
    if ((rc = graph_upload(ctx, w.graph, in))) return rc;
    GNN_HIP(hipMemcpyAsync(w.d_label.get(), label_host, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    in.label = w.d_label.get();
    const SpreadOut dev = {nullptr, land.dev<int32_t>(best), land.dev<uint32_t>(best_score), land.dev<uint32_t>(second_score), land.dev<ull>(total),
                           land.dev<int32_t>(first)};
    if ((rc = spread_run(ctx, fn, in, dev, changed_host, iterations_host, converged_host))) return rc;
    if (score_host_or_null)                                   // straight from the buffer the last iteration wrote; copy_out synchronises
        GNN_HIP(hipMemcpyAsync(score_host_or_null, w.F[*iterations_host & 1].get(), (size_t)n * n_classes * sizeof(uint32_t), hipMemcpyDeviceToHost,
                               ctx->stream));
    return land.copy_out(ctx);
}

extern "C" int gnn_debug_spread_groups(gnn_ctx* ctx, int groups) {
    if (int rc = check_ctx(ctx)) return rc;
    if (groups < 0 || groups > 65535) {
        set_error("gnn_debug_spread_groups: " + std::to_string(groups) + " workgroups is outside [0, 65535]");
        return GNN_ERR_ARG;
    }
    ctx->sprd.groups = groups;
    return GNN_OK;
}

extern "C" int gnn_debug_spread_skip(gnn_ctx* ctx, int on) {
    if (int rc = check_ctx(ctx)) return rc;
    ctx->sprd.skip = on != 0;
    return GNN_OK;
}

extern "C" int gnn_debug_spread_ms(gnn_ctx* ctx, double* ms_out, int64_t capacity, int64_t* n_out) {
    if (int rc = check_ctx(ctx)) return rc;
    return ctx->sprd.passes.out(ctx, "gnn_debug_spread_ms", ms_out, capacity, n_out);
}
