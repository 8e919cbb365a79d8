// The keyed-sum row table of the graph consumers that contract rows (gnn_avglink.hip, gnn_communities.hip; DESIGN.md section 5u, "the
// row table"): a row's entries, keyed by a mapped column, are summed into a table, and the finished table is walked once.  Included
// behind gnn_nn_frag.h (nn_reserve, launch_1d); everything here has internal linkage.
//   row classes  by the row's upper bound u, so a table never overflows: up to wave_limit = min(wave_rows, slots / 4) one wave with its
//                quarter of the table in LDS; up to `slots` the workgroup with the whole table; beyond, the workgroup with a uint64[n]
//                accumulator in global memory and a list of the keys touched.  rt_file files a row on one of three lists by that rule,
//                rt_rows walks the lists.  Every sum is an integer add, and a policy's choices go through a total order: no output
//                depends on the class, the table's size, the entries' order or the grid.
//   table        keys int32 (RT_EMPTY: free), sums uint64: an atomicCAS on the key, a 64-bit add on the sum, linear probing from a
//                multiplicative hash.  A walk clears what it reads: the table is all free between rows.
//   policy P     what a consumer supplies, all static:
//                  Args           its kernel argument, derived from RtArgs
//                  Best           what a walk keeps: none(), take(const Best&), wave_reduce()
//                  SIDE           gather adds a sum aside (communities' w_ia), which visit receives; without it a row pays no wave sum,
//                                 no LDS atomic and no shared word for it
//                  PLACED         visit uses `pos`, the entry's place among the row's finished keys
//                  gather(a, R, me, coop, side, f)   f(key, weight), key in [0, a.m), for R's entries by `coop` workers of which this is `me`
//                  bound(a, R, at)   the row's upper bound: what it was filed by; `at`: whatever a placing policy's visit needs of the
//                                 row, read once
//                  visit(a, R, u, at, key, sum, pos, side, best)   one finished key, by the thread that walks it
//                  finish(a, R, best, count)   the row's results, by one thread
// Only integer atomics; no loop waits for another workgroup: every loop's termination argument stands next to it.  Every store is
// guarded by its bound.
#pragma once

namespace gnn {
namespace {

typedef unsigned long long ull;

constexpr int RT_SLOTS_MAX = 4096;
constexpr int RT_THREADS = 256;
constexpr int64_t RT_DENSE_CELLS = (int64_t)1 << 24;    // the accumulators' cells, all workgroups together
constexpr int RT_EMPTY = -1;

struct RtArgs {
    int64_t m, stride;         // rows; the allocation's rows (the lists' and the accumulators' stride)
    int slots, wave_limit, dense_groups;
    const int32_t* rows;       // [3][stride]: the launch's rows by class
    const ull* nrows;          // [3]
    ull* totals;               // [3]
    ull* dense;                // [dense_groups][stride], all zero between rows
    int32_t* touched;          // [dense_groups][stride]
};

__device__ __forceinline__ ull rt_wave_sum(ull v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);      // Ends: o halves towards 0
    return v;
}

// LDS traffic of one wave's lanes becomes visible to its other lanes: nothing moves across, and the wave's DS operations are done
__device__ __forceinline__ void rt_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// (key, s) into a table of T slots that holds fewer than T other keys: linear probing from a multiplicative hash
__device__ __forceinline__ void rt_insert(int32_t* keys, ull* sums, int T, int key, ull s) {
    unsigned h = (unsigned)(((ull)((unsigned)key * 2654435761u) * (ull)T) >> 32);      // < T
    for (int p = 0; p < T; ++p) {                             // Ends: p grows towards T; a free slot or the key's own is met before
        const int prev = atomicCAS(&keys[h], RT_EMPTY, key);
        if (prev == RT_EMPTY || prev == key) {
            atomicAdd(&sums[h], s);
            return;
        }
        h = h + 1 == (unsigned)T ? 0u : h + 1;
    }
}

// the table size a row of upper bound u takes of `most` >= u slots: results do not depend on it, the walk's length does
__device__ __forceinline__ int rt_table(int u, int most, int least) { return min(most, max(least, 2 * u)); }

// the workgroup's LDS: the table, the waves' bests, the finished keys' count and, for a policy with SIDE, the sum aside
template <typename P>
struct RtLds {
    int32_t* keys;             // [RT_SLOTS_MAX], all RT_EMPTY between rows
    ull* sums;                 // [RT_SLOTS_MAX], all zero between rows
    typename P::Best* red;     // [RT_THREADS / 64]
    int* cnt;                  // zero between rows
    ull* side;                 // zero between rows; NULL without SIDE
};

// R by one wave, its table the T slots at keys / sums
template <typename P>
__device__ __forceinline__ void rt_row_wave(const typename P::Args& a, int R, int32_t* keys, ull* sums, int slice) {
    const int lane = threadIdx.x & 63;
    int64_t at = 0;
    const int u = P::bound(a, R, at);
    if (u < 1 || u > slice) return;                           // never: the row was filed by its bound
    const int T = rt_table(u, slice, 64);
    ull side = 0;
    P::gather(a, R, lane, 64, side, [&](int key, ull s) { rt_insert(keys, sums, T, key, s); });
    if constexpr (P::SIDE) side = rt_wave_sum(side);
    rt_wave_sync();
    typename P::Best b = P::Best::none();
    int count = 0;
    for (int s0 = 0; s0 < T; s0 += 64) {                      // Ends: s0 grows towards T; uniform in the wave
        const int s = s0 + lane;
        const int key = s < T ? keys[s] : RT_EMPTY;
        const ull full = __ballot(key != RT_EMPTY);
        if (key != RT_EMPTY) {
            const ull S = sums[s];
            keys[s] = RT_EMPTY;
            sums[s] = 0;
            P::visit(a, R, u, at, key, S, count + __popcll(full & ((1ull << lane) - 1ull)), side, b);
        }
        count += __popcll(full);
    }
    rt_wave_sync();                                           // the slots are clear for the wave's next row
    b.wave_reduce();
    if (lane == 0) P::finish(a, R, b, min(count, u));
}

// the workgroup's best of its threads', in thread 0
template <typename B>
__device__ __forceinline__ void rt_block_reduce(B& b, B* red) {
    b.wave_reduce();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < RT_THREADS / 64; ++w) b.take(red[w]);      // Ends: w grows towards 4
}

// what ends a workgroup's row: thread 0 writes the results and clears the words of the row
template <typename P>
__device__ __forceinline__ void rt_row_end(const typename P::Args& a, int R, const typename P::Best& b, int count, const RtLds<P>& l) {
    if (threadIdx.x == 0) {
        P::finish(a, R, b, count);
        *l.cnt = 0;
        if constexpr (P::SIDE) *l.side = 0;
    }
    __syncthreads();
}

// R by the whole workgroup (every thread calls it), its table the first T of the `slots`
template <typename P>
__device__ __forceinline__ void rt_row_block(const typename P::Args& a, int R, const RtLds<P>& l) {
    const int tid = threadIdx.x;
    int64_t at = 0;
    const int u = P::bound(a, R, at);
    if (u < 1 || u > a.slots) return;                         // never; uniform
    const int T = rt_table(u, a.slots, RT_THREADS);
    ull side = 0;
    P::gather(a, R, tid, RT_THREADS, side, [&](int key, ull s) { rt_insert(l.keys, l.sums, T, key, s); });
    if constexpr (P::SIDE)
        if (side) atomicAdd(l.side, side);
    __syncthreads();
    if constexpr (P::SIDE) side = *l.side;
    typename P::Best b = P::Best::none();
    for (int s = tid; s < T; s += RT_THREADS) {               // Ends: s grows towards T
        const int key = l.keys[s];
        if (key == RT_EMPTY) continue;
        const ull S = l.sums[s];
        l.keys[s] = RT_EMPTY;
        l.sums[s] = 0;
        P::visit(a, R, u, at, key, S, P::PLACED ? atomicAdd(l.cnt, 1) : 0, side, b);
    }
    rt_block_reduce(b, l.red);                                // its barrier: every add to cnt and every read of side is done
    rt_row_end<P>(a, R, b, min(*l.cnt, u), l);
}

// R by the whole workgroup with its accumulator in global memory: a key's first add finds 0 there (every weight is > 0)
template <typename P>
__device__ __forceinline__ void rt_row_dense(const typename P::Args& a, int R, const RtLds<P>& l) {
    const int tid = threadIdx.x;
    ull* const dense = a.dense + (int64_t)blockIdx.x * a.stride;
    int32_t* const touched = a.touched + (int64_t)blockIdx.x * a.stride;
    int64_t at = 0;
    const int u = P::bound(a, R, at);
    if (u < 1) return;                                        // never; uniform
    ull side = 0;
    P::gather(a, R, tid, RT_THREADS, side, [&](int key, ull s) {
        const ull old = atomicAdd(dense + key, s);            // key < m <= stride: gather
        if (old == 0) {
            const int at = atomicAdd(l.cnt, 1);
            if (at < a.m) touched[at] = key;                  // always: at most m keys
        }
    });
    if constexpr (P::SIDE)
        if (side) atomicAdd(l.side, side);
    __syncthreads();
    if constexpr (P::SIDE) side = *l.side;
    const int n_keys = (int)min<int64_t>(min(*l.cnt, u), a.m);
    typename P::Best b = P::Best::none();
    for (int p = tid; p < n_keys; p += RT_THREADS) {          // Ends: p grows towards n_keys
        const int key = touched[p];
        if ((unsigned)key >= (ull)a.m) continue;              // never
        // written by atomics of this workgroup: the load goes where they went
        const ull S = __hip_atomic_load(dense + key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(dense + key, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        P::visit(a, R, u, at, key, S, p, side, b);                // p < n_keys <= u
    }
    rt_block_reduce(b, l.red);
    rt_row_end<P>(a, R, b, n_keys, l);
}

// The body of a kernel of grid = the groups, RT_THREADS threads: the first dense_groups workgroups take the dense rows g, g +
// dense_groups, ..., then every workgroup the workgroup rows g, g + groups, ..., then its waves the wave rows w, w + 4 * groups, ...
template <typename P>
__device__ __forceinline__ void rt_rows(const typename P::Args& a) {
    __shared__ int32_t keys[RT_SLOTS_MAX];
    __shared__ ull sums[RT_SLOTS_MAX];
    __shared__ typename P::Best red[RT_THREADS / 64];
    __shared__ int cnt;
    __shared__ ull side;                                      // referenced with SIDE only
    const int tid = threadIdx.x, wave = tid >> 6;
    RtLds<P> l = {keys, sums, red, &cnt, nullptr};
    if constexpr (P::SIDE) l.side = &side;
    for (int s = tid; s < RT_SLOTS_MAX; s += RT_THREADS) {    // Ends: s grows towards RT_SLOTS_MAX
        keys[s] = RT_EMPTY;
        sums[s] = 0;
    }
    if (tid == 0) {
        cnt = 0;
        if constexpr (P::SIDE) side = 0;
    }
    __syncthreads();
    const int64_t nwave = (int64_t)min(a.nrows[0], (ull)a.m), nblock = (int64_t)min(a.nrows[1], (ull)a.m),
                  ndense = (int64_t)min(a.nrows[2], (ull)a.m);
    if (blockIdx.x == 0 && tid < 3) a.totals[tid] += a.nrows[tid];
    if ((int)blockIdx.x < a.dense_groups)
        for (int64_t w = blockIdx.x; w < ndense; w += a.dense_groups) {      // Ends: w grows towards ndense
            const int R = a.rows[2 * a.stride + w];
            if ((unsigned)R < (ull)a.m) rt_row_dense<P>(a, R, l);            // always; uniform: w is the workgroup's
        }
    for (int64_t w = blockIdx.x; w < nblock; w += gridDim.x) {               // Ends: w grows towards nblock
        const int R = a.rows[a.stride + w];
        if ((unsigned)R < (ull)a.m) rt_row_block<P>(a, R, l);                // always; uniform
    }
    const int slice = a.slots / 4;                            // a wave's quarter of the table
    for (int64_t w = (int64_t)blockIdx.x * 4 + wave; w < nwave; w += (int64_t)gridDim.x * 4) {      // Ends: w grows towards nwave
        const int R = a.rows[w];
        if ((unsigned)R < (ull)a.m) rt_row_wave<P>(a, R, keys + wave * slice, sums + wave * slice, slice);      // always; no barrier here
    }
}

// The class of row i of upper bound u (-1: it has no entries) filed on its list, by every thread of the wave
__device__ __forceinline__ void rt_file(int64_t stride, int i, int u, int slots, int wave_limit, int32_t* rows, ull* nrows) {
    const int lane = threadIdx.x & 63;
    const ull below = (1ull << lane) - 1ull;
    const int cls = u < 1 ? -1 : (u <= wave_limit ? 0 : (u <= slots ? 1 : 2));
    for (int k = 0; k < 3; ++k) {                             // Ends: three classes
        const ull mask = __ballot(cls == k);
        if (!mask) continue;                                  // uniform
        const int leader = __ffsll((long long)mask) - 1;
        ull base = 0;
        if (lane == leader) base = atomicAdd(nrows + k, (ull)__popcll(mask));
        base = __shfl(base, leader);
        const ull at = base + (ull)__popcll(mask & below);
        if (cls == k && at < (ull)stride) rows[(int64_t)k * stride + (int64_t)at] = i;      // always: a row is filed once
    }
}

// the symmetric graph's weights (gnn_csr_sym.h) as the sums of entry buffer 0
__global__ __launch_bounds__(256) void rt_widen_kernel(int64_t cells, const int64_t* __restrict__ soff, int64_t n, const uint32_t* __restrict__ sq,
                                                       ull* __restrict__ sum) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x < cells && x < soff[n]) sum[x] = sq[x];
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

struct RtPlan {
    int wave_limit, groups, dense_groups;
};

// What a run settles before its first launch, for n > 0 rows: the class limit, the grid, and the lists and accumulators standing, the
// accumulators zeroed on the ctx's stream
inline int rt_plan(gnn_ctx* ctx, int64_t n, RowTable& t, RtPlan& p) {
    p.wave_limit = std::min(t.wave_rows, t.slots / 4);
    p.groups = t.groups > 0 ? t.groups : (int)std::min<int64_t>((n + 3) / 4, 8 * (int64_t)std::max(ctx->cu_count, 1));
    p.dense_groups = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(p.groups, 64), RT_DENSE_CELLS / n));
    int rc = nn_reserve(ctx, t.rows, (size_t)3 * n);
    if (!rc) rc = nn_reserve(ctx, t.dense, (size_t)p.dense_groups * n);
    if (!rc) rc = nn_reserve(ctx, t.touched, (size_t)p.dense_groups * n);
    if (rc) return rc;
    GNN_HIP(hipMemsetAsync(t.dense.get(), 0, (size_t)p.dense_groups * n * sizeof(ull), ctx->stream));
    return GNN_OK;
}

// the body of the debug knobs `slots` and `wave_rows`, which return the value before the call; knob: NULL with ctx
inline int rt_knob(gnn_ctx* ctx, const char* fn, int* knob, int value) {
    if (int rc = check_ctx(ctx)) return rc;
    if (value < -1 || value > RT_SLOTS_MAX) {
        set_error(std::string(fn) + ": " + std::to_string(value) + " is outside [-1, " + std::to_string(RT_SLOTS_MAX) + "]");
        return GNN_ERR_ARG;
    }
    const int before = *knob;
    if (value >= 0) *knob = value;
    return before;
}

// the body of the debug setter `groups`; knob: NULL with ctx
inline int rt_set_groups(gnn_ctx* ctx, const char* fn, int* knob, int groups) {
    if (int rc = check_ctx(ctx)) return rc;
    if (groups < 0 || groups > 65535) {
        set_error(std::string(fn) + ": " + std::to_string(groups) + " workgroups is outside [0, 65535]");
        return GNN_ERR_ARG;
    }
    *knob = groups;
    return GNN_OK;
}

}  // namespace
}  // namespace gnn
