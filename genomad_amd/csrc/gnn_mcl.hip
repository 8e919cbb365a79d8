// Markov clustering of a similarity graph (include/genomad_nn.h, "Markov clusters"): van Dongen's MCL in integers
// throughout - the definition is sequence.markov_clusters, and every output here equals it bit for bit.  ONE = 2^30 is a column's flow,
// W = 2^24 a similarity of 1.  The matrix has a fixed width of `select` entries per column (idx int32, val uint32, rows ascending) and a
// length per column, and is double buffered.
//   validate, symmetrise   gnn_csr_sym.h, shared with the other consumers of the graph.  A row's entries stand in arrival order:
//                nothing downstream depends on it - the table is keyed by row index, and prune has a strict order.
//   initial      mc_lds_kernel<true>: column j = prune(its edges' weights - of parallel edges the largest - and its loop).
//   iteration    mc_lds_kernel<false>, one launch per iteration: workgroups loop over columns.  The products p_ik * p_kj of column j
//                are added into an LDS table keyed by i: open addressing, the slot claimed by a compare-and-swap, the value a 64-bit
//                integer add - exact, in any order.  A column whose rows do not fit the table is pushed on the overflow list and left
//                alone; mc_dense_kernel finishes those with one uint64[n] accumulator per workgroup in global memory (integer atomics,
//                a list of the rows touched, cleared by that list).  Both run mc_finish on what they gathered: t = e >> 30, u = t * ONE
//                / max t, y = pow(u) (products, an integer square root and fourth root: floor operations only), the cutoff y *
//                precision >= sum y, a radix select of the `select` largest (y, -i) on integer keys, p = y * ONE / sum, a bitonic sort
//                by row, the comparison with the column's predecessor and one add to the iteration's `changed` counter.  The host
//                reads that counter, 8 bytes, once per iteration.
//   interpret    every (i, j) of the final matrix joins i and j in gnn_nn_frag.h's union-find (a link points to the smaller index: a
//                tree's root is its smallest member); label, size, attractor, flow and is_attractor follow per row.
// No float is compared or added anywhere; the one float operation is the estimate of the integer square root, corrected by integer
// comparisons.  No float atomics, no inline assembly, no loop that waits for another workgroup: every loop's termination argument
// stands next to it.  Every store into the matrix, the tables and the lists is guarded by its bound.
#include <cmath>

#include "gnn_nn_frag.h"
#include "gnn_csr_sym.h"

namespace gnn {
namespace {

typedef unsigned long long ull;

constexpr int SELECT_MAX = 1024;                 // the sort buffer
constexpr int PRECISION_MAX = 1 << 20;
constexpr int MAX_ITER_MAX = 10000;
constexpr int LDS_SLOTS = 4096;                  // the table: 16 KB of keys + 32 KB of sums - two workgroups per CU
constexpr ull ONE = 1ull << 30;
constexpr double W = CSR_W;                      // 2^24
constexpr int THREADS = 256;

struct MclArgs {
    int64_t n;
    int select, precision, a4, slots;
    const int32_t* olen;       // the previous matrix (iteration)
    const int32_t* oidx;
    const uint32_t* oval;
    int32_t* nlen;             // the matrix written
    int32_t* nidx;
    uint32_t* nval;
    const int64_t* soff;       // the symmetric graph (initial): [n + 1]
    const int32_t* sidx;
    const uint32_t* sq;
    const uint8_t* ok;         // [n]
    ull* changed;              // the iteration's counter
    ull* ovf_count;            // columns on the overflow list
    int32_t* ovf_list;         // [n]
    ull* dense;                // mc_dense_kernel: [gridDim.x][n], all zero between columns
    int32_t* touched;          // [gridDim.x][n]
};

// what mc_finish works with besides the table, all in LDS
struct Scratch {
    ull* red;                  // [4]
    int* hist;                 // [256]
    ull* sort;                 // [SELECT_MAX]
    int* cnt;                  // [2]: entries in sort; the selection's remaining rank
    ull* prefix;               // the selection's key so far
};

// Sums and maxima over the workgroup; every thread calls them.  The first barrier keeps red[] from a reader of the call before.
__device__ __forceinline__ ull blk_sum(ull v, ull* red) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}
__device__ __forceinline__ ull blk_max(ull v, ull* red) {
    for (int o = 32; o; o >>= 1) {
        const ull w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const ull a = red[0] > red[1] ? red[0] : red[1], b = red[2] > red[3] ? red[2] : red[3];
    return a > b ? a : b;
}

// floor(sqrt(x)), x <= 2^60: the float64 estimate is off by one at the most, integer comparisons correct it.  Ends: each loop moves r
// towards the root and stops there.
__device__ __forceinline__ ull mc_isqrt(ull x) {
    ull r = (ull)sqrt((double)x);
    while (r * r > x) --r;
    while ((r + 1) * (r + 1) <= x) ++r;
    return r;
}

// u^(a4 / 4) in 2^-30 fixed point, u <= ONE: every product floored
__device__ __forceinline__ ull mc_pow(ull u, int a4) {
    const ull h = mc_isqrt(u * ONE), g = mc_isqrt(h * ONE);
    ull r = ONE;
    for (int k = 0; k < (a4 >> 2); ++k) r = (r * u) >> 30;      // Ends: k grows to a4 / 4 <= 8
    if ((a4 & 3) >= 2) r = (r * h) >> 30;
    if (a4 & 1) r = (r * g) >> 30;
    return r;
}

// gnn_debug_mcl_pow: the passes' own power, one value per thread
__global__ __launch_bounds__(256) void mc_pow_kernel(int64_t n, int a4, const ull* __restrict__ u, ull* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = mc_pow(u[i], a4);
}

// The LDS table as mc_finish reads it: position p is a slot, idx < 0 an empty one.
struct LdsTab {
    int* key;
    ull* val;
    int P;
    __device__ __forceinline__ int idx(int p) const { return key[p]; }
    __device__ __forceinline__ ull get(int p) const { return val[p]; }
    __device__ __forceinline__ void set(int p, ull v) const { val[p] = v; }
};

// The dense accumulator: position p is the p-th row touched.  Its values were written by atomics of this workgroup: the loads go
// where those went.
struct DenseTab {
    const int32_t* touched;
    ull* dense;
    int P;
    __device__ __forceinline__ int idx(int p) const { return touched[p]; }
    __device__ __forceinline__ ull get(int p) const { return __hip_atomic_load(dense + touched[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ void set(int p, ull v) const {
        __hip_atomic_store(dense + touched[p], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// Row i gets v in the LDS table of `slots` slots: added (MAX false) or as a maximum (MAX true).  false: no slot is left for it.
// Ends: probe grows to slots.  A slot's key changes once, from -1, by the compare-and-swap; the load may be older than that, never wrong.
template <bool MAX>
__device__ __forceinline__ bool lds_insert(int* key, ull* val, int slots, int i, ull v) {
    if (slots <= 0) return false;
    unsigned h = ((unsigned)i * 2654435761u) % (unsigned)slots;
    for (int probe = 0; probe < slots; ++probe) {
        int k = __hip_atomic_load(key + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (k == -1) k = atomicCAS(key + h, -1, i);
        if (k == -1 || k == i) {
            if (MAX) atomicMax(val + h, v); else atomicAdd(val + h, v);
            return true;
        }
        h = h + 1 == (unsigned)slots ? 0 : h + 1;
    }
    return false;
}

// Column j from what the table holds - iteration: the sums e; INIT: the weights y - to the matrix a.n*, compared with a.o* (iteration).
// Every thread of the workgroup calls it; thread t owns the positions t, t + 256, ... in every pass.
template <bool INIT, class Tab>
__device__ void mc_finish(const MclArgs& a, const Tab& tab, int64_t j, const Scratch& s) {
    const int tid = threadIdx.x;
    // every loop over p below ends: p grows by 256 towards tab.P
    if (!INIT) {
        ull mx = 0;
        for (int p = tid; p < tab.P; p += THREADS)
            if (tab.idx(p) >= 0) {
                const ull t = tab.get(p) >> 30;
                tab.set(p, t);
                mx = t > mx ? t : mx;
            }
        const ull m = blk_max(mx, s.red);
        if (m)
            for (int p = tid; p < tab.P; p += THREADS)
                if (tab.idx(p) >= 0) {
                    const ull t = tab.get(p);
                    if (t) tab.set(p, mc_pow(t * ONE / m, a.a4));
                }
    }
    // ---- prune: the cutoff
    ull part = 0;
    for (int p = tid; p < tab.P; p += THREADS)
        if (tab.idx(p) >= 0) part += tab.get(p);
    const ull S = blk_sum(part, s.red);
    part = 0;
    for (int p = tid; p < tab.P; p += THREADS)
        if (tab.idx(p) >= 0) {
            const ull y = tab.get(p);
            if (!y) continue;
            if (y * (ull)a.precision >= S) ++part; else tab.set(p, 0);
        }
    const ull kept = blk_sum(part, s.red);
    // ---- the `select` largest under (y descending, i ascending): the keys (y << 24) | (2^24 - 1 - i) are distinct and below 2^55; the
    // select-th largest of them is found digit by digit, 8 bits at a time from the top
    if (kept > (ull)a.select) {
        if (tid == 0) {
            *s.prefix = 0;
            s.cnt[1] = a.select;
        }
        for (int d = 6; d >= 0; --d) {                        // Ends: d falls to 0
            s.hist[tid] = 0;
            __syncthreads();
            const ull pre = *s.prefix;
            for (int p = tid; p < tab.P; p += THREADS) {
                const int i = tab.idx(p);
                if (i < 0) continue;
                const ull y = tab.get(p);
                if (!y) continue;
                const ull key = (y << 24) | (ull)(0xffffff - i);
                if ((key >> (8 * d) >> 8) == pre) atomicAdd(s.hist + (int)((key >> (8 * d)) & 255), 1);
            }
            __syncthreads();
            if (tid == 0) {
                int rem = s.cnt[1], digit = 255;
                for (; digit > 0; --digit) {                  // Ends: digit falls to 0
                    if (s.hist[digit] >= rem) break;
                    rem -= s.hist[digit];
                }
                *s.prefix = (pre << 8) | (ull)digit;
                s.cnt[1] = rem;
            }
            __syncthreads();
        }
        const ull last = *s.prefix;
        for (int p = tid; p < tab.P; p += THREADS) {
            const int i = tab.idx(p);
            if (i < 0) continue;
            const ull y = tab.get(p);
            if (y && ((y << 24) | (ull)(0xffffff - i)) < last) tab.set(p, 0);
        }
    }
    // ---- p = y * ONE / S', zeros dropped, into the sort buffer
    part = 0;
    for (int p = tid; p < tab.P; p += THREADS)
        if (tab.idx(p) >= 0) part += tab.get(p);
    const ull S2 = blk_sum(part, s.red);
    if (tid == 0) s.cnt[0] = 0;
    __syncthreads();
    if (S2)
        for (int p = tid; p < tab.P; p += THREADS) {
            const int i = tab.idx(p);
            if (i < 0) continue;
            const ull y = tab.get(p);
            if (!y) continue;
            const ull pv = y * ONE / S2;                      // the one division per survivor
            if (!pv) continue;
            const int at = atomicAdd(s.cnt, 1);
            if (at < SELECT_MAX) s.sort[at] = ((ull)(unsigned)i << 32) | pv;     // always: at most `select` survive
        }
    __syncthreads();
    const int c = min(min(s.cnt[0], SELECT_MAX), a.select);
    int n2 = 1;
    while (n2 < c) n2 <<= 1;                                  // Ends: n2 doubles towards c <= 1024
    for (int p = c + tid; p < n2; p += THREADS) s.sort[p] = ~0ull;
    __syncthreads();
    // ---- ascending by row: a bitonic sort of n2 keys.  Ends: k doubles towards n2, h halves towards 0
    for (int k = 2; k <= n2; k <<= 1)
        for (int h = k >> 1; h > 0; h >>= 1) {
            for (int t = tid; t < n2; t += THREADS) {
                const int o = t ^ h;
                if (o > t) {
                    const ull x = s.sort[t], y = s.sort[o];
                    if ((x > y) == ((t & k) == 0)) {
                        s.sort[t] = y;
                        s.sort[o] = x;
                    }
                }
            }
            __syncthreads();
        }
    // ---- the column, and whether it differs from its predecessor
    const int olen = INIT ? 0 : a.olen[j];
    bool ch = !INIT && olen != c;
    const int64_t at0 = j * a.select;
    for (int r = tid; r < c; r += THREADS) {                  // c <= select: no store leaves the column
        const int i = (int)(s.sort[r] >> 32);
        const uint32_t pv = (uint32_t)s.sort[r];
        a.nidx[at0 + r] = i;
        a.nval[at0 + r] = pv;
        if (!INIT && r < olen && (a.oidx[at0 + r] != i || a.oval[at0 + r] != pv)) ch = true;
    }
    const int any = __syncthreads_or(ch);
    if (tid == 0) {
        a.nlen[j] = c;
        if (!INIT && any) atomicAdd(a.changed, 1ull);
    }
}

// The entries that column j is made from, handed to put(i, v): INIT - its edges' weights; iteration - the products p_ik * p_kj, wave
// w taking the sources k = w, w + 4, ... of the old column j and its lanes the entries of column k.
template <bool INIT, class Put>
__device__ __forceinline__ void mc_gather(const MclArgs& a, int64_t j, Put&& put) {
    const int tid = threadIdx.x;
    if (INIT) {
        const int64_t b = a.soff[j], e = a.soff[j + 1];
        for (int64_t x = b + tid; x < e; x += THREADS) put(a.sidx[x], (ull)a.sq[x]);           // Ends: x grows towards e
    } else {
        const int lane = tid & 63, wave = tid >> 6, len = min(a.olen[j], a.select);
        for (int sidx = wave; sidx < len; sidx += 4) {                                           // Ends: sidx grows towards len
            const int k = a.oidx[j * a.select + sidx];
            const ull pkj = a.oval[j * a.select + sidx];
            const int lk = min(a.olen[k], a.select);
            for (int x = lane; x < lk; x += 64)                                                  // Ends: x grows towards lk
                put(a.oidx[(int64_t)k * a.select + x], (ull)a.oval[(int64_t)k * a.select + x] * pkj);
        }
    }
}

// an upper bound of the rows column j gathers: the table is sized by it, so that a short column costs a short table
template <bool INIT>
__device__ __forceinline__ int64_t mc_bound(const MclArgs& a, int64_t j, ull* red) {
    ull part = 0;
    if (INIT) {
        part = threadIdx.x == 0 ? (ull)(a.soff[j + 1] - a.soff[j]) + 1 : 0;
    } else {
        const int len = min(a.olen[j], a.select);
        for (int x = threadIdx.x; x < len; x += THREADS) part += (ull)min(a.olen[a.oidx[j * a.select + x]], a.select);      // Ends: x grows towards len
    }
    return (int64_t)blk_sum(part, red);
}

// INIT: the loop of node j joins its column - the largest weight there, W without one
template <class Tab>
__device__ __forceinline__ ull mc_loop_weight(const Tab& tab, ull* red) {
    ull mx = 0;
    for (int p = threadIdx.x; p < tab.P; p += THREADS)        // Ends: p grows towards tab.P
        if (tab.idx(p) >= 0) {
            const ull y = tab.get(p);
            mx = y > mx ? y : mx;
        }
    const ull m = blk_max(mx, red);
    return m ? m : (ull)W;
}

#define MC_SCRATCH()                         \
    __shared__ ull s_red[4];                 \
    __shared__ int s_hist[256];              \
    __shared__ ull s_sort[SELECT_MAX];       \
    __shared__ int s_cnt[2];                 \
    __shared__ ull s_prefix;                 \
    const Scratch s = {s_red, s_hist, s_sort, s_cnt, &s_prefix}

// grid = the groups, 256 threads; workgroup g takes the columns g, g + groups, ...  LDS: the table 48 KB, the sort buffer 8 KB.
template <bool INIT>
__global__ __launch_bounds__(THREADS) void mc_lds_kernel(MclArgs a) {
    __shared__ int key[LDS_SLOTS];
    __shared__ ull val[LDS_SLOTS];
    __shared__ int over;
    MC_SCRATCH();
    const int tid = threadIdx.x;
    const int slots = min(a.slots, LDS_SLOTS);
    for (int p = tid; p < slots; p += THREADS) {              // Ends: p grows towards slots
        key[p] = -1;
        val[p] = 0;
    }
    if (tid == 0) over = 0;
    __syncthreads();
    for (int64_t j = blockIdx.x; j < a.n; j += gridDim.x) {   // Ends: j grows towards n
        if (INIT ? !a.ok[j] : a.olen[j] == 0) {               // an empty column stays empty (uniform: j is the workgroup's)
            if (tid == 0) a.nlen[j] = 0;
            continue;
        }
        // the table of this column: twice its bound, at least 64 slots, at most all.  No result depends on its size
        const int64_t bound = mc_bound<INIT>(a, j, s_red);
        const int used = (int)min<int64_t>(slots, max<int64_t>(64, 2 * bound));
        mc_gather<INIT>(a, j, [&](int i, ull v) {
            if (!lds_insert<INIT>(key, val, used, i, v)) over = 1;
        });
        __syncthreads();
        const LdsTab tab = {key, val, used};
        if (INIT && !over) {
            const ull loop = mc_loop_weight(tab, s_red);
            if (tid == 0 && !lds_insert<true>(key, val, used, (int)j, loop)) over = 1;
            __syncthreads();
        }
        if (over) {                                           // uniform: read behind a barrier
            if (tid == 0) {
                const ull at = atomicAdd(a.ovf_count, 1ull);
                if (at < (ull)a.n) a.ovf_list[at] = (int32_t)j;          // always: a column is pushed once
            }
        } else {
            mc_finish<INIT>(a, tab, j, s);
        }
        __syncthreads();
        for (int p = tid; p < used; p += THREADS) {           // Ends: p grows towards used
            key[p] = -1;
            val[p] = 0;
        }
        if (tid == 0) over = 0;
        __syncthreads();
    }
}

// The columns of the overflow list, with one dense accumulator per workgroup: a.dense + g * n is all zero here and when the kernel ends.
template <bool INIT>
__global__ __launch_bounds__(THREADS) void mc_dense_kernel(MclArgs a) {
    __shared__ int tcount;
    MC_SCRATCH();
    const int tid = threadIdx.x;
    ull* const dense = a.dense + (int64_t)blockIdx.x * a.n;
    int32_t* const touched = a.touched + (int64_t)blockIdx.x * a.n;
    const int64_t total = (int64_t)min<ull>(*a.ovf_count, (ull)a.n);
    if (tid == 0) tcount = 0;
    __syncthreads();
    for (int64_t w = blockIdx.x; w < total; w += gridDim.x) { // Ends: w grows towards total
        const int64_t j = a.ovf_list[w];
        // a row's first add finds 0 there (every value added is > 0): that thread files the row.  At most n rows: at < n always
        mc_gather<INIT>(a, j, [&](int i, ull v) {
            if ((unsigned)i >= (ull)a.n) return;              // never: the matrix and the graph hold rows below n
            const ull old = INIT ? atomicMax(dense + i, v) : atomicAdd(dense + i, v);
            if (old == 0) {
                const int at = atomicAdd(&tcount, 1);
                if (at < a.n) touched[at] = i;
            }
        });
        __syncthreads();
        if (INIT) {
            const DenseTab tab = {touched, dense, (int)min<int64_t>(tcount, a.n)};
            const ull loop = mc_loop_weight(tab, s_red);
            if (tid == 0) {                                   // j is not among its own partners: the slot is 0
                __hip_atomic_store(dense + j, loop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const int at = atomicAdd(&tcount, 1);
                if (at < a.n) touched[at] = (int32_t)j;
            }
            __syncthreads();
        }
        const DenseTab tab = {touched, dense, (int)min<int64_t>(tcount, a.n)};
        mc_finish<INIT>(a, tab, j, s);
        __syncthreads();
        for (int p = tid; p < tab.P; p += THREADS) tab.set(p, 0);        // Ends: p grows towards tab.P
        if (tid == 0) tcount = 0;
        __syncthreads();
    }
}

// ---- interpret -----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void mc_parent_kernel(int64_t n, int32_t* __restrict__ parent, int32_t* __restrict__ size) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    parent[i] = (int32_t)i;
    size[i] = 0;
}

// one thread per column: every entry (i, j) joins i and j
__global__ __launch_bounds__(256) void mc_link_kernel(int64_t n, int select, const int32_t* __restrict__ len, const int32_t* __restrict__ idx,
                                                      int32_t* __restrict__ parent) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int l = min(len[j], select);
    int top = (int)j;
    for (int r = 0; r < l; ++r) {                             // Ends: r grows towards l
        const int i = idx[j * select + r];
        if (i >= 0 && i < n && i != j) top = cl_join(parent, i, top);
    }
}

// a launch of its own behind the links: nn_root's plain loads see every one
__global__ __launch_bounds__(256) void mc_flatten_kernel(int64_t n, const uint8_t* __restrict__ ok, const int32_t* __restrict__ parent,
                                                         int32_t* __restrict__ size, int64_t* __restrict__ label) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (!ok[i]) {
        label[i] = -1;
        return;
    }
    const int r = nn_root(parent, (int)i);
    label[i] = r;
    atomicAdd(size + r, 1);
}

__global__ __launch_bounds__(256) void mc_summarise_kernel(int64_t n, int select, const uint8_t* __restrict__ ok, const int32_t* __restrict__ len,
                                                           const int32_t* __restrict__ idx, const uint32_t* __restrict__ val,
                                                           const int32_t* __restrict__ size, const int64_t* __restrict__ label,
                                                           int64_t* __restrict__ size_out, int64_t* __restrict__ attractor,
                                                           uint32_t* __restrict__ flow, uint8_t* __restrict__ is_attractor) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    int64_t best = -1;
    uint32_t top = 0;
    bool self = false;
    const int l = ok[j] ? min(len[j], select) : 0;
    for (int r = 0; r < l; ++r) {                             // Ends: r grows towards l.  Rows ascend: the first maximum is the smallest row
        const int i = idx[j * select + r];
        const uint32_t p = val[j * select + r];
        if (p > top) {
            top = p;
            best = i;
        }
        self |= i == j && p > 0;
    }
    size_out[j] = ok[j] ? size[label[j]] : 0;
    attractor[j] = best;
    flow[j] = top;
    is_attractor[j] = self;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

struct MclIn : CsrGraph {       // the graph on the device
    int a4, select, precision, max_iter;
};

int check_mcl_args(const std::string& f, int64_t n, int64_t nnz, int a4, int select, int precision, int max_iter) {
    const auto bad = [&](const char* what, int64_t v, const char* range) {
        set_error(f + ": " + what + " " + std::to_string(v) + " is outside " + range);
        return GNN_ERR_ARG;
    };
    if (int rc = graph_check(f, n, nnz)) return rc;
    if (a4 < 5 || a4 > 32) return bad("inflation_quarters", a4, "[5, 32]: the inflation is a multiple of 0.25 in [1.25, 8]");
    if (select < 1 || select > SELECT_MAX) return bad("select", select, "[1, 1024]");
    if (precision < 1 || precision > PRECISION_MAX) return bad("precision", precision, "[1, 2^20]");
    if (max_iter < 0 || max_iter > MAX_ITER_MAX) return bad("max_iter", max_iter, "[0, 10000]");
    return GNN_OK;
}

int mcl_groups(const gnn_ctx* ctx) {
    return ctx->mcl.groups > 0 ? ctx->mcl.groups : 2 * std::max(ctx->cu_count, 1);
}

// n > 0 rows: the graph on the device -> the five arrays on the device and iterations, converged, changed on the host.  The ctx's
// stream is synchronised once for the verdict on the graph and once per iteration.
int mcl_run(gnn_ctx* ctx, const char* fn, const MclIn& in, int64_t* label, int64_t* size, int64_t* attractor, uint32_t* flow,
            uint8_t* is_attractor, int64_t* changed_host, int64_t* iterations_host, int* converged_host) {
    MclWorkspace& m = ctx->mcl;
    m.have = false;
    m.passes.begin();
    m.overflow.clear();
    const int64_t n = in.n;
    const int groups = mcl_groups(ctx);
    const int dense_groups = (int)std::max<int64_t>(1, std::min<int64_t>(groups, ((int64_t)1 << 27) / n));
    const size_t cells = (size_t)n * in.select;
    int rc = nn_reserve(ctx, m.ok, (size_t)n);
    const size_t flag = (size_t)2 * (in.max_iter + 1);       // the graph's flag stands behind the passes' counters
    if (!rc) rc = m.count.reserve(ctx, flag + 1);
    if (!rc) rc = m.count.zero(ctx, 0, flag + 1);
    if (rc) return rc;
    {
        PassLog::Scope setup(ctx, m.passes);                  // open across the read below: nothing is settled there
        if ((rc = graph_validate(ctx, fn, in, m.ok.get(), m.count, flag))) return rc;
        for (int b = 0; b < 2 && !rc; ++b) {
            rc = nn_reserve(ctx, m.len[b], (size_t)n);
            if (!rc) rc = nn_reserve(ctx, m.idx[b], cells);
            if (!rc) rc = nn_reserve(ctx, m.val[b], cells);
        }
        if (!rc) rc = nn_reserve(ctx, m.deg, (size_t)n);
        if (!rc) rc = nn_reserve(ctx, m.soff, (size_t)n + 1);
        if (!rc) rc = nn_reserve(ctx, m.cursor, (size_t)n);
        if (!rc) rc = nn_reserve(ctx, m.sidx, (size_t)std::max<int64_t>(2 * in.nnz, 1));
        if (!rc) rc = nn_reserve(ctx, m.sq, (size_t)std::max<int64_t>(2 * in.nnz, 1));
        if (!rc) rc = nn_reserve(ctx, m.ovf_list, (size_t)n);
        if (!rc) rc = nn_reserve(ctx, m.dense, (size_t)dense_groups * n);
        if (!rc) rc = nn_reserve(ctx, m.touched, (size_t)dense_groups * n);
        if (!rc) rc = nn_reserve(ctx, m.parent, (size_t)n);
        if (!rc) rc = nn_reserve(ctx, m.size, (size_t)n);
        if (rc) return rc;
        GNN_HIP(hipMemsetAsync(m.dense.get(), 0, (size_t)dense_groups * n * sizeof(ull), ctx->stream));
        if ((rc = csr_symmetrise(ctx->stream, n, in.indptr, in.col, in.sim, m.ok.get(), m.deg.get(), m.soff.get(), m.cursor.get(), m.sidx.get(),
                                 m.sq.get())))
            return rc;
    }
    MclArgs a;
    a.n = n;
    a.select = in.select;
    a.precision = in.precision;
    a.a4 = in.a4;
    a.slots = m.lds_slots;
    a.soff = m.soff.get();
    a.sidx = m.sidx.get();
    a.sq = m.sq.get();
    a.ok = m.ok.get();
    a.ovf_list = m.ovf_list.get();
    a.dense = m.dense.get();
    a.touched = m.touched.get();
    // pass it = 0: the initial matrix into buffer 0; pass it >= 1: iteration it, from buffer (it - 1) & 1 into buffer it & 1
    const auto pass = [&](int it) -> int {
        a.olen = it ? m.len[(it - 1) & 1].get() : nullptr;
        a.oidx = it ? m.idx[(it - 1) & 1].get() : nullptr;
        a.oval = it ? m.val[(it - 1) & 1].get() : nullptr;
        a.nlen = m.len[it & 1].get();
        a.nidx = m.idx[it & 1].get();
        a.nval = m.val[it & 1].get();
        a.changed = m.count.dev() + 2 * it;
        a.ovf_count = m.count.dev() + 2 * it + 1;
        hipLaunchKernelGGL(it ? mc_lds_kernel<false> : mc_lds_kernel<true>, dim3((unsigned)std::min<int64_t>(groups, n)), dim3(THREADS), 0,
                           ctx->stream, a);
        GNN_HIP(hipGetLastError());
        hipLaunchKernelGGL(it ? mc_dense_kernel<false> : mc_dense_kernel<true>, dim3((unsigned)dense_groups), dim3(THREADS), 0, ctx->stream, a);
        GNN_HIP(hipGetLastError());
        return GNN_OK;
    };
    {
        PassLog::Scope init(ctx, m.passes);
        if ((rc = pass(0))) return rc;
    }
    int it = 0;
    bool converged = false;
    while (it < in.max_iter && !converged) {                  // Ends: it grows towards max_iter
        ++it;
        {
            PassLog::Scope iteration(ctx, m.passes);
            if ((rc = pass(it))) return rc;
        }
        ull changed = 0;
        if ((rc = m.count.read(ctx, (size_t)2 * it, 1, &changed))) return rc;
        m.passes.settle();
        changed_host[it - 1] = (int64_t)changed;
        converged = changed == 0;
    }
    const int cur = it & 1;
    {
        ProfScope prof(ctx, GNN_K_NEIGHBOURS);
        if ((rc = launch_1d(mc_parent_kernel, n, ctx->stream, n, m.parent.get(), m.size.get()))) return rc;
        if ((rc = launch_1d(mc_link_kernel, n, ctx->stream, n, in.select, m.len[cur].get(), m.idx[cur].get(), m.parent.get()))) return rc;
        if ((rc = launch_1d(mc_flatten_kernel, n, ctx->stream, n, m.ok.get(), m.parent.get(), m.size.get(), label))) return rc;
        if ((rc = launch_1d(mc_summarise_kernel, n, ctx->stream, n, in.select, m.ok.get(), m.len[cur].get(), m.idx[cur].get(), m.val[cur].get(),
                            m.size.get(), label, size, attractor, flow, is_attractor)))
            return rc;
    }
    // the columns every pass pushed on the overflow list, the initial matrix first: read once, behind everything
    m.overflow.assign((size_t)it + 1, 0);
    std::vector<ull> counts((size_t)2 * (it + 1));
    if ((rc = m.count.read(ctx, 0, counts.size(), counts.data()))) return rc;
    m.passes.settle();
    for (int k = 0; k <= it; ++k) m.overflow[k] = (int64_t)counts[2 * k + 1];
    *iterations_host = it;
    *converged_host = converged;
    m.have = true;
    m.n = n;
    m.select = in.select;
    m.cur = cur;
    return GNN_OK;
}

// what both entry points check before the ctx is looked at
int mcl_check(const char* fn, const MclIn& in, const void* label, const void* size, const void* attractor, const void* flow, const void* is_attractor,
              const void* changed, const void* iterations, const void* converged) {
    const std::string f(fn);
    if (int rc = check_mcl_args(f, in.n, in.nnz, in.a4, in.select, in.precision, in.max_iter)) return rc;
    return nn_check_required(f,
                             in.indptr && (in.nnz == 0 || (in.col && in.sim)) && iterations && converged && (in.max_iter == 0 || changed) &&
                                 (in.n == 0 || (label && size && attractor && flow && is_attractor)),
                             "indptr, col, sim, the five outputs, changed, iterations and converged");
}

// n == 0: the definition's answer - one iteration that changes nothing
void mcl_empty(gnn_ctx* ctx, int max_iter, int64_t* changed_host, int64_t* iterations_host, int* converged_host) {
    ctx->mcl.have = true;
    ctx->mcl.n = 0;
    ctx->mcl.passes.begin();
    ctx->mcl.overflow.clear();
    if (max_iter > 0) changed_host[0] = 0;
    *iterations_host = max_iter > 0;
    *converged_host = max_iter > 0;
}

}  // namespace
}  // namespace gnn

using namespace gnn;

extern "C" int gnn_mcl_dev(gnn_ctx* ctx, const int64_t* indptr_dev, const int32_t* col_dev, const float* sim_dev, const uint8_t* valid_dev_or_null,
                           int64_t n, int64_t nnz, int inflation_quarters, int select, int precision, int max_iter, int64_t* label_dev,
                           int64_t* size_dev, int64_t* attractor_dev, uint32_t* flow_dev, uint8_t* is_attractor_dev, int64_t* changed_host,
                           int64_t* iterations_host, int* converged_host) {
    const char* const fn = "gnn_mcl_dev";
    const MclIn in = {{indptr_dev, col_dev, sim_dev, valid_dev_or_null, n, nnz}, inflation_quarters, select, precision, max_iter};
    if (int rc = mcl_check(fn, in, label_dev, size_dev, attractor_dev, flow_dev, is_attractor_dev, changed_host, iterations_host, converged_host))
        return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (n == 0) {
        mcl_empty(ctx, max_iter, changed_host, iterations_host, converged_host);
        return GNN_OK;
    }
    return mcl_run(ctx, fn, in, label_dev, size_dev, attractor_dev, flow_dev, is_attractor_dev, changed_host, iterations_host, converged_host);
}

extern "C" int gnn_mcl(gnn_ctx* ctx, const int64_t* indptr_host, const int32_t* col_host, const float* sim_host, const uint8_t* valid_host_or_null,
                       int64_t n, int64_t nnz, int inflation_quarters, int select, int precision, int max_iter, int64_t* label_host,
                       int64_t* size_host, int64_t* attractor_host, uint32_t* flow_host, uint8_t* is_attractor_host, int64_t* changed_host,
                       int64_t* iterations_host, int* converged_host) {
    const char* const fn = "gnn_mcl";
    MclIn in = {{indptr_host, col_host, sim_host, valid_host_or_null, n, nnz}, inflation_quarters, select, precision, max_iter};
    if (int rc = mcl_check(fn, in, label_host, size_host, attractor_host, flow_host, is_attractor_host, changed_host, iterations_host,
                           converged_host))
        return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (n == 0) {
        mcl_empty(ctx, max_iter, changed_host, iterations_host, converged_host);
        return GNN_OK;
    }
    MclWorkspace& m = ctx->mcl;
    m.have = false;
    // every buffer stands before a copy is enqueued.  d_out: [label | size | attractor | flow (u32) | is_attractor (u8)]
    int rc = graph_reserve(ctx, m.graph, n, nnz);
    Landing land(m.d_out);
    const int label = land.add(label_host, n), size = land.add(size_host, n), attractor = land.add(attractor_host, n),
              flow = land.add(flow_host, n), is_attractor = land.add(is_attractor_host, n);
    if (!rc) rc = land.reserve(ctx);
    if (rc) return rc;
    if ((rc = graph_upload(ctx, m.graph, in))) return rc;
    rc = mcl_run(ctx, fn, in, land.dev<int64_t>(label), land.dev<int64_t>(size), land.dev<int64_t>(attractor), land.dev<uint32_t>(flow),
                 land.dev<uint8_t>(is_attractor), changed_host, iterations_host, converged_host);
    return rc ? rc : land.copy_out(ctx);
}

extern "C" int gnn_mcl_matrix(gnn_ctx* ctx, int64_t n, int select, int32_t* length_host, int32_t* idx_host, uint32_t* val_host) {
    const char* const fn = "gnn_mcl_matrix";
    if (int rc = check_ctx(ctx)) return rc;
    const MclWorkspace& m = ctx->mcl;
    if (!m.have || m.n != n || (n > 0 && m.select != select)) {
        set_error(std::string(fn) + ": no gnn_mcl* of the same (n, select) = (" + std::to_string(n) + ", " + std::to_string(select) +
                  ") was this ctx's last Markov clustering");
        return GNN_ERR_STATE;
    }
    if (n == 0) return GNN_OK;
    if (int rc = nn_check_required(fn, length_host && idx_host && val_host, "length, idx and val")) return rc;
    const size_t cells = (size_t)n * select;
    GNN_HIP(hipMemcpyAsync(length_host, m.len[m.cur].get(), (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    GNN_HIP(hipMemcpyAsync(idx_host, m.idx[m.cur].get(), cells * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    GNN_HIP(hipMemcpyAsync(val_host, m.val[m.cur].get(), cells * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    GNN_HIP(hipStreamSynchronize(ctx->stream));
    return GNN_OK;
}

extern "C" int gnn_debug_mcl_lds(gnn_ctx* ctx, int slots) {
    if (int rc = check_ctx(ctx)) return rc;
    if (slots < -1 || slots > LDS_SLOTS) {
        set_error("gnn_debug_mcl_lds: " + std::to_string(slots) + " slots is outside [-1, " + std::to_string(LDS_SLOTS) + "]");
        return GNN_ERR_ARG;
    }
    const int before = ctx->mcl.lds_slots;
    if (slots >= 0) ctx->mcl.lds_slots = slots;
    return before;
}

extern "C" int gnn_debug_mcl_groups(gnn_ctx* ctx, int groups) {
    if (int rc = check_ctx(ctx)) return rc;
    if (groups < 0 || groups > 65535) {
        set_error("gnn_debug_mcl_groups: " + std::to_string(groups) + " workgroups is outside [0, 65535]");
        return GNN_ERR_ARG;
    }
    ctx->mcl.groups = groups;
    return GNN_OK;
}

extern "C" int gnn_debug_mcl_pow(gnn_ctx* ctx, const uint64_t* u_host, int64_t n, int inflation_quarters, uint64_t* out_host) {
    const std::string fn = "gnn_debug_mcl_pow";
    const auto bad = [&](const char* what, int64_t v, const char* range) {
        set_error(fn + ": " + what + " " + std::to_string(v) + " is outside " + range);
        return GNN_ERR_ARG;
    };
    if (inflation_quarters < 5 || inflation_quarters > 32) return bad("inflation_quarters", inflation_quarters, "[5, 32]");
    if (n < 0 || n > CSR_N_MAX) return bad("n", n, "[0, 2^24]");
    if (int rc = nn_check_required(fn, n == 0 || (u_host && out_host), "u and out")) return rc;
    for (int64_t i = 0; i < n; ++i)                           // Ends: i grows towards n
        if (u_host[i] > ONE) return bad("u", (int64_t)std::min<uint64_t>(u_host[i], INT64_MAX), "[0, 2^30]");
    if (int rc = check_ctx(ctx)) return rc;
    if (n == 0) return GNN_OK;
    DevBuf<ull> u, out;
    int rc = u.reserve((size_t)n);
    if (!rc) rc = out.reserve((size_t)n);
    if (rc) return rc;
    GNN_HIP(hipMemcpyAsync(u.get(), u_host, (size_t)n * sizeof(ull), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = launch_1d(mc_pow_kernel, n, ctx->stream, n, inflation_quarters, u.get(), out.get()))) return rc;
    GNN_HIP(hipMemcpyAsync(out_host, out.get(), (size_t)n * sizeof(ull), hipMemcpyDeviceToHost, ctx->stream));
    GNN_HIP(hipStreamSynchronize(ctx->stream));               // before the buffers go
    return GNN_OK;
}

extern "C" int gnn_debug_mcl_ms(gnn_ctx* ctx, double* ms_out, int64_t capacity, int64_t* n_out) {
    if (int rc = check_ctx(ctx)) return rc;
    return ctx->mcl.passes.out(ctx, "gnn_debug_mcl_ms", ms_out, capacity, n_out);
}

extern "C" int gnn_debug_mcl_overflow(gnn_ctx* ctx, int64_t* count_out, int64_t capacity, int64_t* n_out) {
    if (int rc = check_ctx(ctx)) return rc;
    if (!n_out || capacity < 0 || (capacity > 0 && !count_out)) {
        set_error("bad argument to gnn_debug_mcl_overflow: n_out is required, and count_out for a capacity > 0");
        return GNN_ERR_ARG;
    }
    const std::vector<int64_t>& v = ctx->mcl.overflow;
    *n_out = (int64_t)v.size();
    for (int64_t i = 0; i < std::min<int64_t>(capacity, (int64_t)v.size()); ++i) count_out[i] = v[i];
    return GNN_OK;
}
