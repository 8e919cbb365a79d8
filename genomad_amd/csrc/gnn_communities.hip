// Modularity communities of a similarity graph (include/genomad_nn.h, "modularity communities"): Louvain's
// levels with a synchronous move rule, in integers throughout - the definition is sequence.modularity_communities, and every output
// here equals it bit for bit.  W = 2^24 is a similarity of 1; M2 < 2^58 is the graph's doubled weight; r = 64 * resolution.
//   validate, symmetrise   gnn_csr_sym.h, shared with the other consumers of the graph.  The host reads one word; GNN_ERR_ARG before
//                anything else runs, the outputs untouched.
//   graph        per level m nodes; node i owns the segment (off[i], len[i]) of one of two entry buffers (idx int32, sum uint64), self
//                entry included, parallel entries allowed (level 0 has them apart; every consumer below adds them).
//   level start  comm[i] = i, tot[i] = k[i] = the row's sum (one wave per node), the nodes filed by their rows' lengths on three
//                lists, Qnum of the identity by the score and verdict launches.  Level 0 also sums M2, which the host checks.
//   want         per filed node i of community a: the entries j != i keyed by comm[j] and summed into the row table of gnn_row_table.h
//                (policy CmTable<true>), those of a itself summed aside as w_ia.  The table's walk takes D(i, c) = 64 M2 (w_ic -
//                w_ia) - r k_i (tot_c + k_i - tot_a) in signed 128 bits and keeps the largest D > 0, among equals the smaller c, into
//                want_c[i] and the two words of want_d[i].
//   row classes  gnn_row_table.h's, by the row's length (the contraction: by the upper bound of the new row).  Every sum is an integer
//                add and every choice goes through a total order: no output depends on the class, the table's size, the entries' order
//                or the grid.
//   pick         one wave per node: a wanting node i moves unless an entry j != i wants to move, sits in comm[i] or in i's target and
//                has a priority (D, h, -j) that is not smaller than i's.  It writes new_comm[i], adds k[i] to its community's new total
//                and counts the movers.
//   score        one wave per node: the weights of the entries inside new_comm's communities (64-bit adds) and the squares of the new
//                totals (128 bits: two words, the carry taken from the low word's add); the verdict launch (one thread) forms Qnum =
//                64 M2 in - r sum tot^2, compares it with the assignment's and writes the verdict.  The host reads one record per sweep
//                (moved, the sums, the verdict, Qnum) and, behind an accepted sweep, swaps the two assignments.
//   level end    the entries with equal comm join their ends (cl_join), a launch of its own flattens (nn_root); the roots are numbered
//                by a scan (nn_scan: the order of the smallest member), the members counted, scanned and scattered (the order inside a
//                list matters to nothing), the upper bounds len summed per component and scanned into the new segments' starts.  The
//                contraction (policy CmTable<false>) gathers all rows of a component's members, keyed by the column's component
//                number, self entries kept, by the same three classes into the other entry buffer.  The map row -> node and node ->
//                smallest row follow, and level_label is written.
// Only integer atomics (LDS: keys and sums; global: the accumulators, the lists' counters, totals and sums).  No float is added or
// compared, no inline assembly, no loop that waits for another workgroup: every loop's termination argument stands next to it.
// Every store is guarded by its bound.
#include "gnn_nn_frag.h"
#include "gnn_csr_sym.h"
#include "gnn_row_table.h"

namespace gnn {
namespace {

typedef unsigned __int128 u128;
typedef __int128 i128;

constexpr int64_t NNZ_END = (int64_t)1 << 30;    // entries of the upper triangle: a row's upper bound and its sum stay in their words
constexpr ull M2_END = 1ull << 58;
constexpr int R_MAX = 256;
constexpr int LEVELS_MAX = 32;
constexpr int SWEEPS_MAX = 1 << 20;
// the counters
enum : size_t {
    C_FLAG = 0,                // a CSR that is none
    C_M2 = 1,                  // two words: the doubled weight
    C_MOVED = 3,               // the sweep's record: movers, the inner weight, the squares' two words, the verdict, Qnum's two words
    C_IN = 4,
    C_SQ = 5,
    C_VERDICT = 7,
    C_QNUM = 8,
    C_COMPONENTS = 10,         // the level's end
    C_COMMUNITIES = 11,
    C_WANT_ROWS = 12,          // three: the level's nodes by class
    C_CONTRACT_ROWS = 15,      // three: the new nodes by class
    C_TOTALS = 18,             // six: the call's rows by class, want launches and contractions
    C_WORDS = 24
};
constexpr int LEVEL_STATS = 7;                   // nodes, communities, sweeps, accepted, moved, rejected, split

// x added to the 128-bit sum at w[0] (low), w[1]: the carry is taken from the low add's own return, so every wrap is seen once
__device__ __forceinline__ void cm_add128(ull* w, u128 x) {
    const ull lo = (ull)x, hi = (ull)(x >> 64);
    ull carry = 0;
    if (lo) {
        const ull old = atomicAdd(w, lo);
        carry = old + lo < old ? 1ull : 0ull;
    }
    if (hi + carry) atomicAdd(w + 1, hi + carry);            // hi < 2^63 here: no wrap of its own
}

// The gain of node i (weight k) moving from a (total ta, w_ia = wa) into c (total tc, w_ic = wc): exact, below 2^126 in magnitude
__device__ __forceinline__ i128 cm_gain(ull m2x64, int r, ull k, ull wc, ull wa, ull tc, ull ta) {
    return (i128)(u128)m2x64 * ((i128)(u128)wc - (i128)(u128)wa) -
           ((i128)r * (i128)(u128)k) * ((i128)(u128)tc + (i128)(u128)k - (i128)(u128)ta);
}

struct Best {
    ull lo, hi;                // D > 0
    int c;                     // c < 0: none
    static __device__ __forceinline__ Best none() { return {0ull, 0ull, -1}; }
    // the larger D, among equals the smaller c
    __device__ __forceinline__ void take(ull olo, ull ohi, int oc) {
        if (oc < 0) return;
        if (c >= 0) {
            if (ohi < hi || (ohi == hi && (olo < lo || (olo == lo && oc >= c)))) return;
        }
        lo = olo;
        hi = ohi;
        c = oc;
    }
    __device__ __forceinline__ void take(const Best& o) { take(o.lo, o.hi, o.c); }
    __device__ __forceinline__ void wave_reduce() {
        for (int o = 32; o; o >>= 1) {                        // Ends: o halves towards 0
            const ull olo = __shfl_xor(lo, o), ohi = __shfl_xor(hi, o);
            const int oc = __shfl_xor(c, o);
            take(olo, ohi, oc);
        }
    }
};

// the priority (D, h, -i) of mover j is smaller than that of mover i
__device__ __forceinline__ bool cm_lower(ull jlo, ull jhi, unsigned jh, int j, ull ilo, ull ihi, unsigned ih, int i) {
    if (jhi != ihi) return jhi < ihi;
    if (jlo != ilo) return jlo < ilo;
    if (jh != ih) return jh < ih;
    return j > i;
}

__device__ __forceinline__ unsigned cm_hash(int i, int s) { return ((unsigned)i + 1u) * 2654435761u + (unsigned)s * 40503u; }

struct CmArgs : RtArgs {         // m: the level's nodes; stride: the graph's rows
    int64_t cap;               // elements of an entry buffer
    const int64_t* off;        // the source graph
    const int32_t* len;
    const int32_t* idx;
    const ull* sum;
    // want
    const int32_t* comm;
    const ull* tot;
    const ull* k;
    ull m2x64;
    int r;
    int32_t* want_c;
    ull* want_d;
    // contraction
    const int32_t* comp;
    const int64_t* numoff;
    const int64_t* mstart;
    const int32_t* mlist;
    const int32_t* ub;
    const int64_t* noff;
    int32_t* nlen;
    int32_t* nidx;
    ull* nsum;
};

// the entries of one source row, by `coop` workers of which this is `me`: f(column, weight)
template <typename F>
__device__ __forceinline__ void cm_row(const CmArgs& a, int src, int me, int coop, F&& f) {
    const int64_t b = a.off[src];
    const int l = a.len[src];
    if (b < 0 || l < 0 || b + l > a.cap) return;              // never: the segments lie in the buffer
    for (int x = me; x < l; x += coop) {                      // Ends: x grows towards l
        const int c = a.idx[b + x];
        if ((unsigned)c < (ull)a.m) f(c, a.sum[b + x]);       // always: the entries name nodes below m
    }
}

// The two launches as policies of the row table (gnn_row_table.h).  WANT: node R's best move.  Otherwise: the contraction of component R.
template <bool WANT>
struct CmTable {
    typedef CmArgs Args;
    typedef gnn::Best Best;
    static constexpr bool SIDE = WANT, PLACED = !WANT;

    // What R's table receives: f(key, weight), key < m.  WANT: R's entries j != R under comm[j], those of R's own community added to
    // `side` instead.  Otherwise: the entries of all members of component R under their columns' component numbers, self entries kept.
    template <typename F>
    static __device__ __forceinline__ void gather(const CmArgs& a, int R, int me, int coop, ull& side, F&& f) {
        if (WANT) {
            const int own = a.comm[R];
            cm_row(a, R, me, coop, [&](int c, ull s) {
                if (c == R) return;
                const int key = a.comm[c];
                if (key == own)
                    side += s;
                else if ((unsigned)key < (ull)a.m)            // always
                    f(key, s);
            });
        } else {
            const int64_t p0 = a.mstart[R], p1 = a.mstart[R + 1];
            if (p0 < 0 || p1 > a.m) return;                   // never: the lists hold the level's nodes
            for (int64_t p = p0; p < p1; ++p) {               // Ends: p grows towards p1
                const int src = a.mlist[p];
                if ((unsigned)src >= (ull)a.m) continue;      // never
                cm_row(a, src, me, coop, [&](int c, ull s) {
                    const int root = a.comp[c];
                    if ((unsigned)root >= (ull)a.m) return;   // never
                    const int64_t key = a.numoff[root];
                    if (key >= 0 && key < a.m) f((int)key, s);      // always
                });
            }
        }
    }

    static __device__ __forceinline__ int bound(const CmArgs& a, int R, int64_t&) { return WANT ? a.len[R] : a.ub[R]; }

    // WANT takes the key's gain (wa: w_ia), otherwise the key becomes entry `pos` of the new row
    static __device__ __forceinline__ void visit(const CmArgs& a, int R, int u, int64_t, int key, ull S, int pos, ull wa, Best& b) {
        if (WANT) {
            const i128 d = cm_gain(a.m2x64, a.r, a.k[R], S, wa, a.tot[key], a.tot[a.comm[R]]);
            if (d > 0) b.take((ull)(u128)d, (ull)((u128)d >> 64), key);
        } else {
            const int64_t nb = a.noff[R];
            if (pos < u && nb >= 0 && nb + u <= a.cap) {      // always: the distinct keys are at most the entries
                a.nidx[nb + pos] = key;
                a.nsum[nb + pos] = S;
            }
        }
    }

    // the row's results
    static __device__ __forceinline__ void finish(const CmArgs& a, int R, const Best& b, int count) {
        if (WANT) {
            a.want_c[R] = b.c;
            a.want_d[2 * (int64_t)R] = b.c >= 0 ? b.lo : 0ull;
            a.want_d[2 * (int64_t)R + 1] = b.c >= 0 ? b.hi : 0ull;
        } else {
            a.nlen[R] = count;
        }
    }
};

// grid = the groups, RT_THREADS threads: rt_rows
template <bool WANT>
__global__ __launch_bounds__(RT_THREADS) void cm_table_kernel(CmArgs a) {
    rt_rows<CmTable<WANT>>(a);
}

// one thread per row: the state before level 0
__global__ __launch_bounds__(256) void cm_rows_init_kernel(int64_t n, const uint8_t* __restrict__ ok, int32_t* __restrict__ map,
                                                           int32_t* __restrict__ noderow) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    map[i] = ok[i] ? (int32_t)i : -1;
    noderow[i] = (int32_t)i;
}

// one thread per node: a level's first assignment, and the nodes filed by their rows' lengths
__global__ __launch_bounds__(256) void cm_level_init_kernel(int64_t m, int64_t stride, int slots, int wave_limit, const int32_t* __restrict__ len,
                                                            int32_t* __restrict__ comm, int32_t* __restrict__ want_c, ull* __restrict__ want_d,
                                                            int32_t* __restrict__ parent, int32_t* __restrict__ rows, ull* __restrict__ nrows) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int u = 0;
    if (i < m) {
        u = len[i];
        comm[i] = (int32_t)i;
        want_c[i] = -1;
        want_d[2 * i] = 0;
        want_d[2 * i + 1] = 0;
        parent[i] = (int32_t)i;
    }
    rt_file(stride, (int)i, u, slots, wave_limit, rows, nrows);
}

// one wave per node: k[i] = tot[i] = the row's sum; m2 (not NULL at level 0) receives their sum in two words
__global__ __launch_bounds__(256) void cm_degree_kernel(int64_t m, int64_t cap, const int64_t* __restrict__ off, const int32_t* __restrict__ len,
                                                        const ull* __restrict__ sum, ull* __restrict__ k, ull* __restrict__ tot,
                                                        ull* __restrict__ m2) {
    const int lane = threadIdx.x & 63;
    u128 all = 0;
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < m; i += (int64_t)gridDim.x * 4) {      // Ends: i grows towards m
        const int64_t b = off[i];
        const int l = len[i];
        ull s = 0;
        if (b >= 0 && l >= 0 && b + l <= cap)                 // always
            for (int x = lane; x < l; x += 64) s += sum[b + x];      // Ends: x grows towards l
        s = rt_wave_sum(s);
        if (lane == 0) {
            k[i] = s;
            tot[i] = s;
        }
        all += s;
    }
    if (m2 && lane == 0 && all) cm_add128(m2, all);
}

// one wave per node: blocked or not, new_comm[i], its community's new total, the movers
__global__ __launch_bounds__(256) void cm_pick_kernel(int64_t m, int64_t cap, int sweep, const int64_t* __restrict__ off, const int32_t* __restrict__ len,
                                                      const int32_t* __restrict__ idx, const int32_t* __restrict__ comm,
                                                      const int32_t* __restrict__ want_c, const ull* __restrict__ want_d, const ull* __restrict__ k,
                                                      int32_t* __restrict__ new_comm, ull* __restrict__ new_tot, ull* __restrict__ moved) {
    const int lane = threadIdx.x & 63;
    ull movers = 0;
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < m; i += (int64_t)gridDim.x * 4) {      // Ends: i grows towards m
        const int own = comm[i];
        int target = want_c[i];
        if ((unsigned)target < (ull)m) {                      // uniform in the wave
            const ull ilo = want_d[2 * i], ihi = want_d[2 * i + 1];
            const unsigned ih = cm_hash((int)i, sweep);
            const int64_t b = off[i];
            const int l = len[i];
            bool blocked = false;
            if (b >= 0 && l >= 0 && b + l <= cap)             // always
                for (int x = lane; x < l; x += 64) {          // Ends: x grows towards l
                    const int j = idx[b + x];
                    if (j == i || (unsigned)j >= (ull)m) continue;
                    if (want_c[j] < 0) continue;
                    const int cj = comm[j];
                    if (cj != own && cj != target) continue;
                    blocked |= !cm_lower(want_d[2 * (int64_t)j], want_d[2 * (int64_t)j + 1], cm_hash(j, sweep), j, ilo, ihi, ih, (int)i);
                }
            if (__ballot(blocked)) target = own;
        } else {
            target = own;
        }
        if (lane == 0) {
            new_comm[i] = target;
            const ull ki = k[i];
            if (ki && (unsigned)target < (ull)m) atomicAdd(new_tot + target, ki);
            movers += target != own;
        }
    }
    if (lane == 0 && movers) atomicAdd(moved, movers);
}

// one wave per node: the weights inside the communities of `comm` and the squares of their totals, into in[0] and sq[0 .. 1]
__global__ __launch_bounds__(256) void cm_score_kernel(int64_t m, int64_t cap, const int64_t* __restrict__ off, const int32_t* __restrict__ len,
                                                       const int32_t* __restrict__ idx, const ull* __restrict__ sum, const int32_t* __restrict__ comm,
                                                       const ull* __restrict__ tot, ull* __restrict__ in, ull* __restrict__ sq) {
    const int lane = threadIdx.x & 63;
    ull inner = 0;
    u128 squares = 0;
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < m; i += (int64_t)gridDim.x * 4) {      // Ends: i grows towards m
        const int own = comm[i];
        const int64_t b = off[i];
        const int l = len[i];
        if (b >= 0 && l >= 0 && b + l <= cap)                 // always
            for (int x = lane; x < l; x += 64) {              // Ends: x grows towards l
                const int j = idx[b + x];
                if ((unsigned)j < (ull)m && comm[j] == own) inner += sum[b + x];
            }
        if (lane == 0) squares += (u128)tot[i] * tot[i];      // the community founded by i; an empty one adds 0
    }
    inner = rt_wave_sum(inner);                               // below M2 < 2^58
    if (lane == 0) {
        if (inner) atomicAdd(in, inner);
        if (squares) cm_add128(sq, squares);                  // below M2^2 < 2^116
    }
}

// one thread: Qnum = 64 M2 in - r sq against the assignment's; rec = [moved, in, sq lo, sq hi, verdict, Qnum lo, Qnum hi] (two's
// complement).  first: the level's own start, which is what later sweeps have to exceed
__global__ void cm_verdict_kernel(ull m2x64, int r, int first, ull* __restrict__ rec) {
    if (blockIdx.x || threadIdx.x) return;
    const i128 q = (i128)((u128)m2x64 * rec[1]) - (i128)((u128)(ull)r * (((u128)rec[3] << 64) | rec[2]));
    const i128 prev = (i128)(((u128)rec[6] << 64) | rec[5]);
    const bool better = first || q > prev;
    rec[4] = better ? 1ull : 0ull;
    if (better) {
        rec[5] = (ull)(u128)q;
        rec[6] = (ull)((u128)q >> 64);
    }
}

// one wave per node: the entries inside a community join their ends
__global__ __launch_bounds__(256) void cm_join_kernel(int64_t m, int64_t cap, const int64_t* __restrict__ off, const int32_t* __restrict__ len,
                                                      const int32_t* __restrict__ idx, const int32_t* __restrict__ comm, int32_t* __restrict__ parent) {
    const int lane = threadIdx.x & 63;
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < m; i += (int64_t)gridDim.x * 4) {      // Ends: i grows towards m
        const int own = comm[i];
        const int64_t b = off[i];
        const int l = len[i];
        if (b < 0 || l < 0 || b + l > cap) continue;          // never
        for (int x = lane; x < l; x += 64) {                  // Ends: x grows towards l
            const int j = idx[b + x];
            if (j < i && j >= 0 && comm[j] == own) cl_join(parent, (int)i, j);      // the pair stands at both ends: once is enough
        }
    }
}

// one thread per node, behind the joins: its component's smallest node, the roots flagged, the communities that have a member
// counted - a node with entries has k > 0, so a founder's community is empty exactly where its total is 0 and its k is not
__global__ __launch_bounds__(256) void cm_flatten_kernel(int64_t m, const uint8_t* __restrict__ live, const int32_t* __restrict__ parent,
                                                         const ull* __restrict__ tot, const ull* __restrict__ k, int32_t* __restrict__ comp,
                                                         int32_t* __restrict__ flag, ull* __restrict__ communities) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool founder = false;
    if (i < m) {
        const bool is = !live || live[i];
        const int root = nn_root(parent, (int)i);
        comp[i] = root;
        flag[i] = is && root == (int)i;
        founder = is && (tot[i] > 0 || k[i] == 0);
    }
    const ull mask = __ballot(founder);
    if (mask && (threadIdx.x & 63) == __ffsll((long long)mask) - 1) atomicAdd(communities, (ull)__popcll(mask));
}

// one thread per node: its component's members and the upper bound of its new row
__global__ __launch_bounds__(256) void cm_members_kernel(int64_t m, const uint8_t* __restrict__ live, const int32_t* __restrict__ comp,
                                                         const int64_t* __restrict__ numoff, const int32_t* __restrict__ len,
                                                         int32_t* __restrict__ mcount, int32_t* __restrict__ ub) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m || (live && !live[i])) return;
    const int64_t v = numoff[comp[i]];                        // comp[i] < m: cm_flatten_kernel
    if (v < 0 || v >= m) return;                              // never
    atomicAdd(mcount + v, 1);
    if (len[i] > 0) atomicAdd(ub + v, len[i]);                // the sum over all nodes is the entries of the buffer: below 2^31
}

// one thread per node: into its component's list through the cursor
__global__ __launch_bounds__(256) void cm_scatter_kernel(int64_t m, const uint8_t* __restrict__ live, const int32_t* __restrict__ comp,
                                                         const int64_t* __restrict__ numoff, const int64_t* __restrict__ mstart,
                                                         ull* __restrict__ mcursor, int32_t* __restrict__ mlist) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m || (live && !live[i])) return;
    const int64_t v = numoff[comp[i]];
    if (v < 0 || v >= m) return;                              // never
    const int64_t at = (int64_t)atomicAdd(mcursor + v, 1ull);
    if (at < mstart[v + 1] && at < m) mlist[at] = (int32_t)i;      // always
}

// one thread per slot of the new level: filed by its upper bound; a node without entries gets its empty row here.  The counts of the
// level's end go where the host reads them.
__global__ __launch_bounds__(256) void cm_contract_file_kernel(int64_t m, int64_t stride, int slots, int wave_limit, const int32_t* __restrict__ ub,
                                                               const int64_t* __restrict__ numoff, int32_t* __restrict__ nlen,
                                                               int32_t* __restrict__ rows, ull* __restrict__ nrows, ull* __restrict__ components) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int u = 0;
    if (v < m) {
        u = ub[v];
        nlen[v] = 0;
    }
    if (v == 0) *components = (ull)numoff[m];
    rt_file(stride, (int)v, u, slots, wave_limit, rows, nrows);
}

// one thread per row and per node (m <= n): the maps follow the contraction
__global__ __launch_bounds__(256) void cm_relabel_kernel(int64_t n, int64_t m, const int32_t* __restrict__ comp, const int32_t* __restrict__ flag,
                                                         const int64_t* __restrict__ numoff, int32_t* __restrict__ map,
                                                         const int32_t* __restrict__ noderow, int32_t* __restrict__ new_noderow) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < m && flag[i]) {
        const int64_t v = numoff[i];
        if (v >= 0 && v < m) new_noderow[v] = noderow[i];     // always.  A component's smallest node holds its smallest row
    }
    if (i < n) {
        const int node = map[i];
        if ((unsigned)node < (ull)m) {
            const int64_t v = numoff[comp[node]];
            if (v >= 0 && v < m) map[i] = (int32_t)v;         // always
        }
    }
}

// one thread per row: the labelling of the level
__global__ __launch_bounds__(256) void cm_label_kernel(int64_t n, int64_t m, const int32_t* __restrict__ map, const int32_t* __restrict__ noderow,
                                                       int64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int node = map[i];
    out[i] = (unsigned)node < (ull)m ? (int64_t)noderow[node] : -1;
}

// one thread per row: label = `from` (NULL: every valid row alone), and the members counted at the label
__global__ __launch_bounds__(256) void cm_final_kernel(int64_t n, const uint8_t* __restrict__ ok, const int64_t* __restrict__ from,
                                                       int64_t* __restrict__ label, int32_t* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t l = from ? from[i] : (ok[i] ? i : -1);
    label[i] = l;
    if (l >= 0 && l < n) atomicAdd(count + l, 1);
}

__global__ __launch_bounds__(256) void cm_size_kernel(int64_t n, const int64_t* __restrict__ label, const int32_t* __restrict__ count,
                                                      int64_t* __restrict__ size) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t l = label[i];
    size[i] = l >= 0 && l < n ? count[l] : 0;
}

// test aid: per operand row [m2x64, r, k, wc, wa, tc, ta, in, sq lo, sq hi, prev lo, prev hi] -> [D lo, D hi, Qnum lo, Qnum hi, Qnum > prev]
__global__ __launch_bounds__(256) void cm_gain_kernel(int64_t n, const ull* __restrict__ ops, ull* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const ull* o = ops + 12 * i;
    const i128 d = cm_gain(o[0], (int)o[1], o[2], o[3], o[4], o[5], o[6]);
    ull rec[7] = {0, o[7], o[8], o[9], 0, o[10], o[11]};
    const i128 q = (i128)((u128)o[0] * rec[1]) - (i128)((u128)(ull)(int)o[1] * (((u128)rec[3] << 64) | rec[2]));
    const i128 prev = (i128)(((u128)rec[6] << 64) | rec[5]);
    out[5 * i] = (ull)(u128)d;
    out[5 * i + 1] = (ull)((u128)d >> 64);
    out[5 * i + 2] = (ull)(u128)q;
    out[5 * i + 3] = (ull)((u128)q >> 64);
    out[5 * i + 4] = q > prev ? 1ull : 0ull;
}

// ---- label components ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void lc_init_kernel(int64_t n, int32_t* __restrict__ parent) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) parent[i] = (int32_t)i;
}

// one thread per row: its existing entries whose ends carry the same label join them
__global__ __launch_bounds__(256) void lc_join_kernel(int64_t n, const int64_t* __restrict__ indptr, const int32_t* __restrict__ col,
                                                      const float* __restrict__ sim, const uint8_t* __restrict__ ok, const int64_t* __restrict__ label,
                                                      int32_t* __restrict__ parent) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !ok[i] || label[i] < 0) return;
    for (int64_t x = indptr[i]; x < indptr[i + 1]; ++x) {     // Ends: x grows towards the row's end
        const int c = col[x];                                 // in (i, n): validated
        if (mc_weight(sim[x]) > 0 && ok[c] && label[c] == label[i]) cl_join(parent, (int)i, c);
    }
}

__global__ __launch_bounds__(256) void lc_out_kernel(int64_t n, const uint8_t* __restrict__ ok, const int64_t* __restrict__ label,
                                                     const int32_t* __restrict__ parent, int64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = ok[i] && label[i] >= 0 ? (int64_t)nn_root(parent, (int)i) : -1;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

struct CommIn : CsrGraph {      // the graph on the device
    int r, max_levels, max_sweeps;
};

struct CommOut {               // device
    int64_t* label;
    int64_t* size;
    int64_t* level_label;      // [max_levels][n]
};

struct CommHost {
    int64_t* stats;            // [max_levels][LEVEL_STATS]
    uint64_t* qnum;            // [max_levels][2]
    int64_t* levels;
    int* complete;
    uint64_t* m2;
};

// the graph's limits here: a row's upper bound and its sum stay in their words
int cm_graph_check(const std::string& f, int64_t n, int64_t nnz) { return graph_check(f, n, nnz, NNZ_END, "[0, 2^30)"); }

int communities_check(const char* fn, const CommIn& in, const CommOut& out, const CommHost& h) {
    const std::string f(fn);
    const auto bad = [&](const char* what, int64_t v, const char* range) {
        set_error(f + ": " + what + " " + std::to_string(v) + " is outside " + range);
        return GNN_ERR_ARG;
    };
    if (int rc = cm_graph_check(f, in.n, in.nnz)) return rc;
    if (in.r < 1 || in.r > R_MAX) return bad("r", in.r, "[1, 256]: the resolution is a multiple of 1/64 in [1/64, 4]");
    if (in.max_levels < 1 || in.max_levels > LEVELS_MAX) return bad("max_levels", in.max_levels, "[1, 32]");
    if (in.max_sweeps < 1 || in.max_sweeps > SWEEPS_MAX) return bad("max_sweeps", in.max_sweeps, "[1, 2^20]");
    return nn_check_required(f,
                             in.indptr && (in.nnz == 0 || (in.col && in.sim)) && h.stats && h.qnum && h.levels && h.complete && h.m2 &&
                                 (in.n == 0 || (out.label && out.size && out.level_label)),
                             "indptr, col, sim, label, size, level_label, level_stats, level_qnum, levels, complete and m2");
}

// validate: the verdict on the graph and the rows' validity in w.ok; one synchronise
int cm_validate(gnn_ctx* ctx, const char* fn, CommunitiesWorkspace& w, const CsrGraph& g) {
    int rc = nn_reserve(ctx, w.ok, (size_t)g.n);
    if (!rc) rc = w.count.reserve(ctx, C_WORDS);
    if (!rc) rc = w.count.zero(ctx, 0, C_WORDS);
    if (rc) return rc;
    return graph_validate(ctx, fn, g, w.ok.get(), w.count, C_FLAG);
}

// n > 0 rows: the graph on the device -> label, size and level_label on the device, the rest on the host.  The ctx's stream is
// synchronised once for the verdict on the graph, once per level's start and end and once per sweep.
int communities_run(gnn_ctx* ctx, const char* fn, const CommIn& in, const CommOut& out, const CommHost& h) {
    CommunitiesWorkspace& w = ctx->cmt;
    w.passes.begin();
    const int64_t n = in.n;
    const size_t entries = (size_t)std::max<int64_t>(2 * in.nnz, 1);
    const int slots = w.table.slots;
    RtPlan plan;
    int rc = GNN_OK;
    ull m2 = 0;
    ull qnum[2] = {0, 0};
    int cur = 0;                                              // the entry buffer of the level
    int64_t m = n;                                            // its nodes
    const uint8_t* live = nullptr;                            // level 0: w.ok; later every node below m counts
    int64_t n_live = 0;

    CmArgs a = {};
    // The level's start on the graph in buffer `cur`: the first assignment, k, the lists and Qnum of the identity (into qnum)
    const auto level_start = [&](bool first) -> int {
        if ((rc = w.count.zero(ctx, C_MOVED, C_COMPONENTS - C_MOVED))) return rc;
        if ((rc = w.count.zero(ctx, C_WANT_ROWS, 3))) return rc;
        if ((rc = launch_1d(cm_level_init_kernel, m, ctx->stream, m, n, slots, plan.wave_limit, w.len[cur].get(), w.comm[0].get(),
                            w.want_c.get(), w.want_d.get(), w.parent.get(), w.table.rows.get(), w.count.dev() + C_WANT_ROWS)))
            return rc;
        const unsigned wgrid = (unsigned)std::min<int64_t>((m + 3) / 4, plan.groups);
        hipLaunchKernelGGL(cm_degree_kernel, dim3(wgrid), dim3(256), 0, ctx->stream, m, (int64_t)entries, w.off[cur].get(), w.len[cur].get(),
                           w.sum[cur].get(), w.k.get(), w.tot[0].get(), first ? w.count.dev() + C_M2 : nullptr);
        GNN_HIP(hipGetLastError());
        if (first) {
            ull words[2] = {0, 0};
            if ((rc = w.count.read(ctx, C_M2, 2, words))) return rc;
            if (words[1] || words[0] >= M2_END) {
                set_error(std::string(fn) + ": the graph's doubled weight is not below 2^58");
                return GNN_ERR_ARG;
            }
            m2 = words[0];
            if (m2 == 0) return GNN_OK;
        }
        hipLaunchKernelGGL(cm_score_kernel, dim3(wgrid), dim3(256), 0, ctx->stream, m, (int64_t)entries, w.off[cur].get(), w.len[cur].get(),
                           w.idx[cur].get(), w.sum[cur].get(), w.comm[0].get(), w.tot[0].get(), w.count.dev() + C_IN, w.count.dev() + C_SQ);
        GNN_HIP(hipGetLastError());
        hipLaunchKernelGGL(cm_verdict_kernel, dim3(1), dim3(1), 0, ctx->stream, m2 * 64, in.r, 1, w.count.dev() + C_MOVED);
        GNN_HIP(hipGetLastError());
        return w.count.read(ctx, C_QNUM, 2, qnum);
    };

    {
        PassLog::Scope setup(ctx, w.passes);                  // open across the reads below: nothing is settled there
        if ((rc = cm_validate(ctx, fn, w, in))) return rc;
        rc = nn_reserve(ctx, w.cursor, (size_t)n);
        if (!rc) rc = nn_reserve(ctx, w.sq, entries);
        for (int b = 0; b < 2 && !rc; ++b) {
            rc = nn_reserve(ctx, w.off[b], (size_t)n + 1);
            if (!rc) rc = nn_reserve(ctx, w.len[b], (size_t)n);
            if (!rc) rc = nn_reserve(ctx, w.idx[b], entries);
            if (!rc) rc = nn_reserve(ctx, w.sum[b], entries);
            if (!rc) rc = nn_reserve(ctx, w.comm[b], (size_t)n);
            if (!rc) rc = nn_reserve(ctx, w.tot[b], (size_t)n);
            if (!rc) rc = nn_reserve(ctx, w.noderow[b], (size_t)n);
        }
        for (DevBuf<int32_t>* b : {&w.want_c, &w.parent, &w.comp, &w.flag, &w.ub, &w.mcount, &w.mlist, &w.map})
            if (!rc) rc = nn_reserve(ctx, *b, (size_t)n);
        if (!rc) rc = nn_reserve(ctx, w.k, (size_t)n);
        if (!rc) rc = nn_reserve(ctx, w.want_d, (size_t)2 * n);
        if (!rc) rc = nn_reserve(ctx, w.mcursor, (size_t)n);
        if (!rc) rc = nn_reserve(ctx, w.numoff, (size_t)n + 1);
        if (!rc) rc = nn_reserve(ctx, w.mstart, (size_t)n + 1);
        if (!rc) rc = rt_plan(ctx, n, w.table, plan);
        if (rc) return rc;
        if ((rc = csr_symmetrise(ctx->stream, n, in.indptr, in.col, in.sim, w.ok.get(), w.len[0].get(), w.off[0].get(), w.cursor.get(),
                                 w.idx[0].get(), w.sq.get())))
            return rc;
        if ((rc = launch_1d(rt_widen_kernel, (int64_t)entries, ctx->stream, (int64_t)entries, w.off[0].get(), n, w.sq.get(), w.sum[0].get()))) return rc;
        if ((rc = launch_1d(cm_rows_init_kernel, n, ctx->stream, n, w.ok.get(), w.map.get(), w.noderow[0].get()))) return rc;
        live = w.ok.get();
        if ((rc = level_start(true))) return rc;
    }

    a.stride = n;
    a.cap = (int64_t)entries;
    a.slots = slots;
    a.wave_limit = plan.wave_limit;
    a.dense_groups = plan.dense_groups;
    a.rows = w.table.rows.get();
    a.dense = w.table.dense.get();
    a.touched = w.table.touched.get();
    a.k = w.k.get();
    a.m2x64 = m2 * 64;
    a.r = in.r;
    a.want_c = w.want_c.get();
    a.want_d = w.want_d.get();
    a.comp = w.comp.get();
    a.numoff = w.numoff.get();
    a.mstart = w.mstart.get();
    a.mlist = w.mlist.get();
    a.ub = w.ub.get();

    int levels = 0, nr = 0;                                   // nr: the node -> row map in use
    bool complete = m2 == 0, capped = false;
    while (m2 > 0 && levels < in.max_levels && !complete) {   // Ends: levels grows towards max_levels
        if (levels == 0) {                                    // the valid rows are level 0's nodes
            std::vector<uint8_t> ok((size_t)n);
            GNN_HIP(hipMemcpyAsync(ok.data(), w.ok.get(), (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
            GNN_HIP(hipStreamSynchronize(ctx->stream));
            for (uint8_t v : ok) n_live += v != 0;
        }
        const int64_t nodes = levels == 0 ? n_live : m;
        const unsigned wgrid = (unsigned)std::min<int64_t>((m + 3) / 4, plan.groups);
        a.m = m;
        a.off = w.off[cur].get();
        a.len = w.len[cur].get();
        a.idx = w.idx[cur].get();
        a.sum = w.sum[cur].get();
        a.nrows = w.count.dev() + C_WANT_ROWS;
        a.totals = w.count.dev() + C_TOTALS;
        int c = 0;                                            // the assignment in use: comm[c], tot[c]
        int64_t sweeps = 0, accepted = 0, moved = 0, rejected = 0;
        bool ended = false;
        while (sweeps < in.max_sweeps && !ended) {            // Ends: sweeps grows towards max_sweeps
            ull rec[7] = {0, 0, 0, 0, 0, 0, 0};
            {
                PassLog::Scope sweep(ctx, w.passes);
                if ((rc = w.count.zero(ctx, C_MOVED, 4))) return rc;
                GNN_HIP(hipMemsetAsync(w.tot[c ^ 1].get(), 0, (size_t)m * sizeof(ull), ctx->stream));
                a.comm = w.comm[c].get();
                a.tot = w.tot[c].get();
                hipLaunchKernelGGL(cm_table_kernel<true>, dim3((unsigned)plan.groups), dim3(RT_THREADS), 0, ctx->stream, a);
                GNN_HIP(hipGetLastError());
                hipLaunchKernelGGL(cm_pick_kernel, dim3(wgrid), dim3(256), 0, ctx->stream, m, a.cap, (int)sweeps, a.off, a.len, a.idx, a.comm,
                                   w.want_c.get(), w.want_d.get(), w.k.get(), w.comm[c ^ 1].get(), w.tot[c ^ 1].get(), w.count.dev() + C_MOVED);
                GNN_HIP(hipGetLastError());
                hipLaunchKernelGGL(cm_score_kernel, dim3(wgrid), dim3(256), 0, ctx->stream, m, a.cap, a.off, a.len, a.idx, a.sum,
                                   w.comm[c ^ 1].get(), w.tot[c ^ 1].get(), w.count.dev() + C_IN, w.count.dev() + C_SQ);
                GNN_HIP(hipGetLastError());
                hipLaunchKernelGGL(cm_verdict_kernel, dim3(1), dim3(1), 0, ctx->stream, a.m2x64, in.r, 0, w.count.dev() + C_MOVED);
                GNN_HIP(hipGetLastError());
            }
            if ((rc = w.count.read(ctx, C_MOVED, 7, rec))) return rc;
            w.passes.settle();
            ++sweeps;
            if (rec[0] == 0) {
                ended = true;
            } else if (!rec[4]) {
                rejected = 1;
                ended = true;
            } else {
                c ^= 1;
                ++accepted;
                moved += (int64_t)rec[0];
            }
        }
        if (!ended) capped = true;                            // max_sweeps sweeps, the last one accepted
        int64_t communities = nodes, components = nodes;
        if (accepted) {
            PassLog::Scope end(ctx, w.passes);
            const int nxt = cur ^ 1;
            if ((rc = w.count.zero(ctx, C_COMPONENTS, 2))) return rc;
            if ((rc = w.count.zero(ctx, C_CONTRACT_ROWS, 3))) return rc;
            GNN_HIP(hipMemsetAsync(w.mcount.get(), 0, (size_t)m * sizeof(int32_t), ctx->stream));
            GNN_HIP(hipMemsetAsync(w.ub.get(), 0, (size_t)m * sizeof(int32_t), ctx->stream));
            hipLaunchKernelGGL(cm_join_kernel, dim3(wgrid), dim3(256), 0, ctx->stream, m, a.cap, a.off, a.len, a.idx, w.comm[c].get(), w.parent.get());
            GNN_HIP(hipGetLastError());
            if ((rc = launch_1d(cm_flatten_kernel, m, ctx->stream, m, live, w.parent.get(), w.tot[c].get(), w.k.get(), w.comp.get(), w.flag.get(),
                                w.count.dev() + C_COMMUNITIES)))
                return rc;
            if ((rc = nn_scan(ctx->stream, w.flag.get(), m, w.numoff.get(), nullptr))) return rc;
            if ((rc = launch_1d(cm_members_kernel, m, ctx->stream, m, live, w.comp.get(), w.numoff.get(), w.len[cur].get(), w.mcount.get(),
                                w.ub.get())))
                return rc;
            if ((rc = nn_scan(ctx->stream, w.mcount.get(), m, w.mstart.get(), w.mcursor.get()))) return rc;
            if ((rc = nn_scan(ctx->stream, w.ub.get(), m, w.off[nxt].get(), nullptr))) return rc;
            if ((rc = launch_1d(cm_scatter_kernel, m, ctx->stream, m, live, w.comp.get(), w.numoff.get(), w.mstart.get(), w.mcursor.get(),
                                w.mlist.get())))
                return rc;
            if ((rc = launch_1d(cm_contract_file_kernel, m, ctx->stream, m, n, slots, plan.wave_limit, w.ub.get(), w.numoff.get(),
                                w.len[nxt].get(), w.table.rows.get(), w.count.dev() + C_CONTRACT_ROWS, w.count.dev() + C_COMPONENTS)))
                return rc;
            a.nrows = w.count.dev() + C_CONTRACT_ROWS;
            a.totals = w.count.dev() + C_TOTALS + 3;
            a.noff = w.off[nxt].get();
            a.nlen = w.len[nxt].get();
            a.nidx = w.idx[nxt].get();
            a.nsum = w.sum[nxt].get();
            hipLaunchKernelGGL(cm_table_kernel<false>, dim3((unsigned)plan.groups), dim3(RT_THREADS), 0, ctx->stream, a);
            GNN_HIP(hipGetLastError());
            if ((rc = launch_1d(cm_relabel_kernel, n, ctx->stream, n, m, w.comp.get(), w.flag.get(), w.numoff.get(), w.map.get(), w.noderow[nr].get(),
                                w.noderow[nr ^ 1].get())))
                return rc;
            ull ends[2] = {0, 0};
            if ((rc = w.count.read(ctx, C_COMPONENTS, 2, ends))) return rc;
            components = (int64_t)ends[0];
            communities = (int64_t)ends[1];
            if (components < 1 || components > m) {           // never
                set_error(std::string(fn) + ": a level ended with " + std::to_string(components) + " components of " + std::to_string(m) + " nodes");
                return GNN_ERR_STATE;
            }
            cur = nxt;
            nr ^= 1;
            m = components;
            live = nullptr;
            if ((rc = level_start(false))) return rc;         // Qnum of the level's labelling, and the next level's start
        } else {
            complete = !capped;
        }
        if ((rc = launch_1d(cm_label_kernel, n, ctx->stream, n, m, w.map.get(), w.noderow[nr].get(), out.level_label + (int64_t)levels * n))) return rc;
        int64_t* const s = h.stats + (int64_t)levels * LEVEL_STATS;
        s[0] = nodes;
        s[1] = communities;
        s[2] = sweeps;
        s[3] = accepted;
        s[4] = moved;
        s[5] = rejected;
        s[6] = components - communities;
        h.qnum[2 * levels] = qnum[0];
        h.qnum[2 * levels + 1] = qnum[1];
        ++levels;
        if (!accepted) break;                                 // a level without an accepted sweep is the last
    }
    // the last level's labelling is the result; the member counts stand in mcount
    GNN_HIP(hipMemsetAsync(w.mcount.get(), 0, (size_t)n * sizeof(int32_t), ctx->stream));
    if ((rc = launch_1d(cm_final_kernel, n, ctx->stream, n, w.ok.get(), levels ? out.level_label + (int64_t)(levels - 1) * n : nullptr, out.label,
                        w.mcount.get())))
        return rc;
    if ((rc = launch_1d(cm_size_kernel, n, ctx->stream, n, out.label, w.mcount.get(), out.size))) return rc;
    ull totals[6] = {0, 0, 0, 0, 0, 0};
    if ((rc = w.count.read(ctx, C_TOTALS, 6, totals))) return rc;
    w.passes.settle();
    for (int k = 0; k < 6; ++k) w.class_rows[k] = (int64_t)totals[k];
    *h.levels = levels;
    *h.complete = complete;
    *h.m2 = m2;
    return GNN_OK;
}

// n == 0: the definition's answer - no level
void communities_empty(gnn_ctx* ctx, const CommHost& h) {
    ctx->cmt.passes.begin();
    for (int k = 0; k < 6; ++k) ctx->cmt.class_rows[k] = 0;
    *h.levels = 0;
    *h.complete = 1;
    *h.m2 = 0;
}

// n > 0: label -> out on the device
int components_run(gnn_ctx* ctx, const char* fn, const CsrGraph& g, const int64_t* label, int64_t* out) {
    CommunitiesWorkspace& w = ctx->cmt;
    const int64_t n = g.n;
    int rc = nn_reserve(ctx, w.parent, (size_t)n);
    if (rc) return rc;
    if ((rc = cm_validate(ctx, fn, w, g))) return rc;
    if ((rc = launch_1d(lc_init_kernel, n, ctx->stream, n, w.parent.get()))) return rc;
    if ((rc = launch_1d(lc_join_kernel, n, ctx->stream, n, g.indptr, g.col, g.sim, w.ok.get(), label, w.parent.get()))) return rc;
    return launch_1d(lc_out_kernel, n, ctx->stream, n, w.ok.get(), label, w.parent.get(), out);
}

int components_check(const char* fn, const int64_t* indptr, const int32_t* col, const float* sim, int64_t n, int64_t nnz, const int64_t* label,
                     const int64_t* out) {
    if (int rc = cm_graph_check(fn, n, nnz)) return rc;
    return nn_check_required(fn, indptr && (nnz == 0 || (col && sim)) && (n == 0 || (label && out)), "indptr, col, sim, label and out");
}

}  // namespace
}  // namespace gnn

using namespace gnn;

extern "C" int gnn_communities_dev(gnn_ctx* ctx, const int64_t* indptr_dev, const int32_t* col_dev, const float* sim_dev, const uint8_t* valid_dev_or_null,
                                   int64_t n, int64_t nnz, int r, int max_levels, int max_sweeps, int64_t* label_dev, int64_t* size_dev,
                                   int64_t* level_label_dev, int64_t* level_stats_host, uint64_t* level_qnum_host, int64_t* levels_host,
                                   int* complete_host, uint64_t* m2_host) {
    const char* const fn = "gnn_communities_dev";
    const CommIn in = {{indptr_dev, col_dev, sim_dev, valid_dev_or_null, n, nnz}, r, max_levels, max_sweeps};
    const CommOut out = {label_dev, size_dev, level_label_dev};
    const CommHost h = {level_stats_host, level_qnum_host, levels_host, complete_host, m2_host};
    if (int rc = communities_check(fn, in, out, h)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (n == 0) {
        communities_empty(ctx, h);
        return GNN_OK;
    }
    return communities_run(ctx, fn, in, out, h);
}

extern "C" int gnn_communities(gnn_ctx* ctx, const int64_t* indptr_host, const int32_t* col_host, const float* sim_host, const uint8_t* valid_host_or_null,
                               int64_t n, int64_t nnz, int r, int max_levels, int max_sweeps, int64_t* label_host, int64_t* size_host,
                               int64_t* level_label_host, int64_t* level_stats_host, uint64_t* level_qnum_host, int64_t* levels_host,
                               int* complete_host, uint64_t* m2_host) {
    const char* const fn = "gnn_communities";
    CommIn in = {{indptr_host, col_host, sim_host, valid_host_or_null, n, nnz}, r, max_levels, max_sweeps};
    const CommOut host = {label_host, size_host, level_label_host};
    const CommHost h = {level_stats_host, level_qnum_host, levels_host, complete_host, m2_host};
    if (int rc = communities_check(fn, in, host, h)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (n == 0) {
        communities_empty(ctx, h);
        return GNN_OK;
    }
    CommunitiesWorkspace& w = ctx->cmt;
    // the results stand in a scratch of their own and reach the caller behind a run that succeeded: d_out = [label | size | level_label]
    int rc = graph_reserve(ctx, w.graph, n, nnz);
    Landing land(w.d_out);
    const int label = land.add((int64_t*)nullptr, n), size = land.add((int64_t*)nullptr, n),
              level_label = land.add((int64_t*)nullptr, (int64_t)max_levels * n);
    if (!rc) rc = land.reserve(ctx);
    if (rc) return rc;
    if ((rc = graph_upload(ctx, w.graph, in))) return rc;
    const CommOut dev = {land.dev<int64_t>(label), land.dev<int64_t>(size), land.dev<int64_t>(level_label)};
    if ((rc = communities_run(ctx, fn, in, dev, h))) return rc;
    GNN_HIP(hipMemcpyAsync(label_host, dev.label, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    GNN_HIP(hipMemcpyAsync(size_host, dev.size, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (*levels_host > 0)                                     // only the levels that ran
        GNN_HIP(hipMemcpyAsync(level_label_host, dev.level_label, (size_t)*levels_host * n * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    GNN_HIP(hipStreamSynchronize(ctx->stream));
    return GNN_OK;
}

extern "C" int gnn_label_components_dev(gnn_ctx* ctx, const int64_t* indptr_dev, const int32_t* col_dev, const float* sim_dev,
                                        const uint8_t* valid_dev_or_null, int64_t n, int64_t nnz, const int64_t* label_dev, int64_t* out_dev) {
    const char* const fn = "gnn_label_components_dev";
    if (int rc = components_check(fn, indptr_dev, col_dev, sim_dev, n, nnz, label_dev, out_dev)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (n == 0) return GNN_OK;
    return components_run(ctx, fn, {indptr_dev, col_dev, sim_dev, valid_dev_or_null, n, nnz}, label_dev, out_dev);
}

extern "C" int gnn_label_components(gnn_ctx* ctx, const int64_t* indptr_host, const int32_t* col_host, const float* sim_host,
                                    const uint8_t* valid_host_or_null, int64_t n, int64_t nnz, const int64_t* label_host, int64_t* out_host) {
    const char* const fn = "gnn_label_components";
    if (int rc = components_check(fn, indptr_host, col_host, sim_host, n, nnz, label_host, out_host)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (n == 0) return GNN_OK;
    CommunitiesWorkspace& w = ctx->cmt;
    int rc = graph_reserve(ctx, w.graph, n, nnz);
    Landing land(w.d_out);
    const int label = land.add((int64_t*)nullptr, n), out = land.add(out_host, n);
    if (!rc) rc = land.reserve(ctx);
    if (rc) return rc;
    CsrGraph g = {indptr_host, col_host, sim_host, valid_host_or_null, n, nnz};
    if ((rc = graph_upload(ctx, w.graph, g))) return rc;
    GNN_HIP(hipMemcpyAsync(land.dev<int64_t>(label), label_host, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = components_run(ctx, fn, g, land.dev<int64_t>(label), land.dev<int64_t>(out)))) return rc;
    return land.copy_out(ctx);
}

extern "C" int gnn_debug_communities_slots(gnn_ctx* ctx, int slots) {
    return rt_knob(ctx, "gnn_debug_communities_slots", ctx ? &ctx->cmt.table.slots : nullptr, slots);
}

extern "C" int gnn_debug_communities_wave_rows(gnn_ctx* ctx, int entries) {
    return rt_knob(ctx, "gnn_debug_communities_wave_rows", ctx ? &ctx->cmt.table.wave_rows : nullptr, entries);
}

extern "C" int gnn_debug_communities_groups(gnn_ctx* ctx, int groups) {
    return rt_set_groups(ctx, "gnn_debug_communities_groups", ctx ? &ctx->cmt.table.groups : nullptr, groups);
}

extern "C" int gnn_debug_communities_gain(gnn_ctx* ctx, const uint64_t* operands_host, int64_t n, uint64_t* out_host) {
    const char* const fn = "gnn_debug_communities_gain";
    if (n < 0 || n > CSR_N_MAX) {
        set_error(std::string(fn) + ": n " + std::to_string(n) + " is outside [0, 2^24]");
        return GNN_ERR_ARG;
    }
    if (int rc = nn_check_required(fn, n == 0 || (operands_host && out_host), "operands and out")) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (n == 0) return GNN_OK;
    DevBuf<ull> ops, out;
    int rc = ops.reserve((size_t)12 * n);
    if (!rc) rc = out.reserve((size_t)5 * n);
    if (rc) return rc;
    GNN_HIP(hipMemcpyAsync(ops.get(), operands_host, (size_t)12 * n * sizeof(ull), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = launch_1d(cm_gain_kernel, n, ctx->stream, n, ops.get(), out.get()))) return rc;
    GNN_HIP(hipMemcpyAsync(out_host, out.get(), (size_t)5 * n * sizeof(ull), hipMemcpyDeviceToHost, ctx->stream));
    GNN_HIP(hipStreamSynchronize(ctx->stream));               // before the buffers go
    return GNN_OK;
}

extern "C" int gnn_debug_communities_ms(gnn_ctx* ctx, double* ms_out, int64_t capacity, int64_t* n_out) {
    if (int rc = check_ctx(ctx)) return rc;
    return ctx->cmt.passes.out(ctx, "gnn_debug_communities_ms", ms_out, capacity, n_out);
}

extern "C" int gnn_debug_communities_classes(gnn_ctx* ctx, int64_t* rows_out) {
    if (int rc = check_ctx(ctx)) return rc;
    if (int rc = nn_check_required("gnn_debug_communities_classes", rows_out != nullptr, "rows_out")) return rc;
    for (int k = 0; k < 6; ++k) rows_out[k] = ctx->cmt.class_rows[k];
    return GNN_OK;
}
