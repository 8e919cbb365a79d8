// Average linkage over a similarity graph (include/genomad_nn.h, "average linkage"): the UPGMA tree of the graph
// by rounds of reciprocal best pairs, in integers throughout - the definition is sequence.average_linkage, and every output here
// equals it bit for bit.  W = 2^24 is a similarity of 1; S(A, B) is the sum of q between two clusters, S / (|A| |B|) their average.
//   validate, symmetrise   gnn_csr_sym.h, shared with gnn_mcl.hip and gnn_spread.hip.  The host reads one word; GNN_ERR_ARG before
//                anything else runs, the outputs untouched.
//   state        per node: map (the cluster that absorbed it in the last pair launch, else itself; a live cluster maps to itself),
//                size, best, bestS, partner (the cluster it absorbed in the last pair launch, else -1), ub (the upper bound of its
//                next segment); per live cluster a segment (off, len) in one of two entry buffers (idx int32, sum uint64).  Per
//                absorbed node the merge record, written once by the absorbing cluster's thread.
//   init         map = identity, size = 1, the records cleared, ub = the degree; the symmetric graph's q widened into buffer 0.
//   contraction  one launch per round, from buffer r & 1 into the other.  A surviving cluster R walks its one or two source rows, maps
//                every column through map[], drops map[c] == R and adds the 64-bit sums into a table keyed by the mapped column - an
//                atomicCAS on the key, a 64-bit add on the sum.  The table's walk writes R's new segment, which starts at the exclusive
//                scan (nn_scan) of the upper bounds len[A] + len[B], and takes the best neighbour under al_order (size[] is the pair
//                launch's) with the stop test into best[R] / bestS[R].  Round 0 is the same launch with map = identity: parallel
//                entries are summed there.
//   row classes  by the upper bound, so a table never overflows: up to min(wave_rows, slots / 4) one wave with its quarter of the
//                table in LDS; up to `slots` the workgroup with the whole table; beyond, the workgroup with a uint64[n] accumulator in
//                global memory and a list of the columns touched (gnn_mcl.hip's scheme).  The pair launch files the rows on three
//                lists.  Every sum is an integer add and every choice goes through al_order and the smaller id: no output depends on
//                the class, the table's size, the entries' order or the grid.
//   pair         one thread per node: best[A] = B, best[B] = A, A < B merges.  A's thread writes the record at B, adds the sizes,
//                sets partner and ub; B's thread sets map[B] = A.  It counts the merges; the host reads that counter, 8 bytes.
// Only integer atomics (LDS: keys and sums; global: the accumulator, the lists' and the rounds' counters).  No float is added or
// compared, no inline assembly, no loop that waits for another workgroup: every loop's termination argument stands next to it.
// Every store is guarded by its bound.
#include "gnn_nn_frag.h"
#include "gnn_csr_sym.h"

namespace gnn {
namespace {

typedef unsigned long long ull;
typedef unsigned __int128 u128;

constexpr int64_t N_MAX = (int64_t)1 << 24;      // the graph's limit (gnn_mcl)
constexpr int64_t STOP_END = (int64_t)1 << 30;   // q < 2^30: a stop at or above it names nothing
constexpr int MAX_ROUNDS_MAX = 1 << 20;
constexpr int SLOTS_MAX = 4096;
constexpr int THREADS = 256;
constexpr int64_t DENSE_CELLS = (int64_t)1 << 24;       // the accumulators' cells, all workgroups together
constexpr int EMPTY = -1;
// the counters: two slots of [merged, wave rows, workgroup rows, dense rows] - the pair launch of round r counts in slot r & 1 and
// clears the other -, the call's rows by class, the verdict on the graph
constexpr size_t CNT_TOTALS = 8, CNT_FLAG = 11, CNT_WORDS = 12;

// The order of the best scan and the stop test: s1 / d1 against s2 / d2 as s1 * d2 against s2 * d1, exact in 128 bits
__device__ __forceinline__ int al_order(ull s1, ull d1, ull s2, ull d2) {
    const u128 l = (u128)s1 * d2, r = (u128)s2 * d1;
    return l < r ? -1 : (l > r ? 1 : 0);
}

struct Best {
    ull S;
    int d, id;                 // id < 0: none
};

// the larger S / d, among equals the smaller id
__device__ __forceinline__ void al_take(Best& b, ull S, int d, int id) {
    if (id < 0) return;
    if (b.id >= 0) {
        const int o = al_order(S, (ull)d, b.S, (ull)b.d);
        if (o < 0 || (o == 0 && id >= b.id)) return;
    }
    b.S = S;
    b.d = d;
    b.id = id;
}

__device__ __forceinline__ void al_wave_reduce(Best& b) {
    for (int o = 32; o; o >>= 1) {                            // Ends: o halves towards 0
        const ull S = __shfl_xor(b.S, o);
        const int d = __shfl_xor(b.d, o), id = __shfl_xor(b.id, o);
        al_take(b, S, d, id);
    }
}

// LDS traffic of one wave's lanes becomes visible to its other lanes: nothing moves across, and the wave's DS operations are done
__device__ __forceinline__ void al_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

struct AlArgs {
    int64_t n, cap;            // cap: elements of an entry buffer
    ull stop_q;
    int slots, wave_limit, dense_groups;
    const int64_t* off;        // the segments of the source buffer: [n + 1]
    const int64_t* noff;       // of the target buffer: the scan of ub
    int32_t* len;              // [n]
    const int32_t* idx;        // source
    const ull* sum;
    int32_t* nidx;             // target
    ull* nsum;
    const int32_t* map;
    const int32_t* size;
    const int32_t* partner;
    const int32_t* ub;
    int32_t* best;
    ull* bestS;
    const int32_t* rows;       // [3][n]
    const ull* nrows;          // the slot: [merged, wave rows, workgroup rows, dense rows]
    ull* totals;               // [3]
    ull* dense;                // [dense_groups][n], all zero between rows
    int32_t* touched;          // [dense_groups][n]
};

// The entries of R's source rows, relabelled, self entries dropped: f(column, sum), by `coop` workers of which this is `me`
template <typename F>
__device__ __forceinline__ void al_gather(const AlArgs& a, int R, int me, int coop, F&& f) {
    for (int s = 0; s < 2; ++s) {                             // Ends: two sources at the most
        const int src = s ? a.partner[R] : R;
        if ((unsigned)src >= (ull)a.n) break;                 // no partner
        const int64_t b = a.off[src];
        const int l = a.len[src];
        if (b < 0 || l < 0 || b + l > a.cap) break;           // never: the segments lie in the buffer
        for (int x = me; x < l; x += coop) {                  // Ends: x grows towards l
            const int c = a.idx[b + x];
            if ((unsigned)c >= (ull)a.n) continue;            // never: the entries name rows below n
            const int m = a.map[c];
            if (m == R || (unsigned)m >= (ull)a.n) continue;
            f(m, a.sum[b + x]);
        }
    }
}

// (key, s) into a table of T slots that holds fewer than T other keys: linear probing from a multiplicative hash
__device__ __forceinline__ void al_insert(int32_t* keys, ull* sums, int T, int key, ull s) {
    unsigned h = (unsigned)(((ull)((unsigned)key * 2654435761u) * (ull)T) >> 32);      // < T
    for (int p = 0; p < T; ++p) {                             // Ends: p grows towards T; a free slot or the key's own is met before
        const int prev = atomicCAS(&keys[h], EMPTY, key);
        if (prev == EMPTY || prev == key) {
            atomicAdd(&sums[h], s);
            return;
        }
        h = h + 1 == (unsigned)T ? 0u : h + 1;
    }
}

// the stop test and the row's results, by one thread
__device__ __forceinline__ void al_finish(const AlArgs& a, int R, const Best& b, int count) {
    const bool named = b.id >= 0 && al_order(b.S, (ull)b.d, a.stop_q * (ull)a.size[R], 1ull) >= 0;
    a.best[R] = named ? b.id : -1;
    a.bestS[R] = b.id >= 0 ? b.S : 0ull;
    a.len[R] = count;
}

// the table size a row of upper bound u takes of `most` >= u slots: results do not depend on it, the walk's length does
__device__ __forceinline__ int al_table(int u, int most, int least) { return min(most, max(least, 2 * u)); }

// R by one wave, its table the T slots at keys / sums
__device__ __forceinline__ void al_row_wave(const AlArgs& a, int R, int32_t* keys, ull* sums, int slice) {
    const int lane = threadIdx.x & 63;
    const int u = a.ub[R];
    const int64_t nb = a.noff[R];
    if (u < 1 || u > slice || nb < 0 || nb + u > a.cap) return;      // never: the pair launch filed the row by its bound
    const int T = al_table(u, slice, 64);
    al_gather(a, R, lane, 64, [&](int m, ull s) { al_insert(keys, sums, T, m, s); });
    al_wave_sync();
    Best b = {0ull, 0, -1};
    int count = 0;
    for (int s0 = 0; s0 < T; s0 += 64) {                      // Ends: s0 grows towards T; uniform in the wave
        const int s = s0 + lane;
        const int key = s < T ? keys[s] : EMPTY;
        const ull full = __ballot(key != EMPTY);
        if (key != EMPTY) {
            const ull S = sums[s];
            keys[s] = EMPTY;
            sums[s] = 0;
            const int pos = count + __popcll(full & ((1ull << lane) - 1ull));
            if (pos < u) {                                    // always: the distinct columns are at most the entries
                a.nidx[nb + pos] = key;
                a.nsum[nb + pos] = S;
            }
            al_take(b, S, a.size[key], key);
        }
        count += __popcll(full);
    }
    al_wave_sync();                                           // the slots are clear for the wave's next row
    al_wave_reduce(b);
    if (lane == 0) al_finish(a, R, b, min(count, u));
}

// the workgroup's best of its threads', in thread 0
__device__ __forceinline__ void al_block_reduce(Best& b, Best* red) {
    al_wave_reduce(b);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < THREADS / 64; ++w) al_take(b, red[w].S, red[w].d, red[w].id);
}

// R by the whole workgroup (every thread calls it), its table the first T of the `slots`
__device__ __forceinline__ void al_row_block(const AlArgs& a, int R, int32_t* keys, ull* sums, int* cnt, Best* red) {
    const int tid = threadIdx.x;
    const int u = a.ub[R];
    const int64_t nb = a.noff[R];
    if (u < 1 || u > a.slots || nb < 0 || nb + u > a.cap) return;      // never; uniform
    const int T = al_table(u, a.slots, THREADS);
    al_gather(a, R, tid, THREADS, [&](int m, ull s) { al_insert(keys, sums, T, m, s); });
    __syncthreads();
    Best b = {0ull, 0, -1};
    for (int s = tid; s < T; s += THREADS) {                  // Ends: s grows towards T
        const int key = keys[s];
        if (key == EMPTY) continue;
        const ull S = sums[s];
        keys[s] = EMPTY;
        sums[s] = 0;
        const int pos = atomicAdd(cnt, 1);
        if (pos < u) {                                        // always
            a.nidx[nb + pos] = key;
            a.nsum[nb + pos] = S;
        }
        al_take(b, S, a.size[key], key);
    }
    al_block_reduce(b, red);                                  // its barrier: every add to cnt is done
    if (tid == 0) {
        al_finish(a, R, b, min(*cnt, u));
        *cnt = 0;
    }
    __syncthreads();
}

// R by the whole workgroup with its accumulator in global memory: a column's first add finds 0 there (every sum is > 0)
__device__ __forceinline__ void al_row_dense(const AlArgs& a, int R, int* cnt, Best* red) {
    const int tid = threadIdx.x;
    ull* const dense = a.dense + (int64_t)blockIdx.x * a.n;
    int32_t* const touched = a.touched + (int64_t)blockIdx.x * a.n;
    const int u = a.ub[R];
    const int64_t nb = a.noff[R];
    if (u < 1 || nb < 0 || nb + u > a.cap) return;            // never; uniform
    al_gather(a, R, tid, THREADS, [&](int m, ull s) {
        const ull old = atomicAdd(dense + m, s);              // m < n: al_gather
        if (old == 0) {
            const int at = atomicAdd(cnt, 1);
            if (at < a.n) touched[at] = m;                    // always: at most n columns
        }
    });
    __syncthreads();
    const int P = (int)min<int64_t>(min(*cnt, u), a.n);
    Best b = {0ull, 0, -1};
    for (int p = tid; p < P; p += THREADS) {                  // Ends: p grows towards P
        const int key = touched[p];
        if ((unsigned)key >= (ull)a.n) continue;              // never
        // written by atomics of this workgroup: the load goes where they went
        const ull S = __hip_atomic_load(dense + key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(dense + key, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        a.nidx[nb + p] = key;                                 // p < P <= u
        a.nsum[nb + p] = S;
        al_take(b, S, a.size[key], key);
    }
    al_block_reduce(b, red);
    if (tid == 0) {
        al_finish(a, R, b, P);
        *cnt = 0;
    }
    __syncthreads();
}

// grid = the groups, 256 threads: the first dense_groups workgroups take the dense rows g, g + dense_groups, ..., then every workgroup
// the workgroup rows g, g + groups, ..., then its waves the wave rows w, w + 4 * groups, ...
__global__ __launch_bounds__(THREADS) void al_contract_kernel(AlArgs a) {
    __shared__ int32_t keys[SLOTS_MAX];
    __shared__ ull sums[SLOTS_MAX];
    __shared__ Best red[THREADS / 64];
    __shared__ int cnt;
    const int tid = threadIdx.x, wave = tid >> 6;
    for (int s = tid; s < SLOTS_MAX; s += THREADS) {          // Ends: s grows towards SLOTS_MAX
        keys[s] = EMPTY;
        sums[s] = 0;
    }
    if (tid == 0) cnt = 0;
    __syncthreads();
    const int64_t nwave = (int64_t)min(a.nrows[1], (ull)a.n), nblock = (int64_t)min(a.nrows[2], (ull)a.n),
                  ndense = (int64_t)min(a.nrows[3], (ull)a.n);
    if (blockIdx.x == 0 && tid < 3) a.totals[tid] += a.nrows[1 + tid];
    if ((int)blockIdx.x < a.dense_groups)
        for (int64_t w = blockIdx.x; w < ndense; w += a.dense_groups) {      // Ends: w grows towards ndense
            const int R = a.rows[2 * a.n + w];
            if ((unsigned)R < (ull)a.n) al_row_dense(a, R, &cnt, red);       // always; uniform: w is the workgroup's
        }
    for (int64_t w = blockIdx.x; w < nblock; w += gridDim.x) {               // Ends: w grows towards nblock
        const int R = a.rows[a.n + w];
        if ((unsigned)R < (ull)a.n) al_row_block(a, R, keys, sums, &cnt, red);      // always; uniform
    }
    const int slice = a.slots / 4;                            // a wave's quarter of the table
    for (int64_t w = (int64_t)blockIdx.x * 4 + wave; w < nwave; w += (int64_t)gridDim.x * 4) {      // Ends: w grows towards nwave
        const int R = a.rows[w];
        if ((unsigned)R < (ull)a.n) al_row_wave(a, R, keys + wave * slice, sums + wave * slice, slice);      // always; no barrier on this path
    }
}

// The class of a row of upper bound u (-1: it has no entries) filed on its list, and `merged` counted, by every thread of the wave
__device__ __forceinline__ void al_file(int64_t n, int i, int u, int merged, int slots, int wave_limit, int32_t* rows, ull* slot) {
    const int lane = threadIdx.x & 63;
    const ull below = (1ull << lane) - 1ull;
    const int cls = u < 1 ? -1 : (u <= wave_limit ? 0 : (u <= slots ? 1 : 2));
    for (int k = 0; k < 3; ++k) {                             // Ends: three classes
        const ull mask = __ballot(cls == k);
        if (!mask) continue;                                  // uniform
        const int leader = __ffsll((long long)mask) - 1;
        ull base = 0;
        if (lane == leader) base = atomicAdd(slot + 1 + k, (ull)__popcll(mask));
        base = __shfl(base, leader);
        const ull at = base + (ull)__popcll(mask & below);
        if (cls == k && at < (ull)n) rows[(int64_t)k * n + (int64_t)at] = i;      // always: a row is filed once
    }
    const ull m = __ballot(merged != 0);
    if (m && lane == __ffsll((long long)m) - 1) atomicAdd(slot, (ull)__popcll(m));
}

// one thread per node: the state of round 0 and the cleared records
__global__ __launch_bounds__(256) void al_init_kernel(int64_t n, int slots, int wave_limit, const int32_t* __restrict__ len, int32_t* __restrict__ map,
                                                      int32_t* __restrict__ size, int32_t* __restrict__ best, ull* __restrict__ bestS,
                                                      int32_t* __restrict__ partner, int32_t* __restrict__ ub, int32_t* __restrict__ parent,
                                                      ull* __restrict__ weight, int32_t* __restrict__ size_a, int32_t* __restrict__ size_b,
                                                      int32_t* __restrict__ round, int32_t* __restrict__ rows, ull* __restrict__ slot) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int u = 0;
    if (i < n) {
        u = len[i];
        map[i] = (int32_t)i;
        size[i] = 1;
        best[i] = -1;
        bestS[i] = 0;
        partner[i] = -1;
        ub[i] = u;
        parent[i] = -1;
        weight[i] = 0;
        size_a[i] = 0;
        size_b[i] = 0;
        round[i] = 0;
    }
    al_file(n, (int)i, u, 0, slots, wave_limit, rows, slot);
}

// the symmetric graph's weights as the sums of buffer 0
__global__ __launch_bounds__(256) void al_widen_kernel(int64_t cells, const int64_t* __restrict__ soff, int64_t n, const uint32_t* __restrict__ sq,
                                                       ull* __restrict__ sum) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x < cells && x < soff[n]) sum[x] = sq[x];
}

// one thread per node: the reciprocal test.  Only A's thread touches size[A], partner[A], ub[A] and the record at B = best[A]; only
// B's thread touches map[B], which is also what tells a live cluster: nothing here reads what another thread of the launch writes.
__global__ __launch_bounds__(256) void al_pair_kernel(int64_t n, int r, int slots, int wave_limit, const uint8_t* __restrict__ ok,
                                                      const int32_t* __restrict__ best, const ull* __restrict__ bestS, const int32_t* __restrict__ len,
                                                      int32_t* __restrict__ map, int32_t* __restrict__ size, int32_t* __restrict__ partner,
                                                      int32_t* __restrict__ ub, int32_t* __restrict__ parent, ull* __restrict__ weight,
                                                      int32_t* __restrict__ size_a, int32_t* __restrict__ size_b, int32_t* __restrict__ round,
                                                      int32_t* __restrict__ rows, ull* __restrict__ slot, ull* __restrict__ other) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < 4) other[threadIdx.x] = 0;      // the next pair launch counts there
    int u = 0, merged = 0;
    if (i < n) {
        int pt = -1;
        if (ok[i] && map[i] == (int32_t)i) {                  // a live cluster
            u = len[i];
            const int B = best[i];
            if ((unsigned)B < (ull)n && best[B] == (int32_t)i) {
                if (i < B) {                                  // absorbs B
                    const int sa = size[i], sb = size[B];
                    pt = B;
                    u += len[B];
                    parent[B] = (int32_t)i;
                    weight[B] = bestS[i];
                    size_a[B] = sa;
                    size_b[B] = sb;
                    round[B] = r;
                    size[i] = sa + sb;
                    merged = 1;
                } else {                                      // is absorbed
                    map[i] = B;
                    u = 0;
                }
            }
        }
        partner[i] = pt;
        ub[i] = u;
    }
    al_file(n, (int)i, u, merged, slots, wave_limit, rows, slot);
}

__global__ __launch_bounds__(256) void al_order_kernel(int64_t n, const ull* __restrict__ quads, int32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = al_order(quads[4 * i], quads[4 * i + 1], quads[4 * i + 2], quads[4 * i + 3]);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

struct AvglinkIn {
    const int64_t* indptr;     // device
    const int32_t* col;
    const float* sim;
    const uint8_t* valid;      // device, or NULL: every row
    int64_t n, nnz, stop_q;
    int max_rounds;
};

struct AvglinkOut {            // device
    int32_t* parent;
    ull* weight;
    int32_t* size_a;
    int32_t* size_b;
    int32_t* round;
};

int avglink_check(const char* fn, const AvglinkIn& in, const AvglinkOut& out, const void* merged, const void* rounds, const void* complete) {
    const std::string f(fn);
    const auto bad = [&](const char* what, int64_t v, const char* range) {
        set_error(f + ": " + what + " " + std::to_string(v) + " is outside " + range);
        return GNN_ERR_ARG;
    };
    if (in.n < 0 || in.n > N_MAX) return bad("n", in.n, "[0, 2^24]");
    if (in.nnz < 0) return bad("nnz", in.nnz, "[0, 2^63)");
    if (in.stop_q < 1 || in.stop_q >= STOP_END) return bad("stop_q", in.stop_q, "[1, 2^30): stop is a similarity in (0, 64)");
    if (in.max_rounds < 1 || in.max_rounds > MAX_ROUNDS_MAX) return bad("max_rounds", in.max_rounds, "[1, 2^20]");
    return nn_check_required(f,
                             in.indptr && (in.nnz == 0 || (in.col && in.sim)) && merged && rounds && complete &&
                                 (in.n == 0 || (out.parent && out.weight && out.size_a && out.size_b && out.round)),
                             "indptr, col, sim, the five per-node outputs, merged_per_round, rounds and complete");
}

// n > 0 rows: the graph on the device -> the records on the device and merged_per_round, rounds, complete on the host.  The ctx's
// stream is synchronised once for the verdict on the graph and once per round.
int avglink_run(gnn_ctx* ctx, const char* fn, const AvglinkIn& in, const AvglinkOut& out, int64_t* merged_host, int64_t* rounds_host,
                int* complete_host) {
    AvglinkWorkspace& w = ctx->avl;
    w.passes.begin();
    const int64_t n = in.n;
    const size_t entries = (size_t)std::max<int64_t>(2 * in.nnz, 1);
    const int slots = w.slots, wave_limit = std::min(w.wave_rows, slots / 4);
    const int groups = w.groups > 0 ? w.groups : (int)std::min<int64_t>((n + 3) / 4, 8 * (int64_t)std::max(ctx->cu_count, 1));
    const int dense_groups = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(groups, 64), DENSE_CELLS / n));
    int rc = nn_reserve(ctx, w.ok, (size_t)n);
    if (!rc) rc = w.count.reserve(ctx, CNT_WORDS);
    if (!rc) rc = w.count.zero(ctx, 0, CNT_WORDS);
    if (rc) return rc;
    {
        PassLog::Scope setup(ctx, w.passes);                  // open across the read below: nothing is settled there
        if ((rc = launch_1d(mc_validate_kernel, n, ctx->stream, n, in.nnz, in.indptr, in.col, in.sim, in.valid, w.ok.get(), w.count.dev() + CNT_FLAG)))
            return rc;
        ull bad = 0;
        if ((rc = w.count.read(ctx, CNT_FLAG, 1, &bad))) return rc;
        if (bad) {
            set_error(std::string(fn) + ": the graph is no upper-triangle CSR of " + std::to_string(n) + " rows and " + std::to_string(in.nnz) +
                      " entries with similarities below 64: indptr must rise from 0 to nnz, a row's col lie in (row, n), sim be finite");
            return GNN_ERR_ARG;
        }
        rc = nn_reserve(ctx, w.len, (size_t)n);
        if (!rc) rc = nn_reserve(ctx, w.cursor, (size_t)n);
        if (!rc) rc = nn_reserve(ctx, w.sq, entries);
        for (int b = 0; b < 2 && !rc; ++b) {
            rc = nn_reserve(ctx, w.off[b], (size_t)n + 1);
            if (!rc) rc = nn_reserve(ctx, w.idx[b], entries);
            if (!rc) rc = nn_reserve(ctx, w.sum[b], entries);
        }
        for (DevBuf<int32_t>* b : {&w.map, &w.size, &w.best, &w.partner, &w.ub})
            if (!rc) rc = nn_reserve(ctx, *b, (size_t)n);
        if (!rc) rc = nn_reserve(ctx, w.bestS, (size_t)n);
        if (!rc) rc = nn_reserve(ctx, w.rows, (size_t)3 * n);
        if (!rc) rc = nn_reserve(ctx, w.dense, (size_t)dense_groups * n);
        if (!rc) rc = nn_reserve(ctx, w.touched, (size_t)dense_groups * n);
        if (rc) return rc;
        GNN_HIP(hipMemsetAsync(w.dense.get(), 0, (size_t)dense_groups * n * sizeof(ull), ctx->stream));
        if ((rc = csr_symmetrise(ctx->stream, n, in.indptr, in.col, in.sim, w.ok.get(), w.len.get(), w.off[0].get(), w.cursor.get(), w.idx[0].get(),
                                 w.sq.get())))
            return rc;
        if ((rc = launch_1d(al_widen_kernel, (int64_t)entries, ctx->stream, (int64_t)entries, w.off[0].get(), n, w.sq.get(), w.sum[0].get()))) return rc;
        // the lists of round 0 stand in slot 1, as a pair launch before it would have left them
        if ((rc = launch_1d(al_init_kernel, n, ctx->stream, n, slots, wave_limit, w.len.get(), w.map.get(), w.size.get(), w.best.get(), w.bestS.get(),
                            w.partner.get(), w.ub.get(), out.parent, out.weight, out.size_a, out.size_b, out.round, w.rows.get(), w.count.dev() + 4)))
            return rc;
    }
    AlArgs a;
    a.n = n;
    a.cap = (int64_t)entries;
    a.stop_q = (ull)in.stop_q;
    a.slots = slots;
    a.wave_limit = wave_limit;
    a.dense_groups = dense_groups;
    a.len = w.len.get();
    a.map = w.map.get();
    a.size = w.size.get();
    a.partner = w.partner.get();
    a.ub = w.ub.get();
    a.best = w.best.get();
    a.bestS = w.bestS.get();
    a.rows = w.rows.get();
    a.totals = w.count.dev() + CNT_TOTALS;
    a.dense = w.dense.get();
    a.touched = w.touched.get();
    const int limit = (int)std::min<int64_t>(in.max_rounds, n + 1);      // a round that is not the last merges a pair: n rounds at the most
    int r = 0;
    bool complete = false;
    while (r < limit && !complete) {                          // Ends: r grows towards limit
        const int cur = r & 1;
        ull* const slot = w.count.dev() + 4 * cur;
        ull* const other = w.count.dev() + 4 * (cur ^ 1);     // what the launch before counted
        {
            PassLog::Scope round(ctx, w.passes);
            if ((rc = nn_scan(ctx->stream, w.ub.get(), n, w.off[cur ^ 1].get(), nullptr))) return rc;
            a.off = w.off[cur].get();
            a.noff = w.off[cur ^ 1].get();
            a.idx = w.idx[cur].get();
            a.sum = w.sum[cur].get();
            a.nidx = w.idx[cur ^ 1].get();
            a.nsum = w.sum[cur ^ 1].get();
            a.nrows = other;
            hipLaunchKernelGGL(al_contract_kernel, dim3((unsigned)groups), dim3(THREADS), 0, ctx->stream, a);
            GNN_HIP(hipGetLastError());
            if ((rc = launch_1d(al_pair_kernel, n, ctx->stream, n, r, slots, wave_limit, w.ok.get(), w.best.get(), w.bestS.get(), w.len.get(),
                                w.map.get(), w.size.get(), w.partner.get(), w.ub.get(), out.parent, out.weight, out.size_a, out.size_b, out.round,
                                w.rows.get(), slot, other)))
                return rc;
        }
        ull merged = 0;
        if ((rc = w.count.read(ctx, (size_t)4 * cur, 1, &merged))) return rc;
        w.passes.settle();
        merged_host[r] = (int64_t)merged;
        complete = merged == 0;
        ++r;
    }
    ull totals[3] = {0, 0, 0};
    if ((rc = w.count.read(ctx, CNT_TOTALS, 3, totals))) return rc;
    for (int k = 0; k < 3; ++k) w.class_rows[k] = (int64_t)totals[k];
    *rounds_host = r;
    *complete_host = complete;
    return GNN_OK;
}

// n == 0: the definition's answer - one round that merges nothing
void avglink_empty(gnn_ctx* ctx, int64_t* merged_host, int64_t* rounds_host, int* complete_host) {
    ctx->avl.passes.begin();
    for (int k = 0; k < 3; ++k) ctx->avl.class_rows[k] = 0;
    merged_host[0] = 0;
    *rounds_host = 1;
    *complete_host = 1;
}

// the body of the two debug knobs that return the value before the call
int avglink_knob(gnn_ctx* ctx, const char* fn, int* knob, int value) {
    if (int rc = check_ctx(ctx)) return rc;
    if (value < -1 || value > SLOTS_MAX) {
        set_error(std::string(fn) + ": " + std::to_string(value) + " is outside [-1, " + std::to_string(SLOTS_MAX) + "]");
        return GNN_ERR_ARG;
    }
    const int before = *knob;
    if (value >= 0) *knob = value;
    return before;
}

}  // namespace
}  // namespace gnn

using namespace gnn;

extern "C" int gnn_avglink_dev(gnn_ctx* ctx, const int64_t* indptr_dev, const int32_t* col_dev, const float* sim_dev, const uint8_t* valid_dev_or_null,
                               int64_t n, int64_t nnz, int64_t stop_q, int max_rounds, int32_t* parent_dev, uint64_t* weight_dev, int32_t* size_a_dev,
                               int32_t* size_b_dev, int32_t* round_dev, int64_t* merged_per_round_host, int64_t* rounds_host, int* complete_host) {
    const char* const fn = "gnn_avglink_dev";
    const AvglinkIn in = {indptr_dev, col_dev, sim_dev, valid_dev_or_null, n, nnz, stop_q, max_rounds};
    const AvglinkOut out = {parent_dev, reinterpret_cast<ull*>(weight_dev), size_a_dev, size_b_dev, round_dev};
    if (int rc = avglink_check(fn, in, out, merged_per_round_host, rounds_host, complete_host)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (n == 0) {
        avglink_empty(ctx, merged_per_round_host, rounds_host, complete_host);
        return GNN_OK;
    }
    return avglink_run(ctx, fn, in, out, merged_per_round_host, rounds_host, complete_host);
}

extern "C" int gnn_avglink(gnn_ctx* ctx, const int64_t* indptr_host, const int32_t* col_host, const float* sim_host, const uint8_t* valid_host_or_null,
                           int64_t n, int64_t nnz, int64_t stop_q, int max_rounds, int32_t* parent_host, uint64_t* weight_host, int32_t* size_a_host,
                           int32_t* size_b_host, int32_t* round_host, int64_t* merged_per_round_host, int64_t* rounds_host, int* complete_host) {
    const char* const fn = "gnn_avglink";
    AvglinkIn in = {indptr_host, col_host, sim_host, valid_host_or_null, n, nnz, stop_q, max_rounds};
    const AvglinkOut host = {parent_host, reinterpret_cast<ull*>(weight_host), size_a_host, size_b_host, round_host};
    if (int rc = avglink_check(fn, in, host, merged_per_round_host, rounds_host, complete_host)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (n == 0) {
        avglink_empty(ctx, merged_per_round_host, rounds_host, complete_host);
        return GNN_OK;
    }
    AvglinkWorkspace& w = ctx->avl;
    // every buffer stands before a copy is enqueued.  d_out: [parent (i32) | weight (u64) | size_a (i32) | size_b (i32) | round (i32)]
    int rc = nn_reserve(ctx, w.d_indptr, (size_t)n + 1);
    if (!rc) rc = nn_reserve(ctx, w.d_col, (size_t)std::max<int64_t>(nnz, 1));
    if (!rc) rc = nn_reserve(ctx, w.d_sim, (size_t)std::max<int64_t>(nnz, 1));
    if (!rc) rc = nn_reserve(ctx, w.d_valid, (size_t)n);
    Landing land(w.d_out);
    const int parent = land.add(parent_host, n), weight = land.add(host.weight, n), size_a = land.add(size_a_host, n),
              size_b = land.add(size_b_host, n), round = land.add(round_host, n);
    if (!rc) rc = land.reserve(ctx);
    if (rc) return rc;
    GNN_HIP(hipMemcpyAsync(w.d_indptr.get(), indptr_host, (size_t)(n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    if (nnz > 0) {
        GNN_HIP(hipMemcpyAsync(w.d_col.get(), col_host, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        GNN_HIP(hipMemcpyAsync(w.d_sim.get(), sim_host, (size_t)nnz * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    }
    if (valid_host_or_null) GNN_HIP(hipMemcpyAsync(w.d_valid.get(), valid_host_or_null, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    in.indptr = w.d_indptr.get();
    in.col = w.d_col.get();
    in.sim = w.d_sim.get();
    in.valid = valid_host_or_null ? w.d_valid.get() : nullptr;
    const AvglinkOut dev = {land.dev<int32_t>(parent), land.dev<ull>(weight), land.dev<int32_t>(size_a), land.dev<int32_t>(size_b),
                            land.dev<int32_t>(round)};
    if ((rc = avglink_run(ctx, fn, in, dev, merged_per_round_host, rounds_host, complete_host))) return rc;
    return land.copy_out(ctx);
}

extern "C" int gnn_debug_avglink_slots(gnn_ctx* ctx, int slots) {
    return ctx ? avglink_knob(ctx, "gnn_debug_avglink_slots", &ctx->avl.slots, slots) : check_ctx(ctx);
}

extern "C" int gnn_debug_avglink_wave_rows(gnn_ctx* ctx, int entries) {
    return ctx ? avglink_knob(ctx, "gnn_debug_avglink_wave_rows", &ctx->avl.wave_rows, entries) : check_ctx(ctx);
}

extern "C" int gnn_debug_avglink_groups(gnn_ctx* ctx, int groups) {
    if (int rc = check_ctx(ctx)) return rc;
    if (groups < 0 || groups > 65535) {
        set_error("gnn_debug_avglink_groups: " + std::to_string(groups) + " workgroups is outside [0, 65535]");
        return GNN_ERR_ARG;
    }
    ctx->avl.groups = groups;
    return GNN_OK;
}

extern "C" int gnn_debug_avglink_order(gnn_ctx* ctx, const uint64_t* quads_host, int64_t n, int32_t* out_host) {
    const char* const fn = "gnn_debug_avglink_order";
    if (n < 0 || n > N_MAX) {
        set_error(std::string(fn) + ": n " + std::to_string(n) + " is outside [0, 2^24]");
        return GNN_ERR_ARG;
    }
    if (int rc = nn_check_required(fn, n == 0 || (quads_host && out_host), "quads and out")) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (n == 0) return GNN_OK;
    DevBuf<ull> quads;
    DevBuf<int32_t> out;
    int rc = quads.reserve((size_t)4 * n);
    if (!rc) rc = out.reserve((size_t)n);
    if (rc) return rc;
    GNN_HIP(hipMemcpyAsync(quads.get(), quads_host, (size_t)4 * n * sizeof(ull), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = launch_1d(al_order_kernel, n, ctx->stream, n, quads.get(), out.get()))) return rc;
    GNN_HIP(hipMemcpyAsync(out_host, out.get(), (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    GNN_HIP(hipStreamSynchronize(ctx->stream));               // before the buffers go
    return GNN_OK;
}

extern "C" int gnn_debug_avglink_ms(gnn_ctx* ctx, double* ms_out, int64_t capacity, int64_t* n_out) {
    if (int rc = check_ctx(ctx)) return rc;
    return ctx->avl.passes.out(ctx, "gnn_debug_avglink_ms", ms_out, capacity, n_out);
}

extern "C" int gnn_debug_avglink_classes(gnn_ctx* ctx, int64_t* rows_out) {
    if (int rc = check_ctx(ctx)) return rc;
    if (int rc = nn_check_required("gnn_debug_avglink_classes", rows_out != nullptr, "rows_out")) return rc;
    for (int k = 0; k < 3; ++k) rows_out[k] = ctx->avl.class_rows[k];
    return GNN_OK;
}
