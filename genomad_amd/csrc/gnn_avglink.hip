// Average linkage over a similarity graph (include/genomad_nn.h, "average linkage"): the UPGMA tree of the graph
// by rounds of reciprocal best pairs, in integers throughout - the definition is sequence.average_linkage, and every output here
// equals it bit for bit.  W = 2^24 is a similarity of 1; S(A, B) is the sum of q between two clusters, S / (|A| |B|) their average.
//   validate, symmetrise   gnn_csr_sym.h, shared with the other consumers of the graph.  The host reads one word; GNN_ERR_ARG before
//                anything else runs, the outputs untouched.
//   state        per node: map (the cluster that absorbed it in the last pair launch, else itself; a live cluster maps to itself),
//                size, best, bestS, partner (the cluster it absorbed in the last pair launch, else -1), ub (the upper bound of its
//                next segment); per live cluster a segment (off, len) in one of two entry buffers (idx int32, sum uint64).  Per
//                absorbed node the merge record, written once by the absorbing cluster's thread.
//   init         map = identity, size = 1, the records cleared, ub = the degree; the symmetric graph's q widened into buffer 0.
//   contraction  one launch per round, from buffer r & 1 into the other: the row table of gnn_row_table.h under the policy AlContract.
//                A surviving cluster R walks its one or two source rows, maps every column through map[], drops map[c] == R and adds
//                the 64-bit sums into the table keyed by the mapped column.  The table's walk writes R's new segment, which starts at
//                the exclusive scan (nn_scan) of the upper bounds len[A] + len[B], and takes the best neighbour under al_order (size[]
//                is the pair launch's) with the stop test into best[R] / bestS[R].  Round 0 is the same launch with map = identity:
//                parallel entries are summed there.
//   row classes  gnn_row_table.h's, by the upper bound; the pair launch files the rows on the three lists.  Every sum is an integer add
//                and every choice goes through al_order and the smaller id: no output depends on the class, the table's size, the
//                entries' order or the grid.
//   pair         one thread per node: best[A] = B, best[B] = A, A < B merges.  A's thread writes the record at B, adds the sizes,
//                sets partner and ub; B's thread sets map[B] = A.  It counts the merges; the host reads that counter, 8 bytes.
// Only integer atomics (LDS: keys and sums; global: the accumulator, the lists' and the rounds' counters).  No float is added or
// compared, no inline assembly, no loop that waits for another workgroup: every loop's termination argument stands next to it.
// Every store is guarded by its bound.
#include "gnn_nn_frag.h"
#include "gnn_csr_sym.h"
#include "gnn_row_table.h"

namespace gnn {
namespace {

typedef unsigned __int128 u128;

constexpr int64_t STOP_END = (int64_t)1 << 30;   // q < 2^30: a stop at or above it names nothing
constexpr int MAX_ROUNDS_MAX = 1 << 20;
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
    static __device__ __forceinline__ Best none() { return {0ull, 0, -1}; }
    // the larger S / d, among equals the smaller id
    __device__ __forceinline__ void take(ull oS, int od, int oid) {
        if (oid < 0) return;
        if (id >= 0) {
            const int o = al_order(oS, (ull)od, S, (ull)d);
            if (o < 0 || (o == 0 && oid >= id)) return;
        }
        S = oS;
        d = od;
        id = oid;
    }
    __device__ __forceinline__ void take(const Best& o) { take(o.S, o.d, o.id); }
    __device__ __forceinline__ void wave_reduce() {
        for (int o = 32; o; o >>= 1) {                        // Ends: o halves towards 0
            const ull oS = __shfl_xor(S, o);
            const int od = __shfl_xor(d, o), oid = __shfl_xor(id, o);
            take(oS, od, oid);
        }
    }
};

struct AlArgs : RtArgs {         // m = stride = the graph's rows
    int64_t cap;               // elements of an entry buffer
    ull stop_q;
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
};

// The contraction as a policy of the row table (gnn_row_table.h)
struct AlContract {
    typedef AlArgs Args;
    typedef gnn::Best Best;
    static constexpr bool SIDE = false, PLACED = true;

    // The entries of R's source rows, relabelled, self entries dropped
    template <typename F>
    static __device__ __forceinline__ void gather(const AlArgs& a, int R, int me, int coop, ull&, F&& f) {
        for (int s = 0; s < 2; ++s) {                         // Ends: two sources at the most
            const int src = s ? a.partner[R] : R;
            if ((unsigned)src >= (ull)a.m) break;             // no partner
            const int64_t b = a.off[src];
            const int l = a.len[src];
            if (b < 0 || l < 0 || b + l > a.cap) break;       // never: the segments lie in the buffer
            for (int x = me; x < l; x += coop) {              // Ends: x grows towards l
                const int c = a.idx[b + x];
                if ((unsigned)c >= (ull)a.m) continue;        // never: the entries name rows below n
                const int m = a.map[c];
                if (m == R || (unsigned)m >= (ull)a.m) continue;
                f(m, a.sum[b + x]);
            }
        }
    }

    // what the pair launch filed the row by, and where its new segment starts; 0 where that would not lie in the buffer (never)
    static __device__ __forceinline__ int bound(const AlArgs& a, int R, int64_t& nb) {
        const int u = a.ub[R];
        nb = a.noff[R];
        return nb < 0 || nb + u > a.cap ? 0 : u;
    }

    // the key becomes entry `pos` of R's new segment and stands for the best neighbour (size[] is the pair launch's)
    static __device__ __forceinline__ void visit(const AlArgs& a, int R, int u, int64_t nb, int key, ull S, int pos, ull, Best& b) {
        if (pos < u) {                                        // always: the distinct columns are at most the entries; nb + u <= cap: bound
            a.nidx[nb + pos] = key;
            a.nsum[nb + pos] = S;
        }
        b.take(S, a.size[key], key);
    }

    // the stop test and the row's results
    static __device__ __forceinline__ void finish(const AlArgs& a, int R, const Best& b, int count) {
        const bool named = b.id >= 0 && al_order(b.S, (ull)b.d, a.stop_q * (ull)a.size[R], 1ull) >= 0;
        a.best[R] = named ? b.id : -1;
        a.bestS[R] = b.id >= 0 ? b.S : 0ull;
        a.len[R] = count;
    }
};

// grid = the groups, RT_THREADS threads: rt_rows
__global__ __launch_bounds__(RT_THREADS) void al_contract_kernel(AlArgs a) { rt_rows<AlContract>(a); }

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
    rt_file(n, (int)i, u, slots, wave_limit, rows, slot + 1);
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
    rt_file(n, (int)i, u, slots, wave_limit, rows, slot + 1);
    const ull m = __ballot(merged != 0);                      // the merges, counted at the slot's head by every thread of the wave
    if (m && (threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(slot, (ull)__popcll(m));
}

__global__ __launch_bounds__(256) void al_order_kernel(int64_t n, const ull* __restrict__ quads, int32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = al_order(quads[4 * i], quads[4 * i + 1], quads[4 * i + 2], quads[4 * i + 3]);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

struct AvglinkIn : CsrGraph {   // the graph on the device
    int64_t stop_q;
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
    if (int rc = graph_check(f, in.n, in.nnz)) return rc;
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
    const int slots = w.table.slots;
    RtPlan plan;
    int rc = nn_reserve(ctx, w.ok, (size_t)n);
    if (!rc) rc = w.count.reserve(ctx, CNT_WORDS);
    if (!rc) rc = w.count.zero(ctx, 0, CNT_WORDS);
    if (rc) return rc;
    {
        PassLog::Scope setup(ctx, w.passes);                  // open across the read below: nothing is settled there
        if ((rc = graph_validate(ctx, fn, in, w.ok.get(), w.count, CNT_FLAG))) return rc;
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
        if (!rc) rc = rt_plan(ctx, n, w.table, plan);
        if (rc) return rc;
        if ((rc = csr_symmetrise(ctx->stream, n, in.indptr, in.col, in.sim, w.ok.get(), w.len.get(), w.off[0].get(), w.cursor.get(), w.idx[0].get(),
                                 w.sq.get())))
            return rc;
        if ((rc = launch_1d(rt_widen_kernel, (int64_t)entries, ctx->stream, (int64_t)entries, w.off[0].get(), n, w.sq.get(), w.sum[0].get()))) return rc;
        // the lists of round 0 stand in slot 1, as a pair launch before it would have left them
        if ((rc = launch_1d(al_init_kernel, n, ctx->stream, n, slots, plan.wave_limit, w.len.get(), w.map.get(), w.size.get(), w.best.get(),
                            w.bestS.get(), w.partner.get(), w.ub.get(), out.parent, out.weight, out.size_a, out.size_b, out.round, w.table.rows.get(),
                            w.count.dev() + 4)))
            return rc;
    }
    AlArgs a;
    a.m = a.stride = n;
    a.cap = (int64_t)entries;
    a.stop_q = (ull)in.stop_q;
    a.slots = slots;
    a.wave_limit = plan.wave_limit;
    a.dense_groups = plan.dense_groups;
    a.len = w.len.get();
    a.map = w.map.get();
    a.size = w.size.get();
    a.partner = w.partner.get();
    a.ub = w.ub.get();
    a.best = w.best.get();
    a.bestS = w.bestS.get();
    a.rows = w.table.rows.get();
    a.totals = w.count.dev() + CNT_TOTALS;
    a.dense = w.table.dense.get();
    a.touched = w.table.touched.get();
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
            a.nrows = other + 1;                            // behind `merged`
            hipLaunchKernelGGL(al_contract_kernel, dim3((unsigned)plan.groups), dim3(RT_THREADS), 0, ctx->stream, a);
            GNN_HIP(hipGetLastError());
            if ((rc = launch_1d(al_pair_kernel, n, ctx->stream, n, r, slots, plan.wave_limit, w.ok.get(), w.best.get(), w.bestS.get(),
                                w.len.get(), w.map.get(), w.size.get(), w.partner.get(), w.ub.get(), out.parent, out.weight, out.size_a, out.size_b,
                                out.round, w.table.rows.get(), slot, other)))
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

}  // namespace
}  // namespace gnn

using namespace gnn;

extern "C" int gnn_avglink_dev(gnn_ctx* ctx, const int64_t* indptr_dev, const int32_t* col_dev, const float* sim_dev, const uint8_t* valid_dev_or_null,
                               int64_t n, int64_t nnz, int64_t stop_q, int max_rounds, int32_t* parent_dev, uint64_t* weight_dev, int32_t* size_a_dev,
                               int32_t* size_b_dev, int32_t* round_dev, int64_t* merged_per_round_host, int64_t* rounds_host, int* complete_host) {
    const char* const fn = "gnn_avglink_dev";
    const AvglinkIn in = {{indptr_dev, col_dev, sim_dev, valid_dev_or_null, n, nnz}, stop_q, max_rounds};
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
    AvglinkIn in = {{indptr_host, col_host, sim_host, valid_host_or_null, n, nnz}, stop_q, max_rounds};
    const AvglinkOut host = {parent_host, reinterpret_cast<ull*>(weight_host), size_a_host, size_b_host, round_host};
    if (int rc = avglink_check(fn, in, host, merged_per_round_host, rounds_host, complete_host)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (n == 0) {
        avglink_empty(ctx, merged_per_round_host, rounds_host, complete_host);
        return GNN_OK;
    }
    AvglinkWorkspace& w = ctx->avl;
    // every buffer stands before a copy is enqueued.  d_out: [parent (i32) | weight (u64) | size_a (i32) | size_b (i32) | round (i32)]
    int rc = graph_reserve(ctx, w.graph, n, nnz);
    Landing land(w.d_out);
    const int parent = land.add(parent_host, n), weight = land.add(host.weight, n), size_a = land.add(size_a_host, n),
              size_b = land.add(size_b_host, n), round = land.add(round_host, n);
    if (!rc) rc = land.reserve(ctx);
    if (rc) return rc;
    if ((rc = graph_upload(ctx, w.graph, in))) return rc;
    const AvglinkOut dev = {land.dev<int32_t>(parent), land.dev<ull>(weight), land.dev<int32_t>(size_a), land.dev<int32_t>(size_b),
                            land.dev<int32_t>(round)};
    if ((rc = avglink_run(ctx, fn, in, dev, merged_per_round_host, rounds_host, complete_host))) return rc;
    return land.copy_out(ctx);
}

extern "C" int gnn_debug_avglink_slots(gnn_ctx* ctx, int slots) {
    return rt_knob(ctx, "gnn_debug_avglink_slots", ctx ? &ctx->avl.table.slots : nullptr, slots);
}

extern "C" int gnn_debug_avglink_wave_rows(gnn_ctx* ctx, int entries) {
    return rt_knob(ctx, "gnn_debug_avglink_wave_rows", ctx ? &ctx->avl.table.wave_rows : nullptr, entries);
}

extern "C" int gnn_debug_avglink_groups(gnn_ctx* ctx, int groups) {
    return rt_set_groups(ctx, "gnn_debug_avglink_groups", ctx ? &ctx->avl.table.groups : nullptr, groups);
}

extern "C" int gnn_debug_avglink_order(gnn_ctx* ctx, const uint64_t* quads_host, int64_t n, int32_t* out_host) {
    const char* const fn = "gnn_debug_avglink_order";
    if (n < 0 || n > CSR_N_MAX) {
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
