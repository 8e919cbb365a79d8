// Representatives among encoder embeddings (include/genomad_nn.h, "representatives"): greedy incremental
// clusters, as dereplication tools form them.  The rows arrive in PRIORITY ORDER (index = rank).  Walked in that order a row founds a
// cluster - it is a representative - unless an earlier representative is within the threshold; otherwise it is a member of the most
// similar such representative, ties to the smaller rank.  Stars, not chains: every member is within the threshold of its
// representative and no two representatives are within the threshold of each other.
// The walk is sequential; here it is deterministic synchronous rounds over the states of their start:
//   an UNDECIDED row with an edge to a smaller-rank row that became a representative in the previous round (FRESH) turns MEMBER;
//   otherwise an UNDECIDED row with no edge to a smaller-rank UNDECIDED row turns FRESH;  otherwise it stays UNDECIDED.
// By induction over the rank the representatives are the walk's (the lexicographically first maximal independent set): a row turns
// FRESH only when every smaller-rank neighbour is decided and none of them is a representative - one would have been FRESH in some
// earlier round while the row was UNDECIDED, and made it a MEMBER in the round after -, and it turns MEMBER only behind a
// representative of smaller rank.  WORST CASE: a path walked end to end needs as many rounds as it has rows; `rounds` is returned.
//   prepare    nn_prepare (gnn_neighbours.hip), as it is: the neighbour search's fragments and flags, in its buffers.
//   init       state = UNDECIDED or INVALID, flag = key = size = 0, the live maps, the count of undecided rows.
//   round      the tile parts of gnn_nn_frag.h - 64 rows' fragments in LDS, the base streamed in steps of 256 columns, NN_PRODUCTS'
//              three products per k-step in their order, the same scale, the UPPER TRIANGLE only: the value of the pair i < j
//              is the f32 gnn_neighbours returns for query i and base row j.  state[] is read-only during the launch.  For i < j with
//              s >= threshold, column j UNDECIDED and row i FRESH or UNDECIDED: HIT or WAIT is ORed into flag[j].  A workgroup whose
//              row tile holds no FRESH or UNDECIDED row leaves before it loads fragments; a wave whose two column blocks hold no
//              UNDECIDED column skips the step's k-loop: later rounds touch few rows.
//   decide     one thread per row: the rule above on (state, flag); FRESH of the previous round turns REP; the flag is cleared; the
//              undecided count and the live maps are brought up to date.
//   assign     only if a row is MEMBER; the round kernel's other instance with rows = representatives, columns = members: a 64-bit
//              atomicMax at key[j] of nn_key(nn_image(s), i).  A pass of its own: a representative of smaller rank may be decided in a
//              later round than the one that made j a member.
//   finish     rep and the exact f32 sim from the key; integer adds of the sizes at the representative.
//   summarise  every row takes its representative's size; an invalid row is -1 / NaN / 0.
// Flags are ORs, keys maxima, sizes integer adds: nothing depends on the order the workgroups run in or on the split of the base.  No
// kernel loop waits for another workgroup; every loop's termination argument stands next to it.
#include <cmath>

#include "gnn_nn_frag.h"

namespace gnn {
namespace {


enum : uint8_t { ST_INVALID = 0, ST_UNDECIDED = 1, ST_FRESH = 2, ST_REP = 3, ST_MEMBER = 4 };
enum : unsigned { FL_HIT = 1, FL_WAIT = 2 };

// grid = padded rows / 256 (padded is a multiple of 64: a wave is one row tile).  count[0] must be zero before the launch.
__global__ __launch_bounds__(256) void rp_init_kernel(int64_t n, int64_t padded, const uint8_t* __restrict__ valid, uint8_t* __restrict__ state,
                                                      unsigned* __restrict__ flag, unsigned long long* __restrict__ key,
                                                      unsigned long long* __restrict__ size, uint8_t* __restrict__ row_live,
                                                      uint8_t* __restrict__ col_live, unsigned long long* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= padded) return;                 // whole waves leave
    const bool ok = i < n && valid[i];
    state[i] = ok ? ST_UNDECIDED : ST_INVALID;
    flag[i] = 0;
    key[i] = 0;
    size[i] = 0;
    const unsigned long long und = __ballot(ok);
    if ((threadIdx.x & 63) == 0) {
        if (und) atomicAdd(count, (unsigned long long)__popcll(und));
        row_live[i / 64] = und != 0;
        col_live[i / 32] = (unsigned)und != 0;
        col_live[i / 32 + 1] = (und >> 32) != 0;
    }
}

struct TileArgs {
    const uint4* frag;         // round_up(n, 64) / 32 blocks: rows and columns alike
    const uint8_t* state;      // [round_up(n, 64)], read-only during the launch
    const uint8_t* row_live;   // round kernel: [tiles] the tile holds a FRESH or UNDECIDED row
    const uint8_t* col_live;   // round kernel: [blocks of 32] the block holds an UNDECIDED row
    int64_t n;
    int64_t split_rows;        // base rows per workgroup: a multiple of 32
    float scale;               // 2^-16 for cosine, 1 for dot
    float threshold;
    unsigned* flag;            // round kernel
    unsigned long long* key;   // assign kernel
};

// grid = (row tiles, base ranges), 256 threads.  LDS: the tile's fragments 128 KB and what its rows contribute.
// ASSIGN false: the round kernel (rows FRESH -> HIT, UNDECIDED -> WAIT; columns UNDECIDED; OR into flag).
// ASSIGN true:  the assign kernel (rows FRESH or REP; columns MEMBER; max into key).
template <bool ASSIGN>
__global__ __launch_bounds__(256) void rp_tile_kernel(TileArgs a) {
    __shared__ uint4 qs[2 * BLK_U4];
    __shared__ uint8_t lsrc[QT];           // what an edge from the tile's row says: 0 = nothing
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    TileRange t;
    if (!nn_tile_range(t, a.split_rows, a.n, true)) return;
    const int64_t r0 = t.r0, b1 = t.b1;
    uint8_t src = 0;
    if (tid < QT) {
        const uint8_t st = a.state[r0 + tid];              // state[] covers the padded rows
        src = ASSIGN ? (st == ST_FRESH || st == ST_REP) : (st == ST_FRESH ? FL_HIT : st == ST_UNDECIDED ? FL_WAIT : 0);
    }
    if (ASSIGN) {
        if (!__syncthreads_or(src)) return;                // no representative in the tile (uniform: the whole workgroup leaves)
    } else {
        if (!a.row_live[blockIdx.x]) return;               // neither FRESH nor UNDECIDED (one byte: the whole workgroup leaves)
    }
    nn_copy_tile(qs, a.frag, tid);
    if (tid < QT) lsrc[tid] = src;
    __syncthreads();
    const int64_t last_blk = t.last_blk();
    // Whether a step runs: bit nb of the lane's answer says that its column block nb matters.  Round: the block's live byte (the
    // same for the whole wave).  Assign: the lane's own column is a MEMBER.
    auto probe = [&](int64_t c0) -> int {
        int w = 0;
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const int64_t blk = nn_step_blk(c0, wave, nb);
            if (ASSIGN) {
                const int64_t col = nn_blk_col(blk, lane);
                w |= (int)(col < b1 && a.state[col] == ST_MEMBER) << nb;
            } else {
                w |= (int)(blk <= last_blk && a.col_live[blk] != 0) << nb;
            }
        }
        return w;
    };
    // Ends: c0 grows by STEP towards b1.
    int64_t c0 = t.c0;
    int next = probe(c0);
    for (; c0 < b1; c0 += STEP) {
        const int want = next;
        if (c0 + STEP < b1) next = probe(c0 + STEP);       // one step ahead: its latency hides under this step's MFMAs
        if (__ballot(want != 0) == 0) continue;            // wave-uniform, and no barrier follows in the loop
        const uint4* bp[2];
        int cg[2];                         // the lane's column, -1: nothing can end there
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const int64_t col = nn_step_column(a.frag, c0, wave, lane, nb, last_blk, bp[nb]);
            const bool open = ASSIGN ? (want >> nb) & 1 : col < b1 && a.state[col] == ST_UNDECIDED;       // round: read behind the MFMAs
            cg[nb] = open ? (int)col : -1;
        }
        f32x16 acc[2][2];
        NN_PRODUCTS(qs, bp, lane, acc);
        // ---- a column is one lane's through all its registers, and the other half-wave's: reduced in the lane, then with one
        // __shfl_xor; one atomic per column and step
        unsigned f[2] = {0, 0};            // round: the flag bits of the lane's two columns
        unsigned long long k[2] = {0, 0};  // assign: their largest keys
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = nn_acc_row(mb, r, lane >> 5);
                const int rg = (int)r0 + row;
                const unsigned s8 = lsrc[row];
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    const float s = acc[mb][nb][r] * a.scale;
                    const bool e = s8 && rg < cg[nb] && s >= a.threshold;           // cg = -1 fails rg < cg; a NaN fails >=
                    if (ASSIGN) {
                        const unsigned long long key = nn_key(nn_image(s), (unsigned)rg);
                        k[nb] = e && key > k[nb] ? key : k[nb];
                    } else {
                        f[nb] |= e ? s8 : 0u;
                    }
                }
            }
        if (__ballot(ASSIGN ? (k[0] | k[1]) != 0 : (f[0] | f[1]) != 0) == 0) continue;      // the common case; wave-uniform
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            if (ASSIGN) {
                const unsigned long long o = __shfl_xor(k[nb], 32);
                const unsigned long long m = o > k[nb] ? o : k[nb];
                if (lane < 32 && m) atomicMax(a.key + cg[nb], m);                   // m > 0 only where cg >= 0
            } else {
                const unsigned o = f[nb] | __shfl_xor(f[nb], 32);
                if (lane < 32 && o) atomicOr(a.flag + cg[nb], o);                   // o > 0 only where cg >= 0
            }
        }
    }
}

// grid = padded rows / 256.  count[0]: the undecided rows, lowered by those that leave; count[1]: the members, ever.
__global__ __launch_bounds__(256) void rp_decide_kernel(int64_t padded, uint8_t* __restrict__ state, unsigned* __restrict__ flag,
                                                        uint8_t* __restrict__ row_live, uint8_t* __restrict__ col_live,
                                                        unsigned long long* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= padded) return;                 // whole waves leave
    const uint8_t st = state[i];
    const unsigned f = flag[i];
    uint8_t nx = st;
    if (st == ST_UNDECIDED) nx = (f & FL_HIT) ? ST_MEMBER : f ? ST_UNDECIDED : ST_FRESH;
    else if (st == ST_FRESH) nx = ST_REP;
    if (nx != st) state[i] = nx;
    if (f) flag[i] = 0;
    const unsigned long long und = __ballot(nx == ST_UNDECIDED), left = __ballot(st == ST_UNDECIDED && nx != ST_UNDECIDED);
    const unsigned long long mem = __ballot(st == ST_UNDECIDED && nx == ST_MEMBER), fresh = __ballot(nx == ST_FRESH);
    if ((threadIdx.x & 63) == 0) {
        if (left) atomicAdd(count, 0ull - (unsigned long long)__popcll(left));     // modulo 2^64: a subtraction
        if (mem) atomicAdd(count + 1, (unsigned long long)__popcll(mem));
        row_live[i / 64] = (und | fresh) != 0;
        col_live[i / 32] = (unsigned)und != 0;
        col_live[i / 32 + 1] = (und >> 32) != 0;
    }
}

// A launch of its own behind the assign kernel: plain loads see every key.  FRESH is a representative the loop's end left so.
__global__ __launch_bounds__(256) void rp_finish_kernel(int64_t n, const uint8_t* __restrict__ state, const unsigned long long* __restrict__ key,
                                                        unsigned long long* __restrict__ size, int64_t* __restrict__ rep,
                                                        float* __restrict__ sim) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint8_t st = state[i];
    int64_t r = -1;
    float s = __uint_as_float(0x7fc00000u);
    if (st == ST_FRESH || st == ST_REP) {
        r = i;
    } else if (st == ST_MEMBER) {
        const unsigned long long k = key[i];
        const int64_t from = (int64_t)nn_key_index(k);
        if (k && from < i) {               // every member has a key (the FRESH row that made it one is a representative): a bound, not a case
            r = from;
            s = nn_unimage((unsigned)(k >> 32));
        }
    }
    rep[i] = r;
    sim[i] = s;
    if (r >= 0) atomicAdd(size + r, 1ull);
}

__global__ __launch_bounds__(256) void rp_summarise_kernel(int64_t n, const int64_t* __restrict__ rep, const unsigned long long* __restrict__ size,
                                                           int64_t* __restrict__ size_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t r = rep[i];
    size_out[i] = r >= 0 ? (int64_t)size[r] : 0;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

int check_rep_args(const char* fn, const void* rows, int64_t n, float threshold, int metric, const void* rep, const void* sim, const void* size,
                   const void* rounds) {
    const std::string f(fn);
    if (int rc = nn_check_rows(f, n, "rows")) return rc;
    if (int rc = nn_check_threshold(f, threshold)) return rc;
    if (int rc = nn_check_metric(f, metric)) return rc;
    return nn_check_required(f, n == 0 || (rows && rep && sim && size && rounds), "the rows, the three outputs and rounds");
}

// n > 0 rows on the device, in priority order -> the three arrays on the device and the number of rounds.  Enqueued on the ctx's
// stream, which is synchronised once per round (the host reads the undecided count) and twice more.
int rp_run(gnn_ctx* ctx, const char* fn, const float* rows_dev, int64_t n, float threshold, int metric, int64_t* rep, float* sim, int64_t* size,
           int64_t* rounds_out) {
    NeighbourWorkspace& w = ctx->nn;
    RepresentativeWorkspace& p = ctx->rp;
    const int64_t padded = round_up(n, QT);
    int rc = nn_prepare(ctx, rows_dev, n, metric, w.bfrag, w.bvalid);
    if (!rc) rc = nn_reserve(ctx, p.state, (size_t)padded);
    if (!rc) rc = nn_reserve(ctx, p.flag, (size_t)padded);
    if (!rc) rc = nn_reserve(ctx, p.key, (size_t)padded);
    if (!rc) rc = nn_reserve(ctx, p.size, (size_t)padded);
    if (!rc) rc = nn_reserve(ctx, p.row_live, (size_t)(padded / 64));
    if (!rc) rc = nn_reserve(ctx, p.col_live, (size_t)(padded / 32));
    if (!rc) rc = p.count.reserve(ctx, 2);
    const int64_t tiles = padded / QT;
    int64_t split_rows, splits;
    if (!rc) rc = nn_tile_grid(ctx, fn, "rows", tiles, n, &split_rows, &splits);
    if (rc) return rc;
    TileArgs a;
    a.frag = w.bfrag.get();
    a.state = p.state.get();
    a.row_live = p.row_live.get();
    a.col_live = p.col_live.get();
    a.n = n;
    a.split_rows = split_rows;
    a.scale = nn_metric_scale(metric);
    a.threshold = threshold;
    a.flag = p.flag.get();
    a.key = p.key.get();
    p.rounds.begin();
    unsigned long long undecided = 0, members = 0;
    {
        ProfScope prof(ctx, GNN_K_NEIGHBOURS);
        if ((rc = p.count.zero(ctx, 0, 2))) return rc;
        if ((rc = launch_1d(rp_init_kernel, padded, ctx->stream, n, padded, w.bvalid, p.state, p.flag, p.key, p.size, p.row_live, p.col_live,
                            p.count.dev())))
            return rc;
    }
    if ((rc = p.count.read(ctx, 0, 1, &undecided))) return rc;       // the one synchronise of a round
    // One round per pass.  Ends: the undecided row of smallest rank is decided in every round - nothing undecided precedes it, so it
    // is flagged HIT (a member) or not at all (a representative) -, the count strictly falls and at most n rounds find a row to
    // decide.  The loop is bounded by n + 1 whatever the device answers, and a round that does not lower the count is an error.
    int64_t rounds = 0;
    while (undecided > 0) {
        if (rounds > n) {
            set_error(std::string(fn) + ": " + std::to_string(undecided) + " rows are undecided after " + std::to_string(rounds) + " rounds of " +
                      std::to_string(n) + " rows");
            return GNN_ERR_STATE;
        }
        {
            PassLog::Scope pass(ctx, p.rounds);
            if ((rc = launch_tiles(rp_tile_kernel<false>, tiles, splits, ctx->stream, a))) return rc;
            if ((rc = launch_1d(rp_decide_kernel, padded, ctx->stream, padded, p.state, p.flag, p.row_live, p.col_live, p.count.dev()))) return rc;
        }
        unsigned long long now = 0;
        if ((rc = p.count.read(ctx, 0, 1, &now))) return rc;
        ++rounds;
        p.rounds.settle();
        if (now >= undecided) {
            set_error(std::string(fn) + ": round " + std::to_string(rounds) + " left " + std::to_string(now) + " of " + std::to_string(undecided) +
                      " undecided rows undecided: the count must fall in every round");
            return GNN_ERR_STATE;
        }
        undecided = now;
    }
    if ((rc = p.count.read(ctx, 1, 1, &members))) return rc;
    ProfScope prof(ctx, GNN_K_NEIGHBOURS);
    if (members > 0 && (rc = launch_tiles(rp_tile_kernel<true>, tiles, splits, ctx->stream, a))) return rc;
    if ((rc = launch_1d(rp_finish_kernel, n, ctx->stream, n, p.state, p.key, p.size, rep, sim))) return rc;
    if ((rc = launch_1d(rp_summarise_kernel, n, ctx->stream, n, rep, p.size, size))) return rc;
    *rounds_out = rounds;
    return GNN_OK;
}

}  // namespace
}  // namespace gnn

using namespace gnn;

extern "C" int gnn_representatives_dev(gnn_ctx* ctx, const float* rows_dev, int64_t n, float threshold, int metric, int64_t* rep_dev,
                                       float* sim_dev, int64_t* size_dev, int64_t* rounds_host) {
    const char* const fn = "gnn_representatives_dev";
    if (int rc = check_rep_args(fn, rows_dev, n, threshold, metric, rep_dev, sim_dev, size_dev, rounds_host)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (n == 0) {
        if (rounds_host) *rounds_host = 0;
        return GNN_OK;
    }
    return rp_run(ctx, fn, rows_dev, n, threshold, metric, rep_dev, sim_dev, size_dev, rounds_host);
}

extern "C" int gnn_representatives(gnn_ctx* ctx, const float* rows_host, int64_t n, float threshold, int metric, int64_t* rep_host,
                                   float* sim_host, int64_t* size_host, int64_t* rounds_host) {
    const char* const fn = "gnn_representatives";
    if (int rc = check_rep_args(fn, rows_host, n, threshold, metric, rep_host, sim_host, size_host, rounds_host)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    if (n == 0) {
        if (rounds_host) *rounds_host = 0;
        return GNN_OK;
    }
    NeighbourWorkspace& w = ctx->nn;
    RepresentativeWorkspace& p = ctx->rp;
    Landing land(p.d_out);
    const int rep = land.add(rep_host, n), sim = land.add(sim_host, n), size = land.add(size_host, n);
    int rc = land.reserve(ctx);                               // both buffers stand before the copy is enqueued
    if (!rc) rc = nn_upload_rows(ctx, rows_host, n);
    if (!rc) rc = rp_run(ctx, fn, w.d_base, n, threshold, metric, land.dev<int64_t>(rep), land.dev<float>(sim), land.dev<int64_t>(size), rounds_host);
    return rc ? rc : land.copy_out(ctx);
}

extern "C" int gnn_debug_representative_round_ms(gnn_ctx* ctx, double* ms_out, int64_t capacity, int64_t* n_out) {
    if (int rc = check_ctx(ctx)) return rc;
    return ctx->rp.rounds.out(ctx, "gnn_debug_representative_round_ms", ms_out, capacity, n_out);
}
