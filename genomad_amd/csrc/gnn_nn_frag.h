// What the device code of the searches over encoder embeddings shares (gnn_neighbours.hip, gnn_clusters.hip, gnn_density.hip,
// gnn_representatives.hip, gnn_linkage.hip, gnn_graph.hip).  All of them run the same k-steps in the same order on the same fragments: a pair's f32 value is the same in each,
// because the steps below exist once.
//   the fragment layout and its constants
//   the parts of a tile kernel, in the order a kernel calls them: nn_copy_tile (the tile's fragments into LDS), nn_tile_range (the
//   workgroup's base range, plain or upper triangle), nn_step_column (a wave's column block of a step, twice), NN_PRODUCTS (the clear
//   and the double-buffered k-loop over nn_load_b and nn_mfma), nn_acc_row (accumulator register -> tile row).  What lies between them
//   - probes, fetches one step ahead, skip rules, barriers, epilogues - is each kernel's own
//   the keys of the integer maxima: nn_image / nn_unimage (f32 <-> u32, order-preserving), nn_key / nn_key_index; a key crosses
//   lanes with HIP's own 64-bit __shfl_xor
//   the union-find: cl_peek, cl_join, nn_root
//   nn_reserve, the one host-side piece that is a template
// The prepare kernel and the host-side prologue (nn_prepare, nn_tile_grid, nn_upload_rows, ...) are compiled once, in
// gnn_neighbours.hip, and declared in gnn_nn_host.h with the rest of what the host code shares.
#pragma once
#include <cmath>

#include "gnn_common.h"

namespace gnn {
namespace {

constexpr int D = GNN_EMBED_DIM;
constexpr int NKS = D / 16;                      // 32 k-steps of a 32x32x16 MFMA
constexpr int QT = 64;                           // query rows per workgroup: two 32-row blocks
constexpr int STEP = 256;                        // base columns per step: 4 waves x two 32-column blocks
constexpr int64_t BLK_U4 = (int64_t)NKS * 2 * 64;   // uint4 per 32-row block of fragments: [k-step 32][hi | lo][lane 64] = 64 KB

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

static inline int64_t round_up(int64_t n, int64_t m) { return (n + m - 1) / m * m; }

// ---- the parts of a tile kernel: grid = (row tiles, base ranges), 256 threads, `uint4 qs[2 * BLK_U4]` in LDS ------------------------

// the fragments of the workgroup's 64 rows (tile blockIdx.x of `frag`) into LDS; the caller's barrier follows
__device__ __forceinline__ void nn_copy_tile(uint4* qs, const uint4* frag, int tid) {
    const uint4* src = frag + (int64_t)blockIdx.x * 2 * BLK_U4;
    for (int i = tid; i < 2 * BLK_U4; i += 256) qs[i] = src[i];
}

struct TileRange {
    int64_t r0;                // the tile's first row
    int64_t b0, b1;            // the workgroup's columns [b0, b1): range blockIdx.y of `split_rows` (a multiple of 32) columns, cut at n
    int64_t c0;                // where the first step begins
    // the 32-column block that holds column b1 - 1; taken behind the early exit, where the compiler knows b1 > 1 and shifts
    __device__ __forceinline__ int64_t last_blk() const { return (b1 - 1) / 32; }
};

// Returns false when the workgroup has nothing to do (the same answer in every thread: the whole workgroup leaves).  Plain: never, the
// host launches no empty range.  upper (the pairs row < col only): no column of the range lies right of the tile's first row;
// otherwise the first step begins at the 32-column block that holds the tile's first row (r0 and b0 are multiples of 32) - a pair's
// value depends on its two rows only, so where a step begins changes nothing.
__device__ __forceinline__ bool nn_tile_range(TileRange& t, int64_t split_rows, int64_t n, bool upper) {
    t.r0 = (int64_t)blockIdx.x * QT;
    t.b0 = (int64_t)blockIdx.y * split_rows;
    t.b1 = min(n, t.b0 + split_rows);
    t.c0 = upper ? max(t.b0, t.r0) : t.b0;
    return !upper || t.b1 > t.r0 + 1;
}

// The step at column c0: wave w takes the 32-column blocks 2 w and 2 w + 1 of its eight, a lane the column lane & 31 of either.
__device__ __forceinline__ int64_t nn_step_blk(int64_t c0, int wave, int nb) { return c0 / 32 + wave * 2 + nb; }
__device__ __forceinline__ int64_t nn_blk_col(int64_t blk, int lane) { return blk * 32 + (lane & 31); }

// Column block nb of the wave.  bp: where the lane reads the block's fragments - a block beyond the range reads the range's last block.
// Returns the lane's column, which may lie at or beyond b1: the caller masks it by its own rule.
__device__ __forceinline__ int64_t nn_step_column(const uint4* frag, int64_t c0, int wave, int lane, int nb, int64_t last_blk, const uint4*& bp) {
    const int64_t blk = nn_step_blk(c0, wave, nb);
    bp = frag + min(blk, last_blk) * BLK_U4 + lane;
    return nn_blk_col(blk, lane);
}

struct BFrag {
    uint4 v[2][2];             // [column block][hi, lo]
};

__device__ __forceinline__ void nn_load_b(BFrag& b, const uint4* const (&bp)[2], int ks) {
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        b.v[nb][0] = bp[nb][ks * 128];
        b.v[nb][1] = bp[nb][ks * 128 + 64];
    }
}

// the three products of one k-step, in the order of logits_mfma_kernel: hi.lo, lo.hi, hi.hi
__device__ __forceinline__ void nn_mfma(const uint4* qs, int ks, int lane, const BFrag& b, f32x16 (&acc)[2][2]) {
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
        const f16x8 ah = __builtin_bit_cast(f16x8, qs[((mb * NKS + ks) * 2) * 64 + lane]);
        const f16x8 al = __builtin_bit_cast(f16x8, qs[((mb * NKS + ks) * 2 + 1) * 64 + lane]);
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const f16x8 bh = __builtin_bit_cast(f16x8, b.v[nb][0]);
            const f16x8 bl = __builtin_bit_cast(f16x8, b.v[nb][1]);
            acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc[mb][nb], 0, 0, 0);
            acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc[mb][nb], 0, 0, 0);
            acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[mb][nb], 0, 0, 0);
        }
    }
}

// A step's products: acc[row block][column block] = the tile's 64 rows x the wave's 64 columns, unscaled, the k-steps in ascending
// order.  This is the one k-loop of the searches: whatever changes here changes every search's values alike.
// A macro, not a function: the compiler optimises a function's loop on its own before it inlines it, the blocks then reach the kernel
// in another order, and the kernels get other schedules than with the loop standing in them - the representatives' round kernel
// issued its B loads in the order (block 1, block 0), waited with vmcnt(0) before its first MFMA and ran 2.6 % slower per round.  As a
// macro the loop is compiled where it stands: that kernel is byte for byte what it was (profiles/nn_skeleton/README.md).
// qs: the tile's fragments in LDS; bp: const uint4* [2] of nn_step_column; acc: f32x16 [2][2], cleared here.
#define NN_PRODUCTS(qs, bp, lane, acc)                                                                                         \
    do {                                                                                                                       \
        _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_)                                                                       \
            _Pragma("unroll") for (int j_ = 0; j_ < 2; ++j_)                                                                   \
                _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) acc[i_][j_][r_] = 0.f;                                       \
        BFrag f0_, f1_;                                                                                                        \
        nn_load_b(f0_, bp, 0);                                                                                                 \
        _Pragma("unroll 1") for (int ks_ = 0; ks_ < NKS; ks_ += 2) { /* k-step ks + 1 is fetched under the MFMAs of ks */      \
            nn_load_b(f1_, bp, ks_ + 1);                                                                                       \
            nn_mfma(qs, ks_, lane, f0_, acc);                                                                                  \
            nn_load_b(f0_, bp, min(ks_ + 2, NKS - 1));                                                                         \
            nn_mfma(qs, ks_ + 1, lane, f1_, acc);                                                                              \
        }                                                                                                                      \
    } while (0)

// C/D layout of a 32x32 product: register r of acc[mb][nb] holds, in the lanes of half-wave `half` (= lane >> 5), the tile row below
// at the column lane & 31 of column block nb.
__device__ __forceinline__ int nn_acc_row(int mb, int r, int half) { return mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * half; }

// ---- the keys of the integer maxima ----------------------------------------------------------------------------------------------
// s (not a NaN) -> a u32 > 0 that orders as s does, and back; -0 counts as +0.  The linkage host code un-images on the CPU.
// `s + 0.f` turns -0 into +0 and must leave every other value as it is: that holds only while f32 denormals are NOT flushed (the
// default for gfx950, and build.sh sets neither fast-math nor a flush).  Under a flush a denormal similarity would come back as 0.
__host__ __device__ __forceinline__ unsigned nn_image(float s) {
    const unsigned u = __builtin_bit_cast(unsigned, s + 0.f);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__host__ __device__ __forceinline__ float nn_unimage(unsigned v) {
    return __builtin_bit_cast(float, v ^ ((v >> 31) ? 0x80000000u : 0xffffffffu));
}

// (hi, index) -> a key whose maximum is the largest hi and, among equals, the smallest index; 0 is no key wherever hi > 0
constexpr unsigned long long LOW32 = 0xffffffffull;
__host__ __device__ __forceinline__ unsigned long long nn_key(unsigned hi, unsigned index) {
    return ((unsigned long long)hi << 32) | (LOW32 - index);
}
__host__ __device__ __forceinline__ unsigned nn_key_index(unsigned long long key) { return (unsigned)(LOW32 - (key & LOW32)); }

// ---- the union-find of the clusters, the density clusters and the single-linkage tree (gnn_clusters.hip, gnn_density.hip,
// gnn_linkage.hip): parent[] is int32 in global
// memory, a link always points to the SMALLER index, a root to itself.
// a load that the compiler neither caches nor hoists; what it returns may still be older than another workgroup's compare-and-swap
__device__ __forceinline__ int cl_peek(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Join the trees of rows a and b; returns a member of the joined tree at or above both (the next edge of the same column starts
// there).  Every value parent[x] ever holds is x or smaller than x, whatever copy of it a load returns.
__device__ __forceinline__ int cl_join(int32_t* parent, int a, int b) {
    // The pre-check: climb both trees with loads.  A stale load returns x itself (the climb stops early) or the one link x ever got:
    // u and v stay members of a's and b's trees, and equal ones prove one tree.  Ends: a step goes to p < u, and u >= 0.
    int u = a, v = b;
    for (;;) {
        const int p = cl_peek(parent + u);
        if (p == u) break;
        u = p;
    }
    for (;;) {
        const int p = cl_peek(parent + v);
        if (p == v) break;
        v = p;
    }
    // The monotone loop.  It acts on the compare-and-swap's own return only.  old == u: u was a root and now points to the smaller
    // v - done.  Otherwise u had the link old < u already, and joining old with v joins the same trees.  Ends: max(u, v) falls with
    // every pass (the larger of the two is replaced by something smaller than itself) and is >= 0; no pass waits for anybody.
    while (u != v) {
        if (u < v) {
            const int t = u;
            u = v;
            v = t;
        }
        const int old = atomicCAS(parent + u, u, v);
        if (old == u) return v;
        u = old;
    }
    return u;
}

// The root of i's tree by plain loads, for a launch of its own behind the one that linked: there they see every link.  Ends: a step
// of the climb goes to p < r, and r >= 0.
__device__ __forceinline__ int nn_root(const int32_t* __restrict__ parent, int i) {
    int r = i;
    for (;;) {
        const int p = parent[r];
        if (p == r) break;
        r = p;
    }
    return r;
}

// a buffer that grows is freed first: nothing enqueued may still read it
template <typename Tp>
int nn_reserve(gnn_ctx* ctx, DevBuf<Tp>& b, size_t need) {
    if (b.capacity() >= need) return GNN_OK;
    GNN_HIP(hipStreamSynchronize(ctx->stream));
    return reserve_roomy(b, need);
}

}  // namespace
}  // namespace gnn
