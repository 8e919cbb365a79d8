// What the searches over encoder embeddings share (gnn_neighbours.hip, gnn_clusters.hip, gnn_representatives.hip, gnn_linkage.hip): the
// fragment layout and its constants, the prepare kernel and its launcher, the fragment loads and the three-product MFMA step, the
// split of the base over workgroups, the union-find.  All of them run the same k-steps in the same order on the same fragments: a
// pair's f32 value is the same in each.
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
constexpr int64_t SPLIT_MAX = 65280;             // base rows per workgroup at the most: a neighbour list entry holds its row as a 16-bit offset

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

static inline int64_t round_up(int64_t n, int64_t m) { return (n + m - 1) / m * m; }

// ---- prepare: grid = padded rows / 32, 256 threads; wave w of a block takes its rows 8 w .. 8 w + 7, lane l the elements
// 8 l .. 8 l + 7 = the 16-byte fragment chunk (k-step l >> 1, half l & 1).  Rows at or beyond n, and invalid rows, become zero
// fragments with flag 0.  Cosine: the row is first scaled by the power of two that brings its largest element into [0.5, 1) - exact,
// and the norm then neither overflows nor vanishes - the squares are summed per lane in element order and over the lanes by a fixed
// butterfly; y = x / norm * 2^8 (the low limbs of a unit row, about 3e-5, would be f16 subnormals; the tile kernel scales the f32
// result back by 2^-16, exactly).
__global__ __launch_bounds__(256) void nn_prepare_kernel(const float* __restrict__ rows, int64_t n, int cosine, uint4* __restrict__ frag,
                                                         uint8_t* __restrict__ valid) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t blk = blockIdx.x;
    for (int i = 0; i < 8; ++i) {
        const int rb = wave * 8 + i;
        const int64_t row = blk * 32 + rb;
        float x[8];
        bool finite = true;
        float amax = 0.f;
        if (row < n) {
            const float4* src = reinterpret_cast<const float4*>(rows + row * D) + lane * 2;
            const float4 a = src[0], b = src[1];
            x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                finite = finite && fabsf(x[e]) <= 3.4028234663852886e38f;      // false for Inf and for NaN
                amax = fmaxf(amax, fabsf(x[e]));
            }
        } else {
            finite = false;
        }
        bool ok = __all(finite);
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) amax = fmaxf(amax, __shfl_xor(amax, s));
        if (cosine) {
            ok = ok && amax > 0.f;
            if (ok) {
                int ex;
                (void)frexpf(amax, &ex);
                float ss = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    x[e] = ldexpf(x[e], -ex);
                    ss += x[e] * x[e];
                }
#pragma unroll
                for (int s = 32; s > 0; s >>= 1) ss += __shfl_xor(ss, s);
                const float norm = sqrtf(ss);
#pragma unroll
                for (int e = 0; e < 8; ++e) x[e] = x[e] / norm * 256.f;
            }
        }
        f16x8 hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = ok ? x[e] : 0.f;
            hi[e] = (_Float16)v;
            lo[e] = (_Float16)(v - (float)hi[e]);
        }
        uint4* dst = frag + (blk * NKS + (lane >> 1)) * 2 * 64 + (lane & 1) * 32 + rb;
        dst[0] = __builtin_bit_cast(uint4, hi);
        dst[64] = __builtin_bit_cast(uint4, lo);
        if (lane == 0) valid[row] = ok ? 1 : 0;
    }
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

// ---- the union-find of the clusters and of the single-linkage tree (gnn_clusters.hip, gnn_linkage.hip): parent[] is int32 in global
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

// a buffer that grows is freed first: nothing enqueued may still read it
template <typename Tp>
int nn_reserve(gnn_ctx* ctx, DevBuf<Tp>& b, size_t need) {
    if (b.capacity() >= need) return GNN_OK;
    GNN_HIP(hipStreamSynchronize(ctx->stream));
    return reserve_roomy(b, need);
}

// rows_dev[n][512] -> fragments and flags of round_up(n, 64) rows
int nn_prepare(gnn_ctx* ctx, const float* rows_dev, int64_t n, int metric, DevBuf<uint4>& frag, DevBuf<uint8_t>& valid) {
    const int64_t padded = round_up(n, QT);
    int rc = nn_reserve(ctx, frag, (size_t)(padded / 32 * BLK_U4));
    if (!rc) rc = nn_reserve(ctx, valid, (size_t)padded);
    if (rc) return rc;
    if (padded == 0) return GNN_OK;
    ProfScope prof(ctx, GNN_K_NEIGHBOURS);
    hipLaunchKernelGGL(nn_prepare_kernel, dim3((unsigned)(padded / 32)), dim3(256), 0, ctx->stream, rows_dev, n, metric == GNN_KNN_COSINE,
                       frag.get(), valid.get());
    GNN_HIP(hipGetLastError());
    return GNN_OK;
}

// base rows per workgroup: the debug value, or what gives every CU two workgroups; a multiple of 32 in [32, SPLIT_MAX]
int64_t nn_split_rows(const gnn_ctx* ctx, int64_t tiles, int64_t nb) {
    int64_t rows = ctx->nn.split;
    if (rows <= 0) {
        const int64_t want = std::max<int64_t>(1, (2 * std::max(ctx->cu_count, 1) + tiles - 1) / tiles);
        rows = std::max<int64_t>(STEP, (nb + want - 1) / want);
    }
    return std::min(round_up(rows, 32), SPLIT_MAX);
}

}  // namespace
}  // namespace gnn
