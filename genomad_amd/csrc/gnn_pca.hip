// Principal components among encoder embeddings (include/genomad_nn.h, "principal components"): the second
// moments of the unit rows and the projection of rows onto directions, on the device.  The 512 x 512 eigenproblem between them is the
// host's (sequence.pca_from_moments): the matrix is 2 MB whatever n is.
//   prepare    nn_prepare (gnn_neighbours.hip), as it is: the rows' fragments and flags in the neighbour search's buffers, the
//              components' (<= 64 f32 directions) in this file's own.  x_i = (float)hi + (float)lo of row i's fragments is its unit
//              vector times 2^8, exact in f32; an invalid or padded row is a zero fragment and contributes nothing anywhere below.
//   sums       S[d] += q_i[d] in int64, q_i = (hi + lo) * 2^24: the k-means update's arithmetic with one group.  A wave keeps its rows'
//              sums in registers, a workgroup adds them in LDS and ends with one 64-bit add per element.
//   gram       G[a][b] = sum_i x_i[a] x_i[b], a contraction over the ROWS: the k index of the matrix instruction is the row, so the
//              fragment layout (8 consecutive features of a row per lane) is the wrong way round for the 16-bit MFMAs and the f32-input
//              v_mfma_f32_32x32x2_f32 the right way round - lane l holds x[row l >> 5][feature l & 31] for both operands.  grid = (the
//              10 pairs ba <= bb of 128-feature blocks, row ranges), a wave owns 64 x 64 of the 128 x 128 block = 4 accumulators.
//              Rows come through LDS as f32 [row][feature], 32 rows (one fragment block) at a time, converted on the way in, the next
//              32 fetched into registers under the products of these.  Rows are taken in granules of 256 ALIGNED TO THE ABSOLUTE ROW
//              INDEX: within a granule the f32 chain runs in ascending row order from zero, at its end the accumulator p becomes the
//              integer llrint((double)p * 2^16) - G is in units of 2^-32 of u_a . u_b - and integers are added from there on: in
//              registers over the workgroup's granules, then one 64-bit atomicAdd per entry and workgroup.  Integer adds commute, so no
//              bit of G depends on the row split (gnn_debug_set_pca_split) or on the order the workgroups run in.  |p * 2^16| <= 2^40
//              per granule: n <= 2^30 rows cannot overflow (N_MAX).
//   mirror     the six blocks below the diagonal from those above it, and the count of the valid rows.  A diagonal block is computed
//              whole: a * b and b * a are the same f32, so it is symmetric bit for bit.
//   project    the tile parts of gnn_nn_frag.h over the plain rectangle rows x components: the tile is 64 rows in LDS, the columns are
//              the components' fragments, the value of (row i, component c) IS the f32 gnn_neighbours returns for query i and base row
//              c.  Stored: that value minus off[c], one f32 subtraction; NaN at an invalid row or component; nothing at or beyond
//              column ncomp.  Only the waves whose column blocks lie below ncomp run the k-loop.
// Atomics are 64-bit integer adds only, stores are vector stores, no loop waits for another workgroup: every loop's termination
// argument stands next to it.  Memory: the 2 MB of G, 4 KB of S, the components' 128 KB of fragments; nothing grows with n but the
// fragments the neighbour search already keeps.
#include "gnn_nn_frag.h"

namespace gnn {
namespace {

constexpr int64_t N_MAX = (int64_t)1 << 30;      // the int64 sums of more rows could overflow, as in gnn_kmeans.hip
constexpr int NCOMP_MAX = 64;
constexpr int GRANULE = 256;                     // rows of one f32 chain
constexpr int FB = 128;                          // features of a block
constexpr int NFB = D / FB;                      // 4 blocks: 10 pairs ba <= bb
constexpr int NPAIR = NFB * (NFB + 1) / 2;
constexpr int CH = 32;                           // rows staged at a time: one block of fragments
constexpr int XS = FB + 4;                       // floats per staged row: 8 consecutive rows' 16-byte stores cover the 32 banks once

// grid = ceil(rows / per_block), 256 threads: wave w takes the block's rows w, w + 4, ...; lane l the elements 8 l .. 8 l + 7.
__global__ __launch_bounds__(256) void pca_sum_kernel(const uint4* __restrict__ frag, int64_t rows, int64_t per_block,
                                                      unsigned long long* __restrict__ S) {
    __shared__ unsigned long long ls[D];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * per_block, i1 = min(rows, i0 + per_block);
    ls[tid] = 0;
    ls[tid + 256] = 0;
    __syncthreads();
    long long s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // Ends: i grows by 4 towards i1.
    for (int64_t i = i0 + wave; i < i1; i += 4) {
        const uint4* p = frag + (i / 32 * NKS + (lane >> 1)) * 128 + (lane & 1) * 32 + (i & 31);
        const f16x8 hi = __builtin_bit_cast(f16x8, p[0]), lo = __builtin_bit_cast(f16x8, p[64]);
#pragma unroll
        for (int e = 0; e < 8; ++e)     // exact: an f16 times 2^24 is an integer below 2^41 in magnitude, and an f32 holds its 11 bits
            s[e] += (long long)((float)hi[e] * 16777216.f) + (long long)((float)lo[e] * 16777216.f);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e)
        if (s[e]) atomicAdd(&ls[e * 64 + lane], (unsigned long long)s[e]);
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int i = tid + h * 256, e = i >> 6, ln = i & 63;
        if (ls[i]) atomicAdd(S + ln * 8 + e, ls[i]);
    }
}

struct GramArgs {
    const uint4* frag;         // the rows' fragments: nblk blocks of 32 rows
    int64_t nblk;
    int64_t split_blk;         // blocks per workgroup: a multiple of 8 (= GRANULE rows)
    unsigned long long* G;     // [D][D] int64, two's complement; the blocks ba <= bb are written here
};

struct GramStage {
    uint4 v[4][2];             // [item][hi, lo]: item j = part j >> 1 (0: the block ba, 1: bb), k-step wave + 4 (j & 1) of its 8
};

// block c's fragments of the workgroup's feature blocks into registers; items: 2 (a diagonal pair: bb is ba) or 4
__device__ __forceinline__ void pca_fetch(GramStage& st, const uint4* frag, int64_t c, int ba, int bb, int items, int wave, int lane) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j >= items) break;
        const uint4* p = frag + (c * NKS + ((j >> 1) ? bb : ba) * 8 + wave + 4 * (j & 1)) * 128 + lane;
        st.v[j][0] = p[0];
        st.v[j][1] = p[64];
    }
}

__global__ __launch_bounds__(256) void pca_gram_kernel(GramArgs a) {
    __shared__ float xs[2][CH][XS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, wm = wave >> 1, wn = wave & 1;
    int ba = 0, bb = blockIdx.x;
    // the pair: 0..3 -> (0, 0..3), 4..6 -> (1, 1..3), 7, 8 -> (2, 2..3), 9 -> (3, 3).  Ends: ba grows towards NFB - 1.
    while (bb >= NFB - ba) {
        bb -= NFB - ba;
        ++ba;
    }
    bb += ba;
    const int items = ba == bb ? 2 : 4;
    const int64_t c0 = (int64_t)blockIdx.y * a.split_blk, c1 = min(a.nblk, c0 + a.split_blk);      // c0 < nblk: the host launches no empty range
    f32x16 acc[2][2];
    long long gi[2][2][16];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc[m][n][r] = 0.f;
                gi[m][n][r] = 0;
            }
    const float* pa = &xs[0][half][wm * 64 + (lane & 31)];
    const float* pb = &xs[ba == bb ? 0 : 1][half][wn * 64 + (lane & 31)];
    GramStage st;
    pca_fetch(st, a.frag, c0, ba, bb, items, wave, lane);
    // Ends: c grows by one towards c1.
    for (int64_t c = c0; c < c1; ++c) {
        __syncthreads();                   // the products of block c - 1 have read xs
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= items) break;
            const f16x8 hi = __builtin_bit_cast(f16x8, st.v[j][0]), lo = __builtin_bit_cast(f16x8, st.v[j][1]);
            float x[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = (float)hi[e] + (float)lo[e];      // exact: hi + lo is the f32 the prologue split
            float4* dst = reinterpret_cast<float4*>(&xs[j >> 1][lane & 31][(wave + 4 * (j & 1)) * 16 + half * 8]);
            dst[0] = make_float4(x[0], x[1], x[2], x[3]);
            dst[1] = make_float4(x[4], x[5], x[6], x[7]);
        }
        __syncthreads();
        if (c + 1 < c1) pca_fetch(st, a.frag, c + 1, ba, bb, items, wave, lane);       // lands under the products below
        // the rows 2 s and 2 s + 1 of the block per instruction, ascending: a k-ordered fmaf chain per entry
#pragma unroll 4
        for (int s = 0; s < CH / 2; ++s) {
            const float a0 = pa[2 * s * XS], a1 = pa[2 * s * XS + 32], b0 = pb[2 * s * XS], b1 = pb[2 * s * XS + 32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        // the granule's end (c0 is a multiple of 8, so c & 7 counts absolute rows) or the range's: the chain becomes an integer
        if ((c & 7) == 7 || c + 1 == c1) {
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int n = 0; n < 2; ++n)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        gi[m][n][r] += llrint((double)acc[m][n][r] * 65536.0);
                        acc[m][n][r] = 0.f;
                    }
        }
    }
    // C/D layout: register r holds the A index nn_acc_row(m, r, half) and the B index lane & 31
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int fa = ba * FB + wm * 64 + nn_acc_row(m, r, half), fb = bb * FB + wn * 64 + n * 32 + (lane & 31);
                if (gi[m][n][r]) atomicAdd(a.G + fa * D + fb, (unsigned long long)gi[m][n][r]);
            }
}

// cells = max(n, 6 blocks x 128 x 128): G[b][a] = G[a][b] for the blocks ba < bb, and *n_valid += the valid rows.  Every thread
// reaches the ballot.
__global__ __launch_bounds__(256) void pca_mirror_kernel(unsigned long long* __restrict__ G, int64_t n, const uint8_t* __restrict__ valid,
                                                         unsigned long long* __restrict__ n_valid) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (NPAIR - NFB) * FB * FB) {
        int ba = 0, bb = (int)(i / (FB * FB));
        // the pair: 0..2 -> (0, 1..3), 3, 4 -> (1, 2..3), 5 -> (2, 3).  Ends: ba grows towards NFB - 2.
        while (bb >= NFB - 1 - ba) {
            bb -= NFB - 1 - ba;
            ++ba;
        }
        bb += ba + 1;
        const int x = (int)(i / FB) % FB, y = (int)(i % FB);
        G[(bb * FB + y) * D + ba * FB + x] = G[(ba * FB + x) * D + bb * FB + y];
    }
    const int ok = __popcll(__ballot(i < n && valid[i]));
    if ((threadIdx.x & 63) == 0 && ok) atomicAdd(n_valid, (unsigned long long)ok);
}

struct ProjectArgs {
    const uint4* frag;         // the rows: round_up(n, 64) / 32 blocks
    const uint8_t* valid;      // [round_up(n, 64)]
    int64_t n;
    const uint4* cfrag;        // the components: 2 blocks
    const uint8_t* cvalid;     // [64]
    int ncomp;
    float scale;               // 2^-16: cosine
    const float* off;          // [ncomp], or NULL: 0
    float* out;                // [n][ncomp]
};

// grid = row tiles, 256 threads.  LDS: the tile's fragments 128 KB and its rows' flags.
__global__ __launch_bounds__(256) void pca_project_kernel(ProjectArgs a) {
    __shared__ uint4 qs[2 * BLK_U4];
    __shared__ uint8_t lok[QT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
    TileRange t;
    nn_tile_range(t, STEP, a.ncomp, false);                // one range: the columns [0, ncomp)
    nn_copy_tile(qs, a.frag, tid);
    if (tid < QT) lok[tid] = t.r0 + tid < a.n && a.valid[t.r0 + tid];
    __syncthreads();
    if (nn_blk_col(nn_step_blk(t.c0, wave, 0), 0) >= t.b1) return;       // the wave's columns lie beyond ncomp; no barrier follows
    const int64_t last_blk = t.last_blk();
    const uint4* bp[2];
    int64_t col[2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) col[nb] = nn_step_column(a.cfrag, t.c0, wave, lane, nb, last_blk, bp[nb]);
    f32x16 acc[2][2];
    NN_PRODUCTS(qs, bp, lane, acc);
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        if (col[nb] >= t.b1) continue;                     // a padded column is never stored
        const bool cok = a.cvalid[col[nb]];
        const float o = a.off ? a.off[col[nb]] : 0.f;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = nn_acc_row(mb, r, half);
                if (t.r0 + row >= a.n) continue;
                const float s = __fmul_rn(acc[mb][nb][r], a.scale);
                a.out[(t.r0 + row) * a.ncomp + col[nb]] = lok[row] && cok ? (a.off ? __fsub_rn(s, o) : s) : __builtin_nanf("");
            }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

int check_rows(const std::string& f, int64_t n) {
    if (n >= 1 && n <= N_MAX) return GNN_OK;
    set_error(f + ": " + std::to_string(n) + " rows is outside [1, 2^30]: the int64 sums of more rows could overflow");
    return GNN_ERR_ARG;
}

int check_moments_args(const char* fn, const void* rows, int64_t n, const void* G, const void* S, const void* n_valid) {
    const std::string f(fn);
    if (int rc = check_rows(f, n)) return rc;
    return nn_check_required(f, rows && G && S && n_valid, "the rows and the three outputs");
}

int check_project_args(const char* fn, const void* rows, int64_t n, const void* comp, int ncomp, const void* out) {
    const std::string f(fn);
    if (int rc = check_rows(f, n)) return rc;
    if (ncomp < 1 || ncomp > NCOMP_MAX) {
        set_error(f + ": " + std::to_string(ncomp) + " components is outside [1, " + std::to_string(NCOMP_MAX) + "]");
        return GNN_ERR_ARG;
    }
    return nn_check_required(f, rows && comp && out, "the rows, the components and the output");
}

// n >= 1 rows on the device -> G, S and n_valid on the device, enqueued
int pca_moments(gnn_ctx* ctx, const char* fn, const float* rows_dev, int64_t n, int64_t* G, int64_t* S, int64_t* n_valid) {
    NeighbourWorkspace& w = ctx->nn;
    PCAWorkspace& p = ctx->pca;
    p.passes.begin();
    const int64_t granules = (n + GRANULE - 1) / GRANULE;
    int64_t per = p.split / GRANULE;       // granules per workgroup
    if (per <= 0) {
        const int64_t want = std::max<int64_t>(1, (2 * std::max(ctx->cu_count, 1) + NPAIR - 1) / NPAIR);     // every CU about two workgroups
        per = (granules + want - 1) / want;
    }
    const int64_t ranges = (granules + per - 1) / per;
    if (ranges > 65535) {
        set_error(std::string(fn) + ": " + std::to_string(n) + " rows in ranges of " + std::to_string(per * GRANULE) + " are more than 65535 ranges");
        return GNN_ERR_ARG;
    }
    {
        PassLog::Scope pass(ctx, p.passes);
        if (int rc = nn_prepare(ctx, rows_dev, n, GNN_KNN_COSINE, w.bfrag, w.bvalid)) return rc;
    }
    const int64_t padded = round_up(n, QT);
    unsigned long long* const Gu = reinterpret_cast<unsigned long long*>(G);
    unsigned long long* const Su = reinterpret_cast<unsigned long long*>(S);
    {
        PassLog::Scope pass(ctx, p.passes);
        GNN_HIP(hipMemsetAsync(S, 0, (size_t)D * sizeof(int64_t), ctx->stream));
        const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((padded + 63) / 64, 2 * std::max(ctx->cu_count, 1)));
        const int64_t per_block = (padded + blocks - 1) / blocks;
        hipLaunchKernelGGL(pca_sum_kernel, dim3((unsigned)((padded + per_block - 1) / per_block)), dim3(256), 0, ctx->stream, w.bfrag.get(), padded,
                           per_block, Su);
        GNN_HIP(hipGetLastError());
    }
    {
        PassLog::Scope pass(ctx, p.passes);
        GNN_HIP(hipMemsetAsync(G, 0, (size_t)D * D * sizeof(int64_t), ctx->stream));
        GramArgs a;
        a.frag = w.bfrag.get();
        a.nblk = padded / 32;              // the blocks the prologue wrote: nothing beyond them is read
        a.split_blk = per * (GRANULE / CH);
        a.G = Gu;
        hipLaunchKernelGGL(pca_gram_kernel, dim3(NPAIR, (unsigned)ranges), dim3(256), 0, ctx->stream, a);
        GNN_HIP(hipGetLastError());
    }
    PassLog::Scope pass(ctx, p.passes);
    GNN_HIP(hipMemsetAsync(n_valid, 0, sizeof(int64_t), ctx->stream));
    return launch_1d(pca_mirror_kernel, std::max<int64_t>(n, (int64_t)(NPAIR - NFB) * FB * FB), ctx->stream, Gu, n, w.bvalid.get(),
                     reinterpret_cast<unsigned long long*>(n_valid));
}

// n >= 1 rows and ncomp directions on the device -> out[n][ncomp] on the device, enqueued
int pca_project(gnn_ctx* ctx, const float* rows_dev, int64_t n, const float* comp_dev, int ncomp, const float* off_dev, float* out) {
    NeighbourWorkspace& w = ctx->nn;
    PCAWorkspace& p = ctx->pca;
    p.passes.begin();
    {
        PassLog::Scope pass(ctx, p.passes);
        if (int rc = nn_prepare(ctx, rows_dev, n, GNN_KNN_COSINE, w.bfrag, w.bvalid)) return rc;
    }
    {
        PassLog::Scope pass(ctx, p.passes);
        if (int rc = nn_prepare(ctx, comp_dev, ncomp, GNN_KNN_COSINE, p.cfrag, p.cvalid)) return rc;
    }
    PassLog::Scope pass(ctx, p.passes);
    ProjectArgs a;
    a.frag = w.bfrag.get();
    a.valid = w.bvalid.get();
    a.n = n;
    a.cfrag = p.cfrag.get();
    a.cvalid = p.cvalid.get();
    a.ncomp = ncomp;
    a.scale = nn_metric_scale(GNN_KNN_COSINE);
    a.off = off_dev;
    a.out = out;
    return launch_tiles(pca_project_kernel, (n + QT - 1) / QT, 1, ctx->stream, a);
}

}  // namespace
}  // namespace gnn

using namespace gnn;

extern "C" int gnn_pca_moments_dev(gnn_ctx* ctx, const float* rows_dev, int64_t n, int64_t* G_dev, int64_t* S_dev, int64_t* n_valid_dev) {
    const char* const fn = "gnn_pca_moments_dev";
    if (int rc = check_moments_args(fn, rows_dev, n, G_dev, S_dev, n_valid_dev)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    return pca_moments(ctx, fn, rows_dev, n, G_dev, S_dev, n_valid_dev);
}

extern "C" int gnn_pca_moments(gnn_ctx* ctx, const float* rows_host, int64_t n, int64_t* G_host, int64_t* S_host, int64_t* n_valid_host) {
    const char* const fn = "gnn_pca_moments";
    if (int rc = check_moments_args(fn, rows_host, n, G_host, S_host, n_valid_host)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    PCAWorkspace& p = ctx->pca;
    Landing land(p.d_out);
    const int G = land.add(G_host, D * D), S = land.add(S_host, D), n_valid = land.add(n_valid_host, 1);
    int rc = land.reserve(ctx);                               // both buffers stand before a copy is enqueued
    if (!rc) rc = nn_upload_rows(ctx, rows_host, n);
    if (!rc) rc = pca_moments(ctx, fn, ctx->nn.d_base, n, land.dev<int64_t>(G), land.dev<int64_t>(S), land.dev<int64_t>(n_valid));
    if (!rc) rc = land.copy_out(ctx);
    if (!rc) p.passes.settle();
    return rc;
}

extern "C" int gnn_pca_project_dev(gnn_ctx* ctx, const float* rows_dev, int64_t n, const float* components_dev, int ncomp,
                                   const float* off_dev_or_null, float* out_dev) {
    if (int rc = check_project_args("gnn_pca_project_dev", rows_dev, n, components_dev, ncomp, out_dev)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    return pca_project(ctx, rows_dev, n, components_dev, ncomp, off_dev_or_null, out_dev);
}

extern "C" int gnn_pca_project(gnn_ctx* ctx, const float* rows_host, int64_t n, const float* components_host, int ncomp,
                               const float* off_host_or_null, float* out_host) {
    if (int rc = check_project_args("gnn_pca_project", rows_host, n, components_host, ncomp, out_host)) return rc;
    if (int rc = check_ctx(ctx)) return rc;
    PCAWorkspace& p = ctx->pca;
    // [components ncomp x 512 | off ncomp]; every buffer stands before a copy is enqueued
    Landing land(p.d_out);
    land.add(out_host, n * ncomp);
    int rc = nn_reserve(ctx, p.d_comp, (size_t)(NCOMP_MAX * D + NCOMP_MAX));
    if (!rc) rc = land.reserve(ctx);
    if (!rc) rc = nn_upload_rows(ctx, rows_host, n);
    if (rc) return rc;
    float* const off = p.d_comp.get() + NCOMP_MAX * D;
    GNN_HIP(hipMemcpyAsync(p.d_comp.get(), components_host, (size_t)ncomp * D * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    if (off_host_or_null) GNN_HIP(hipMemcpyAsync(off, off_host_or_null, (size_t)ncomp * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    rc = pca_project(ctx, ctx->nn.d_base, n, p.d_comp.get(), ncomp, off_host_or_null ? off : nullptr, land.dev<float>(0));
    if (!rc) rc = land.copy_out(ctx);
    if (!rc) p.passes.settle();
    return rc;
}

extern "C" int gnn_debug_set_pca_split(gnn_ctx* ctx, int64_t rows_per_workgroup) {
    if (int rc = check_ctx(ctx)) return rc;
    if (rows_per_workgroup < 0 || rows_per_workgroup % GRANULE) {
        set_error("gnn_debug_set_pca_split: " + std::to_string(rows_per_workgroup) + " rows per workgroup is not a multiple of " +
                  std::to_string(GRANULE) + " in [0, 2^63) (0 = the library's choice)");
        return GNN_ERR_ARG;
    }
    ctx->pca.split = rows_per_workgroup;
    return GNN_OK;
}

extern "C" int gnn_debug_pca_pass_ms(gnn_ctx* ctx, double* ms_out, int64_t capacity, int64_t* n_out) {
    if (int rc = check_ctx(ctx)) return rc;
    return ctx->pca.passes.out(ctx, "gnn_debug_pca_pass_ms", ms_out, capacity, n_out);
}
