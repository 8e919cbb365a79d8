// Shared declarations of libgenomad_nn_hip.so (host side + kernel launchers).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/genomad_nn.h"
#include "gnn_devmem.h"

namespace gnn {

constexpr int W = GNN_WINDOW;
constexpr int T = GNN_TOKENS;
constexpr int C = GNN_CH;
constexpr int KS = GNN_KSIZE;
constexpr int NP = GNN_PATCHES;
constexpr int PS = GNN_PATCH_SIZE;
constexpr int NPAIR = NP * PS;            // 8400 (patch, slot) pairs per head
constexpr int POOLED = GNN_POOLED;
constexpr int FEAT = GNN_FEAT;
constexpr int HID = GNN_HIDDEN;
constexpr float LRELU = 0.1f;             // igloo.py:48
constexpr float BN_EPS = 1e-3f;           // Keras BatchNormalization default

// ---- fused front end geometry (gnn_fused_x3.hip, gnn_fused_c6.hip) ----
constexpr int FT = 128;                   // rows (token positions) per step of a workgroup
constexpr int FSTEPS = (T + FT - 1) / FT; // 47 steps per window
// rows of a conv1 pair table: 1024 five-mers | 256 (N, 4-mer) | 256 (4-mer, N) | (N, N) | (absent,
// absent) | 257 (absent, token) — see pair_row() in gnn_fused.hip
constexpr int PAIR_ROWS = 1024 + 256 + 256 + 1 + 1 + 257;   // 1795
// logits GEMM on the matrix pipe (gnn_backend.hip): K = 2100 patches padded to k-steps of 16,
// N = 749 pooled positions padded to n-blocks of 32
constexpr int QK_KSTEPS = (NP + 15) / 16;        // 132
constexpr int QK_NBLK = (POOLED + 31) / 32;      // 24

void set_error(const std::string& msg);
bool debug_switch(const char* name);   // gnn_api.hip: environment switch read once, announced on stderr when set

#define GNN_HIP(call)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            gnn::set_error(std::string(#call) + " failed: " + hipGetErrorString(e_));          \
            return GNN_ERR_HIP;                                                                \
        }                                                                                      \
    } while (0)

// Device-resident, re-packed weights.  The raw pointers are views of allocations ctx->owned keeps (upload() below); what is
// allocated without a host image (the all-N constants, WvaTable, the k-mer tables) is a buffer of its own.
struct DeviceWeights {
    // f32 reference layouts
    float* conv1_k = nullptr;   // (6,257,128)
    float* conv1_b = nullptr;
    float* conv_k[2] = {nullptr, nullptr};   // conv2, conv3 (6,128,128)
    float* conv_b[2] = {nullptr, nullptr};
    // IGLOO (patch, slot) pairs, SORTED BY POSITION ("bucket order"): entry e of head h reads
    // activation row pos_sorted[e] and weights weff_sorted[e,:]; pair p*4+j lives at e = slot[p*4+j].
    // bucket_ptr[s] .. bucket_ptr[s+1] are the entries whose position falls into fused step s.
    float* weff_sorted[2] = {nullptr, nullptr};    // (8400,128)  w_mult * w_summer folded
    int32_t* pos_sorted[2] = {nullptr, nullptr};   // (8400,)
    int32_t* slot[2] = {nullptr, nullptr};         // (8400,) pair -> entry
    int32_t* bucket_ptr[2] = {nullptr, nullptr};   // (FSTEPS+1,)
    float* conv1_pairs = nullptr;  // (3, PAIR_ROWS, 128): W1[2j][a] + W1[2j+1][b] per token pair
    float* w_bias[2] = {nullptr, nullptr};   // (2100,)
    float* w_qk[2] = {nullptr, nullptr};     // (2100,749)
    float* w_v[2] = {nullptr, nullptr};      // (128,128) [in][out]
    float* d1_k = nullptr;  // (256,512) BN folded
    float* d1_b = nullptr;
    float* d2_k = nullptr;  // (512,512) BN folded
    float* d2_b = nullptr;
    float* d3_k = nullptr;  // (512,3)
    float* d3_b = nullptr;
    uint16_t* d1_frag = nullptr;   // BN-folded Dense512 kernels in MFMA fragment order, f16 hi / lo (dense_mfma_kernel):
    uint16_t* d2_frag = nullptr;   // [kstep][nblk 16][plane 2][lane 64][8]
    // fused path packs (gnn_pack.hip): MFMA fragment order, bf16 hi / lo planes
    uint16_t* conv_frag[2] = {nullptr, nullptr};  // conv2, conv3: [kstep 48][nblk 4][plane 2][lane 64][8]
    uint16_t* wv_frag[2] = {nullptr, nullptr};    // head A, B:   [kstep 8][nblk 4][plane 2][lane 64][8]
    uint16_t* wqk_frag[2] = {nullptr, nullptr};   // head A, B:   [kstep 132][nblk 24][plane 2][lane 64][8], zero padded
    uint16_t* wqk_frag_h[2] = {nullptr, nullptr}; // the same with f16 hi / lo limbs (logits GEMM of GNN_PREC_F16X3)
    uint16_t* conv_frag_h[2] = {nullptr, nullptr};   // the same fragment layouts with f16 hi / lo limbs (GNN_PREC_F16X3)
    uint16_t* wv_frag_h[2] = {nullptr, nullptr};
    // f16 + MX-fp6-correction packs (gnn_fused_c6.hip): [k32 step][nblk 4][f16 even 1 KiB | f16 odd 1 KiB | fp6 dwords 0-3 1 KiB |
    // fp6 dwords 4-5 512 B], scale words as above, pair tables in the gather's lane order (bias folded), entry ranges per step
    uint32_t* conv_c6[2] = {nullptr, nullptr};
    uint32_t* wv_c6[2] = {nullptr, nullptr};
    float* conv1_pairs6 = nullptr;
    float* weff6[2] = {nullptr, nullptr};      // folded IGLOO weights, entry pairs x [i 8][entry parity][block 4][4 ch]
    int32_t* bucket_ptr6[2] = {nullptr, nullptr};
    DevBuf<float> c6_yp_const;   // (2, 749, 128) / (2, 8400): the f16c6 kernel's yp and mp of an all-N window (padding skip)
    DevBuf<float> c6_mp_const;
    // Toom-Cook F(3,6) front end (gnn_fused_tc.hip): transformed conv weights [k16 unit 8][xi 8][nblk 4][hi | lo][lane 64][8] f16,
    // the power of two the inverse transform multiplies by, IGLOO entry ranges per 96-row step, all-N window outputs
    uint16_t* tc_frag[2] = {nullptr, nullptr};
    float tc_inv_s[2] = {1.f, 1.f};
    int32_t* bucket_ptr96[2] = {nullptr, nullptr};
    DevBuf<float> tc_yp_const;
    DevBuf<float> tc_mp_const;
    DevBuf<float> tc_wva_tbl;     // head A's y @ w_v per 9-mer: gnn_fused_tc.hip, WvaTable (1.38 GB)
    // k-mer tables of GNN_PREC_F16X3TK (gnn_fused_tk.hip, gnn_build_kmer_tables): x2 per 14-mer (137.4 GB), head A's pair products per
    // (entry, 9-mer) (8.8 GB), that kernel's outputs of an all-N window.  gnn_drop_kmer_tables frees them on their own
    DevBuf<float> tk_x2_tbl;
    DevBuf<float> tk_mpa_tbl;
    DevBuf<float> tk_x1t_tbl;     // x1 over WvaTable's index space (1.38 GB): head A's entries at 9-mers MpaTable has no column for
    DevBuf<float> tk_pt_tbl;      // conv2's six tap tables over WvaTable's index space (8.3 GB): the rows the 14-mer table cannot index
    DevBuf<float> tk_yp_const;
    DevBuf<float> tk_mp_const;
    DevBuf<float> x3_yp_const[2];  // the same of gnn_fused_x3.hip: [0] bf16 limbs, [1] f16 limbs
    DevBuf<float> x3_mp_const[2];
};

struct Workspace {
    int64_t chunk = 0;          // windows per launch
    DevBuf<uint16_t> tokens;    // (chunk, 5997)           f32 path only
    DevBuf<float> x[3];         // (chunk,5997,128) each, f32 path only
    int64_t x_chunk = 0;        // windows the x buffers hold
    DevBuf<float> mp;           // (chunk, 2, 8400) pair dot products in bucket order
    DevBuf<float> m;            // (chunk, 2, 2100)  bias + the four pair products of every patch
    DevBuf<float> yp;           // (chunk, 2, 749, 128)
    DevBuf<float> logits;       // (chunk, 2, 749)
    DevBuf<float> alpha;        // (chunk, 2, 749)   (tap)
    DevBuf<float> feat;         // (chunk, 256)
};

// ---- the contig front end's window rule and persistent buffers (gnn_contigs.hip, gnn_occlude.hip) ----
constexpr int MIN_TAIL = 2500;        // nn_classification.py:68  seq_windows(seq, 6000, 2500, ...)
constexpr int MAX_N = 4000;           // nn_classification.py:70  window_n > 0 and count("N") > 4000 -> skip
constexpr int64_t PIECE = 64ll << 20; // bytes per host->device piece of the sequence buffer

// ---- region calls (gnn_regions.hip): persistent, grow-only; a sibling of the other groups of ContigWorkspace ----
// Per contig 16 B (bin and tile CSR), per tile of `tile` bins 98 B (transfer matrix 72, entry vector 24, composed back pointers 1,
// exit state 1), per bin 1 B (back pointers) - what gnn_region_states_dev needs - and, for gnn_call_regions alone, 14 B per bin (the
// track 12, the states 1, the flags 1), 12 B per 256 bins (the block tables) and 65 B per region.
struct RegionWorkspace {
    int tile = 256;                              // bins per tile (gnn_debug_set_region_tile); no result depends on it
    PinnedBuf<int64_t> h_off;                    // host image of d_off; rewritten only after `tables_read`
    hipEvent_t tables_read = nullptr;            // recorded behind the upload of h_off
    DevBuf<int64_t> d_off;                       // [bin_off (n_contigs + 1) | tile_off (n_contigs + 1)]
    DevBuf<int64_t> d_transfer, d_entry;         // 9 and 3 per tile
    DevBuf<uint8_t> d_comp, d_exit;              // 1 per tile each
    DevBuf<uint8_t> d_psi;                       // 1 per bin
    // gnn_call_regions
    DevBuf<float> d_track;                       // 3 per bin
    DevBuf<uint8_t> d_state, d_flag;             // 1 per bin each
    DevBuf<int32_t> d_blk_count;                 // flags per block of 256 bins
    DevBuf<int64_t> d_blk_off;                   // their exclusive prefix sums, then the total
    DevBuf<int64_t> d_r_contig, d_r_lo, d_r_hi, d_r_evidence, d_r_qsum;      // 1, 1, 1, 1 and 3 per region
    DevBuf<uint8_t> d_r_state;
    ~RegionWorkspace() {
        if (tables_read) (void)hipEventDestroy(tables_read);
    }
};

// ---- interval embeddings (gnn_intervals.hip): persistent, grow-only; a sibling of the other groups of ContigWorkspace ----
// Per interval 16 B (its member range) for gnn_interval_fold_dev, and 1 B per row of ONE slice (the kept flags); gnn_embed_intervals
// adds, per interval, 4 KB for the sums S and U (8 KB under GNN_STRAND_BOTH) and 20 B of score sums, count and coherence, and 12 B
// per window of one slab (the combined scores of BOTH).
struct IntervalWorkspace {
    PinnedBuf<int64_t> h_range;                  // host image of d_range; rewritten only after `tables_read`
    PinnedBuf<uint8_t> h_kept;                   // ... and of d_kept
    hipEvent_t tables_read = nullptr;            // recorded behind their uploads
    DevBuf<int64_t> d_range;                     // [w_lo (n_intervals) | w_hi (n_intervals)]
    DevBuf<uint8_t> d_kept;                      // gnn_interval_fold_dev: the slice's kept flags
    // gnn_embed_intervals
    std::vector<int64_t> w_lo, w_hi;
    DevBuf<float> d_sum, d_unit, d_sum_rev, d_unit_rev;      // HID per interval each
    DevBuf<float> d_score_sum, d_coherence;      // 3 and 1 per interval
    DevBuf<int32_t> d_count;
    DevBuf<float> d_mix;                         // one slab's combined window scores
    ~IntervalWorkspace() {
        if (tables_read) (void)hipEventDestroy(tables_read);
    }
};

// ---- nearest neighbours (gnn_neighbours.hip): persistent, grow-only.  Per base row 2 KB of f16 fragments + 1 B flag (and, for the
// host entry point, its 2 KB of f32); per query row of ONE slab of 16384 the same, 8 k B per base range of partial lists and 12 k B
// of results.  Nothing of the neighbour search grows with the number of queries; the match (gnn_graph.hip) prepares all its query rows
// at once into qfrag / qvalid.
struct NeighbourWorkspace {
    int64_t split = 0;                           // base rows per workgroup (gnn_debug_set_neighbour_split); 0: the library's choice
    DevBuf<uint4> bfrag, qfrag;                  // [32-row block][k-step 32][hi | lo][lane 64] x 16 B
    DevBuf<uint8_t> bvalid, qvalid;
    DevBuf<float> psim;                          // partial lists [query of the slab][range][k]
    DevBuf<int32_t> pidx;
    DevBuf<float> d_base, d_query;               // gnn_neighbours: the base's rows and one slab's query rows
    DevBuf<int64_t> d_out;                       // gnn_neighbours: one slab's [idx | sim (f32)], a Landing
};

// HIP-event timing of what is enqueued on ctx->stream while the scope lives, filed under kernel id `id` (gnn_profile_get); defined
// behind gnn_ctx
struct ProfScope {
    gnn_ctx* ctx;
    int id;
    hipEvent_t a = nullptr, b = nullptr;
    ProfScope(gnn_ctx* c, int kid);
    ~ProfScope();
};

}  // namespace gnn

// ---- the host side that the analyses over encoder embeddings share: the prologue (gnn_neighbours.hip, which also holds the prepare
// kernel and the scan), PassLog, HostCounters, Landing
#include "gnn_nn_host.h"

namespace gnn {

// ---- clusters (gnn_clusters.hip): persistent, grow-only.  The fragments and flags are NeighbourWorkspace's bfrag / bvalid (and d_base
// for the host entry point); here 20 B per row and, for gnn_cluster alone, its 32 B of results.  Nothing is n x n.
struct ClusterWorkspace {
    DevBuf<int32_t> parent;                      // union-find: a link points to a smaller index, a root to itself
    DevBuf<int32_t> degree, size;                // edges at the row; rows of the tree, at its root
    DevBuf<unsigned long long> key;              // at the root: max of (degree << 32) | (2^32 - 1 - row) over the tree
    DevBuf<int64_t> d_out;                       // gnn_cluster: [label | degree | size | rep], a Landing
};

// ---- density clusters (gnn_density.hip): persistent, grow-only.  The fragments and flags are NeighbourWorkspace's bfrag / bvalid (and
// d_base for the host entry point); here 21 B per row, one byte per (row tile, base range) and, for gnn_density alone, its 37 B of
// results.  Nothing is n x n.
struct DensityWorkspace {
    DevBuf<int32_t> parent;                      // union-find over the core rows: a link points to a smaller index, a root to itself
    DevBuf<int32_t> degree, size;                // edges at the row; rows that carry the label, at the label's row
    DevBuf<unsigned long long> key;              // at a row that is not core: max of (image of the similarity << 32) | (2^32 - 1 - core row)
    DevBuf<uint8_t> core;                        // [round_up(n, 64)]: degree + 1 >= min_points at a valid row
    DevBuf<uint8_t> flag;                        // [tiles * splits]: the count pass saw an edge in the workgroup's pairs
    DevBuf<int64_t> d_out;                       // gnn_density: [label | degree | size | anchor | sim (f32) | kind (u8)], a Landing
};

// ---- representatives (gnn_representatives.hip): persistent, grow-only.  The fragments and flags are NeighbourWorkspace's bfrag /
// bvalid (and d_base for the host entry point); here 21 B per row (padded to 64), one live byte per 64 and per 32 rows, two counters
// and, for gnn_representatives alone, its 20 B of results.  Nothing is n x n.
struct RepresentativeWorkspace {
    DevBuf<uint8_t> state;                       // INVALID, UNDECIDED, FRESH, REP or MEMBER
    DevBuf<unsigned> flag;                       // HIT | WAIT of the round, cleared by its decide
    DevBuf<unsigned long long> key;              // at a member: max of (image of the similarity << 32) | (2^32 - 1 - representative)
    DevBuf<unsigned long long> size;             // at a representative: the rows of its cluster
    DevBuf<uint8_t> row_live, col_live;          // per 64 rows: a FRESH or UNDECIDED row; per 32 rows: an UNDECIDED row
    HostCounters count;                          // [undecided rows, members]: the host reads one of them, once per round
    DevBuf<int64_t> d_out;                       // gnn_representatives: [rep | size | sim (f32)], a Landing
    PassLog rounds;                              // profiling on: HIP-event time of every round of the last call
};

// ---- single-linkage tree (gnn_linkage.hip): persistent, grow-only.  The fragments and flags are NeighbourWorkspace's bfrag / bvalid
// (and d_base for the host entry point); here 40 B per row and one counter.  Nothing is n x n.
struct LinkageWorkspace {
    DevBuf<int32_t> parent;                      // union-find: a link points to a smaller index, a root to itself
    DevBuf<int32_t> comp;                        // the root of the row's tree at the start of the round
    DevBuf<unsigned long long> best;             // at a row: max of (image of the similarity << 32) | (2^32 - 1 - partner), 0: none
    DevBuf<unsigned long long> cbest;            // at a root: max of (image << 32) | (2^32 - 1 - lo) over its rows' best pairs
    DevBuf<int32_t> chi;                         // at a root: min of hi among the rows that match cbest
    DevBuf<int32_t> ea, eb;                      // the edges recorded so far, in no order: lo, hi
    DevBuf<unsigned> es;                         // and the image of their similarity
    HostCounters count;                          // edges recorded so far: the host reads it, once per round
    PassLog rounds;                              // profiling on: HIP-event time of every round of the last call
    // the density tree (gnn_density_tree*) alone: 4 B per row, and 12 B per row and neighbour of the self-search's lists
    DevBuf<float> core;                          // the row's core similarity, NaN at an invalid row
    DevBuf<int64_t> nidx;                        // gnn_neighbours_dev's [n][min_points - 1] lists, of which only sim is read
    DevBuf<float> nsim;
    PassLog tree_rounds;                         // the rounds of the last gnn_density_tree* call
};

// ---- similarity graph (gnn_graph.hip): persistent, grow-only.  The fragments and flags are NeighbourWorkspace's bfrag / bvalid (and
// d_base for the host entry points); here 12 B per (row, base range) of counters and offsets and, for gnn_graph_count / gnn_graph_fill
// alone, 8 B per row and 8 B per edge of results.  Nothing is n x n.
// The match (gnn_match_*: the same passes over the rectangle query x base) shares all of it - a fill belongs to the ctx's last count of
// either kind - and prepares ALL its query rows at once into NeighbourWorkspace's qfrag / qvalid: 2 KB + 1 B per query row, 12 B per
// (query row, base range) of counters and offsets and, for gnn_match_count / gnn_match_fill alone, the query's 2 KB of f32 per row.
struct GraphWorkspace {
    DevBuf<int32_t> cnt;                         // [n * splits]: the edges of row i among the columns of range p, at i * splits + p
    DevBuf<int64_t> off;                         // [n * splits + 1]: their exclusive prefix sums, then the total
    // what the last count call ran with: the fill runs the same grid, and answers GNN_ERR_STATE for another (n, threshold, metric)
    bool counted = false;
    bool rect = false;                           // it was a gnn_match_count*: n query rows against nb base rows
    int64_t n = 0, nb = 0;                       // the graph: nb = n
    uint32_t threshold_bits = 0;
    int metric = 0;
    int64_t split_rows = 0, splits = 0;
    int64_t total = 0;                           // edges
    bool host_rows = false;                      // NeighbourWorkspace's d_base still holds the rows gnn_graph_count / gnn_match_count uploaded
    DevBuf<float> d_query;                       // gnn_match_count: the query's rows - the match's own, no other search writes here
    DevBuf<int64_t> d_out;                       // a Landing: gnn_graph_count's indptr [n + 1]; gnn_graph_fill's [col (i32) | sim (f32)]
    PassLog passes;                              // profiling on: HIP-event time of the last count call's [count pass, scan]
};

// ---- spherical k-means (gnn_kmeans.hip): persistent, grow-only.  The rows' fragments and flags are NeighbourWorkspace's bfrag / bvalid
// (and d_base for the host entry points); here 8 B per row (9 B with the farthest-first init), 2 KB + 1 B of fragments and 4 KB + 8 B
// of sums per centroid, one 128 KB one-column base, five counters and, for gnn_kmeans / gnn_centroids alone, their results and the
// init's 2 KB per centroid.  Nothing is n x k.
struct KMeansWorkspace {
    int lds_k = 128;                             // up to this many groups the update adds in LDS first (gnn_debug_set_kmeans_lds); no result depends on it
    DevBuf<uint4> cfrag;                         // the centroids' fragments (first: the init's), as NeighbourWorkspace's
    DevBuf<uint8_t> cvalid;
    DevBuf<unsigned long long> key;              // at a row: max of (image of the similarity << 32) | (2^32 - 1 - centroid), 0: none
    DevBuf<unsigned long long> S;                // [k][512] int64 sums of the members' 32-bit fixed-point unit rows
    DevBuf<unsigned long long> cnt;              // [k] members
    DevBuf<uint4> one;                           // farthest-first: the fragments of the last pick as a base of one row (63 zero rows)
    DevBuf<uint8_t> one_valid, picked;           // its flags [64]; per row: it is a pick
    HostCounters count;                          // [changed labels, valid rows, invalid init rows, bad labels, the farthest row's key]:
                                                 // the host reads them once at the start and once per assignment
    DevBuf<float> d_init;                        // gnn_kmeans: the init's rows
    DevBuf<int64_t> d_out;                       // a Landing.  gnn_kmeans: [label | sim (f32) | size | init_rows | centroids (f32)]; gnn_centroids: [label | size | centroids]
    PassLog passes;                              // profiling on: HIP-event time of the last call's [init, then per assignment: assign,
                                                 // and behind every assignment but the last: update, finish, prepare]
};

// ---- principal components (gnn_pca.hip): persistent, grow-only.  The rows' fragments and flags are NeighbourWorkspace's bfrag / bvalid
// (and d_base for the host entry points); here the components' 128 KB of fragments and, for the host entry points alone, their
// arguments and results.  Nothing here grows with n but gnn_pca_project's own output.
struct PCAWorkspace {
    int64_t split = 0;                           // rows per workgroup of the Gram pass (gnn_debug_set_pca_split): a multiple of 256; 0: the library's choice; no result depends on it
    DevBuf<uint4> cfrag;                         // the components' fragments, as NeighbourWorkspace's
    DevBuf<uint8_t> cvalid;
    DevBuf<float> d_comp;                        // gnn_pca_project: [components 64 x 512 | off 64]
    DevBuf<int64_t> d_out;                       // a Landing.  gnn_pca_moments: [G 512 x 512 | S 512 | n_valid]; gnn_pca_project: [n][ncomp] (f32)
    PassLog passes;                              // profiling on: the last call's passes, which the _dev entry points leave pending (they do not
                                                 // synchronise).  moments: [prepare, sums, gram, mirror]; project: [prepare rows, prepare components, project]
};

// ---- label transfer (gnn_votes.hip): persistent, grow-only.  The base's fragments and flags are NeighbourWorkspace's bfrag / bvalid (and
// d_base for the host entry point), one slab's query fragments its qfrag / qvalid (and d_query); here 4 B per padded base column, 8 B
// of keys per (query row of a slab, class), one flag and, for gnn_vote alone, the labels and one slab's 28 B of results per cell.
// Nothing is n_query x n_base.
struct VoteWorkspace {
    int lds_c = 16;                              // up to this many classes a workgroup votes in LDS first (gnn_debug_set_vote_lds); no result depends on it
    DevBuf<int32_t> blabel;                      // [round_up(n_base, 64)]: the column's class; -1: unlabelled, invalid or padded
    DevBuf<unsigned long long> key;              // [query rows of the slab][classes]: max of (image of the similarity << 32) | (2^32 - 1 - base row), 0: none
    HostCounters flag;                           // a label outside [-1, n_classes): the host reads it, once per call
    DevBuf<int64_t> d_label;                     // gnn_vote: the labels
    DevBuf<int64_t> d_out;                       // gnn_vote: one slab's [count | weight | nearest | nearest_sim (f32)], a Landing
    PassLog passes;                              // profiling on: the last call's [labels, then per slab of queries: votes, finish]; gnn_vote_dev
                                                 // leaves its last slab's pending
};

// ---- what the consumers of the similarity graph's CSR share (gnn_csr_sym.h, gnn_row_table.h) ----
// the graph of a host-pointer entry point on the device
struct GraphStaging {
    DevBuf<int64_t> d_indptr;                    // [n + 1]
    DevBuf<int32_t> d_col;                       // [nnz]
    DevBuf<float> d_sim;
    DevBuf<uint8_t> d_valid;                     // [n]
};

// the keyed-sum row table (gnn_row_table.h): its debug knobs and what its three row classes need
struct RowTable {
    int slots = 4096;                            // slots of the LDS table: 0 .. 4096; no result depends on it
    int wave_rows = 256;                         // the longest upper bound one wave takes; no result depends on it
    int groups = 0;                              // workgroups of a launch; 0: the library's choice; no result depends on it
    DevBuf<int32_t> rows;                        // [3][n]: the rows of a launch by class - wave, workgroup, dense
    DevBuf<unsigned long long> dense;            // [dense workgroups][n]: all zero between rows
    DevBuf<int32_t> touched;                     // [dense workgroups][n]
};

// ---- Markov clusters (gnn_mcl.hip): persistent, grow-only.  Two matrices of 8 B per (row, select) and 4 B per row, the symmetric graph
// (16 B per edge, 21 B per row), one uint64[n] accumulator and one int32[n] list per workgroup of the overflow pass (at most 2^27 cells
// in all), 12 B per row of lists and union-find, two counters per iteration and, for gnn_mcl alone, the graph and its 29 B of results per row.
struct MclWorkspace {
    int lds_slots = 4096;                        // slots of the LDS table (gnn_debug_mcl_lds): 0 .. 4096; no result depends on it
    int groups = 0;                              // workgroups of a pass (gnn_debug_mcl_groups); 0: two per CU; no result depends on it
    DevBuf<int32_t> len[2], idx[2];              // the matrix, double buffered: [n], [n][select] rows ascending
    DevBuf<uint32_t> val[2];                     // [n][select]: flow in units of 2^-30
    DevBuf<uint8_t> ok;                          // [n]: the row takes part
    DevBuf<int32_t> deg;                         // the symmetric graph: edges at the row, both ends counted
    DevBuf<int64_t> soff;                        // [n + 1]: their exclusive prefix sums
    DevBuf<unsigned long long> cursor;           // [n]: where the row's next entry goes
    DevBuf<int32_t> sidx;                        // [soff[n]]: the partner
    DevBuf<uint32_t> sq;                         // and the edge's integer weight
    HostCounters count;                          // [pass][changed columns, overflow columns], pass 0 the initial matrix; behind them the graph's
                                                 // flag.  The host reads one of them, once per iteration
    DevBuf<int32_t> ovf_list;                    // [n]: the columns of a pass whose rows did not fit the LDS table
    DevBuf<unsigned long long> dense;            // [overflow workgroups][n]: all zero between columns
    DevBuf<int32_t> touched;                     // [overflow workgroups][n]: the rows of the column at work
    DevBuf<int32_t> parent, size;                // union-find over the final matrix; rows of the tree, at its root
    bool have = false;                           // the ctx's last gnn_mcl* succeeded: gnn_mcl_matrix may read buffer `cur`
    int64_t n = 0;
    int select = 0, cur = 0;
    GraphStaging graph;                          // gnn_mcl: the graph
    DevBuf<int64_t> d_out;                       // gnn_mcl: [label | size | attractor | flow (u32) | is_attractor (u8)], a Landing
    PassLog passes;                              // profiling on: HIP-event time of the last call's [validate + symmetrise, initial matrix, then every iteration]
    std::vector<int64_t> overflow;               // the last call's overflow columns: [initial matrix, then every iteration]
};

// ---- label spreading (gnn_spread.hip): persistent, grow-only.  The symmetric graph with its transition weights (8 B per entry, 20 B per
// row), two score matrices of 4 B per (row, class), 18 B per row of seeds, marks, lists and `first`, one counter per iteration and, for
// gnn_spread alone, the graph, the labels and its 24 B of results per row.
struct SpreadWorkspace {
    int groups = 0;                              // workgroups of an iteration (gnn_debug_spread_groups); 0: the library's choice; no result depends on it
    bool skip = true;                            // the dirty-row rule (gnn_debug_spread_skip); no result depends on it
    DevBuf<uint8_t> ok;                          // [n]: the row takes part
    DevBuf<int32_t> deg;                         // the symmetric graph: entries at the row, both ends counted
    DevBuf<int64_t> soff;                        // [n + 1]: their exclusive prefix sums
    DevBuf<unsigned long long> cursor;           // [n]: where the row's next entry goes
    DevBuf<int32_t> sidx;                        // [soff[n]]: the partner j
    DevBuf<uint32_t> sp;                         // and the entry's weight q, then its transition mass p_ij
    DevBuf<int32_t> seed;                        // [n]: the class of a seed, -1 for every other row
    DevBuf<uint32_t> F[2];                       // [n][n_classes]: the scores, double buffered
    DevBuf<uint8_t> mark[2];                     // [n]: the row or a neighbour of it changed in the iteration that wrote the array
    DevBuf<int32_t> rows, long_rows;             // the rows an iteration computes: one wave each, one workgroup each
    HostCounters count;                          // [iteration] changed rows; behind them [short rows, long rows, the verdict on graph and labels]
    GraphStaging graph;                          // gnn_spread: the graph, its rows' validity and the labels
    DevBuf<int64_t> d_label;
    DevBuf<int64_t> d_out;                       // gnn_spread: [best (i32) | best_score (u32) | second_score (u32) | total (u64) | first (i32)], a Landing
    PassLog passes;                              // profiling on: HIP-event time of the last call's [validate + symmetrise, then every iteration]
};

// ---- average linkage (gnn_avglink.hip): persistent, grow-only.  The symmetric graph and two entry buffers (12 B per entry each, two
// entries per edge), about 70 B per row of state, lists and records, at most 2^24 cells of dense accumulators (192 MB) and, for
// gnn_avglink alone, the graph and its 24 B of results per row.
struct AvglinkWorkspace {
    RowTable table;                              // the row table's knobs (gnn_debug_avglink_slots, _wave_rows, _groups), lists and accumulators
    DevBuf<uint8_t> ok;                          // [n]: the row takes part
    DevBuf<int32_t> len;                         // [n]: entries of the live cluster's segment (first the symmetric graph's degrees)
    DevBuf<int64_t> off[2];                      // [n + 1]: where a segment starts in entry buffer b
    DevBuf<unsigned long long> cursor;           // [n]: symmetrise's
    DevBuf<int32_t> idx[2];                      // the entries, ping-pong: the neighbour cluster
    DevBuf<unsigned long long> sum[2];           // and S, the sum of q between the two clusters
    DevBuf<uint32_t> sq;                         // symmetrise's weights, widened into sum[0]
    DevBuf<int32_t> map, size, best, partner, ub;      // [n] each: see gnn_avglink.hip
    DevBuf<unsigned long long> bestS;            // [n]
    HostCounters count;                          // [2][merged, wave rows, workgroup rows, dense rows], then the call's class totals [3], then the verdict
    GraphStaging graph;                          // gnn_avglink: the graph
    DevBuf<int64_t> d_out;                       // gnn_avglink: [parent (i32) | weight (u64) | size_a (i32) | size_b (i32) | round (i32)], a Landing
    PassLog passes;                              // profiling on: HIP-event time of the last call's [validate + symmetrise, then every round]
    int64_t class_rows[3] = {0, 0, 0};           // the last call's rows by class, all rounds (gnn_debug_avglink_classes)
};

// ---- modularity communities (gnn_communities.hip): persistent, grow-only.  The symmetric graph and two entry buffers (12 B per entry
// each, two entries per edge, + 4 B of symmetrise's weights), about 190 B per row of state, lists and maps, at most 2^24 cells of dense
// accumulators (192 MB) and, for gnn_communities / gnn_label_components alone, the graph and the results.
struct CommunitiesWorkspace {
    RowTable table;                              // the row table's knobs (gnn_debug_communities_slots, _wave_rows, _groups), lists and accumulators
    DevBuf<uint8_t> ok;                          // [n]: the row takes part
    DevBuf<int32_t> len[2];                      // [n]: entries of a node's segment in entry buffer b
    DevBuf<int64_t> off[2];                      // [n + 1]: where it starts
    DevBuf<unsigned long long> cursor;           // [n]: symmetrise's
    DevBuf<int32_t> idx[2];                      // the entries, ping-pong over the levels: the neighbour node
    DevBuf<unsigned long long> sum[2];           // and the summed weight
    DevBuf<uint32_t> sq;                         // symmetrise's weights, widened into sum[0]
    DevBuf<int32_t> comm[2];                     // [n]: the assignment and the sweep's proposal
    DevBuf<unsigned long long> tot[2];           // [n]: their communities' totals
    DevBuf<unsigned long long> k;                // [n]: a node's weight
    DevBuf<int32_t> want_c;                      // [n]: the community a node wants, -1: none
    DevBuf<unsigned long long> want_d;           // [n][2]: its gain D, low and high word
    DevBuf<int32_t> parent, comp, flag, ub, mcount, mlist;      // [n] each: the level's end, see gnn_communities.hip
    DevBuf<int64_t> numoff, mstart;              // [n + 1]: a component's number, where its member list starts
    DevBuf<unsigned long long> mcursor;          // [n]
    DevBuf<int32_t> map;                         // [n]: row -> its node, -1: an invalid row
    DevBuf<int32_t> noderow[2];                  // [n]: node -> its smallest row
    HostCounters count;                          // see gnn_communities.hip, "the counters"
    GraphStaging graph;                          // gnn_communities, gnn_label_components: the graph
    DevBuf<int64_t> d_out;                       // gnn_communities: [label | size | level_label], gnn_label_components: [label | out]; a Landing
    PassLog passes;                              // profiling on: the last call's [setup, then per level every sweep and, behind an accepted one, the level's end]
    int64_t class_rows[6] = {0, 0, 0, 0, 0, 0};  // the last call's rows by class: the want launches', the contractions' (gnn_debug_communities_classes)
};

// ---- k-nearest-neighbour graph (gnn_knn_graph.hip): persistent, grow-only.  Per row 20 k B of lists (the search's int64 / f32 and the
// ordered int32 / f32) and 36 B of length, counter, offset, cursor and class lists; per edge 16 B (the packed entries and the radix
// class's second buffer) and, for gnn_knn_graph_count / gnn_knn_graph_fill alone, 8 B per row and 9 B per edge of results.  Nothing is
// n x n.  The search's own buffers are NeighbourWorkspace's.
struct KnnGraphWorkspace {
    int wave_rows = 64;                          // the longest row one wave orders (gnn_debug_knn_graph_wave_rows): 1 .. 64; no result depends on it
    int group_rows = 2048;                       // the longest row a workgroup orders in LDS (gnn_debug_knn_graph_group_rows): 1 .. 4096; no result depends on it
    DevBuf<int64_t> nidx;                        // [n][k]: the self-search's lists, as gnn_neighbours_dev writes them
    DevBuf<float> nsim;
    DevBuf<int32_t> lidx;                        // [n][k]: a row's neighbours ascending, the first len[i] of them
    DevBuf<float> lsim;                          // and their similarities
    DevBuf<int32_t> len;                         // [n]
    DevBuf<int32_t> cnt;                         // [n]: the edges row i owns
    DevBuf<int64_t> off;                         // [n + 1]: their exclusive prefix sums, then the total
    DevBuf<unsigned long long> cursor;           // [n]: where the row's next edge goes
    DevBuf<int32_t> rows;                        // [2][n]: the rows a workgroup orders in LDS, then those it orders by radix
    DevBuf<unsigned long long> pairs[2];         // [total]: an edge as partner << 32 | similarity bits; [1]: the radix class's other buffer
    HostCounters count;                          // [0], [1]: the rows of the two workgroup classes
    // what the last count call ran with: the fill answers GNN_ERR_STATE for another (n, k, mode, weight, metric)
    bool counted = false;
    bool host_rows = false;                      // it was a gnn_knn_graph_count
    int64_t n = 0;
    int k = 0, mode = 0, weight = 0, metric = 0;
    int64_t total = 0;                           // edges
    int64_t class_rows[2] = {0, 0};              // the rows of the LDS class and of the radix class
    int wave_limit = 0, group_limit = 0;         // the class limits the count ran with: the fill's
    DevBuf<int64_t> d_out;                       // a Landing: gnn_knn_graph_count's indptr [n + 1]; gnn_knn_graph_fill's [col (i32) | sim (f32) | mutual (u8)]
    PassLog passes;                              // profiling on: the last count's [search, lists, count, scan + classes], behind them every fill's [fill, order, finish]
};

// ---- t-SNE layout (gnn_tsne.hip): persistent, grow-only.  The symmetric graph (12 B per entry, 25 B per row), 24 B per row of Y, gains
// and updates, 40 B per row of integer sums, 8 B per iterate of Z and, for the host entry points alone, the graph and their arguments
// and results.  Nothing is n x n.
struct TsneWorkspace {
    int split = 0;                               // workgroups over the columns of the repel pass (gnn_debug_tsne_split); 0: two workgroups per CU; no result depends on it
    DevBuf<uint8_t> ok;                          // [n]: the row takes part
    DevBuf<int32_t> deg;                         // the symmetric graph: edges at the row, both ends counted
    DevBuf<int64_t> soff;                        // [n + 1]: their exclusive prefix sums
    DevBuf<unsigned long long> cursor;           // [n]: where the row's next entry goes
    DevBuf<int32_t> sidx;                        // [soff[n]]: the partner
    DevBuf<uint32_t> sq;                         // the entry's integer weight
    DevBuf<float> sp;                            // and its affinity p = q / M2
    DevBuf<int32_t> long_list;                   // [n]: the rows whose entries a workgroup attracts
    DevBuf<float> y, gain, upd;                  // [n][2] each
    DevBuf<long long> zi, rx, ry;                // [n]: the repel pass's sums, zero between passes
    DevBuf<long long> ax, ay;                    // [n]: the attract pass's sums
    DevBuf<unsigned long long> ztrace;           // [n_iter + 1]: Z of every iterate, accumulated where it stands
    HostCounters count;                          // [the graph's and the init's flag, M2, rows of the long list]: the host reads the flag, once
    GraphStaging graph;                          // gnn_tsne, gnn_tsne_forces: the graph
    DevBuf<int64_t> d_out;                       // a Landing.  gnn_tsne: [layout (f32) | z_trace | valid (u8) | init (f32)]; gnn_tsne_forces: [zi | rx | ry | ax | ay | m2 | Y (f32)]
    PassLog passes;                              // profiling on: the last gnn_tsne* call's [setup, the loop, the final Z and the results]
};

struct ContigWorkspace {
    hipStream_t copy_stream = nullptr;
    std::vector<hipEvent_t> piece_done;
    // host side of the span table
    std::vector<int64_t> starts, ids;
    std::vector<int32_t> lens, window_n, counts;
    // device side
    DevBuf<uint8_t> seq;
    DevBuf<int64_t> d_starts, d_ids;             // the span table: one element per candidate window ...
    DevBuf<int32_t> d_lens, d_window_n, d_counts;
    DevBuf<float> d_scores;                      // ... and GNN_CLASSES per window
    DevBuf<uint8_t> d_bases;
    DevBuf<float> d_out;
    // gnn_classify_contigs_embed: one slab's window embeddings (f32) and the per-contig running sums / kept-window counts
    DevBuf<float> d_emb, d_emb_sum;
    DevBuf<int32_t> d_emb_kept;
    // gnn_scan_contigs: CSR offsets of every contig's windows and bins, the track (3 f32 per bin) and its cover counts
    std::vector<int64_t> win_off, bin_off;
    DevBuf<int64_t> d_win_off, d_bin_off;
    DevBuf<float> d_track;
    DevBuf<int32_t> d_cover;
    // the *_strand entry points: the reverse windows' and the combined (`both`) scores, GNN_CLASSES per window each; the scores of
    // one slab's batch [forward | reverse] before the split; the per-contig means of each strand ([forward | reverse] rows); the
    // reverse strand's own embedding sums and kept-window counts
    DevBuf<float> d_scores_rev, d_scores_mix, d_slab_scores, d_out_strand;
    DevBuf<float> d_emb_sum_rev;
    DevBuf<int32_t> d_emb_kept_rev;
    // gnn_occlude_contigs (gnn_occlude.hip): CSR offsets of every window's blocks, and ONE slab's occluded scores (12 B per pair; the
    // deltas replace them in place) - nothing here grows with the number of pairs of a call
    std::vector<int64_t> blk_off;
    DevBuf<int64_t> d_blk_off;
    DevBuf<float> d_occ;
    // gnn_attribute_contigs (gnn_attrib.hip): ONE slab's maps, bias and logits (24 nb + 24 B per window of the slab)
    DevBuf<float> d_attr;
    // gnn_call_regions / gnn_region_states_dev (gnn_regions.hip)
    RegionWorkspace regions;
    // gnn_embed_intervals / gnn_interval_fold_dev (gnn_intervals.hip)
    IntervalWorkspace intervals;

    // What the buffer groups hold, in windows / contigs + 1 / bins.  The head-room is counted in elements, so a buffer with
    // several elements per window or bin holds fewer of them than its neighbours: the smallest member decides.
    size_t span_cap() const {
        return std::min({d_starts.capacity(), d_ids.capacity(), d_lens.capacity(), d_window_n.capacity(), d_counts.capacity(),
                         d_scores.capacity() / GNN_CLASSES});
    }
    size_t strand_cap() const { return std::min(d_scores_rev.capacity(), d_scores_mix.capacity()) / GNN_CLASSES; }
    size_t off_cap() const { return std::min(d_win_off.capacity(), d_bin_off.capacity()); }
    size_t bin_cap() const { return std::min(d_track.capacity() / GNN_CLASSES, d_cover.capacity()); }
};

// The window rule, once: seq_windows(seq, 6000, 2500, max_windows) of the reference (sequence.py:150-167) with the window start
// advancing by `stride` instead of 6000.  Window 0 always exists; window k > 0 exists while no earlier window reached the contig's
// end and its own length is at least MIN_TAIL.  f(k, length).  At stride == W this is the loop gnn_classify_contigs always ran.
template <typename F>
static inline void for_each_window(int64_t len, int64_t stride, int single_window, F&& f) {
    for (int64_t k = 0; k * stride < len; ++k) {
        const int64_t l = std::min<int64_t>(W, len - k * stride);
        if (l < MIN_TAIL && k > 0) break;             // a short tail is dropped, a short first window kept
        f(k, l);
        if (l < MIN_TAIL || (single_window && k == 0) || k * stride + W >= len) break;
    }
}

// The window table, once: the rule above over every contig of `offsets`, f(contig, k, length) per window in table order.  Counts
// the windows and the stride-wide bins (ceil(length / stride) per contig) and, where a CSR array [n_contigs + 1] is given, files
// the running counts per contig.  The offsets are validated before anything is written.
struct WindowWalk {
    int64_t* win_off = nullptr;
    int64_t* bin_off = nullptr;
    int64_t windows = 0, bins = 0;
};
template <typename F>
static int walk_windows(const int64_t* offsets, int64_t n_contigs, int64_t stride, int single_window, WindowWalk& out, F&& f) {
    for (int64_t c = 0; c < n_contigs; ++c)
        if (offsets[c + 1] < offsets[c]) {
            set_error("contig offsets are not non-decreasing");
            return GNN_ERR_ARG;
        }
    out.windows = out.bins = 0;
    if (out.win_off) out.win_off[0] = 0;
    if (out.bin_off) out.bin_off[0] = 0;
    for (int64_t c = 0; c < n_contigs; ++c) {
        const int64_t len = offsets[c + 1] - offsets[c];
        for_each_window(len, stride, single_window, [&](int64_t k, int64_t l) {
            f(c, k, l);
            ++out.windows;
        });
        out.bins += (len + stride - 1) / stride;
        if (out.win_off) out.win_off[c + 1] = out.windows;
        if (out.bin_off) out.bin_off[c + 1] = out.bins;
    }
    return GNN_OK;
}

// The N rule, once (nn_classification.py:70): a contig's first window is always kept, a later one unless it holds more than
// MAX_N literal 'N'.  Decides which windows enter a contig's score, embedding and track - on the device and on the host.
__host__ __device__ inline bool window_kept(int32_t window_n, int32_t n_count) {
    return window_n == 0 || n_count <= MAX_N;
}

// Grow-only with some head-room (amortised).
template <typename Tp>
static int reserve_roomy(DevBuf<Tp>& b, size_t need) {
    return b.reserve(need, need / 4 + 64);
}

// A group that is sized together is re-allocated as a whole: every member is emptied before the first one grows.
template <typename... Bufs>
static void reset_all(Bufs&... bufs) {
    (bufs.reset(), ...);
}

// One thread per cell, 256 per block: kernel(args...) on `stream`.  The arguments convert to the kernel's parameter types here, so
// a DevBuf goes in as the pointer it owns.
template <typename... P, typename... A>
static int launch_1d(void (*kernel)(P...), int64_t cells, hipStream_t stream, A&&... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, static_cast<P>(args)...);
    GNN_HIP(hipGetLastError());
    return GNN_OK;
}

// The tile grids of the analyses over encoder embeddings: (row tiles, base ranges) workgroups of 256 threads.
template <typename... P, typename... A>
static int launch_tiles(void (*kernel)(P...), int64_t tiles, int64_t splits, hipStream_t stream, A&&... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)tiles, (unsigned)splits), dim3(256), 0, stream, static_cast<P>(args)...);
    GNN_HIP(hipGetLastError());
    return GNN_OK;
}

// What an attribution call adds to a pass of classify_chunks (gnn_attrib.hip): device buffers, row i = window i of the pass.
// contrib[n][2][attrib_bins(bin)][3]; bias[n][3] and logits[n][3] may be NULL.
struct AttribOut {
    int bin;
    float* contrib;
    float* bias;
    float* logits;
};
static inline int attrib_bins(int bin) { return (POOLED + bin - 1) / bin; }      // the last bin may be short

struct ProfileSlot {
    double total_ms = 0.0;
    int64_t launches = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

}  // namespace gnn

struct gnn_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool has_weights = false;
    gnn::DeviceWeights w;
    gnn::Workspace ws;
    // second workspace + stream: the back end of chunk i runs beside the front end of chunk i+1 (classify_chunks)
    gnn::Workspace ws_alt;
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_front[2] = {nullptr, nullptr}, ev_back[2] = {nullptr, nullptr};
    bool back_pending[2] = {false, false};   // ev_back[i] recorded on stream2 and not yet waited for by `stream`
    int buf_cur = 0;                         // which of the two alternating workspaces `ws` currently is
    int64_t chunk_fused = 16384;     // windows per launch of a fused front end (gnn_set_chunk): larger grids amortise the launch's tail (185.9 vs
                                     // 184.6 k windows/s against 8192, profiles/r04/backend_overlap_ab.txt); 13 GB of workspace at full size, one set.
                                     // The DEFAULT is a ceiling, not a demand: classify_chunks clamps it to a quarter of the device memory that is
                                     // free when the workspace first grows, and any size (explicit or not) is halved and retried when the
                                     // allocation fails (shared / partitioned GPUs)
    int64_t alt_failed_chunk = 0;    // a second workspace of this many windows did not fit (classify_chunks does not retry at or above it)
    bool chunk_explicit = false;     // gnn_set_chunk was called: no clamp against free memory, only the halve-and-retry on failure
    int64_t chunk_f32 = 64;
    bool profile = false;
    gnn::ProfileSlot prof[GNN_K_COUNT];
    std::vector<hipEvent_t> event_pool;
    std::vector<gnn::DevBuf<unsigned char>> owned;   // the weight packs (gnn::upload)
    int cu_count = 0;
    int last_split = 1;                           // workgroups per window of the last streaming-kernel launch (gnn_debug_last_split)
    bool time_split = true;                       // x3 kernel: several workgroups per window when a launch is smaller than the chip (gnn_debug_set_time_split)
    bool c6_pad_skip = true;                      // f16c6: copy the all-N tail of a window instead of computing it (gnn_debug_set_pad_skip)
    gnn::DevBuf<unsigned long long> phase_cycles;  // non-null: fused kernel runs its instrumented build
    gnn::ContigWorkspace* contig_ws = nullptr;    // gnn_contigs.hip: persistent buffers of gnn_classify_contigs
    // gnn_classify / gnn_debug_forward (host windows in, host scores out): persistent, grow-only staging - a device slab for
    // the windows and their scores, two pinned bounce buffers the windows go through in pieces (the copy of piece i+1 into
    // its bounce buffer overlaps the DMA of piece i) and a pinned landing buffer for the scores.  No allocation per call.
    gnn::DevBuf<uint8_t> stage_bases;             // W bytes per window
    gnn::DevBuf<float> stage_emb;                 // gnn_embed: the slab's embeddings (grow-only; f32 elements, serves bf16 too)
    gnn::DevBuf<float> emb_scores;                // gnn_embed_dev without a scores pointer: the scores land here (grow-only)
    gnn::DevBuf<float> stage_attr;                // gnn_attribute: the slab's maps, bias and logits (grow-only)
    gnn::DevBuf<float> attr_g;                    // attribution: d logit / d feat of one launch's windows, [chunk][256][3] (gnn_attrib.hip)
    gnn::DevBuf<float> stage_scores;              // GNN_CLASSES per window, as stage_scores_host
    gnn::PinnedBuf<float> stage_scores_host;
    gnn::PinnedBuf<uint8_t> pin[2];
    hipEvent_t pin_ev[2] = {nullptr, nullptr};
    bool pin_busy[2] = {false, false};
    // classify_chunks: staging of a window buffer that is not 4-byte aligned (the streaming kernels fetch bases as aligned dwords)
    gnn::DevBuf<uint8_t> align_buf;
    gnn::NeighbourWorkspace nn;                   // gnn_neighbours.hip
    gnn::ClusterWorkspace cl;                     // gnn_clusters.hip
    gnn::DensityWorkspace dn;                     // gnn_density.hip
    gnn::RepresentativeWorkspace rp;              // gnn_representatives.hip
    gnn::LinkageWorkspace lk;                     // gnn_linkage.hip
    gnn::GraphWorkspace gr;                       // gnn_graph.hip
    gnn::KMeansWorkspace km;                      // gnn_kmeans.hip
    gnn::PCAWorkspace pca;                        // gnn_pca.hip
    gnn::VoteWorkspace vt;                        // gnn_votes.hip
    gnn::MclWorkspace mcl;                        // gnn_mcl.hip
    gnn::SpreadWorkspace sprd;                    // gnn_spread.hip
    gnn::AvglinkWorkspace avl;                    // gnn_avglink.hip
    gnn::CommunitiesWorkspace cmt;                // gnn_communities.hip
    gnn::KnnGraphWorkspace kg;                    // gnn_knn_graph.hip
    gnn::TsneWorkspace ts;                        // gnn_tsne.hip
    // every PassLog above: drain_profile settles them before an event they hold returns to event_pool
    gnn::PassLog* const pass_logs[13] = {&rp.rounds, &lk.rounds, &lk.tree_rounds, &gr.passes,  &km.passes,  &pca.passes, &vt.passes,
                                         &mcl.passes, &sprd.passes, &avl.passes, &cmt.passes, &kg.passes, &ts.passes};
    // RCCL communicator of this ctx (gnn_comm.hip); ncclComm_t kept opaque here
    void* comm = nullptr;
    int comm_ranks = 1, comm_rank = 0;
    gnn::DevBuf<unsigned char> comm_scratch;
};

namespace gnn {

inline ProfScope::ProfScope(gnn_ctx* c, int kid) : ctx(c), id(kid) {
    if (!ctx->profile) return;
    auto take = [&]() {
        hipEvent_t e = nullptr;
        if (!ctx->event_pool.empty()) {
            e = ctx->event_pool.back();
            ctx->event_pool.pop_back();
        } else if (hipEventCreate(&e) != hipSuccess) {
            e = nullptr;
        }
        return e;
    };
    a = take();
    b = take();
    if (a) (void)hipEventRecord(a, ctx->stream);
}
inline ProfScope::~ProfScope() {
    if (!ctx->profile || !a || !b) return;
    (void)hipEventRecord(b, ctx->stream);
    ctx->prof[id].pending.emplace_back(a, b);
}

// The one way a weight pack reaches the device: an allocation ctx->owned keeps until gnn_destroy, filled from the host.
template <typename Tp>
int upload(gnn_ctx* ctx, const Tp* host, size_t count, Tp** dev) {
    DevBuf<unsigned char> b;
    if (int rc = b.upload(reinterpret_cast<const unsigned char*>(host), count * sizeof(Tp))) return rc;
    *dev = reinterpret_cast<Tp*>(b.get());
    ctx->owned.emplace_back(std::move(b));
    return GNN_OK;
}
template <typename Tp>
int upload(gnn_ctx* ctx, const std::vector<Tp>& v, Tp** dev) {
    return upload(ctx, v.data(), v.size(), dev);
}

// The padding skip's constants: a fused front end runs ONCE on an all-N window and its yp (2, 749, 128) and mp (2, 8400) are
// kept; the kernels copy them for a window's all-N tail instead of computing it.  run(bases, yp, mp) fills the kernel's Args
// and enqueues one window on ctx->stream.
template <typename Run>
int all_n_consts(gnn_ctx* ctx, DevBuf<float>& yp, DevBuf<float>& mp, Run&& run) {
    DevBuf<uint8_t> bn;
    int rc = bn.reserve(W);
    if (!rc) rc = yp.reserve((size_t)2 * POOLED * C);
    if (!rc) rc = mp.reserve((size_t)2 * NPAIR);
    if (rc) return rc;
    hipError_t e = hipMemsetAsync(bn, 'N', W, ctx->stream);
    if (e == hipSuccess) {
        run(bn.get(), yp.get(), mp.get());
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);      // before bn goes
    if (e == hipSuccess) return GNN_OK;
    yp.reset();           // no constants rather than unwritten ones
    mp.reset();
    set_error(std::string("the all-N window's launch failed: ") + hipGetErrorString(e));
    return GNN_ERR_HIP;
}

// ---- kernel launchers (each enqueues on ctx->stream, returns gnn_status) ----
int launch_tokenize(gnn_ctx* ctx, const uint8_t* bases, int64_t n, uint16_t* tokens);
int launch_onehot(gnn_ctx* ctx, const uint8_t* bases, int64_t n, int dtype, void* out);
int launch_synth(gnn_ctx* ctx, uint64_t seed, int64_t first, int64_t n, uint8_t* bases);
int launch_span_count(gnn_ctx* ctx, const uint8_t* seq, const int64_t* starts, const int32_t* lens, int64_t n,
                      int byte, int32_t* counts);
int launch_materialize(gnn_ctx* ctx, const uint8_t* seq, const int64_t* starts, const int32_t* lens, int64_t n,
                       uint8_t* bases);
// the same spans as reverse-complement windows (gnn_encode.hip, revcomp_kernel); bases must be 4-byte aligned, as above
int launch_revcomp(gnn_ctx* ctx, const uint8_t* seq, const int64_t* starts, const int32_t* lens, int64_t n,
                   uint8_t* bases);
// occluded windows (gnn_encode.hip, occlude_kernel): window i of the span table materialised with [lo, hi) set to 'N'.  By pairs
// (blk_off != NULL): out row r is pair pair0 + r of the CSR blk_off[n_windows + 1], its window found on the device, its block
// [j * block, (j + 1) * block).  By spans (blk_off == NULL): out row r is span r with [lo[r], hi[r]).  bases 4-byte aligned
int launch_occlude(gnn_ctx* ctx, const uint8_t* seq, const int64_t* starts, const int32_t* lens, const int64_t* blk_off,
                   int64_t n_windows, int64_t pair0, int block, const int32_t* lo, const int32_t* hi, int64_t n_rows, uint8_t* bases);
// the N rule's masked mean per contig (gnn_contigs.hip, masked_segment_mean_kernel)
int launch_masked_segment_mean(gnn_ctx* ctx, const float* scores, const int64_t* ids, const int32_t* window_n, const int32_t* counts,
                               int64_t n, int64_t n_seg, float* out);
int launch_front_f32(gnn_ctx* ctx, const uint8_t* bases, int64_t n);         // -> ws.mp, ws.yp (+ ws.x)
// ws.mp, ws.yp -> scores; emb_dev != NULL: also h1 (the encoder embedding) as emb_dev[n][GNN_EMBED_DIM] of emb_dtype (gnn_emb_dtype)
// dense = false: everything up to ws.feat; the dense head is then the attribution's (launch_attrib_head, which writes the scores)
int launch_backend(gnn_ctx* ctx, int64_t n, int precision, float* scores_dev, void* emb_dev = nullptr, int emb_dtype = GNN_EMB_F32,
                   bool dense = true);
// attribution (gnn_attrib.hip): precision and bin checked under the entry point's name; the head kernel (ws.feat -> scores, ctx->attr_g,
// bias, logits) and the contribution kernel (ws.alpha, ws.yp, ctx->attr_g -> contrib) of the n windows in ctx->ws, whose outputs
// are rows row0 .. row0 + n - 1 of `at`
int check_attrib_args(int precision, int bin, const char* fn);
int launch_attrib_head(gnn_ctx* ctx, int64_t n, float* scores_dev, const AttribOut& at, int64_t row0);
int launch_attrib_contrib(gnn_ctx* ctx, int64_t n, const AttribOut& at, int64_t row0);
// one pass of the hot path over n windows whose padded bases are on the device (gnn_api.hip)
// defer_last: leave the last chunk's back end pending on the second stream (gnn_classify_dev_async).  flush_backend()
// makes ctx->stream wait for whatever is pending (the end of a synchronous classify_chunks); finish_pending() waits for it on
// the host - every other entry point that enqueues on ctx->stream, reads scores or touches the workspaces calls it first
// emb_dev != NULL: window i's embedding goes to row i of emb_dev (the rows of a chunk are its own, whichever workspace it ran in)
// attr != NULL: window i's contribution map, bias and logits go to row i of attr's buffers; scores_dev may then be NULL
int classify_chunks(gnn_ctx* ctx, const uint8_t* bases_dev, int64_t n, int precision, float* scores_dev, bool defer_last = false,
                    void* emb_dev = nullptr, int emb_dtype = GNN_EMB_F32, const AttribOut* attr = nullptr);
size_t emb_elem_bytes(int emb_dtype);   // bytes of one embedding value (gnn_api.hip); 0 for a bad gnn_emb_dtype
int flush_backend(gnn_ctx* ctx);
int finish_pending(gnn_ctx* ctx);
// The entry preamble (gnn_api.hip): a NULL ctx is an error, the ctx's device becomes current, and - unless flush is false - what an
// asynchronous classification left pending is finished.
int check_ctx(gnn_ctx* ctx, bool flush = true);
// GNN_OK, or the error of an embedding asked of GNN_PREC_F16C6 under the entry point's name (gnn_api.hip)
int check_embed_precision(int precision, const char* fn);
void free_stage(gnn_ctx* ctx);         // gnn_api.hip: staging of the host-buffer entry points

// ---- the contig front end's steps (gnn_contigs.hip); gnn_occlude.hip runs the same ones ----
// What every contig entry point is given.
struct ContigIn {
    gnn_ctx* ctx;
    const uint8_t* seq;          // the packed contigs, on the host (seq_on_host) or on the device
    int seq_on_host;
    int64_t seq_bytes;
    const int64_t* offsets;      // host, [n_contigs + 1]
    int64_t n_contigs;
    int single_window, precision;
    int64_t stride;              // W, or a scan's stride
};

// Where a call's kernels read the packed sequence.  Already on the device: the caller's pointer, and upto() has nothing to do.  On
// the host: w.seq, which begin() reserves and upto() fills in PIECEs on the copy stream while earlier pieces are classified on
// the ctx stream.  This is the only code that writes w.seq or touches the copy stream.
class SeqFeed {
  public:
    int begin(const ContigIn& in, ContigWorkspace& w);
    // every piece that holds a byte below `end` is on its way, and the ctx stream waits for the last of them
    int upto(int64_t end);
    const uint8_t* dev() const { return dev_; }

  private:
    gnn_ctx* ctx_ = nullptr;
    ContigWorkspace* w_ = nullptr;
    const uint8_t* host_ = nullptr;      // NULL: nothing to upload
    const uint8_t* dev_ = nullptr;
    int64_t bytes_ = 0, n_pieces_ = 0, uploaded_ = 0;
};

// Entry: check_ctx, the arguments every contig call shares (`outputs_ok`: the caller's verdict on its own pointers; the message
// names `fn`), the offsets against the buffer, and the ctx's workspace, created on first use.
int contig_begin(const ContigIn& in, const char* fn, bool outputs_ok, ContigWorkspace** w);
// Plan: the host side of the span table (w.starts / lens / ids / window_n) by walk_windows at in.stride; csr: also w.win_off and
// w.bin_off; block > 0: also w.blk_off, the CSR of every window's blocks of `block` bases.
int plan_windows(const ContigIn& in, ContigWorkspace& w, bool csr, int block);
// The per-window device tables hold the planned windows (grown as a group) and the four uploads are enqueued on the ctx stream.
int upload_span_table(gnn_ctx* ctx, ContigWorkspace& w);
// One slab [a, a + m) of the span table: what its windows read is uploaded, their N are counted into w.d_counts, they are
// materialised into w.d_bases - the forward windows, then the reverse ones, whichever are asked for - and the batch is classified:
// scores[(fwd + rev) * m][GNN_CLASSES], emb[(fwd + rev) * m][HID] unless NULL, and the maps of `attr` unless NULL.
int slab_pass(const ContigIn& in, ContigWorkspace& w, SeqFeed& feed, int64_t a, int64_t m, bool fwd, bool rev, float* scores,
              float* emb, const AttribOut* attr = nullptr);
// After the counts came back (w.counts): the N rule per window on the host.  mask[i] = 1 / 0 and the contig ids of the kept
// windows, compacted, where asked for; returns how many are kept.
int64_t kept_windows(const ContigWorkspace& w, uint8_t* mask_or_null, int64_t* ids_or_null);
void free_contig_ws(gnn_ctx* ctx);
// GNN_OK, or GNN_ERR_ARG under the entry point's name for a stride outside [1, 6000] / a strand outside gnn_strand
int check_stride(int stride, const char* fn);
int check_strand(int strand, const char* fn);
// lanes of the embedding folds (gnn_contigs.hip, gnn_intervals.hip): x 4 columns = one 2 KB row per step, read as float4s
constexpr int FOLD_THREADS = HID / 4;

int launch_front_c6(gnn_ctx* ctx, const uint8_t* bases, int64_t n);             // GNN_PREC_F16C6 -> ws.mp, ws.yp
int launch_front_x3(gnn_ctx* ctx, const uint8_t* bases, int64_t n, int precision);   // GNN_PREC_F16X3 / BF16X3 (gnn_fused_x3.hip) -> ws.mp, ws.yp
int launch_front_tc(gnn_ctx* ctx, const uint8_t* bases, int64_t n);             // GNN_PREC_F16X3TC (gnn_fused_tc.hip) -> ws.mp, ws.yp
int launch_front_tk(gnn_ctx* ctx, const uint8_t* bases, int64_t n);             // GNN_PREC_F16X3TK (gnn_fused_tk.hip) -> ws.mp, ws.yp
int build_kmer_tables(gnn_ctx* ctx, size_t reserve);                             // gnn_fused_tk.hip: GNN_ERR_NOMEM when free memory < tables + reserve
void free_kmer_tables(gnn_ctx* ctx);
size_t kmer_tables_bytes();
int build_wva_rows_table(gnn_ctx* ctx, const float* w_kc, float* tbl);          // gnn_fused_tc.hip: x1(row) @ w for every row of WvaTable's index space
int pack_fused_tc_weights(gnn_ctx* ctx, const gnn_weights* w);                   // after pack_fused_c6_weights (shares its pair tables)
int pack_fused_x3_consts(gnn_ctx* ctx);                                          // all-N window outputs of that kernel (after the other packs)

// host-side packing for the fused paths (gnn_pack.hip)
int pack_fused_weights(gnn_ctx* ctx, const gnn_weights* w);
// K x N row-major f32 -> [kstep][nblk][plane hi, lo][lane 64][8 x 16 bit] (bf16 or f16 limbs), zero padded (gnn_pack.hip)
std::vector<uint16_t> pack_frags(const float* wmat, int K, int N, bool f16 = false);
int pack_fused_c6_weights(gnn_ctx* ctx, const gnn_weights* w);
int c6_rows_per_step();
int c6_pack_matrix(const float* wmat, int K, int N, std::vector<uint32_t>& out);   // host only (tests)
// conv1 pair tables (3, PAIR_ROWS, 128): W1[2j][a] + W1[2j+1][b] for every token pair of adjacent positions (gnn_api.hip)
void build_conv1_pair_tables(const float* conv1_kernel, std::vector<float>& pt);

}  // namespace gnn
