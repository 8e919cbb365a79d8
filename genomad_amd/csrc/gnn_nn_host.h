// What the host code of the analyses over encoder embeddings shares (gnn_neighbours.hip, gnn_clusters.hip, gnn_density.hip,
// gnn_representatives.hip, gnn_linkage.hip, gnn_graph.hip, gnn_kmeans.hip, gnn_pca.hip, gnn_votes.hip, gnn_mcl.hip, gnn_spread.hip).  Host only, and
// included by gnn_common.h, in front of the workspaces that hold these types.
//   the prologue: nn_check_metric / nn_check_rows / nn_check_threshold / nn_check_required (an argument check's text exists once),
//   nn_metric_scale, nn_prepare, nn_tile_grid, nn_upload_rows, nn_scan (the one block-wide exclusive scan)
//   PassLog: the one way an analysis times its passes - scoped events, filed behind a synchronise, read by a gnn_debug_*_ms
//   HostCounters: device words the host reads behind one synchronise
//   Landing: the result buffer of a host-pointer entry point - slices carved once, copied out once
// The launches (launch_1d, launch_tiles) stand in gnn_common.h.  The bodies that are no templates are compiled once, in
// gnn_neighbours.hip - but the three checks and Landing's arithmetic, which are inline: tests/native/nn_host_check.cpp runs them
// without the library.
#pragma once
#include <cmath>
#include <utility>

struct gnn_ctx;

namespace gnn {

// ---- the prologue.  `f` is the name an error message carries.
int nn_check_metric(const std::string& f, int metric);      // GNN_OK, or GNN_ERR_ARG for a metric outside gnn_knn_metric
// n in [0, 2^31), or GNN_ERR_ARG; noun: "rows", "base rows" (the count comes first), or "n_query", "n_base" (the name comes first)
inline int nn_check_rows(const std::string& f, int64_t n, const char* noun) {
    if (n >= 0 && n < ((int64_t)1 << 31)) return GNN_OK;
    const bool named = noun[0] == 'n' && noun[1] == '_';
    set_error(f + ": " + (named ? noun + (" " + std::to_string(n)) : std::to_string(n) + " " + noun) + " is outside [0, 2^31)");
    return GNN_ERR_ARG;
}
inline int nn_check_threshold(const std::string& f, float threshold) {
    if (std::isfinite(threshold)) return GNN_OK;
    set_error(f + ": threshold " + std::to_string(threshold) + " is outside (-inf, inf): a finite f32 is required");
    return GNN_ERR_ARG;
}
// ok, or GNN_ERR_ARG: "bad argument to <f>: <what> are required"
inline int nn_check_required(const std::string& f, bool ok, const char* what) {
    if (ok) return GNN_OK;
    set_error("bad argument to " + f + ": " + what + " are required");
    return GNN_ERR_ARG;
}
float nn_metric_scale(int metric);                           // what a tile kernel multiplies its products by: 2^-16 for cosine, 1 for dot
// rows_dev[n][GNN_EMBED_DIM] -> fragments and flags of round_up(n, 64) rows
int nn_prepare(gnn_ctx* ctx, const float* rows_dev, int64_t n, int metric, DevBuf<uint4>& frag, DevBuf<uint8_t>& valid);
// The tile grid of `tiles` row tiles over nb `noun` ("rows", "base rows"): base rows per workgroup - the debug value, or what gives
// every CU two workgroups; a multiple of 32 - and the number of such ranges, or GNN_ERR_ARG for more than 65535 of them.
int nn_tile_grid(const gnn_ctx* ctx, const std::string& fn, const char* noun, int64_t tiles, int64_t nb, int64_t* split_rows, int64_t* splits);
int nn_upload_rows(gnn_ctx* ctx, const float* rows_host, int64_t n);      // n rows into ctx->nn.d_base, enqueued on the ctx's stream
// Exclusive int64 prefix sums of the m counters into off[0 .. m), their total into off[m] and, unless cursor is NULL, the sums into
// cursor[0 .. m) as well: one block on `stream` (the region calls, the similarity graph, the Markov clusters, label spreading).
int nn_scan(hipStream_t stream, const int32_t* cnt, int64_t m, int64_t* off, unsigned long long* cursor);

// ---- PassLog: the HIP-event times of the passes of an analysis's last call, while profiling is on.  begin() at the start of a call;
// a Scope around what a pass enqueues; settle() where the code has just synchronised the stream; out() is the body of a
// gnn_debug_*_ms entry point.  A pending pair is also in ctx->prof[].pending: drain_profile (gnn_api.hip) settles every log of the ctx
// before it returns an event to the pool, so no log ever reads an event that somebody else has recorded again.
class PassLog {
  public:
    void begin() {
        pending_.clear();
        ms_.clear();
    }
    // log == NULL: a plain ProfScope (a helper that only some of its callers time)
    struct Scope {
        ProfScope prof;
        Scope(gnn_ctx* ctx, PassLog* log) : prof(ctx, GNN_K_NEIGHBOURS) {
            if (log && prof.a && prof.b) log->pending_.emplace_back(prof.a, prof.b);
        }
        Scope(gnn_ctx* ctx, PassLog& log) : Scope(ctx, &log) {}
    };
    void settle();             // every pending pair has completed: its elapsed ms joins the filed ones, in the order of the scopes
    // behind the entry point's check_ctx: synchronises and settles if anything is pending, then *n_out = the entries, of which
    // min(capacity, entries) go to ms_out
    int out(gnn_ctx* ctx, const char* fn, double* ms_out, int64_t capacity, int64_t* n_out);

  private:
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending_;
    std::vector<float> ms_;
};

// ---- HostCounters: uint64 words that kernels count in and the host reads, each read behind everything enqueued - a synchronise.
class HostCounters {
  public:
    int reserve(gnn_ctx* ctx, size_t words);
    unsigned long long* dev() const { return dev_.get(); }
    int zero(gnn_ctx* ctx, size_t first, size_t words);
    int read(gnn_ctx* ctx, size_t first, size_t words, unsigned long long* out);

  private:
    DevBuf<unsigned long long> dev_;
    PinnedBuf<unsigned long long> host_;         // as large as the largest single read
};

// ---- Landing: where the results of one host-pointer call (or of one slab of it) stand on the device, carved from a grow-only
// buffer of the workspace.  add() every slice, reserve() before anything is enqueued, hand dev<T>(i) to the kernels, copy_out().
// Every slice starts at a multiple of 16 bytes (the k-means kernels move centroids as 16-byte vectors).
constexpr int LANDING_SLICES = 8;
inline size_t landing_place(size_t* total, size_t bytes) {      // where a slice of `bytes` goes: the end so far, which then moves on
    const size_t at = *total;
    *total = (at + bytes + 15) / 16 * 16;
    return at;
}
class Landing {
  public:
    explicit Landing(DevBuf<int64_t>& buf) : buf_(buf) {}
    // count elements that copy_out() brings to host_ptr; NULL: the slice is the call's own (an upload, scratch).  Returns its index.
    template <typename Tp>
    int add(Tp* host_ptr, int64_t count) {
        if (n_ < LANDING_SLICES) {
            const size_t bytes = (size_t)count * sizeof(Tp);
            s_[n_] = {host_ptr, landing_place(&total_, bytes), bytes};
        }
        return n_++;
    }
    int reserve(gnn_ctx* ctx);             // grows the buffer to the total (freed first: nn_reserve)
    size_t at(int i) const { return s_[i].at; }               // the slice's offset in bytes
    template <typename Tp>
    Tp* dev(int i) const {                                    // behind reserve()
        return reinterpret_cast<Tp*>(reinterpret_cast<char*>(buf_.get()) + s_[i].at);
    }
    size_t bytes() const { return total_; }
    bool ok() const { return n_ <= LANDING_SLICES; }          // false behind a ninth add(): reserve() then answers GNN_ERR_STATE
    int copy_out(gnn_ctx* ctx) const;      // one copy per slice that has a host pointer and a byte, then one synchronise

  private:
    struct Slice {
        void* host;
        size_t at, bytes;
    };
    DevBuf<int64_t>& buf_;
    Slice s_[LANDING_SLICES];
    int n_ = 0;
    size_t total_ = 0;
};

}  // namespace gnn
