// Stand-alone check of the parts of gnn_nn_host.h that need no device: Landing's offsets and the shared argument checks' texts.
// Built and run by tests/test_nn_host_host.py under AddressSanitizer and UBSan; it touches no GPU and makes no HIP call (the one
// DevBuf here stays empty).  Exit status 0: every check held; otherwise the failed ones are on stderr.
#include <cstdio>
#include <cstdint>
#include <string>

#include "gnn_common.h"

static std::string last_error;
void gnn::set_error(const std::string& msg) { last_error = msg; }

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

using namespace gnn;

static void landing() {
    size_t total = 0;
    CHECK(landing_place(&total, 0) == 0 && total == 0);              // an empty slice takes no room
    CHECK(landing_place(&total, 1) == 0 && total == 16);
    CHECK(landing_place(&total, 16) == 16 && total == 32);
    CHECK(landing_place(&total, 17) == 32 && total == 64);

    DevBuf<int64_t> buf;                                             // never allocated: only the offsets are looked at
    int64_t i64[4];
    float f32[4];
    uint8_t u8[4];
    // gnn_density at n = 3: four int64 arrays, one f32, one u8
    Landing d(buf);
    for (int i = 0; i < 4; ++i) CHECK(d.add(i64, 3) == i);
    CHECK(d.add(f32, 3) == 4 && d.add(u8, 3) == 5 && d.ok());
    for (int i = 0; i < 4; ++i) CHECK(d.at(i) == (size_t)32 * i);
    CHECK(d.at(4) == 128 && d.at(5) == 144);
    CHECK(d.bytes() == 160 && d.bytes() % sizeof(int64_t) == 0);
    // gnn_kmeans at n = 0, k = 3: two empty slices share an offset with the next one, the centroids start at a multiple of 16
    Landing k(buf);
    k.add(i64, 0);
    k.add(f32, 0);
    k.add(i64, 3);
    k.add(i64, 3);
    const int cent = k.add(f32, 3 * 512);
    CHECK(k.at(0) == 0 && k.at(1) == 0 && k.at(2) == 0 && k.at(3) == 32 && k.at(cent) == 64);
    CHECK(k.bytes() == 64 + 3 * 512 * 4);
    // eight slices fit, a ninth does not and moves nothing
    Landing e(buf);
    for (int i = 0; i < LANDING_SLICES; ++i) CHECK(e.add(u8, 1) == i);
    CHECK(e.ok() && e.bytes() == 16 * LANDING_SLICES);
    CHECK(e.add(u8, 1) == LANDING_SLICES && !e.ok() && e.bytes() == 16 * LANDING_SLICES);
    CHECK(Landing(buf).bytes() == 0 && Landing(buf).ok());
}

static void checks() {
    const int64_t top = (int64_t)1 << 31;
    CHECK(nn_check_rows("f", 0, "rows") == GNN_OK && nn_check_rows("f", top - 1, "n_base") == GNN_OK);
    CHECK(nn_check_rows("gnn_cluster", -1, "rows") == GNN_ERR_ARG && last_error == "gnn_cluster: -1 rows is outside [0, 2^31)");
    CHECK(nn_check_rows("gnn_neighbours", top, "base rows") == GNN_ERR_ARG &&
          last_error == "gnn_neighbours: 2147483648 base rows is outside [0, 2^31)");
    CHECK(nn_check_rows("gnn_vote", -5, "n_query") == GNN_ERR_ARG && last_error == "gnn_vote: n_query -5 is outside [0, 2^31)");
    CHECK(nn_check_rows("gnn_match_count", top, "n_base") == GNN_ERR_ARG &&
          last_error == "gnn_match_count: n_base 2147483648 is outside [0, 2^31)");
    CHECK(nn_check_threshold("f", 0.5f) == GNN_OK && nn_check_threshold("f", -3.4e38f) == GNN_OK);
    CHECK(nn_check_threshold("gnn_graph_count", NAN) == GNN_ERR_ARG &&
          last_error == "gnn_graph_count: threshold nan is outside (-inf, inf): a finite f32 is required");
    CHECK(nn_check_threshold("gnn_density", INFINITY) == GNN_ERR_ARG &&
          last_error == "gnn_density: threshold inf is outside (-inf, inf): a finite f32 is required");
    last_error.clear();
    CHECK(nn_check_required("f", true, "x") == GNN_OK && last_error.empty());
    CHECK(nn_check_required("gnn_cluster", false, "the rows and the four outputs") == GNN_ERR_ARG &&
          last_error == "bad argument to gnn_cluster: the rows and the four outputs are required");
}

int main() {
    landing();
    checks();
    if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}
