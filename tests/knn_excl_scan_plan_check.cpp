// knn_excl_scan_plan_check.cpp -- stand-alone check of the route of radad_knn_search_excl_scan (knn_excl_scan_route, knn_plan.h) and of
// its workspace layout, driven by tests/test_knn_excl_scan_plan.py.  No GPU, no HIP: it includes the planner header alone.
//
// The route must be RADAD_EXCL_SCAN_TILE exactly when the plain search of the batch would take the certified tile scan:
// knn_tile_eligibility at the user searches' margin, and the tuning state not on its fp32 fallback.  The table walks every
// combination of the boundaries the contract names -- 16 / 17 queries, 16 383 / 16 384 rows (and 49 152: where k = 128 becomes a
// tile-scan shape), dim 64 / 96, k 128 / 129 (and 10, 58 / 59: the sample's limit on a 16 384-row store), plane on / off, fp32
// fallback idle / active, fp32 / fp16 store -- and states the expected route of the named corner cases literally.
#include <cstdio>
#include <cstdlib>

#include "knn_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                                                                        \
    do {                                                                                        \
        if (!(cond)) { ++failures; printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

static StoreFacts facts(int64_t n, int dim, int hi_off, int f16) {
    StoreFacts s;
    s.ntotal = n; s.dim = dim; s.metric = RADAD_METRIC_L2; s.hi_off = hi_off; s.f16 = f16;
    return s;
}

int main() {
    static_assert(RADAD_EXCL_SCAN_TILE == 0 && RADAD_EXCL_SCAN_EXACT == 1, "the header's route values");
    int lines = 0, tiles = 0;
    for (int64_t n : {16383, 16384, 20480, 49152, 1000000})
        for (int dim : {64, 96, 512})
            for (int64_t nq : {1, 16, 17, 300, 1024})
                for (int k : {1, 10, 58, 59, 128, 129, 1024})
                    for (int hi_off : {0, 1})
                        for (int skip : {0, 8})
                            for (int f16 : {0, 1}) {
                                const StoreFacts s = facts(n, dim, hi_off, f16);
                                const int route = knn_excl_scan_route(s, nq, k, skip);
                                const bool plain_tile = skip == 0 && knn_tile_eligibility(s, nq, k, KNN_MARGIN).eligible;
                                CHECK(route == (plain_tile ? RADAD_EXCL_SCAN_TILE : RADAD_EXCL_SCAN_EXACT),
                                      "n %lld dim %d nq %lld k %d hi_off %d skip %d f16 %d: route %d", (long long)n, dim, (long long)nq, k, hi_off, skip, f16, route);
                                // what the eligibility itself must say at the boundaries of the contract
                                if (nq <= 16 && k + KNN_MARGIN <= 32 && dim <= 512) CHECK(route == RADAD_EXCL_SCAN_EXACT, "16 or fewer queries stream");
                                if (n < 16384 || dim % 64 != 0 || k > 128 || hi_off || skip) CHECK(route == RADAD_EXCL_SCAN_EXACT, "outside the tile scan's shapes");
                                if (nq >= 17 && n >= 49152 && dim % 64 == 0 && k <= 128 && !hi_off && !skip) CHECK(route == RADAD_EXCL_SCAN_TILE, "a tile-scan shape");
                                printf("route n%lld_d%d_q%lld_k%d_off%d_skip%d_f16%d %d\n", (long long)n, dim, (long long)nq, k, hi_off, skip, f16, route);
                                ++lines;
                                tiles += route == RADAD_EXCL_SCAN_TILE;
                            }
    // the named corners, literally
    CHECK(knn_excl_scan_route(facts(16384, 64, 0, 0), 17, 10, 0) == RADAD_EXCL_SCAN_TILE, "17 queries, 16 384 rows");
    CHECK(knn_excl_scan_route(facts(16384, 64, 0, 0), 16, 10, 0) == RADAD_EXCL_SCAN_EXACT, "16 queries");
    CHECK(knn_excl_scan_route(facts(16383, 64, 0, 0), 17, 10, 0) == RADAD_EXCL_SCAN_EXACT, "16 383 rows");
    CHECK(knn_excl_scan_route(facts(16384, 96, 0, 0), 17, 10, 0) == RADAD_EXCL_SCAN_EXACT, "dim 96");
    CHECK(knn_excl_scan_route(facts(49152, 64, 0, 0), 17, 128, 0) == RADAD_EXCL_SCAN_TILE, "k 128");
    CHECK(knn_excl_scan_route(facts(49152, 64, 0, 0), 17, 129, 0) == RADAD_EXCL_SCAN_EXACT, "k 129");
    CHECK(knn_excl_scan_route(facts(16384, 64, 0, 0), 17, 58, 0) == RADAD_EXCL_SCAN_TILE, "k 58 on 16 384 rows");
    CHECK(knn_excl_scan_route(facts(16384, 64, 0, 0), 17, 59, 0) == RADAD_EXCL_SCAN_EXACT, "k 59 on 16 384 rows: the sample holds 128 entries");
    CHECK(knn_excl_scan_route(facts(16384, 64, 1, 0), 17, 10, 0) == RADAD_EXCL_SCAN_EXACT, "plane off");
    CHECK(knn_excl_scan_route(facts(16384, 64, 0, 0), 17, 10, 3) == RADAD_EXCL_SCAN_EXACT, "fp32 fallback active");
    CHECK(knn_excl_scan_route(facts(16384, 64, 0, 1), 17, 10, 0) == RADAD_EXCL_SCAN_TILE, "an fp16 store is its own plane");
    CHECK(tiles > 0 && tiles < lines, "both routes occur (%d of %d)", tiles, lines);

    // the route never changes the tuning state: it takes the count by value; a KnnTuning on its fallback is read, not counted down
    {
        KnnTuning t;
        t.hi_skip = 8;
        CHECK(knn_excl_scan_route(facts(20480, 64, 0, 0), 300, 10, t.hi_skip) == RADAD_EXCL_SCAN_EXACT && t.hi_skip == 8, "hi_skip read only");
    }

    // the layout: bitmap words cover every row, the bias array (tile route only) lies behind them and holds one float per row
    for (int64_t n : {1, 63, 64, 65, 16384, 20480, 1000001}) {
        const StoreFacts s = facts(n, 64, 0, 0);
        const ExclScanLayout t = knn_excl_scan_layout(s, RADAD_EXCL_SCAN_TILE), x = knn_excl_scan_layout(s, RADAD_EXCL_SCAN_EXACT);
        CHECK(t.n_words * 64 >= n && (t.n_words - 1) * 64 < n && x.n_words == t.n_words, "n %lld words %lld", (long long)n, (long long)t.n_words);
        CHECK(t.admit == 0 && t.bias >= (size_t)t.n_words * 8 && t.bias % 256 == 0, "bias behind the bitmap");
        CHECK(t.bytes >= t.bias + (size_t)n * 4 && x.bytes >= (size_t)x.n_words * 8 && x.bytes < t.bytes, "bytes");
    }
    printf("lines %d tile %d\n", lines, tiles);
    if (failures) { printf("knn_excl_scan_plan_check: %d FAILED\n", failures); return 1; }
    printf("knn_excl_scan_plan_check: ok\n");
    return 0;
}
