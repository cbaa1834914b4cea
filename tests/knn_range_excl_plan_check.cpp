// knn_range_excl_plan_check.cpp -- stand-alone check of the host-only plan of radad_knn_range_search_excl / _excl_pq
// (knn_range_excl_plan, knn_plan.h), driven by tests/test_knn_range_excl_plan.py.  No GPU, no HIP: it includes the planner header alone.
//
//   * over the grid of tests/knn_range_plan_check.cpp, in both modes and whatever m is, the route equals knn_range_plan's;
//   * the buffers hold 4096 entries and the scan is one launch on the tile route;
//   * one set for the batch: the biased instantiation (whatever the plane: biased == hi_q) and one pre-pass launch on the tile route;
//   * one set per query: the plan is knn_range_plan's plan, member for member -- no bias forced, no pre-pass, no scrub launch;
//   * the exact pass's lists are RangeLayout's, unchanged, with the bitmap and the bias array behind them in the batch mode.
#include <cstdio>
#include <cstdlib>

#include "knn_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                                                                        \
    do {                                                                                        \
        if (!(cond)) { ++failures; printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

static StoreFacts facts(int64_t n, int dim, int hi_off, int f16, int cap_boost = 1, int metric = RADAD_METRIC_L2) {
    StoreFacts s;
    s.ntotal = n; s.dim = dim; s.metric = metric; s.hi_off = hi_off; s.f16 = f16; s.cap_boost = cap_boost;
    return s;
}

static bool same_plan(const ScanPlan& a, const ScanPlan& b) {
    return a.kind == b.kind && a.nq == b.nq && a.k == b.k && a.l2 == b.l2 && a.n_qtiles == b.n_qtiles && a.n_splits == b.n_splits &&
           a.chunk_rows == b.chunk_rows && a.ksel == b.ksel && a.ksel_sq == b.ksel_sq && a.s_splits == b.s_splits && a.emit_cap == b.emit_cap &&
           a.cap == b.cap && a.plen == b.plen && a.n_parts == b.n_parts && a.sq_rows_per_wave == b.sq_rows_per_wave && a.sq_ksplit == b.sq_ksplit &&
           a.sq_lds == b.sq_lds && a.dense_plen == b.dense_plen && a.xgroup == b.xgroup && a.reported_qtiles == b.reported_qtiles &&
           a.block_threads == b.block_threads && a.hi_q == b.hi_q && a.mu == b.mu;
}

int main() {
    static_assert(KNN_RANGE_EXCL_BATCH == 0 && KNN_RANGE_EXCL_PER_QUERY == 1, "the two modes");
    int lines = 0, tiles = 0;
    for (int64_t n : {16383, 16384, 20480, 49152, 1000000})
        for (int dim : {64, 96, 512})
            for (int64_t nq : {1, 16, 17, 300, 1024})
                for (int m : {1, 10, 58, 59, 128, 129, 1024})
                    for (int hi_off : {0, 1})
                        for (int skip : {0, 8})
                            for (int f16 : {0, 1})
                                for (int metric : {RADAD_METRIC_L2, RADAD_METRIC_COSINE}) {
                                    const StoreFacts s = facts(n, dim, hi_off, f16, 1, metric);
                                    const RangePlan r = knn_range_plan(s, nq, m, skip);
                                    for (int mode : {KNN_RANGE_EXCL_BATCH, KNN_RANGE_EXCL_PER_QUERY})
                                        for (int tags : {0, 1, 4, 64}) {
                                            const RangeExclPlan x = knn_range_excl_plan(s, nq, m, mode, tags, skip);
                                            CHECK(x.mode == mode && x.route == r.route, "n %lld dim %d nq %lld m %d hi_off %d skip %d f16 %d mode %d: route %d, the range plan's %d",
                                                  (long long)n, dim, (long long)nq, m, hi_off, skip, f16, mode, x.route, r.route);
                                            CHECK(x.launches == r.launches && x.scrub_launches == 0, "launches %d, scrub %d", x.launches, x.scrub_launches);
                                            CHECK(x.facts.cap_boost == 4 && x.facts.ntotal == n && x.facts.dim == dim && x.facts.metric == metric,
                                                  "the caller's facts with the forced boost");
                                            CHECK(same_plan(x.plan, r.plan), "the scan plan apart from the bias is the range plan's");
                                            if (x.route == RADAD_RANGE_TILE) {
                                                CHECK(x.plan.kind == RADAD_SCAN_HI_TILE && x.plan.emit_cap == 4096 && x.plan.plen == 4096 && x.plan.n_parts == 1,
                                                      "emit_cap %d", x.plan.emit_cap);
                                                CHECK(x.launches == 1, "%d launches", x.launches);
                                                CHECK(x.plan.hi_q, "the tile scan runs f16 queries with a scale");
                                            } else {
                                                CHECK(x.launches == 0 && x.plan.emit_cap == 0, "exact route: no tile plan");
                                            }
                                            if (mode == KNN_RANGE_EXCL_BATCH) {
                                                CHECK(x.plan.biased == x.plan.hi_q, "one set for the batch: the biased instantiation whatever the plane");
                                                CHECK(x.prepass_launches == (x.route == RADAD_RANGE_TILE ? 1 : 0), "%d pre-pass launches", x.prepass_launches);
                                            } else {
                                                CHECK(x.plan.biased == r.plan.biased && x.prepass_launches == 0, "one set per query: the plain range search's own plan");
                                            }
                                            if (knn_exact_fits(dim, m)) {
                                                const RangeLayout B = knn_range_layout(x.facts, nq, m);
                                                const RangeExclLayout E = knn_range_excl_layout(x.facts, nq, m, x.route);
                                                CHECK(E.lists.xk == B.xk && E.lists.xi == B.xi && E.lists.bytes == B.bytes && E.lists.xgroup == B.xgroup &&
                                                      E.lists.xslots == B.xslots, "RangeLayout is reused for the exact pass");
                                                CHECK(E.n_words == (n + 63) / 64 && E.admit == B.bytes && E.admit % 256 == 0 && E.bias % 256 == 0 &&
                                                      E.bias >= E.admit + (size_t)E.n_words * 8, "the bitmap behind the lists");
                                                CHECK(E.bytes >= E.bias + (x.route == RADAD_RANGE_TILE ? (size_t)n * 4 : 0), "the bias array behind the bitmap");
                                            }
                                            if (metric == RADAD_METRIC_L2 && tags == 4)
                                                printf("plan n%lld_d%d_q%lld_m%d_off%d_skip%d_f16%d_mode%d %d %d %d %d %d\n", (long long)n, dim, (long long)nq, m,
                                                       hi_off, skip, f16, mode, x.route, x.plan.emit_cap, x.launches, x.plan.biased ? 1 : 0, x.prepass_launches);
                                            ++lines;
                                            tiles += x.route == RADAD_RANGE_TILE;
                                        }
                                }
    CHECK(tiles > 0 && tiles < lines, "both routes occur (%d of %d)", tiles, lines);

    // the named shapes of the GPU tests, literally
    for (int metric : {RADAD_METRIC_L2, RADAD_METRIC_IP, RADAD_METRIC_COSINE})
        for (int mode : {KNN_RANGE_EXCL_BATCH, KNN_RANGE_EXCL_PER_QUERY}) {
            for (int64_t nq : {17, 299, 300}) {
                const RangeExclPlan t = knn_range_excl_plan(facts(16640 + 37, 64, 0, 0, 1, metric), nq, 64, mode, 4, 0);
                CHECK(t.route == RADAD_RANGE_TILE && t.plan.emit_cap == 4096 && t.launches == 1, "the GPU tests' store, q %lld", (long long)nq);
                // an un-centred IP / cosine plane has no bias of its own: only the batch mode forces the biased instantiation there
                if (metric != RADAD_METRIC_L2)
                    CHECK(t.plan.biased == (mode == KNN_RANGE_EXCL_BATCH), "metric %d mode %d biased %d", metric, mode, (int)t.plan.biased);
                const RangeExclPlan w = knn_range_excl_plan(facts(16640 + 37, 128, 0, 0, 1, metric), nq, 64, mode, 4, 0);
                CHECK(w.route == RADAD_RANGE_TILE && w.launches == 1, "... at dim 128");
            }
            CHECK(knn_range_excl_plan(facts(16640 + 37, 64, 0, 0, 1, metric), 3, 64, mode, 4, 0).route == RADAD_RANGE_EXACT, "q = 3");
            CHECK(knn_range_excl_plan(facts(3000, 36, 0, 0, 1, metric), 40, 64, mode, 4, 0).route == RADAD_RANGE_EXACT, "d = 36");
            CHECK(knn_range_excl_plan(facts(1000, 64, 0, 0, 1, metric), 40, 64, mode, 4, 0).route == RADAD_RANGE_EXACT, "n = 1000");
            CHECK(knn_range_excl_plan(facts(16640 + 37, 64, 1, 0, 1, metric), 40, 64, mode, 4, 0).route == RADAD_RANGE_EXACT, "plane off");
            CHECK(knn_range_excl_plan(facts(16640 + 37, 64, 0, 0, 1, metric), 300, 64, mode, 4, 8).route == RADAD_RANGE_EXACT, "skip = 8");
            const RangeExclPlan b = knn_range_excl_plan(facts(1000000, 512, 0, 0, 1, RADAD_METRIC_COSINE), 1024, 128, mode, 1, 0);
            CHECK(b.route == RADAD_RANGE_TILE && b.launches == 1 && b.plan.emit_cap == 4096, "the benchmark's store");
        }

    // the tuning state is read, never written
    {
        KnnTuning t;
        t.hi_skip = 8;
        const RangeExclPlan x = knn_range_excl_plan(facts(20480, 64, 0, 0), 300, 64, KNN_RANGE_EXCL_PER_QUERY, 4, t.hi_skip);
        CHECK(x.route == RADAD_RANGE_EXACT && t.hi_skip == 8 && t.cap_boost == 1, "hi_skip read only");
    }
    printf("lines %d tile %d\n", lines, tiles);
    if (failures) { printf("knn_range_excl_plan_check: %d FAILED\n", failures); return 1; }
    printf("knn_range_excl_plan_check: ok\n");
    return 0;
}
