// knn_range_plan_check.cpp -- stand-alone check of the host-only plan of radad_knn_range_search (knn_range_plan, knn_plan.h), driven by
// tests/test_knn_range_plan.py.  No GPU, no HIP: it includes the planner header alone.
//
//   * over the grid of tests/knn_excl_scan_pq_plan_check.cpp the route equals knn_excl_scan_route at k = 1, whatever max_per_query is;
//   * the facts the plan is made from are the caller's with cap_boost forced to 4 (whatever the handle's own): emit_cap == 4096 on the
//     tile route, the plan is the plain search's at k = 1;
//   * one scan launch on the tile route (knn_hi_phases with one_go), none on the exact route;
//   * the exact pass's lists are laid out for k = max_per_query (knn_range_layout), within the exact kernel's LDS.
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

int main() {
    static_assert(RADAD_RANGE_TILE == 0 && RADAD_RANGE_EXACT == 1, "the routes radad_knn_last_range reports");
    int lines = 0, tiles = 0;
    for (int64_t n : {16383, 16384, 20480, 49152, 1000000})
        for (int dim : {64, 96, 512})
            for (int64_t nq : {1, 16, 17, 300, 1024})
                for (int m : {1, 10, 58, 59, 128, 129, 1024})
                    for (int hi_off : {0, 1})
                        for (int skip : {0, 8})
                            for (int f16 : {0, 1})
                                for (int boost : {1, 4}) {
                                    const StoreFacts s = facts(n, dim, hi_off, f16, boost);
                                    const RangePlan x = knn_range_plan(s, nq, m, skip);
                                    const int want = knn_excl_scan_route(s, nq, 1, skip) == RADAD_EXCL_SCAN_TILE ? RADAD_RANGE_TILE : RADAD_RANGE_EXACT;
                                    CHECK(x.route == want, "n %lld dim %d nq %lld m %d hi_off %d skip %d f16 %d: route %d, knn_excl_scan_route at k = 1 %d",
                                          (long long)n, dim, (long long)nq, m, hi_off, skip, f16, x.route, want);
                                    const bool shape = nq >= 17 && dim % 64 == 0 && !hi_off && n >= 16384 && skip == 0;
                                    CHECK((x.route == RADAD_RANGE_TILE) == shape, "the route in words: n %lld dim %d nq %lld hi_off %d skip %d", (long long)n,
                                          dim, (long long)nq, hi_off, skip);
                                    CHECK(x.facts.cap_boost == 4 && x.facts.ntotal == n && x.facts.dim == dim && x.facts.hi_off == hi_off &&
                                          x.facts.f16 == f16 && x.facts.metric == s.metric, "the caller's facts with the forced boost");
                                    CHECK(x.plan.nq == nq && x.plan.k == 1 && x.plan.ksel == 1 + KNN_MARGIN, "the plain search's plan at k = 1");
                                    if (x.route == RADAD_RANGE_TILE) {
                                        CHECK(x.plan.kind == RADAD_SCAN_HI_TILE, "tile route, plan kind %d", x.plan.kind);
                                        CHECK(x.plan.emit_cap == 4096 && x.plan.plen == 4096 && x.plan.n_parts == 1, "emit_cap %d", x.plan.emit_cap);
                                        CHECK(x.launches == 1, "%d launches", x.launches);
                                        CHECK(x.plan.s_splits >= 8, "the preconditions of the tile scan (a sample that never runs): %d", x.plan.s_splits);
                                    } else {
                                        CHECK(x.plan.kind != RADAD_SCAN_HI_TILE && x.plan.emit_cap == 0, "exact route: no tile plan");
                                        CHECK(x.launches == 0, "exact route: %d scan launches", x.launches);
                                    }
                                    // max_per_query and the handle's own boost change nothing of the route or the scan
                                    const RangePlan y = knn_range_plan(facts(n, dim, hi_off, f16, 1), nq, 1, skip);
                                    CHECK(y.route == x.route && y.plan.emit_cap == x.plan.emit_cap && y.launches == x.launches && y.plan.kind == x.plan.kind,
                                          "the plan depends on max_per_query or on the handle's cap_boost");
                                    // the exact pass at k = max_per_query
                                    if (knn_exact_fits(dim, m)) {
                                        const RangeLayout B = knn_range_layout(x.facts, nq, m);
                                        CHECK(B.xgroup == knn_exact_group(dim, m) && B.xslots == knn_exact_slots(nq, m, B.xgroup) && B.xslots >= 1, "grouping");
                                        CHECK(B.xk == 0 && B.xi >= (size_t)B.xslots * KX_SLICES * m * 8 && B.bytes >= B.xi + (size_t)B.xslots * KX_SLICES * m * 4 &&
                                              B.xi % 256 == 0, "layout");
                                        CHECK(knn_exact_lds_bytes(dim, m) <= KX_LDS_MAX, "LDS");
                                    }
                                    if (boost == 1)
                                        printf("plan n%lld_d%d_q%lld_m%d_off%d_skip%d_f16%d %d %d %d\n", (long long)n, dim, (long long)nq, m, hi_off, skip, f16,
                                               x.route, x.plan.emit_cap, x.launches);
                                    ++lines;
                                    tiles += x.route == RADAD_RANGE_TILE;
                                }
    CHECK(tiles > 0 && tiles < lines, "both routes occur (%d of %d)", tiles, lines);

    // the named shapes of the GPU tests, literally
    for (int metric : {RADAD_METRIC_L2, RADAD_METRIC_IP, RADAD_METRIC_COSINE}) {
        for (int64_t nq : {17, 300}) {
            const RangePlan g = knn_range_plan(facts(20480, 64, 0, 0, 1, metric), nq, 64, 0);
            CHECK(g.route == RADAD_RANGE_TILE && g.plan.emit_cap == 4096 && g.launches == 1, "n 20480 d 64 q %lld", (long long)nq);
            const RangePlan t = knn_range_plan(facts(16640 + 37, 64, 0, 0, 1, metric), nq, 64, 0);
            CHECK(t.route == RADAD_RANGE_TILE && t.plan.emit_cap == 4096 && t.launches == 1, "the GPU tests' store, q %lld", (long long)nq);
            const RangePlan w = knn_range_plan(facts(16640 + 37, 128, 0, 0, 1, metric), nq, 64, 0);
            CHECK(w.route == RADAD_RANGE_TILE && w.launches == 1, "... at dim 128");
        }
        CHECK(knn_range_plan(facts(20480, 64, 0, 0, 1, metric), 16, 64, 0).route == RADAD_RANGE_EXACT, "q = 16");
        CHECK(knn_range_plan(facts(20480, 64, 0, 0, 1, metric), 3, 64, 0).route == RADAD_RANGE_EXACT, "q = 3");
        CHECK(knn_range_plan(facts(16383, 64, 0, 0, 1, metric), 300, 64, 0).route == RADAD_RANGE_EXACT, "n = 16383");
        CHECK(knn_range_plan(facts(1000, 64, 0, 0, 1, metric), 300, 64, 0).route == RADAD_RANGE_EXACT, "n = 1000");
        CHECK(knn_range_plan(facts(20480, 96, 0, 0, 1, metric), 300, 64, 0).route == RADAD_RANGE_EXACT, "d = 96");
        CHECK(knn_range_plan(facts(20480, 36, 0, 0, 1, metric), 300, 64, 0).route == RADAD_RANGE_EXACT, "d = 36");
        CHECK(knn_range_plan(facts(20480, 64, 1, 0, 1, metric), 300, 64, 0).route == RADAD_RANGE_EXACT, "plane off");
        CHECK(knn_range_plan(facts(20480, 64, 0, 0, 1, metric), 300, 64, 8).route == RADAD_RANGE_EXACT, "skip = 8");
    }
    {
        const RangePlan b = knn_range_plan(facts(1000000, 512, 0, 0, 1, RADAD_METRIC_COSINE), 1024, 128, 0);
        CHECK(b.route == RADAD_RANGE_TILE && b.launches == 1 && b.plan.emit_cap == 4096, "the benchmark's store");
    }

    // the tuning state is read, never written
    {
        KnnTuning t;
        t.hi_skip = 8;
        const RangePlan x = knn_range_plan(facts(20480, 64, 0, 0), 300, 64, t.hi_skip);
        CHECK(x.route == RADAD_RANGE_EXACT && t.hi_skip == 8 && t.cap_boost == 1, "hi_skip read only");
    }
    printf("lines %d tile %d\n", lines, tiles);
    if (failures) { printf("knn_range_plan_check: %d FAILED\n", failures); return 1; }
    printf("knn_range_plan_check: ok\n");
    return 0;
}
