// knn_excl_scan_pq_plan_check.cpp -- stand-alone check of the host-only plan of radad_knn_search_excl_scan_pq (knn_excl_scan_pq_plan,
// knn_plan.h), driven by tests/test_knn_excl_scan_pq_plan.py.  No GPU, no HIP: it includes the planner header alone.
//
//   * the route is knn_excl_scan_route's over the whole grid of tests/knn_excl_scan_plan_check.cpp, whatever m;
//   * the facts the plan is made from are the caller's with cap_boost forced to 4 (whatever the handle's own): emit_cap is
//     min(RF_STAGE_MAX, max(4096, 32 (k + margin))) on the tile route, a speaker of 1500 rows fits it, and the re-rank stages it;
//   * scrub launches: 0 on the exact route and at m == 0, else 1 (sample) + (phases - 1) (each k_kth_floor) + 1 (re-rank), with the
//     phases recomputed here from knn_hi_phases; one workgroup per query;
//   * the smallest store (a multiple of 256 rows, dim 64, k = 100, 40 queries) this call's plan scans in two phases: printed for the GPU
//     test that needs the scrub in front of k_kth_floor.
#include <cstdio>
#include <cstdlib>

#include "knn_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                                                                        \
    do {                                                                                        \
        if (!(cond)) { ++failures; printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

static StoreFacts facts(int64_t n, int dim, int hi_off, int f16, int cap_boost = 1) {
    StoreFacts s;
    s.ntotal = n; s.dim = dim; s.metric = RADAD_METRIC_L2; s.hi_off = hi_off; s.f16 = f16; s.cap_boost = cap_boost;
    return s;
}

// the phases of the tile scan as knn.hip launches them for a plan
static int phases_of(const ScanPlan& p, int64_t n, int64_t nq) {
    return (int)knn_hi_phases(n, nq, (int64_t)8 * p.s_splits * KW_M, knn_hi_one_go(p, n)).size() - 1;
}

int main() {
    static_assert(KNN_EXCL_SCAN_PQ_CAP_BOOST == 4, "the widened candidate buffers");
    int lines = 0, tiles = 0, multi = 0;
    for (int64_t n : {16383, 16384, 20480, 49152, 1000000})
        for (int dim : {64, 96, 512})
            for (int64_t nq : {1, 16, 17, 300, 1024})
                for (int k : {1, 10, 58, 59, 128, 129, 1024})
                    for (int hi_off : {0, 1})
                        for (int skip : {0, 8})
                            for (int f16 : {0, 1})
                                for (int m : {0, 1, 64})
                                    for (int boost : {1, 4}) {
                                        const StoreFacts s = facts(n, dim, hi_off, f16, boost);
                                        const ExclScanPqPlan x = knn_excl_scan_pq_plan(s, nq, k, m, skip);
                                        const int want = knn_excl_scan_route(s, nq, k, skip);
                                        CHECK(x.route == want, "n %lld dim %d nq %lld k %d hi_off %d skip %d f16 %d m %d: route %d, knn_excl_scan_route %d",
                                              (long long)n, dim, (long long)nq, k, hi_off, skip, f16, m, x.route, want);
                                        CHECK(x.facts.cap_boost == 4 && x.facts.ntotal == n && x.facts.dim == dim && x.facts.hi_off == hi_off &&
                                              x.facts.f16 == f16 && x.facts.metric == s.metric, "the caller's facts with the forced boost");
                                        CHECK(x.plan.nq == nq && x.plan.k == k, "the plan is this batch's");
                                        if (x.route == RADAD_EXCL_SCAN_TILE) {
                                            CHECK(x.plan.kind == RADAD_SCAN_HI_TILE, "tile route, plan kind %d", x.plan.kind);
                                            const int ec = std::min(RF_STAGE_MAX, std::max(4096, 32 * (k + KNN_MARGIN)));
                                            CHECK(x.plan.emit_cap == ec && x.plan.emit_cap >= 4096 && x.plan.emit_cap <= RF_STAGE_MAX, "emit_cap %d, expected %d", x.plan.emit_cap, ec);
                                            CHECK(x.plan.emit_cap >= 1500 + 32 * (k + KNN_MARGIN) || k > 75, "a speaker of 1500 rows beside the scan's own ~8..32 (k + margin)");
                                            CHECK(x.plan.plen == x.plan.emit_cap && x.plan.n_parts == 1, "one candidate buffer per query");
                                            CHECK(x.plan.cap == std::max(k + KNN_CERT_EXTRA, 4 * KNN_CERT_CAP), "re-rank cap %d", x.plan.cap);
                                            const int ph = phases_of(x.plan, n, nq);
                                            CHECK(x.phases == ph && ph >= 1, "phases %d, knn_hi_phases %d", x.phases, ph);
                                            CHECK(x.scrub_launches == (m == 0 ? 0 : 1 + (ph - 1) + 1), "m %d phases %d: %d scrub launches", m, ph, x.scrub_launches);
                                            CHECK(x.scrub_grid == (m == 0 ? 0 : nq), "grid %lld", (long long)x.scrub_grid);
                                            multi += ph > 1;
                                        } else {
                                            CHECK(x.plan.kind != RADAD_SCAN_HI_TILE && x.plan.emit_cap == 0, "exact route: no tile plan");
                                            CHECK(x.phases == 0 && x.scrub_launches == 0 && x.scrub_grid == 0, "exact route: no scrub");
                                        }
                                        // the handle's own boost changes nothing of this call's plan
                                        if (boost == 4) {
                                            const ExclScanPqPlan y = knn_excl_scan_pq_plan(facts(n, dim, hi_off, f16, 1), nq, k, m, skip);
                                            CHECK(y.route == x.route && y.plan.emit_cap == x.plan.emit_cap && y.plan.cap == x.plan.cap && y.phases == x.phases &&
                                                  y.scrub_launches == x.scrub_launches, "plan depends on the handle's cap_boost");
                                        }
                                        if (boost == 1)
                                            printf("plan n%lld_d%d_q%lld_k%d_off%d_skip%d_f16%d_m%d %d %d %d\n", (long long)n, dim, (long long)nq, k, hi_off, skip,
                                                   f16, m, x.route, x.phases, x.scrub_launches);
                                        ++lines;
                                        tiles += x.route == RADAD_EXCL_SCAN_TILE;
                                    }
    CHECK(tiles > 0 && tiles < lines && multi > 0, "both routes and multi-phase scans occur (%d of %d, %d)", tiles, lines, multi);

    // the named shapes of the GPU tests, literally
    {
        const ExclScanPqPlan g = knn_excl_scan_pq_plan(facts(20480, 64, 0, 0), 300, 10, 1, 0);
        CHECK(g.route == RADAD_EXCL_SCAN_TILE && g.plan.emit_cap == 4096 && g.phases == 1 && g.scrub_launches == 2 && g.scrub_grid == 300, "the grid's store");
        const ExclScanPqPlan e = knn_excl_scan_pq_plan(facts(4096, 64, 0, 0), 40, 10, 1, 0);
        CHECK(e.route == RADAD_EXCL_SCAN_EXACT && e.scrub_launches == 0, "a 4096-row store");
        const ExclScanPqPlan b = knn_excl_scan_pq_plan(facts(1000000, 512, 0, 0), 1024, 10, 1, 0);
        // (the plain search's 1024-entry buffers take two phases there; a third of 4096 entries holds what the sample's floor alone admits)
        CHECK(b.route == RADAD_EXCL_SCAN_TILE && b.phases == 1 && b.scrub_launches == 2, "the benchmark's store: %d phases, %d launches", b.phases, b.scrub_launches);
        const StoreFacts plain = facts(1000000, 512, 0, 0);
        const ScanPlan pp = knn_finish_plan(plain, 1024, 10, KNN_MARGIN, knn_tile_eligibility(plain, 1024, 10, KNN_MARGIN), true, false);
        CHECK(pp.emit_cap == 1024 && phases_of(pp, 1000000, 1024) == 2, "the plain search of the benchmark's store");
    }

    // the tuning state is read, never written
    {
        KnnTuning t;
        t.hi_skip = 8;
        const ExclScanPqPlan x = knn_excl_scan_pq_plan(facts(20480, 64, 0, 0), 300, 10, 1, t.hi_skip);
        CHECK(x.route == RADAD_EXCL_SCAN_EXACT && t.hi_skip == 8 && t.cap_boost == 1, "hi_skip read only");
    }

    // the smallest store of whole tiles (dim 64, k = 100, 40 queries) that this call's plan scans in two phases
    {
        int64_t two = 0;
        for (int64_t n = 16384; n <= 4 * 1048576 && !two; n += 256) {
            const ExclScanPqPlan x = knn_excl_scan_pq_plan(facts(n, 64, 0, 0), 40, 100, 1, 0);
            if (x.route == RADAD_EXCL_SCAN_TILE && x.phases >= 2) two = n;
        }
        CHECK(two > 0, "no two-phase store below 4 M rows");
        if (two) {
            const ExclScanPqPlan x = knn_excl_scan_pq_plan(facts(two, 64, 0, 0), 40, 100, 1, 0);
            const ExclScanPqPlan y = knn_excl_scan_pq_plan(facts(two - 256, 64, 0, 0), 40, 100, 1, 0);
            CHECK(x.phases == 2 && x.scrub_launches == 3 && (y.route != RADAD_EXCL_SCAN_TILE || y.phases == 1), "the boundary");
            const std::vector<int64_t> r = knn_hi_phases(two, 40, (int64_t)8 * x.plan.s_splits * KW_M, knn_hi_one_go(x.plan, two));
            printf("two_phase_rows %lld first_phase_rows %lld emit_cap %d\n", (long long)two, (long long)r[1], x.plan.emit_cap);
        }
    }
    printf("lines %d tile %d multi %d\n", lines, tiles, multi);
    if (failures) { printf("knn_excl_scan_pq_plan_check: %d FAILED\n", failures); return 1; }
    printf("knn_excl_scan_pq_plan_check: ok\n");
    return 0;
}
