// knn_range_smallq_plan_check.cpp -- stand-alone check of the host-only plan of the range calls with RADAD_KNN_OPT_RANGE_SMALLQ
// (knn_range_plan / knn_range_excl_plan, knn_plan.h), driven by tests/test_knn_range_smallq_plan.py.  No GPU, no HIP: it includes the
// planner header alone.
//
// Over the grid of tests/knn_range_plan_check.cpp, extended by the option (and by RADAD_KNN_OPT_SMALLQ_HI, which gates it), for the plain
// plan and both modes of knn_range_excl_plan:
//   * option 0: route, facts, launches and every member of the plan are what the rule in force before the option gives (restated here);
//   * option 1: RADAD_RANGE_STREAM exactly when the handle is not on its fp32 fallback, the tile route is not taken and the plain
//     search of the batch at k = 1 could stream the plane -- in words: <= 16 queries, dim % 64 == 0, >= 16 384 rows, the plane on,
//     opt_smallq_hi, the f16 query block within the LDS budget; every other plan is the option-0 plan;
//   * the stream plan: kind RADAD_SCAN_HI_SMALLQ, f16 queries, ONE 4096-entry buffer per query, one launch, one wave per slice
//     (never the K-split form), n_splits x 4 x rows_per_wave >= ntotal, the query block alone as LDS;
//   * one set for the batch: biased == hi_q and one pre-pass launch on the stream route too, the bias array laid out as for the tile route;
//   * knn_finish_plan's streaming geometry is what it was before it moved into knn_sq_stream_geometry (the old rule, restated here).
#include <cstdio>
#include <cstdlib>

#include "knn_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                                                                        \
    do {                                                                                        \
        if (!(cond)) { ++failures; printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

static StoreFacts facts(int64_t n, int dim, int hi_off, int f16, int opt, int smallq_hi = 1, int metric = RADAD_METRIC_L2) {
    StoreFacts s;
    s.ntotal = n; s.dim = dim; s.metric = metric; s.hi_off = hi_off; s.f16 = f16; s.opt_smallq_hi = smallq_hi; s.opt_range_smallq = opt;
    return s;
}

static bool same_plan(const ScanPlan& a, const ScanPlan& b) {
    return a.kind == b.kind && a.nq == b.nq && a.k == b.k && a.l2 == b.l2 && a.n_qtiles == b.n_qtiles && a.n_splits == b.n_splits &&
           a.chunk_rows == b.chunk_rows && a.ksel == b.ksel && a.ksel_sq == b.ksel_sq && a.s_splits == b.s_splits && a.emit_cap == b.emit_cap &&
           a.cap == b.cap && a.plen == b.plen && a.n_parts == b.n_parts && a.sq_rows_per_wave == b.sq_rows_per_wave && a.sq_ksplit == b.sq_ksplit &&
           a.sq_lds == b.sq_lds && a.dense_plen == b.dense_plen && a.xgroup == b.xgroup && a.reported_qtiles == b.reported_qtiles &&
           a.block_threads == b.block_threads && a.hi_q == b.hi_q && a.biased == b.biased && a.mu == b.mu;
}

// the range plan as it was before the option: route from knn_excl_scan_route at k = 1, the plain search's plan over the boosted facts
static RangePlan parent_range_plan(const StoreFacts& s, int64_t nq, int fp32_searches_left) {
    RangePlan x;
    const bool tile = knn_excl_scan_route(s, nq, 1, fp32_searches_left) == RADAD_EXCL_SCAN_TILE;
    x.route = tile ? RADAD_RANGE_TILE : RADAD_RANGE_EXACT;
    x.facts = s;
    x.facts.cap_boost = KNN_EXCL_SCAN_PQ_CAP_BOOST;
    const TileEligibility t = knn_tile_eligibility(x.facts, nq, 1, KNN_MARGIN);
    x.plan = knn_finish_plan(x.facts, nq, 1, KNN_MARGIN, t, tile, false);
    if (tile) x.launches = (int)knn_hi_phases(s.ntotal, nq, (int64_t)8 * x.plan.s_splits * KW_M, true).size() - 1;
    return x;
}

// knn_finish_plan's streaming geometry as it was written inline
static void old_stream_geometry(int64_t ntotal, int dim, bool smallq_hi, int ksel_sq, int* rows_per_wave, int* n_splits) {
    const int64_t waves_wanted = 1024 * ((smallq_hi && ksel_sq <= 16) ? 3 : 2);
    const size_t rb = smallq_hi ? (size_t)dim * 2 : (size_t)dim * 4;
    const int64_t rows_min = std::max<int64_t>(16, std::min<int64_t>(128, ceil_div64(ceil_div64(128 * 1024, (int64_t)rb), 16) * 16));
    int64_t rpw = std::max<int64_t>(ceil_div64(ceil_div64(ntotal, waves_wanted), 16) * 16, rows_min);
    while (rpw < 128 && ceil_div64(ceil_div64(ntotal, rpw), 4) * ksel_sq > RF_STAGE_MAX_SMALLQ) rpw += 16;
    *rows_per_wave = (int)rpw;
    *n_splits = (int)ceil_div64(ceil_div64(ntotal, rpw), 4);
}

static void check_stream_plan(const ScanPlan& p, const StoreFacts& s, int64_t nq, int launches) {
    CHECK(p.kind == RADAD_SCAN_HI_SMALLQ && p.hi_q && p.f16_queries(), "kind %d", p.kind);
    CHECK(p.emit_cap == 4096 && p.plen == 4096 && p.n_parts == 1 && launches == 1, "emit_cap %d plen %d n_parts %d launches %d", p.emit_cap,
          p.plen, p.n_parts, launches);
    CHECK(KNN_RANGE_STREAM_CAP == 4096, "the re-rank's sort is sized for 4096 entries");
    CHECK(!p.sq_ksplit && p.n_qtiles == 1 && p.block_threads == SQ_THREADS, "one wave per slice, 256 threads");
    CHECK(p.sq_rows_per_wave >= 16 && p.sq_rows_per_wave % 16 == 0, "rows per wave %d", p.sq_rows_per_wave);
    CHECK((int64_t)p.n_splits * 4 * p.sq_rows_per_wave >= s.ntotal, "n %lld: %d workgroups x 4 x %d rows", (long long)s.ntotal, p.n_splits,
          p.sq_rows_per_wave);
    CHECK((int64_t)(p.n_splits - 1) * 4 * p.sq_rows_per_wave < s.ntotal, "no workgroup wholly beyond the store");
    CHECK(p.sq_lds == 2 * (size_t)nq * (s.dim + 8) && p.sq_lds <= SQ_LDS_BUDGET, "LDS %zu", p.sq_lds);
    CHECK(p.nq == nq && p.k == 1, "the plan's batch");
    // the search's workspace holds the buffers: nq x 4096 entries
    CHECK(knn_search_layout(s, p, RADAD_Q_F32).cand_elems == (size_t)nq * 4096, "candidate buffers");
}

int main() {
    static_assert(RADAD_RANGE_TILE == 0 && RADAD_RANGE_EXACT == 1 && RADAD_RANGE_STREAM == 2, "the routes radad_knn_last_range reports");
    static_assert(RADAD_KNN_OPT_RANGE_SMALLQ == 6, "the option");
    CHECK(StoreFacts().opt_range_smallq == 0, "the default is off");
    int lines = 0, streams = 0, tiles = 0;
    for (int64_t n : {16383, 16384, 20480, 49152, 1000000})
        for (int dim : {64, 96, 512, 5376})
            for (int64_t nq : {1, 16, 17, 300, 1024})
                for (int m : {1, 10, 128, 1024})
                    for (int hi_off : {0, 1})
                        for (int skip : {0, 8})
                            for (int f16 : {0, 1})
                                for (int sq : {0, 1})
                                    for (int opt : {0, 1}) {
                                        const StoreFacts s = facts(n, dim, hi_off, f16, opt, sq);
                                        const RangePlan x = knn_range_plan(s, nq, m, skip);
                                        const RangePlan par = parent_range_plan(s, nq, skip);
                                        const bool tile = par.route == RADAD_RANGE_TILE;
                                        // the conjunction, once through the planner's own predicates and once in words
                                        const bool want = opt == 1 && skip == 0 && !tile && knn_smallq_hi_eligible(s, nq, 1, KNN_MARGIN, false, false);
                                        const bool words = opt == 1 && skip == 0 && nq <= 16 && dim % 64 == 0 && n >= 16384 && !hi_off && sq == 1 &&
                                                           2 * (size_t)nq * (dim + 8) + SQ_SLOT_BYTES <= SQ_LDS_BUDGET;
                                        CHECK(want == words, "the conjunction in words: n %lld dim %d nq %lld hi_off %d skip %d sq %d", (long long)n, dim,
                                              (long long)nq, hi_off, skip, sq);
                                        CHECK((x.route == RADAD_RANGE_STREAM) == want, "n %lld dim %d nq %lld hi_off %d skip %d f16 %d sq %d opt %d: route %d",
                                              (long long)n, dim, (long long)nq, hi_off, skip, f16, sq, opt, x.route);
                                        CHECK(x.facts.cap_boost == 4 && x.facts.ntotal == n && x.facts.dim == dim && x.facts.opt_range_smallq == opt,
                                              "the caller's facts with the forced boost");
                                        if (x.route == RADAD_RANGE_STREAM) {
                                            check_stream_plan(x.plan, x.facts, nq, x.launches);
                                        } else {
                                            CHECK(x.route == par.route && x.launches == par.launches && same_plan(x.plan, par.plan),
                                                  "n %lld dim %d nq %lld opt %d: not the plan in force before the option", (long long)n, dim, (long long)nq, opt);
                                        }
                                        if (opt == 0) CHECK(x.route != RADAD_RANGE_STREAM, "the option is off");
                                        // 16 or fewer queries too wide for the LDS take the tile route, option or not
                                        if (nq == 16 && dim == 5376 && !hi_off && skip == 0 && n >= 16384) CHECK(x.route == RADAD_RANGE_TILE, "16 x 5376");
                                        // both modes of the exclusion plan
                                        for (int mode : {KNN_RANGE_EXCL_BATCH, KNN_RANGE_EXCL_PER_QUERY}) {
                                            const RangeExclPlan e = knn_range_excl_plan(s, nq, m, mode, 4, skip);
                                            CHECK(e.route == x.route && e.launches == x.launches && e.scrub_launches == 0, "mode %d: route %d launches %d", mode,
                                                  e.route, e.launches);
                                            ScanPlan expect = x.plan;
                                            if (mode == KNN_RANGE_EXCL_BATCH) expect.biased = expect.hi_q;
                                            CHECK(same_plan(e.plan, expect), "mode %d: the range plan's plan", mode);
                                            CHECK(e.prepass_launches == (mode == KNN_RANGE_EXCL_BATCH && x.route != RADAD_RANGE_EXACT ? 1 : 0), "mode %d: %d pre-pass launches",
                                                  mode, e.prepass_launches);
                                            if (x.route == RADAD_RANGE_STREAM) {
                                                check_stream_plan(e.plan, e.facts, nq, e.launches);
                                                if (mode == KNN_RANGE_EXCL_BATCH) CHECK(e.plan.biased, "one set for the batch: the biased instantiation");
                                            }
                                            if (knn_exact_fits(dim, m)) {
                                                const RangeLayout B = knn_range_layout(e.facts, nq, m);
                                                const RangeExclLayout E = knn_range_excl_layout(e.facts, nq, m, e.route);
                                                const RangeExclLayout T = knn_range_excl_layout(e.facts, nq, m, RADAD_RANGE_TILE);
                                                CHECK(E.lists.bytes == B.bytes && E.admit == B.bytes && E.bias >= E.admit + (size_t)E.n_words * 8 && E.bias % 256 == 0,
                                                      "the bitmap behind the lists");
                                                CHECK(E.bytes >= E.bias + (e.route != RADAD_RANGE_EXACT ? (size_t)n * 4 : 0), "the bias array behind the bitmap");
                                                if (e.route == RADAD_RANGE_STREAM)
                                                    CHECK(E.admit == T.admit && E.bias == T.bias && E.bytes == T.bytes, "the stream route's layout is the tile route's");
                                            }
                                        }
                                        if (m == 10)
                                            printf("plan n%lld_d%d_q%lld_off%d_skip%d_f16%d_sq%d_opt%d %d %d %d %d %d\n", (long long)n, dim, (long long)nq, hi_off, skip,
                                                   f16, sq, opt, x.route, x.plan.emit_cap, x.launches, x.plan.sq_rows_per_wave, x.plan.n_splits);
                                        ++lines;
                                        streams += x.route == RADAD_RANGE_STREAM;
                                        tiles += x.route == RADAD_RANGE_TILE;
                                    }
    CHECK(streams > 0 && tiles > 0 && streams + tiles < lines, "all three routes occur (%d stream, %d tile of %d)", streams, tiles, lines);

    // the named shapes, literally
    for (int metric : {RADAD_METRIC_L2, RADAD_METRIC_IP, RADAD_METRIC_COSINE}) {
        auto route = [&](int64_t n, int dim, int64_t nq, int hi_off = 0, int skip = 0, int sq = 1, int opt = 1) {
            return knn_range_plan(facts(n, dim, hi_off, 0, opt, sq, metric), nq, 64, skip).route;
        };
        CHECK(route(20480, 64, 1) == RADAD_RANGE_STREAM && route(20480, 64, 16) == RADAD_RANGE_STREAM, "q = 1 and q = 16 at n = 20480, d = 64");
        CHECK(route(20480, 64, 17) == RADAD_RANGE_TILE, "q = 17 is tile");
        CHECK(route(16383, 64, 1) == RADAD_RANGE_EXACT, "n = 16383");
        CHECK(route(20480, 96, 1) == RADAD_RANGE_EXACT, "d = 96");
        CHECK(route(20480, 64, 1, 1) == RADAD_RANGE_EXACT, "plane off");
        CHECK(route(20480, 64, 1, 0, 8) == RADAD_RANGE_EXACT, "skip = 8");
        CHECK(route(20480, 64, 1, 0, 0, 0) == RADAD_RANGE_EXACT, "smallq_hi = 0");
        CHECK(route(20480, 5376, 16) == RADAD_RANGE_TILE, "16 queries of d = 5376 stay tile");
        CHECK(route(20480, 64, 1, 0, 0, 1, 0) == RADAD_RANGE_EXACT && route(20480, 64, 16, 0, 0, 1, 0) == RADAD_RANGE_EXACT, "the option off: exact, as before");
        // the GPU tests' store: 16 677 rows, slices of 128 rows, 33 workgroups, the last one's fourth wave beyond the store
        for (int dim : {64, 128, 576}) {
            const RangePlan g = knn_range_plan(facts(16640 + 37, dim, 0, 0, 1, 1, metric), dim == 576 ? 3 : 16, 64, 0);
            CHECK(g.route == RADAD_RANGE_STREAM && g.plan.sq_rows_per_wave == 128 && g.plan.n_splits == 33, "d %d: route %d, %d rows per wave, %d workgroups",
                  dim, g.route, g.plan.sq_rows_per_wave, g.plan.n_splits);
        }
    }
    {   // a store the plain search would K-split (the reference's own: 25 423 x 5376, one query) runs one wave per slice here
        const StoreFacts s = facts(25423, 5376, 0, 0, 1, 1, RADAD_METRIC_COSINE);
        const ScanPlan plain = knn_finish_plan(s, 1, 15, KNN_MARGIN, knn_tile_eligibility(s, 1, 15, KNN_MARGIN), false, true);
        const RangePlan r = knn_range_plan(s, 1, 64, 0);
        CHECK(plain.sq_ksplit && r.route == RADAD_RANGE_STREAM && !r.plan.sq_ksplit, "K-split");
        check_stream_plan(r.plan, r.facts, 1, r.launches);
        const RangePlan b = knn_range_plan(facts(1000000, 512, 0, 0, 1, 1, RADAD_METRIC_COSINE), 1, 128, 0);
        CHECK(b.route == RADAD_RANGE_STREAM && b.plan.sq_rows_per_wave == 336 && b.plan.n_splits == 745, "the benchmark's store: %d rows per wave, %d workgroups",
              b.plan.sq_rows_per_wave, b.plan.n_splits);
    }

    // knn_finish_plan's streaming geometry did not move
    int compared = 0;
    for (int64_t n : {1, 15, 16, 1000, 16383, 16384, 16677, 25423, 49152, 100000, 1000000, 10000000, 100000000})
        for (int dim : {32, 64, 96, 512, 576, 1024, 3584, 5376})
            for (int64_t nq : {1, 3, 16})
                for (int k : {1, 10, 15, 16, 17, 26})
                    for (int f16 : {0, 1})
                        for (int smallq_hi : {0, 1}) {
                            StoreFacts s = facts(n, dim, 0, f16, 0);
                            s.opt_dense = 0;
                            if (smallq_hi && dim % 64 != 0) continue;
                            const ScanPlan p = knn_finish_plan(s, nq, k, KNN_MARGIN, TileEligibility(), false, smallq_hi != 0);
                            if ((p.kind != RADAD_SCAN_HI_SMALLQ && p.kind != RADAD_SCAN_F32_SMALLQ) || p.sq_ksplit) continue;
                            int rpw, ns;
                            old_stream_geometry(n, dim, smallq_hi != 0, p.ksel_sq, &rpw, &ns);
                            CHECK(p.sq_rows_per_wave == rpw && p.n_splits == ns && p.n_qtiles == 1 && p.n_parts == ns, "n %lld dim %d nq %lld k %d hi %d: %d x %d, was %d x %d",
                                  (long long)n, dim, (long long)nq, k, smallq_hi, p.sq_rows_per_wave, p.n_splits, rpw, ns);
                            ++compared;
                        }
    CHECK(compared > 1000, "streaming plans compared: %d", compared);

    // the tuning state is read, never written
    {
        KnnTuning t;
        t.hi_skip = 8;
        const RangePlan x = knn_range_plan(facts(20480, 64, 0, 0, 1), 1, 64, t.hi_skip);
        CHECK(x.route == RADAD_RANGE_EXACT && t.hi_skip == 8 && t.cap_boost == 1, "hi_skip read only");
    }
    printf("lines %d stream %d tile %d geometry %d\n", lines, streams, tiles, compared);
    if (failures) { printf("knn_range_smallq_plan_check: %d FAILED\n", failures); return 1; }
    printf("knn_range_smallq_plan_check: ok\n");
    return 0;
}
