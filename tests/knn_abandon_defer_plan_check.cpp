// knn_abandon_defer_plan_check.cpp -- stand-alone check of the host side of the deferral of a vetoed tile's live rows (knn_plan.h:
// knn_abandon_defer, knn_defer_list_cap, knn_defer_counter), driven by tests/test_knn_abandon_defer_plan.py.  No GPU, no HIP: it
// includes the planner header alone -- the host launches from the same text.
//
//   * eligibility: a launch defers exactly when it takes the abandoning instantiation (not the sample, not a K split, not a per-call
//     bias, the abandon on), has <= 8 query tiles, is not dealt, is one of the search's first KNN_DEFER_SETS launches, addresses its
//     rows in 32 bits, and the option is on;
//   * the list of a query tile cannot overflow: capacity >= row tiles x KNN_DEFER_MAX_ROWS, for 1 ... 40 000 row tiles;
//   * the tail's grid covers the capacity: tail_splits x tail_rounds >= tail_tiles >= capacity / KW_M, tail_splits a multiple of 8;
//   * hand-computed anchors: 20 000 rows x 17 / 300 queries, and the benchmark's 1 M x 1024 in its two launches;
//   * the counters: inside the launch's own set of deal counters, distinct.
#include <cstdio>
#include <cstdlib>
#include <set>

#include "../include/radad_hip.h"
#include "knn_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                                                                        \
    do {                                                                                        \
        if (!(cond)) { ++failures; printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

static AbandonFacts abandoning(int dim) {
    AbandonFacts a;
    a.opt_abandon = 1; a.rsc = 0; a.sample = false; a.ksplit = 1; a.floors = true; a.per_call_bias = false; a.terms_current = true; a.dim = dim;
    return a;
}
static DeferFacts facts(int64_t rows, int dim, int n_qtiles, int cus = 256, int launch = 0) {
    DeferFacts f;
    f.opt_defer = 1; f.ab_ck = knn_abandon_launch(abandoning(dim)); f.dealt = false; f.launch = launch; f.rows = rows; f.row_bytes = dim * 2;
    f.n_qtiles = n_qtiles; f.cus = cus;
    return f;
}

int main() {
    // ---- eligibility
    {
        const DeferFacts ok = facts(20000, 512, 2);
        CHECK(ok.ab_ck == 1 && knn_abandon_defer(ok).defer, "the plain abandoning launch defers");
        for (int variant = 0; variant < 5; ++variant) {
            AbandonFacts a = abandoning(512);
            if (variant == 0) a.sample = true;
            if (variant == 1) a.ksplit = 2;
            if (variant == 2) a.per_call_bias = true;
            if (variant == 3) a.opt_abandon = 0;
            if (variant == 4) a.rsc = 1;
            DeferFacts f = ok;
            f.ab_ck = knn_abandon_launch(a);
            CHECK(f.ab_ck == 0 && !knn_abandon_defer(f).defer, "abandon variant %d", variant);
        }
        for (int qt = 1; qt <= 12; ++qt) {
            DeferFacts f = ok; f.n_qtiles = qt;
            CHECK(knn_abandon_defer(f).defer == (qt <= KNN_DEFER_MAX_QTILES), "%d query tiles", qt);
        }
        { DeferFacts f = ok; f.dealt = true; CHECK(!knn_abandon_defer(f).defer, "a dealt launch"); }
        { DeferFacts f = ok; f.opt_defer = 0; CHECK(!knn_abandon_defer(f).defer, "the option off"); }
        { DeferFacts f = ok; f.n_qtiles = 0; CHECK(!knn_abandon_defer(f).defer, "no query tile"); }
        for (int l = -1; l <= KNN_DEFER_SETS + 1; ++l) {
            DeferFacts f = ok; f.launch = l;
            CHECK(knn_abandon_defer(f).defer == (l >= 0 && l < KNN_DEFER_SETS), "launch %d", l);
        }
        // the tail addresses a launch's rows through one 32-bit descriptor
        { DeferFacts f = facts(4194240, 512, 4); CHECK(knn_abandon_defer(f).defer, "4 GiB - 64 KiB"); }
        { DeferFacts f = facts(4194241, 512, 4); CHECK(!knn_abandon_defer(f).defer, "one row more"); }
        { DeferFacts f = facts(5000000, 512, 4); CHECK(!knn_abandon_defer(f).defer, "5 M x 512"); }
        { DeferFacts f = facts(5000000, 128, 4); CHECK(knn_abandon_defer(f).defer, "5 M x 128"); }
        // a deal decision in front: the benchmark's launches with both options on are dealt, and then not deferred
        DealFacts df;
        df.opt_deal = 1; df.ab_ck = 1; df.launch = 1; df.row_tiles = 3395; df.n_qtiles = 4; df.n_splits = 64; df.cus = 256;
        DeferFacts f = facts(868928, 512, 4, 256, 1);
        f.dealt = knn_abandon_deal(df).dealt;
        CHECK(f.dealt && !knn_abandon_defer(f).defer, "dealt first");
    }
    // ---- capacity and grid
    for (int cus : {64, 104, 256, 304}) {
        for (int qt = 1; qt <= KNN_DEFER_MAX_QTILES; ++qt) {
            for (int64_t tiles = 1; tiles <= 40000; tiles += (tiles < 600 ? 1 : 97)) {
                for (int64_t rows : {(tiles - 1) * KW_M + 1, tiles * KW_M}) {
                    const DeferPlan d = knn_abandon_defer(facts(rows, 128, qt, cus));
                    CHECK(d.defer, "cus %d qt %d rows %lld", cus, qt, (long long)rows);
                    CHECK(d.list_cap >= tiles * KNN_DEFER_MAX_ROWS && d.list_cap == knn_defer_list_cap(rows), "capacity %lld for %lld tiles", (long long)d.list_cap, (long long)tiles);
                    CHECK((int64_t)d.tail_tiles * KW_M >= d.list_cap && (int64_t)(d.tail_tiles - 1) * KW_M < d.list_cap, "tail tiles %d for %lld", d.tail_tiles, (long long)d.list_cap);
                    CHECK(d.tail_splits >= 8 && d.tail_splits % 8 == 0 && d.tail_rounds >= 1, "grid %d x %d", d.tail_splits, d.tail_rounds);
                    CHECK((int64_t)d.tail_splits * d.tail_rounds >= d.tail_tiles && (int64_t)d.tail_splits * (d.tail_rounds - 1) < d.tail_tiles, "grid %d x %d for %d tiles", d.tail_splits, d.tail_rounds, d.tail_tiles);
                    CHECK(qt * d.tail_splits <= std::max(cus, 8 * qt), "no more workgroups than CUs (or eight per query tile): %d x %d on %d", qt, d.tail_splits, cus);
                }
            }
        }
    }
    // ---- anchors, by hand.  20 000 rows: 79 row tiles, 79 x 16 = 1264 entries, 5 tail tiles -> 8 splits, one round
    for (int qt : {1, 2}) {
        for (int dim : {128, 512}) {
            const DeferPlan d = knn_abandon_defer(facts(20000, dim, qt));
            CHECK(d.defer && d.list_cap == 1264 && d.tail_tiles == 5 && d.tail_splits == 8 && d.tail_rounds == 1, "20 000 x %d, %d query tiles: %lld %d %d %d", dim, qt,
                  (long long)d.list_cap, d.tail_tiles, d.tail_splits, d.tail_rounds);
            printf("anchor n20000_d%d_q%d %lld %d %d %d\n", dim, qt, (long long)d.list_cap, d.tail_tiles, d.tail_splits, d.tail_rounds);
        }
    }
    // 1 M x 512, 1024 queries (4 query tiles) on 256 CUs: launches of 131 072 rows (512 tiles) and 868 928 rows (3395 tiles):
    // 8192 entries = 32 tail tiles -> 32 splits x 1;  54 320 entries = 213 tail tiles -> 64 splits (256 CUs / 4 query tiles) x 4 rounds
    {
        const DeferPlan a = knn_abandon_defer(facts(131072, 512, 4, 256, 0)), b = knn_abandon_defer(facts(868928, 512, 4, 256, 1));
        CHECK(a.defer && a.list_cap == 8192 && a.tail_tiles == 32 && a.tail_splits == 32 && a.tail_rounds == 1, "the benchmark's first launch: %lld %d %d %d",
              (long long)a.list_cap, a.tail_tiles, a.tail_splits, a.tail_rounds);
        CHECK(b.defer && b.list_cap == 54320 && b.tail_tiles == 213 && b.tail_splits == 64 && b.tail_rounds == 4, "the benchmark's second launch: %lld %d %d %d",
              (long long)b.list_cap, b.tail_tiles, b.tail_splits, b.tail_rounds);
        CHECK(knn_defer_list_cap(1000000) == 3907 * 16, "the handle's lists for 1 M rows");
        printf("anchor bench_launch0 %lld %d %d %d\n", (long long)a.list_cap, a.tail_tiles, a.tail_splits, a.tail_rounds);
        printf("anchor bench_launch1 %lld %d %d %d\n", (long long)b.list_cap, b.tail_tiles, b.tail_splits, b.tail_rounds);
    }
    // ---- the counters: a deferring launch counts in its own set of deal counters
    {
        std::set<int> seen;
        for (int s = 0; s < KNN_DEFER_SETS; ++s) {
            for (int qt = 0; qt < KNN_DEFER_MAX_QTILES; ++qt) {
                const int c = knn_defer_counter(s, qt);
                CHECK(c >= knn_deal_counter(s, 0, 0) && c < knn_deal_counter(s, 0, 0) + KNN_DEAL_SLOTS * KNN_DEAL_MAX_QTILES && c < KNN_DEAL_COUNTERS, "set %d qt %d: %d", s, qt, c);
                CHECK(seen.insert(c).second, "counter %d twice", c);
            }
            const int t = knn_defer_tasks_counter(s);
            CHECK(t >= knn_deal_counter(s, 0, 0) && t < knn_deal_counter(s, 0, 0) + KNN_DEAL_SLOTS * KNN_DEAL_MAX_QTILES && seen.insert(t).second, "tasks counter of set %d: %d", s, t);
        }
    }
    static_assert(KNN_DEFER_MAX_ROWS == 16, "the measured setting");
    static_assert(RADAD_KNN_OPT_ABANDON_DEFER == 8, "the option");
    if (failures) { printf("knn_abandon_defer_plan_check: %d FAILED\n", failures); return 1; }
    printf("knn_abandon_defer_plan_check: ok\n");
    return 0;
}
