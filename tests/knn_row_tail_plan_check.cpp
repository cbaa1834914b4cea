// knn_row_tail_plan_check.cpp -- stand-alone check of the host side of the row tail (knn_plan.h: knn_defer_rowtail, knn_rowtail_span,
// knn_rowtail_takes), driven by tests/test_knn_row_tail_plan.py.  No GPU, no HIP: it includes the planner header alone -- the kernel
// walks its groups through the same knn_rowtail_span and the host launches the grid knn_defer_rowtail returns.
//
//   * the grid: n_splits a multiple of 8, at least 8, no more than KNN_ROWTAIL_WG_PER_CU workgroups per CU over all query tiles (or
//     eight per query tile), no more than a full list has groups (in eights); n_splits x rounds covers the capacity, rounds is tight;
//   * the walk: for list capacities from one row tile's (16 entries) to the benchmark's (8192 and 54 320), query tiles 1 ... 8 and
//     64 / 256 / 304 CUs, and counts 0, 1, 15, 16, 17, 33, ..., the capacity: every entry 0 ... count - 1 is taken by exactly one
//     (workgroup, round), no entry >= count is taken, a workgroup never resumes after an empty span, and none needs more than `rounds`;
//   * hand-computed anchors: the benchmark's two launches on 256 CUs, and a 20 000-row store;
//   * which tail takes a list: exactly one of the two for every count.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/radad_hip.h"
#include "knn_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                                                                        \
    do {                                                                                        \
        if (!(cond)) { ++failures; printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

// one list of `count` entries walked by the grid of `plan`: how often each entry is taken
static void walk(const RowTailPlan& plan, int64_t cap, int count, const char* what) {
    std::vector<unsigned char> taken((size_t)std::max<int64_t>(cap, 1), 0);
    int64_t outside = 0;
    int worst_rounds = 0;
    for (int split = 0; split < plan.n_splits; ++split) {
        int round = 0;
        for (;; ++round) {
            const RowTailSpan sp = knn_rowtail_span(split, round, plan.n_splits, count);
            if (sp.n <= 0) break;                       // (the kernel leaves here)
            CHECK(sp.n <= KNN_ROWTAIL_GROUP && sp.first % KNN_ROWTAIL_GROUP == 0, "%s: span %d + %d", what, sp.first, sp.n);
            for (int e = sp.first; e < sp.first + sp.n; ++e) {
                if (e < 0 || e >= count) ++outside;
                else ++taken[(size_t)e];
            }
        }
        worst_rounds = std::max(worst_rounds, round);
        // nothing behind an empty span: the groups of a workgroup ascend
        for (int later = round; later < round + 3; ++later) CHECK(knn_rowtail_span(split, later, plan.n_splits, count).n == 0, "%s: split %d resumes at round %d", what, split, later);
    }
    CHECK(outside == 0, "%s: %lld entries taken at or past the count %d", what, (long long)outside, count);
    int64_t wrong = 0;
    for (int e = 0; e < count; ++e) wrong += taken[(size_t)e] != 1;
    CHECK(wrong == 0, "%s: %lld of %d entries not taken exactly once", what, (long long)wrong, count);
    CHECK(worst_rounds <= plan.rounds, "%s: a workgroup takes %d groups, the plan says %d", what, worst_rounds, plan.rounds);
}

int main() {
    const int64_t caps[] = {16, 32, 48, 256, 1264, 4096, 8192, 8208, 54320, 62512};
    for (int cus : {64, 256, 304}) {
        for (int qt = 1; qt <= KNN_DEFER_MAX_QTILES; ++qt) {
            for (int64_t cap : caps) {
                const RowTailPlan r = knn_defer_rowtail(cap, qt, cus);
                char what[96];
                snprintf(what, sizeof what, "cus %d qt %d cap %lld", cus, qt, (long long)cap);
                CHECK((int64_t)r.groups * KNN_ROWTAIL_GROUP >= cap && (int64_t)(r.groups - 1) * KNN_ROWTAIL_GROUP < cap, "%s: groups %d", what, r.groups);
                CHECK(r.n_splits >= 8 && r.n_splits % 8 == 0, "%s: n_splits %d", what, r.n_splits);
                CHECK(qt * r.n_splits <= std::max(KNN_ROWTAIL_WG_PER_CU * cus, 8 * qt), "%s: %d x %d workgroups", what, qt, r.n_splits);
                CHECK(r.n_splits <= (r.groups + 7) / 8 * 8, "%s: %d workgroups for %d groups", what, r.n_splits, r.groups);
                CHECK((int64_t)r.n_splits * r.rounds >= r.groups && (int64_t)r.n_splits * (r.rounds - 1) < r.groups, "%s: %d x %d for %d groups", what, r.n_splits, r.rounds, r.groups);
                std::vector<int> counts = {0, 1, 15, 16, 17, 31, 32, 33, (int)cap - 1, (int)cap};
                for (int m : {1, 2, 3}) { counts.push_back(r.n_splits * KNN_ROWTAIL_GROUP * m - 1); counts.push_back(r.n_splits * KNN_ROWTAIL_GROUP * m); counts.push_back(r.n_splits * KNN_ROWTAIL_GROUP * m + 1); }
                for (int c : counts) {
                    if (c < 0 || c > cap) continue;
                    char w2[160];
                    snprintf(w2, sizeof w2, "%s count %d", what, c);
                    walk(r, cap, c, w2);
                }
            }
        }
    }
    // no list, no query tile, no CU: no grid
    CHECK(knn_defer_rowtail(0, 4, 256).n_splits == 0 && knn_defer_rowtail(16, 0, 256).n_splits == 0 && knn_defer_rowtail(16, 4, 0).n_splits == 0, "degenerate");
    // ---- anchors, by hand (256 CUs x 2 workgroups = 512; 4 query tiles -> 128 workgroups per query tile)
    //   the benchmark's first launch:  8192 entries =  512 groups -> min(128, 512) = 128 workgroups x 4 rounds
    //   the benchmark's second launch: 54 320 entries = 3395 groups -> 128 workgroups x 27 rounds (26 x 128 = 3328 < 3395)
    //   20 000 rows, 1 or 2 query tiles: 1264 entries = 79 groups -> min(512 or 256, 80) = 80 workgroups x 1 round;
    //   8 query tiles: min(64, 80) = 64 workgroups x 2 rounds
    {
        const RowTailPlan a = knn_defer_rowtail(8192, 4, 256), b = knn_defer_rowtail(54320, 4, 256);
        CHECK(a.groups == 512 && a.n_splits == 128 && a.rounds == 4, "the benchmark's first launch: %d %d %d", a.groups, a.n_splits, a.rounds);
        CHECK(b.groups == 3395 && b.n_splits == 128 && b.rounds == 27, "the benchmark's second launch: %d %d %d", b.groups, b.n_splits, b.rounds);
        printf("anchor bench_launch0 %d %d %d\n", a.groups, a.n_splits, a.rounds);
        printf("anchor bench_launch1 %d %d %d\n", b.groups, b.n_splits, b.rounds);
        for (int qt : {1, 2}) {
            const RowTailPlan c = knn_defer_rowtail(knn_defer_list_cap(20000), qt, 256);
            CHECK(c.groups == 79 && c.n_splits == 80 && c.rounds == 1, "20 000 rows, %d query tiles: %d %d %d", qt, c.groups, c.n_splits, c.rounds);
            printf("anchor n20000_q%d %d %d %d\n", qt, c.groups, c.n_splits, c.rounds);
        }
        const RowTailPlan e = knn_defer_rowtail(knn_defer_list_cap(20000), 8, 256);
        CHECK(e.groups == 79 && e.n_splits == 64 && e.rounds == 2, "20 000 rows, 8 query tiles: %d %d %d", e.groups, e.n_splits, e.rounds);
        printf("anchor n20000_q8 %d %d %d\n", e.groups, e.n_splits, e.rounds);
        // a list of 2051 entries (the benchmark's, a query tile over both launches) is 128 whole groups and one of 3: on 128
        // workgroups the first round and one group of the second
        CHECK(knn_rowtail_span(127, 0, 128, 2051).n == 16 && knn_rowtail_span(0, 1, 128, 2051).n == 3 && knn_rowtail_span(1, 1, 128, 2051).n == 0, "2051 entries: 129 groups");
    }
    // ---- which tail takes a list: one of the two, whatever the count; the lists the benchmark makes go to the row tail
    for (int c : {0, 1, 16, 512, 1792, 2051, 4095, 4096}) CHECK(knn_rowtail_takes(c), "count %d", c);
    for (int c : {4097, 8192, 54320, 62512, 2147483647}) CHECK(!knn_rowtail_takes(c), "count %d", c);
    static_assert(KNN_ROWTAIL_MAX_ENTRIES == 4096, "the measured setting");
    printf("anchor max_entries %d 0 0\n", KNN_ROWTAIL_MAX_ENTRIES);
    static_assert(KNN_ROWTAIL_GROUP == 16 && KNN_ROWTAIL_THREADS == 256, "one MFMA operand of rows, 4 waves x 64 queries");
    if (failures) { printf("knn_row_tail_plan_check: %d FAILED\n", failures); return 1; }
    printf("knn_row_tail_plan_check: ok\n");
    return 0;
}
