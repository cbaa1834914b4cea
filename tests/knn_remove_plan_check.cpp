// Stand-alone check of the host side of radad_knn_remove_ids (csrc/knn_plan.h: knn_remove_plan, knn_remove_layout, KnnTuning::rows_removed).
// No GPU, no HIP header.  tests/test_knn_remove_plan.py builds it (with host sanitizers where available), runs it once and compares
// the lines it prints with tests/knn_remove_ref.py.
//
// For every (store size, stage size, removal pattern) it builds the drop flags and their exclusive prefix sum as the device would,
// plans the removal, checks the plan's shape, and EXECUTES the plan's launches on an integer array exactly as k_remove_move indexes:
// once with the steps of every launch in ascending order and once in descending order.  Both must give a[keep], no step may read a
// store position that another step of the same launch writes, and a direct launch may only write below its own first row.
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <string>
#include <vector>

#include "knn_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        if (!(cond)) {                                                     \
            ++failures;                                                    \
            printf("FAILED %s:%d: ", __FILE__, __LINE__);                  \
            printf(__VA_ARGS__);                                           \
            printf("\n");                                                  \
        }                                                                  \
    } while (0)

static std::vector<unsigned char> pattern_flags(const std::string& pat, int64_t n, int64_t S) {
    std::vector<unsigned char> f((size_t)n, 0);
    auto set = [&](int64_t i) { if (i >= 0 && i < n) f[(size_t)i] = 1; };
    if (pat == "none") {
    } else if (pat == "first") set(0);
    else if (pat == "last") set(n - 1);
    else if (pat == "mid_slab") set(S + S / 2);                       // first removed row in the middle of the second slab
    else if (pat == "boundary") set(S);                               // ... exactly on a slab boundary
    else if (pat == "every_other") { for (int64_t i = 0; i < n; i += 2) set(i); }
    else if (pat == "run") { for (int64_t i = S / 2; i < S / 2 + 2 * S + 3; ++i) set(i); }      // one run across two slab boundaries
    else if (pat == "all_but_one") { for (int64_t i = 0; i < n; ++i) if (i != n / 2) set(i); }
    else if (pat == "all") { for (int64_t i = 0; i < n; ++i) set(i); }
    else if (pat == "random30") {
        uint64_t s = 0x9e3779b97f4a7c15ull ^ (uint64_t)(n * 1315423911ll + S);
        for (int64_t i = 0; i < n; ++i) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            if ((s >> 33) % 100 < 30) set(i);
        }
    }
    return f;
}

// one launch on the integer store `a` / staging `st`; reverse: the steps in descending order
static void run_launch(const RemoveLaunch& l, const RemovePlan& p, const std::vector<unsigned char>& flags, const std::vector<int>& excl,
                       std::vector<int64_t>& a, std::vector<int64_t>& st, bool reverse, const char* tag) {
    const int64_t n = (int64_t)a.size(), S = p.stage_rows;
    std::set<int64_t> store_reads, store_writes;
    for (int64_t step = 0; step < l.rows; ++step) {
        const int64_t w = reverse ? l.rows - 1 - step : step;
        if (l.kind == KNN_REMOVE_SCATTER) {
            const int64_t d = l.dst0 + w;
            CHECK(w < S && d >= 0 && d < n, "%s: scatter step out of bounds (slot %lld -> row %lld)", tag, (long long)w, (long long)d);
            if (!(w < S && d >= 0 && d < n)) continue;
            a[(size_t)d] = st[(size_t)w];
            store_writes.insert(d);
            continue;
        }
        const int64_t i = l.row0 + w;
        CHECK(i < n, "%s: launch reaches past the store", tag);
        if (i >= n || flags[(size_t)i]) continue;
        const int64_t d = i - excl[(size_t)i];
        store_reads.insert(i);
        if (l.kind == KNN_REMOVE_GATHER) {
            const int64_t s = d - l.dst0;
            CHECK(s >= 0 && s < S, "%s: staging slot %lld outside [0, %lld)", tag, (long long)s, (long long)S);
            if (s >= 0 && s < S) st[(size_t)s] = a[(size_t)i];
        } else {
            CHECK(d >= 0 && d < l.row0, "%s: direct launch writes row %lld, not below its first row %lld", tag, (long long)d, (long long)l.row0);
            if (d >= 0 && d < l.row0) { a[(size_t)d] = a[(size_t)i]; store_writes.insert(d); }
        }
    }
    for (int64_t r : store_reads) CHECK(!store_writes.count(r), "%s: row %lld is read and written by the same launch", tag, (long long)r);
}

static void one_case(int64_t n, int64_t opt_S, const std::string& pat) {
    const size_t row_bytes = 2048;
    const int64_t S = knn_remove_stage_rows(row_bytes, opt_S);
    const std::vector<unsigned char> flags = pattern_flags(pat, n, S);
    std::vector<int> excl((size_t)n);
    int64_t r0 = n, removed = 0;
    for (int64_t i = 0; i < n; ++i) {
        excl[(size_t)i] = (int)removed;
        if (flags[(size_t)i]) { if (r0 == n) r0 = i; ++removed; }
    }
    char tag[128];
    snprintf(tag, sizeof(tag), "n%lld S%lld %s", (long long)n, (long long)S, pat.c_str());
    const int64_t n_slabs = knn_remove_n_slabs(n, r0, S);
    std::vector<int> rb((size_t)n_slabs + 1);
    for (int64_t j = 0; j <= n_slabs; ++j) {
        const int64_t row = knn_remove_slab0(r0, S) + j * S;
        rb[(size_t)j] = (j == n_slabs || row >= n) ? (int)removed : excl[(size_t)row];
    }
    const RemovePlan p = knn_remove_plan(n, row_bytes, r0, opt_S, true, rb.data());
    CHECK(p.stage_rows == S && S >= KNN_REMOVE_MIN_STAGE_ROWS, "%s: stage rows", tag);
    // the slabs tile [slab of r0, n) exactly
    if (removed == 0) {
        CHECK(p.slabs.empty() && p.launches.empty() && p.rows_moved == 0, "%s: nothing removed, yet a plan", tag);
    } else {
        CHECK((int64_t)p.slabs.size() == n_slabs && n_slabs >= 1, "%s: slab count", tag);
        int64_t at = r0 / S * S;
        CHECK(p.slab0 == at, "%s: first slab starts at %lld, not %lld", tag, (long long)p.slab0, (long long)at);
        for (const RemoveSlab& s : p.slabs) {
            CHECK(s.row0 == at && s.rows >= 1 && s.rows <= S, "%s: slab at %lld x %lld, expected one at %lld", tag, (long long)s.row0, (long long)s.rows, (long long)at);
            CHECK(s.removed_before == excl[(size_t)s.row0], "%s: removed_before", tag);
            CHECK(s.direct == (s.removed_before >= S), "%s: slab at %lld with %lld removed in front is %s", tag, (long long)s.row0,
                  (long long)s.removed_before, s.direct ? "direct" : "staged");
            int64_t kept = 0;
            for (int64_t i = s.row0; i < s.row0 + s.rows; ++i) kept += !flags[(size_t)i];
            CHECK(s.kept == kept, "%s: kept rows of the slab at %lld", tag, (long long)s.row0);
            at += s.rows;
        }
        CHECK(at == n, "%s: the slabs end at %lld, not at %lld", tag, (long long)at, (long long)n);
    }
    // execute: ascending and descending steps
    for (int reverse = 0; reverse < 2; ++reverse) {
        std::vector<int64_t> a((size_t)n), st((size_t)S, -1);
        for (int64_t i = 0; i < n; ++i) a[(size_t)i] = 1000 + i;
        for (const RemoveLaunch& l : p.launches) run_launch(l, p, flags, excl, a, st, reverse != 0, tag);
        int64_t pos = 0;
        bool same = true;
        for (int64_t i = 0; i < n; ++i) if (!flags[(size_t)i]) { same = same && a[(size_t)pos] == 1000 + i; ++pos; }
        CHECK(same && pos == n - removed, "%s: the store is not a[keep] (%s steps)", tag, reverse ? "descending" : "ascending");
    }
    int direct_slabs = 0, gathers = 0, scatters = 0, directs = 0;
    uint64_t sum = 0;
    for (const RemoveSlab& s : p.slabs) direct_slabs += s.direct;
    for (const RemoveLaunch& l : p.launches) {
        gathers += l.kind == KNN_REMOVE_GATHER; scatters += l.kind == KNN_REMOVE_SCATTER; directs += l.kind == KNN_REMOVE_DIRECT;
        sum = (sum * 1000003ull + (uint64_t)(l.kind + 1) * (uint64_t)(l.row0 * 31 + l.rows * 17 + l.dst0 * 13 + 7)) % 2147483647ull;
    }
    printf("case n%lld_s%lld_%s %lld %lld %lld %zu %d %d %d %d %lld %zu %llu\n", (long long)n, (long long)opt_S, pat.c_str(), (long long)S, (long long)r0,
           (long long)removed, p.slabs.size(), direct_slabs, gathers, scatters, directs, (long long)p.rows_moved, p.bytes_moved, (unsigned long long)sum);
}

static void layouts() {
    const size_t widths[] = {8, 16, 200, 400, 1024, 2048, 65536};
    const int64_t sizes[] = {1, 2047, 2048, 2049, 5000, 1000003};
    for (size_t rb : widths)
        for (int64_t n : sizes)
            for (int64_t opt : {(int64_t)0, (int64_t)1, (int64_t)64, (int64_t)1000})
                for (int l2 = 0; l2 < 2; ++l2) {
                    const int64_t S = knn_remove_stage_rows(rb, opt);
                    const RemoveLayout L = knn_remove_layout(n, rb, S, l2 != 0);
                    const size_t off[] = {L.flags, L.blk, L.excl, L.slab_rb, L.head, L.stage, L.stage_norm, L.bytes};
                    const size_t need[] = {(size_t)L.n_blocks * KNN_REMOVE_SCAN_ROWS, (size_t)(L.n_blocks + 1) * 4, (size_t)n * 4,
                                           (size_t)(L.max_slabs + 1) * 4, 16, (size_t)S * rb, l2 ? (size_t)S * 4 : 0};
                    CHECK(L.n_blocks * KNN_REMOVE_SCAN_ROWS >= n && L.max_slabs * S >= n, "layout: blocks / slabs do not cover the store");
                    for (int i = 0; i < 7; ++i) {
                        CHECK(off[i] % 256 == 0, "layout rb %zu n %lld: array %d is not 256-byte aligned", rb, (long long)n, i);
                        CHECK(off[i] + need[i] <= off[i + 1], "layout rb %zu n %lld: array %d overlaps the next", rb, (long long)n, i);
                    }
                    // the staging buffer does not grow with the store
                    CHECK(L.bytes - L.stage <= al256((size_t)S * rb) + al256((size_t)S * 4), "layout: staging proportional to the store");
                    if (opt == 0) CHECK((size_t)S * rb <= std::max(KNN_REMOVE_STAGE_BYTES, (size_t)KNN_REMOVE_MIN_STAGE_ROWS * rb), "layout: default staging above its bytes");
                }
    printf("layout default_rows_2048 %lld min %lld\n", (long long)knn_remove_stage_rows(2048, 0), (long long)knn_remove_stage_rows(2048, 1));
}

static void tuning() {
    KnnTuning t;
    t.plane_decided(1.f, 0.01f, 1000);
    printf("tuning before_removal appended_1000 %d appended_1001 %d due_1999 %d due_2000 %d\n", (int)t.appended_since_plane(true, 1000),
           (int)t.appended_since_plane(true, 1001), (int)t.plane_rebuild_due(true, 1999), (int)t.plane_rebuild_due(true, 2000));
    KnnTuning u = t;
    u.rows_removed(600);
    printf("tuning removed_to_600 decided %lld appended_600 %d appended_700 %d due_1199 %d due_1200 %d\n", (long long)u.plane_decided_rows,
           (int)u.appended_since_plane(true, 600), (int)u.appended_since_plane(true, 700), (int)u.plane_rebuild_due(true, 1199), (int)u.plane_rebuild_due(true, 1200));
    // a removal that leaves more rows than the plane was decided at changes nothing
    KnnTuning v = t;
    v.rows_removed(1500);
    printf("tuning removed_to_1500 decided %lld\n", (long long)v.plane_decided_rows);
    // without a removal nothing changes; a replan request still fires on any append
    KnnTuning w = u;
    w.replan = true;
    printf("tuning replan due_601 %d due_600 %d\n", (int)w.plane_rebuild_due(true, 601), (int)w.plane_rebuild_due(true, 600));
    KnnTuning z = t;
    z.rows_removed(0);
    printf("tuning removed_all decided %lld due_0 %d due_1 %d\n", (long long)z.plane_decided_rows, (int)z.plane_rebuild_due(true, 0), (int)z.plane_rebuild_due(true, 1));
}

int main() {
    const int64_t sizes[] = {1, 2, 63, 64, 65, 127, 128, 129, 200, 257, 1000, 2049, 3001};
    const int64_t stages[] = {1, 64, 65, 100, 256, 1000};      // (1: below the minimum, raised to it)
    const char* pats[] = {"none", "first", "last", "mid_slab", "boundary", "every_other", "run", "all_but_one", "all", "random30"};
    for (int64_t n : sizes)
        for (int64_t S : stages)
            for (const char* pat : pats) one_case(n, S, pat);
    one_case(5000, 0, "random30");      // the default stage size: one slab
    layouts();
    tuning();
    printf(failures ? "knn_remove_plan_check: %d FAILED\n" : "knn_remove_plan_check: ok\n", failures);
    return failures ? 1 : 0;
}
