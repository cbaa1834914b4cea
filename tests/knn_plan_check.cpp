// knn_plan_check.cpp -- the host-only planner and tuning state of a flat search (csrc/knn_plan.h), without a GPU.
//   1. prints one line per case of a grid of stores and searches: what a fresh handle would launch and allocate (tests/test_knn_plan.py
//      compares the lines with tests/data/knn_plan_table.json);
//   2. checks facts the code and DESIGN.md state about phases, layouts and list counts;
//   3. drives KnnTuning through the retuning policy with exact expectations.
// Exit status 0 = every check passed; a failed check prints its line and the run ends with status 1.
#include "knn_plan.h"

#include <stdio.h>
#include <string>

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static const char* KIND[] = {"f32_tile", "hi_tile", "f32_smallq", "hi_smallq", "f16_tile", "f32_dense"};

// what knn_plan_scan + knn_scan_hi_tile make of a search on a FRESH handle whose plane can be built
struct Planned {
    ScanPlan p;
    SearchLayout L;
    std::vector<int64_t> phases;     // the tile scan's row boundaries (empty for the other scans)
    int splits = 0, launches = 1, n_phases = 0;      // as radad_knn_last_launch / _last_scan_launches / _last_scan_phases report them
};
static Planned plan(const StoreFacts& s, int64_t nq, int k, int margin) {
    Planned out;
    KnnTuning tune;
    const TileEligibility t = knn_tile_eligibility(s, nq, k, margin);
    const bool use_hi = t.eligible && tune.take_tile_turn();
    const bool smallq_hi = knn_smallq_hi_eligible(s, nq, k, margin, use_hi, false) && tune.take_smallq_turn();
    out.p = knn_finish_plan(s, nq, k, margin, t, use_hi, smallq_hi);
    out.L = knn_search_layout(s, out.p, RADAD_Q_F32);
    out.splits = out.p.n_splits;
    if (out.p.kind == RADAD_SCAN_HI_TILE) {
        out.phases = knn_hi_phases(s.ntotal, nq, (int64_t)8 * out.p.s_splits * KW_M, knn_hi_one_go(out.p, s.ntotal));
        out.launches = out.n_phases = (int)out.phases.size() - 1;
        int gq; int64_t gc;
        knn_geometry_wide(out.phases.back() - out.phases[out.phases.size() - 2], nq, &gq, &out.splits, &gc);      // the last launch's
    }
    return out;
}

// every buffer of the workspace, in the order of its offsets, with the bytes its user reads or writes: offsets 256-aligned, no
// buffer reaching into the next one, `bytes` the end of the last
static void check_buffers(const size_t* off, const size_t* size, int n, size_t bytes) {
    for (int i = 0; i < n; ++i) {
        const size_t end = i + 1 < n ? off[i + 1] : bytes;
        CHECK(off[i] % 256 == 0 && end >= off[i] && end - off[i] >= size[i]);
    }
    CHECK(off[0] == 0 && bytes % 256 == 0);
}

static void check_layout(const StoreFacts& s, const ScanPlan& p, const SearchLayout& L, int q_dtype) {
    const size_t nq = (size_t)p.nq, vec = nq * 4, qrow = nq * s.dim * 4;
    const size_t part = (L.cand_elems + (p.kind == RADAD_SCAN_HI_TILE ? nq * KW_SAMPLE_SPLITS * KW_SAMPLE_LIST : 0)) * 4;
    const size_t xlists = (size_t)knn_exact_slots(p.nq, p.k, p.xgroup) * KX_SLICES * p.k;
    const size_t off[] = {L.qf, L.qn, L.qh, L.qscale, L.qconst, L.eps, L.thr, L.ak, L.cnt, L.fcount, L.fsel, L.ps, L.pi, L.xk, L.xi};
    const size_t size[] = {q_dtype == RADAD_Q_BF16 ? qrow : 0, s.metric == RADAD_METRIC_COSINE ? qrow : 0, p.f16_queries() ? nq * s.dim * 2 : 0,
                           vec, vec, vec, vec, vec, vec, 7 * sizeof(int) /* flag_count + 6 statistics */, vec, part, part,
                           xlists * sizeof(double), xlists * sizeof(int)};
    check_buffers(off, size, 15, L.bytes);
    CHECK(L.cand_elems == nq * (size_t)p.n_parts * p.plen);
}

static void print_case(const std::string& name, const StoreFacts& s, int64_t nq, int k, int margin) {
    const Planned c = plan(s, nq, k, margin);
    printf("case %s %s %d %d %d %d %d %d %d %d %d %d %d %d %d %d %zu\n", name.c_str(), KIND[c.p.kind], c.p.reported_qtiles, c.splits,
           c.p.block_threads, c.launches, c.n_phases, c.p.ksel, c.p.ksel_sq, (int)c.p.sq_ksplit, c.p.s_splits, c.p.emit_cap, c.p.cap, c.p.plen,
           c.p.n_parts, c.p.xgroup, c.L.bytes);
    CHECK(c.p.n_parts <= 1024);
    check_layout(s, c.p, c.L, RADAD_Q_F32);
    check_layout(s, c.p, knn_search_layout(s, c.p, RADAD_Q_BF16), RADAD_Q_BF16);
}

static void grid() {
    const int dims[] = {64, 96, 100, 1024, 5376};
    const int64_t rows[] = {0, 7, 1000, 6144, 6145, 16383, 16384, 16640, 40000, 100000, 1000000, 1300000, 10000000};
    const int64_t nqs[] = {1, 16, 17, 64, 300, 2100};
    const int ks[] = {1, 10, 16, 17, 26, 27, 128, 129, 1024};
    const char* variants[] = {"base", "hi_off", "smallq_hi0", "wide_min_q1", "dense0", "cap_boost4"};
    for (int v = 0; v < 6; ++v)
        for (int dim : dims)
            for (int64_t n : rows)
                for (int f16 = 0; f16 < (v ? 1 : 2); ++f16)               // the variants: fp32 store, L2, margin 6
                    for (int cosine = 0; cosine < (v ? 1 : 2); ++cosine)
                        for (int margin : {KNN_MARGIN, 0}) {
                            if (v && margin != KNN_MARGIN) continue;
                            StoreFacts s;
                            s.ntotal = n; s.dim = dim; s.metric = cosine ? RADAD_METRIC_COSINE : RADAD_METRIC_L2; s.f16 = f16;
                            if (v == 1) s.hi_off = 1;
                            if (v == 2) s.opt_smallq_hi = 0;
                            if (v == 3) s.opt_wide_min_q = 1;
                            if (v == 4) s.opt_dense = 0;
                            if (v == 5) s.cap_boost = 4;
                            for (int64_t nq : nqs)
                                for (int k : ks) {
                                    char name[128];
                                    snprintf(name, sizeof(name), "d%d_n%lld_q%lld_k%d_%s_%s_m%d_%s", dim, (long long)n, (long long)nq, k,
                                             f16 ? "f16" : "f32", cosine ? "cos" : "l2", margin, variants[v]);
                                    print_case(name, s, nq, k, margin);
                                }
                        }
}

// ---- facts -----------------------------------------------------------------------------------------------------------------------
static void phase_facts() {
    // dim 512, 1024 queries, k 10: 1 launch when one_go, 2 up to 1.2 M rows, 3 up to 9.5 M
    StoreFacts s;
    s.dim = 512; s.metric = RADAD_METRIC_COSINE;
    for (int64_t n : {16384ll, 20000ll, 50000ll, 100000ll, 131072ll, 200000ll, 400000ll, 1000000ll, 1200000ll, 2000000ll, 5000000ll, 9500000ll}) {
        s.ntotal = n;
        const Planned c = plan(s, 1024, 10, KNN_MARGIN);
        CHECK(c.p.kind == RADAD_SCAN_HI_TILE);
        if (knn_hi_one_go(c.p, n)) CHECK(c.launches == 1);
        else CHECK(c.launches >= 2);
        CHECK(c.launches <= (n <= 1200000 ? 2 : 3));
        if (n == 1000000 || n == 1200000) CHECK(c.launches == 2);
        if (n == 9500000) CHECK(c.launches == 3);
        printf("phases dim 512 nq 1024 k 10 n %lld: %d launch(es)%s\n", (long long)n, c.launches, knn_hi_one_go(c.p, n) ? " (one_go)" : "");
    }
    // boundaries: multiples of KW_M, strictly increasing, ending at n; no last phase was cut shorter than a quarter of its predecessor's span
    for (int dim : {64, 512, 1024})
        for (int64_t nq : {17ll, 300ll, 1024ll, 2100ll, 10240ll})
            for (int k : {1, 10, 128})
                for (int64_t n : {16384ll, 16640ll, 25423ll, 40000ll, 100000ll, 131072ll + 32767, 131072ll + 32768, 163840ll, 1000000ll, 1300000ll,
                                  1441791ll, 1441792ll, 3000000ll, 10000000ll, 12345678ll}) {
                    s.dim = dim; s.ntotal = n;
                    const Planned c = plan(s, nq, k, KNN_MARGIN);
                    if (c.p.kind != RADAD_SCAN_HI_TILE) continue;
                    const std::vector<int64_t>& r = c.phases;
                    CHECK(r.size() >= 2 && r.front() == 0 && r.back() == n);
                    for (size_t i = 1; i < r.size(); ++i) CHECK(r[i] > r[i - 1] && (r[i] % KW_M == 0 || i + 1 == r.size()));
                    if (r.size() >= 3) {
                        int64_t span = (int64_t)8 * c.p.s_splits * KW_M;            // the span of the LAST phase's predecessor
                        for (size_t i = 3; i < r.size(); ++i) span *= 8;
                        // (the quarter is taken BEFORE the last two launches are balanced: up to a quarter of the predecessor's tiles
                        // then move into it from the last phase, knn_hi_phases)
                        const int64_t last = n - r[r.size() - 2], moved = (r[r.size() - 2] - r[r.size() - 3]) - span;
                        CHECK(moved >= 0 && moved <= span / 4 && moved % KW_M == 0 && last + moved >= span / 4);
                    }
                }
}

static void excl_layout_facts() {
    StoreFacts s;
    for (int64_t n : {7ll, 1000ll, 100000ll})
        for (int64_t nq : {1ll, 300ll})
            for (int k : {1, 10, 129})
                for (int64_t n_excl : {0ll, 5ll})
                    for (int begun = 0; begun < 2; ++begun) {
                        s.ntotal = n; s.dim = 512;
                        const ExclLayout L = knn_excl_layout(s, nq, k, k + 10, n_excl, begun != 0);
                        const size_t lists = (size_t)nq * L.kf, xl = n_excl > 0 ? (size_t)L.xslots * KX_SLICES * k : 0, out = (size_t)nq * k;
                        const size_t off[] = {L.fd, L.fi, L.fk, L.count, L.sel, L.admit, L.xk, L.xi, L.bd, L.bi, L.bk, L.own};
                        const size_t size[] = {lists * 4, lists * 8, lists * 8, sizeof(int), (size_t)nq * 4, n_excl > 0 ? (size_t)L.n_words * 8 : 0,
                                               xl * 8, xl * 4, out * 4, out * 8, out * 8, (size_t)nq * 4};
                        check_buffers(off, size, begun ? 12 : 8, L.bytes);
                        CHECK(L.kf == (int)std::min<int64_t>(k + 10, n) && L.whole == (k + 10 > n ? 1 : 0) && L.n_words == (n + 63) / 64);
                        CHECK(L.xgroup == knn_exact_group(s.dim, k) && L.xslots == knn_exact_slots(nq, k, L.xgroup));
                    }
}

// ---- the retuning policy, step by step ---------------------------------------------------------------------------------------------
static void tuning_policy() {
    {   // fresh state
        KnnTuning t;
        CHECK(t.verify_next && t.cap_boost == 1 && t.hi_skip == 0 && !t.replan && t.search_seq == 0 && t.tuned_at == 0);
        CHECK(t.take_tile_turn() && t.take_smallq_turn() && t.hi_skip == 0);
        CHECK(t.slot() == 0 && t.stamp() == 1);
    }
    {   // the ladder: re-decide the plane (rows appended), widen, then 8, 16, ... 512, 512, 512 searches on the fp32 kernels
        KnnTuning t;
        t.plane_decided(1.f, 1e-3f, 1000);
        t.search_seq = 5; t.verify_next = false;
        CHECK(t.appended_since_plane(true, 1500) && !t.appended_since_plane(true, 1000) && !t.appended_since_plane(false, 1500));
        t.mass_rejection(true);
        CHECK(t.replan && t.cap_boost == 1 && t.hi_skip == 0 && t.hi_fail_streak == 0 && t.tuned_at == 5 && t.verify_next);
        t.search_seq = 6; t.verify_next = false;
        t.mass_rejection(false);
        CHECK(t.cap_boost == 4 && t.hi_skip == 0 && t.hi_fail_streak == 0 && t.tuned_at == 6 && t.verify_next);
        const int want[] = {8, 16, 32, 64, 128, 256, 512, 512, 512};
        for (int i = 0; i < 9; ++i) {
            t.search_seq = 7 + i; t.verify_next = false; t.hi_skip = 0;
            t.mass_rejection(false);
            CHECK(t.hi_skip == want[i] && t.hi_fail_streak == i + 1 && t.cap_boost == 4 && t.tuned_at == (uint64_t)(7 + i) && t.verify_next);
        }
    }
    {   // the countdown: eight tile-eligible turns refused, verify_next on the turn that reaches 0; the small-batch one leaves it alone
        KnnTuning t;
        t.cap_boost = 4; t.mass_rejection(false);
        CHECK(t.hi_skip == 8);
        t.verify_next = false;
        for (int i = 0; i < 8; ++i) {
            CHECK(!t.take_tile_turn());
            CHECK(t.hi_skip == 7 - i && t.verify_next == (i == 7));
        }
        CHECK(t.take_tile_turn() && t.hi_skip == 0);
        KnnTuning u;
        u.cap_boost = 4; u.mass_rejection(false);
        u.verify_next = false;
        for (int i = 0; i < 8; ++i) CHECK(!u.take_smallq_turn() && u.hi_skip == 7 - i && !u.verify_next);
        CHECK(u.take_smallq_turn() && !u.verify_next);
    }
    {   // reports that are ignored
        KnnTuning t;
        t.search_seq = 10; t.verify_next = false;
        CHECK(!t.report_is_new(0, 0) && !t.consume_report(0, 0, 100, 100, false) && t.reports_consumed == 0);                  // stamp 0
        CHECK(t.report_is_new(0, 9) && !t.consume_report(0, 9, 10, 63, false) && t.reports_consumed == 1 && t.cap_boost == 1);   // batch < 64
        CHECK(!t.report_is_new(0, 9) && !t.consume_report(0, 9, 100, 100, false) && t.reports_consumed == 1);                  // the same stamp twice
        CHECK(!t.consume_report(1, 10, 16, 64, false) && t.reports_consumed == 2 && t.cap_boost == 1);                         // rejected * 4 <= batch
        CHECK(t.consume_report(0, 11, 17, 64, false) && t.reports_consumed == 3 && t.cap_boost == 4 && t.tuned_at == 10 && t.verify_next);
        CHECK(t.stamp_seen[0] == 11 && t.stamp_seen[1] == 10);
        // the report's search (9, stamp 10) is older than tuned_at = 10: counted, not acted on; search 10 (stamp 11) is not
        t.search_seq = 12;
        CHECK(!t.consume_report(1, 10, 64, 64, false) && t.reports_consumed == 3 && t.hi_skip == 0);      // stamp 10 was seen in slot 1: ignored
        CHECK(!t.consume_report(1, 8 + 1, 64, 64, false) && t.reports_consumed == 4 && t.hi_skip == 0);
        CHECK(t.consume_report(0, 10 + 1 + 2, 64, 64, false) && t.hi_skip == 8 && t.reports_consumed == 5);      // search 12
        // a report that arrives while hi_skip > 0 is counted but does not retune
        t.search_seq = 14;
        const uint64_t tuned = t.tuned_at;
        CHECK(!t.consume_report(1, 14, 64, 64, false) && t.reports_consumed == 6 && t.hi_skip == 8 && t.hi_fail_streak == 1 && t.tuned_at == tuned);
        // with rows appended since the plane was decided the step is the plane's
        KnnTuning a;
        a.search_seq = 3;
        CHECK(a.consume_report(1, 2, 64, 64, true) && a.replan && a.cap_boost == 1);
    }
    {   // stamp wrap: 30 bits
        KnnTuning t;
        t.search_seq = ((uint64_t)1 << 30) + 5;
        const int stamp = (int)((((uint64_t)1 << 30) + 3) & 0x3fffffff) + 1;
        CHECK(stamp == 4 && t.report_search(stamp) == ((uint64_t)1 << 30) + 3);
        t.tuned_at = ((uint64_t)1 << 30) + 3;
        CHECK(t.consume_report(1, stamp, 64, 64, false) && t.cap_boost == 4);
        KnnTuning u;
        u.search_seq = ((uint64_t)1 << 30) + 5; u.tuned_at = ((uint64_t)1 << 30) + 4;
        CHECK(!u.consume_report(1, stamp, 64, 64, false) && u.cap_boost == 1 && u.reports_consumed == 1);
        u.search_seq = ((uint64_t)1 << 30) - 1;
        CHECK(u.stamp() == (1 << 30) && u.slot() == 1 && u.last_slot() == 0);
        u.search_issued();
        CHECK(u.stamp() == 1 && u.search_seq == ((uint64_t)1 << 30));
    }
    {   // the look before the exact pass
        KnnTuning t;
        CHECK(t.looks_before_exact(true, 64, 10000000, 640));            // 64 x 1e7 x 640 = 4.096e11
        CHECK(!t.looks_before_exact(false, 64, 10000000, 640));           // only the tile scan
        CHECK(!t.looks_before_exact(true, 63, 100000000, 640));           // nq >= 64
        CHECK(!t.looks_before_exact(true, 64, 10000000, 624));            // 3.99e11 < 4e11
        CHECK(t.looks_before_exact(true, 1000, 1000000, 400) && !t.looks_before_exact(true, 1000, 999999, 400));
        t.hi_fail_streak = 3;
        CHECK(!t.look_outcome(16, 64, true, false) && !t.verify_next && t.hi_fail_streak == 0 && t.verified_retries == 0);      // a pass
        CHECK(!t.looks_before_exact(true, 64, 10000000, 640));            // verify_next cleared
        KnnTuning f;
        f.search_seq = 2;
        CHECK(f.look_outcome(17, 64, true, false) && f.cap_boost == 4 && f.verified_retries == 1 && f.verify_next && f.tuned_at == 2);
        CHECK(f.look_outcome(17, 64, true, false) && f.hi_skip == 8 && f.hi_fail_streak == 1 && f.verified_retries == 2);
        KnnTuning l;                                                      // a fail on the last attempt clears nothing and tunes nothing
        l.hi_fail_streak = 2;
        CHECK(!l.look_outcome(17, 64, false, false) && l.verify_next && l.hi_fail_streak == 2 && l.cap_boost == 1 && l.verified_retries == 0);
    }
    {   // the plane
        KnnTuning t;
        t.search_seq = 4;
        t.plane_is_new();
        t.plane_decided(2.f, 0.f, 1000);
        CHECK(t.plane_decided_rows == 1000 && t.plane_stat[0] == 2.f && t.plane_stat[1] == 0.f);
        CHECK(!t.plane_rebuild_due(true, 1000));                          // nothing appended
        CHECK(!t.plane_rebuild_due(true, 1999) && t.plane_rebuild_due(true, 2000));      // doubled
        CHECK(!t.plane_rebuild_due(false, 2000));                         // another capacity: the plane is rebuilt anyway
        t.replan = true;
        CHECK(t.plane_rebuild_due(true, 1001) && !t.plane_rebuild_due(true, 1000) && !t.plane_rebuild_due(false, 1001));
        t.plane_dropped_for_rebuild();
        CHECK(t.plane_rebuilds == 1 && t.tuned_at == 4);
        t.plane_wanted();
        CHECK(!t.replan);
        t.verify_next = false;
        t.plane_is_new();
        CHECK(t.verify_next);
        CHECK(!t.plane_outgrown(16.f, 100.f) && !t.replan);               // exactly 8x is within the headroom; a zero decided statistic never asks
        CHECK(t.plane_outgrown(16.001f, 0.f) && t.replan);
        KnnTuning r;
        r.plane_decided(0.f, 1e-3f, 10);
        CHECK(!r.plane_outgrown(1e9f, 8e-3f) && !r.replan && r.plane_outgrown(0.f, 8.1e-3f) && r.replan);
    }
}

int main() {
    grid();
    phase_facts();
    excl_layout_facts();
    tuning_policy();
    printf("%s\n", failures ? "knn_plan_check: FAILED" : "knn_plan_check: ok");
    return failures ? 1 : 0;
}
