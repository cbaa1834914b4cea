// abandon_plan_check.cpp -- stand-alone check of the host side of the tile scan's early abandon (knn_plan.h: knn_abandon_checkpoint,
// knn_abandon_launch, knn_abandon_layout, knn_abandon_tiles), driven by tests/test_abandon_plan.py.  No GPU, no HIP: it includes the
// planner header alone.
//
//   * the checkpoint for every row width 64 ... 16380 the tile scan or anything else can be asked for: 0 below 128 and off multiples of
//     64, else an eighth of the K stages, at least one, always leaving a stage behind it;
//   * which launches take the ABANDON instantiation: RSC 0 and 3 with floors, one workgroup per tile, the handle's own bias, current
//     per-tile norms, the option on -- and nothing else;
//   * the per-query buffer's layout, the per-tile array's length, and that the search workspace (SearchLayout) has not changed.
#include <cstdio>
#include <cstdlib>

#include "knn_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                                                                        \
    do {                                                                                        \
        if (!(cond)) { ++failures; printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

int main() {
    // ---- the checkpoint
    int with = 0;
    for (int dim = 4; dim <= 16380; dim += 4) {
        const int c = knn_abandon_checkpoint(dim);
        const int stages = dim / 64;
        if (dim < 128 || dim % 64 != 0) { CHECK(c == 0, "dim %d: c %d", dim, c); continue; }
        ++with;
        CHECK(c >= 1 && c < stages, "dim %d: c %d of %d stages", dim, c, stages);
        CHECK(c == (stages / 8 > 1 ? stages / 8 : 1), "dim %d: c %d", dim, c);
        CHECK(knn_abandon_suffix_from(dim) == 64 * c && knn_abandon_suffix_from(dim) < dim, "dim %d", dim);
        printf("checkpoint d%d %d\n", dim, c);
    }
    CHECK(with == 16320 / 64 - 1, "widths with a checkpoint: %d", with);
    CHECK(knn_abandon_checkpoint(64) == 0 && knn_abandon_checkpoint(128) == 1 && knn_abandon_checkpoint(512) == 1 &&
          knn_abandon_checkpoint(1024) == 2 && knn_abandon_checkpoint(3584) == 7 && knn_abandon_checkpoint(5376) == 10, "the named widths");
    CHECK(knn_abandon_suffix_from(100) == 0 && knn_abandon_suffix_from(64) == 0, "no suffix where there is no checkpoint");

    // ---- which launches abandon
    int on = 0, lines = 0;
    for (int opt : {0, 1})
        for (int rsc : {0, 1, 2, 3})
            for (int sample : {0, 1})
                for (int ksplit : {1, 2})
                    for (int floors : {0, 1})
                        for (int bias : {0, 1})
                            for (int current : {0, 1})
                                for (int dim : {64, 100, 128, 512, 5376}) {
                                    AbandonFacts f;
                                    f.opt_abandon = opt; f.rsc = rsc; f.sample = sample != 0; f.ksplit = ksplit; f.floors = floors != 0;
                                    f.per_call_bias = bias != 0; f.terms_current = current != 0; f.dim = dim;
                                    const int c = knn_abandon_launch(f);
                                    const bool expect = opt && (rsc == 0 || rsc == 3) && !sample && ksplit == 1 && floors && !bias && current &&
                                                        dim >= 128 && dim % 64 == 0;
                                    CHECK((c > 0) == expect && (c == 0 || c == knn_abandon_checkpoint(dim)),
                                          "opt %d rsc %d sample %d ksplit %d floors %d bias %d current %d dim %d: %d", opt, rsc, sample, ksplit, floors, bias, current, dim, c);
                                    printf("launch o%d_r%d_s%d_k%d_f%d_b%d_c%d_d%d %d\n", opt, rsc, sample, ksplit, floors, bias, current, dim, c);
                                    ++lines;
                                    on += c > 0;
                                }
    CHECK(on == 2 * 3, "abandoning launches in the table: %d of %d", on, lines);     // RSC 0 / 3 x dims 128, 512, 5376
    {
        AbandonFacts f;                             // the defaults alone never abandon: floors, norms and a width must be stated
        CHECK(knn_abandon_launch(f) == 0, "defaults");
        f.floors = true; f.terms_current = true; f.dim = 512;
        CHECK(knn_abandon_launch(f) == 1, "the benchmark's launch: RSC 0, dim 512");
        f.dim = 5376;
        CHECK(knn_abandon_launch(f) == 10, "the reference's width");
        f.rsc = 3;
        CHECK(knn_abandon_launch(f) == 10, "one scale + bias (L2, centred cosine)");
        f.rsc = 2;
        CHECK(knn_abandon_launch(f) == 0, "per-row scales: the plain scan");
    }

    // ---- layouts
    for (int64_t nq : {1, 17, 63, 64, 65, 256, 300, 1024, 10240}) {
        const AbandonLayout L = knn_abandon_layout(nq);
        CHECK(L.rq == 0 && L.slack % 256 == 0 && L.slack >= (size_t)nq * 4 && L.bytes % 256 == 0 && L.bytes >= L.slack + (size_t)nq * 4,
              "nq %lld: rq %zu slack %zu bytes %zu", (long long)nq, L.rq, L.slack, L.bytes);
        printf("layout q%lld %zu %zu %zu\n", (long long)nq, L.rq, L.slack, L.bytes);
    }
    for (int64_t n : {1, 255, 256, 257, 20000, 1000000}) {
        const int64_t t = knn_abandon_tiles(n);
        CHECK(t * KW_M >= n && (t - 1) * KW_M < n, "rows %lld tiles %lld", (long long)n, (long long)t);
    }
    // the counters sit in the search workspace's counter block behind the certificate's seven ints, inside its 256 bytes
    CHECK(KNN_AB_COUNTER0 >= 7 && (KNN_AB_COUNTER0 + 2) * sizeof(int) <= 256, "counter slots");
    {
        StoreFacts s;
        s.ntotal = 1000000; s.dim = 512; s.metric = RADAD_METRIC_COSINE;
        const TileEligibility t = knn_tile_eligibility(s, 1024, 10, KNN_MARGIN);
        const ScanPlan p = knn_finish_plan(s, 1024, 10, KNN_MARGIN, t, t.eligible, false);
        const SearchLayout L = knn_search_layout(s, p, RADAD_Q_F32);
        CHECK(t.eligible && L.fsel - L.fcount == 256, "the counter block of the benchmark's search: %zu bytes", L.fsel - L.fcount);
    }
    if (failures) { printf("abandon_plan_check: %d FAILED\n", failures); return 1; }
    printf("abandon_plan_check: ok\n");
    return 0;
}
