// knn_width_plan_check.cpp -- what the host-only planner (csrc/knn_plan.h) makes of the cases of tests/knn_width_ref.py, without a GPU.
// Reads lines "dim rows f16 metric nq k" (metric: 0 L2, 1 IP, 2 cosine) from standard input and prints, per line,
//   "plan <dim> <rows> <f16> <metric> <nq> <k> <scan kind> <sq_ksplit> <exact group> <exact LDS bytes> <fits>"
// as a fresh handle with default options would plan it (the same steps as tests/knn_plan_check.cpp's plan()); then checks the
// width x k limit of include/radad_hip.h (knn_exact_fits) at its corner values.
// Exit status 0 = every check passed; a failed check prints its line and the run ends with status 1.
#include "knn_plan.h"

#include <stdio.h>

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static const char* KIND[] = {"f32_tile", "hi_tile", "f32_smallq", "hi_smallq", "f16_tile", "f32_dense"};

static void limit_facts() {
    // dim * 4 + 96 k + 16 <= 160 KB with one query per workgroup
    CHECK(knn_exact_fits(16380, 1024) && !knn_exact_fits(16384, 1024));
    CHECK(knn_exact_fits(40932, 1) && !knn_exact_fits(40936, 1));
    CHECK(knn_exact_group(16380, 1024) == 1 && knn_exact_lds_bytes(16380, 1024) == (size_t)16380 * 4 + 96 * 1024 + 16);
    CHECK(knn_exact_lds_bytes(16380, 1024) == KX_LDS_MAX);
    // a launch asks for what the kernel indexes; the formula's 16 bytes are the kernel's static arrival flag (HIP refuses a kernel
    // whose static + dynamic LDS exceed the CU's 160 KB)
    CHECK(knn_exact_dyn_lds_bytes(16380, 1024) + 16 == KX_LDS_MAX && knn_exact_dyn_lds_bytes(64, 10) == (size_t)8 * (64 * 4 + 96 * 10));
    // whatever fits at k fits at every smaller k (the exclusion-aware searches check k_fetch >= k), and the group never makes a
    // configuration that fits with one query per workgroup too large
    for (int dim = 4; dim <= 41000; dim += (dim < 256 ? 4 : 508))
        for (int k = 1; k <= 1024; k += (k < 32 ? 1 : 31)) {
            const size_t one = (size_t)dim * 4 + (size_t)KX_WAVES * k * 12 + 16;
            CHECK(knn_exact_fits(dim, k) == (one <= KX_LDS_MAX));
            if (k > 1 && knn_exact_fits(dim, k)) CHECK(knn_exact_fits(dim, k - 1));
            if (knn_exact_fits(dim, k)) CHECK(knn_exact_lds_bytes(dim, k) <= KX_LDS_MAX && knn_exact_group(dim, k) >= 1);
        }
}

int main() {
    long long dim, rows, f16, metric, nq, k;
    int n_cases = 0;
    while (scanf("%lld %lld %lld %lld %lld %lld", &dim, &rows, &f16, &metric, &nq, &k) == 6) {
        StoreFacts s;
        s.ntotal = rows; s.dim = (int)dim; s.metric = (int)metric; s.f16 = (int)f16;
        KnnTuning tune;
        const TileEligibility t = knn_tile_eligibility(s, nq, (int)k, KNN_MARGIN);
        const bool use_hi = t.eligible && tune.take_tile_turn();
        const bool smallq_hi = knn_smallq_hi_eligible(s, nq, (int)k, KNN_MARGIN, use_hi, false) && tune.take_smallq_turn();
        const ScanPlan p = knn_finish_plan(s, nq, (int)k, KNN_MARGIN, t, use_hi, smallq_hi);
        CHECK(p.kind >= 0 && p.kind < 6);
        printf("plan %lld %lld %lld %lld %lld %lld %s %d %d %zu %d\n", dim, rows, f16, metric, nq, k, KIND[p.kind], (int)p.sq_ksplit, p.xgroup,
               knn_exact_lds_bytes((int)dim, (int)k), (int)knn_exact_fits((int)dim, (int)k));
        CHECK(p.xgroup == knn_exact_group((int)dim, (int)k));
        ++n_cases;
    }
    limit_facts();
    printf("cases %d\n", n_cases);
    printf("%s\n", failures ? "knn_width_plan_check: FAILED" : "knn_width_plan_check: ok");
    return failures ? 1 : 0;
}
