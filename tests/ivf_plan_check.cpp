// ivf_plan_check.cpp -- the host-only planner of an IVF list-scan search (csrc/ivf_plan.h), without a GPU.
//   1. prints one line per case of a grid of indexes and searches: every value of the plan (tests/test_ivf_plan.py compares chosen
//      lines with tests/data/ivf_plan_table.json);
//   2. checks, for every plan, that the layouts do not overlap, that every buffer covers what the kernels index, the task bound, the
//      split, the exact scan's launches and every LDS size;
//   3. asserts values computed by hand from the expressions the plan was moved from.
// Exit status 0 = every check passed; a failed check prints its line and the run ends with status 1.
#include "ivf_plan.h"

#include <stdio.h>
#include <string>

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static const size_t LDS_MAX = 160 * 1024;      // LDS of a CU

// sub-arrays in the order of their offsets, with the bytes their users index: none reaches into the next or past the total
static void check_carved(const size_t* off, const size_t* size, int n, size_t bytes) {
    for (int i = 0; i < n; ++i) {
        const size_t end = i + 1 < n ? off[i + 1] : bytes;
        CHECK(end >= off[i] && end - off[i] >= size[i]);
    }
}

static void check_plan(const IvfFacts& s, int64_t nq, int k, int nprobe_asked, bool has_admit, const IvfPlan& p) {
    const int nprobe = p.nprobe;
    CHECK(nprobe >= 1 && nprobe <= s.nlist && (nprobe == nprobe_asked || nprobe == s.nlist));
    CHECK(p.nq == nq && p.k == k && p.ksel == k + KNN_MARGIN && p.npairs == nq * nprobe);
    const size_t npairs = (size_t)p.npairs;
    CHECK(p.qcap >= 1 && p.qcap <= SQ_NQ);
    CHECK(p.cmargin >= 0 && nprobe + p.cmargin <= std::max(32, nprobe));
    // the refusals, each for its own reason; what a refused plan accepted so far still holds
    if (p.status == IVF_PLAN_TOO_MANY_PAIRS) { CHECK(p.npairs >= (int64_t)1 << 31 || p.T >= (int64_t)1 << 31); return; }
    CHECK(p.npairs < (int64_t)1 << 31 && p.T < (int64_t)1 << 31);
    if (p.status == IVF_PLAN_DIM_TOO_LARGE) { CHECK(!p.hi_route && p.scan_lds > LDS_MAX); return; }
    CHECK(p.scan_lds <= LDS_MAX);
    if (p.status == IVF_PLAN_NPROBE_TOO_LARGE) { CHECK(p.xlds > LDS_MAX); return; }
    CHECK(p.status == IVF_PLAN_OK);

    // ---- layouts
    const size_t nlist = (size_t)s.nlist, T = (size_t)p.T, I = sizeof(int);
    {
        const size_t off[] = {p.tasks.cnt, p.tasks.cur, p.tasks.nt, p.tasks.tl, p.tasks.tp, p.tasks.tc, p.tasks.pq, p.tasks.ps};
        const size_t size[] = {nlist * I, nlist * I, I, T * I, T * I, T * I, npairs * I, npairs * I};
        check_carved(off, size, 8, p.tasks.bytes);
        CHECK(p.tasks.cnt == 0);
        CHECK(p.tasks.bytes == (3 * T + 2 * npairs + 2 * nlist + 1) * I);
        for (size_t o : off) CHECK(o % I == 0);
    }
    {
        const size_t vec = (size_t)nq * 4;
        const size_t off[] = {p.qbuf.qh, p.qbuf.qscale, p.qbuf.qconst, p.qbuf.eps, p.qbuf.cand_cnt, p.qbuf.gbound, p.qbuf.fsel, p.qbuf.fcount};
        const size_t size[] = {p.hi_route ? (size_t)nq * s.dim * 2 : 0, vec, vec, vec, vec, vec, vec, 8 * I};
        check_carved(off, size, 8, p.qbuf.bytes);
        for (size_t o : off) CHECK(o % 256 == 0);
    }
    // ---- buffers
    CHECK(p.ws_a >= npairs * sizeof(float) && p.ws_b >= npairs * sizeof(int64_t));
    CHECK(p.part_s >= npairs * p.ksel * sizeof(float) && p.part_i >= npairs * p.ksel * sizeof(int));
    if (p.hi_route) CHECK(p.ccap >= 1 && p.cand_s >= (size_t)nq * p.ccap * sizeof(float) && p.cand_i >= (size_t)nq * p.ccap * sizeof(int));
    else CHECK(p.cand_s == 0 && p.cand_i == 0);
    CHECK(p.xkey >= (size_t)p.nslots * nprobe * k * sizeof(double) && p.xid >= (size_t)p.nslots * nprobe * k * sizeof(int64_t));
    CHECK(p.xarrive >= (size_t)p.nslots * sizeof(int));
    if (has_admit) CHECK(p.admit_words >= (s.rows + 63) / 64 + 1 && p.admit == (size_t)p.admit_words * 8);      // (+ 1: the spare word)
    else CHECK(p.admit == 0 && p.admit_words == 0);
    // ---- task bound and split
    CHECK(p.T >= std::min<int64_t>(s.nlist, p.npairs) + p.npairs / p.qcap + 1);
    CHECK(p.split >= 1);
    if (p.split > 1) CHECK(p.hi_route && (int64_t)p.split * nprobe * (k + 8) <= p.ccap / 2);
    CHECK(p.scan_grid == p.T * p.split && p.scan_grid < (int64_t)1 << 32);
    CHECK(p.group_small == (p.npairs <= IVG_MAX_PAIRS && s.nlist <= IVG_MAX_LISTS));
    if (p.group_small) CHECK(p.group_lds >= nlist * I);
    // ---- the exact scan's launches: slots 0 .. nq exactly once
    CHECK(p.nslots >= 1 && p.nslots <= nq);
    CHECK((size_t)p.nslots * nprobe * k * 16 <= IVX_PART_BUDGET || p.nslots == 1);
    // (launch i starts at slot i nslots, a multiple of nslots: the last one starts below nq and reaches it)
    CHECK(p.xlaunches >= 1 && (p.xlaunches - 1) * p.nslots < nq && p.xlaunches * p.nslots >= nq);
    CHECK(p.xgrid >= 1 && p.xgrid <= IVX_MAX_GRID && p.xgrid <= p.nslots * nprobe);
    // ---- LDS
    CHECK(p.scan_lds == (p.hi_route ? ivf_hi_lds_bytes(p.qcap, s.dim) : knn_sq_lds_f32(p.qcap, s.dim)));
    CHECK(p.cap >= k && p.refine_lds >= refine_lds_bytes(p.cap) + (p.hi_route ? (size_t)p.ccap * 8 : 0));
    CHECK(p.scan_lds <= LDS_MAX && p.refine_lds <= LDS_MAX && p.xlds <= LDS_MAX && p.group_lds <= LDS_MAX);
    CHECK(p.xlds == ivf_exact_lds_bytes(s.dim, k, nprobe));
}

static void print_case(int dim, int nlist, int64_t nq, int k, int nprobe, bool plane, bool admit) {
    IvfFacts s;
    s.dim = dim; s.nlist = nlist; s.rows = (int64_t)nlist * 100 + 37; s.plane = plane;
    const IvfPlan p = ivf_plan_search(s, nq, k, nprobe, admit);
    check_plan(s, nq, k, nprobe, admit, p);
    printf("case d%d_l%d_q%lld_k%d_p%d_%s_%s %d %d %d %d %lld %lld %d %d %d %d %lld %zu %d %zu %zu %lld %lld %zu %zu",
           dim, nlist, (long long)nq, k, nprobe, plane ? "plane" : "noplane", admit ? "admit" : "all",
           (int)p.status, p.nprobe, p.cmargin, p.qcap, (long long)p.npairs, (long long)p.T, (int)p.group_small, (int)p.hi_route, p.ccap, p.split,
           (long long)p.scan_grid, p.scan_lds, p.cap, p.refine_lds, p.xlds, (long long)p.nslots, (long long)p.xgrid, (size_t)p.xlaunches, p.group_lds);
    printf(" %zu %zu %zu %zu %zu %zu %zu %zu %zu", p.tasks.cnt, p.tasks.cur, p.tasks.nt, p.tasks.tl, p.tasks.tp, p.tasks.tc, p.tasks.pq, p.tasks.ps, p.tasks.bytes);
    printf(" %zu %zu %zu %zu %zu %zu %zu %zu %zu", p.qbuf.qh, p.qbuf.qscale, p.qbuf.qconst, p.qbuf.eps, p.qbuf.cand_cnt, p.qbuf.gbound, p.qbuf.fsel, p.qbuf.fcount,
           p.qbuf.bytes);
    printf(" %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", p.ws_a, p.ws_b, p.part_s, p.part_i, p.cand_s, p.cand_i, p.xkey, p.xid, p.xarrive, p.admit);
}

static const int DIM_QCAP1 = 16384;      // 112 KB / (4 (dim + 4)) = 1
static void grid() {
    const int dims[] = {64, 96, 128, 512, 1024, 5376, DIM_QCAP1};
    const int nlists[] = {8, 64, 4096, 8193};
    const int64_t nqs[] = {1, 16, 17, 128, 129, 1024, 6000};
    const int ks[] = {1, 10, 11, 15, 26};
    for (int dim : dims)
        for (int nlist : nlists)
            for (int64_t nq : nqs)
                for (int k : ks)
                    for (int nprobe : {1, 8, 26, 27, 32, nlist})
                        for (int plane = 0; plane < 2; ++plane)
                            for (int admit = 0; admit < 2; ++admit) print_case(dim, nlist, nq, k, nprobe, plane != 0, admit != 0);
}

// beyond the grid: the exact scan's launch boundary, and rows so wide that a search is refused
static void extras() {
    for (int64_t nq : {1260, 1261, 1300})
        for (int plane = 0; plane < 2; ++plane)
            for (int admit = 0; admit < 2; ++admit) print_case(64, 256, nq, 26, 256, plane != 0, admit != 0);
    for (int dim : {37792, 37824, 40000, 71488, 71552, 80000})
        for (int64_t nq : {1, 17})
            for (int k : {1, 26})
                for (int nprobe : {1, 32, 128, 129, 4096})
                    for (int plane = 0; plane < 2; ++plane) print_case(dim, 4096, nq, k, nprobe, plane != 0, false);
    // 2^31 - 128 pairs: accepted with 16 queries per task, refused at one per task (the task bound passes 2^31); 2^31 + ... pairs
    for (int plane = 0; plane < 2; ++plane) {
        print_case(512, 1 << 20, (1 << 24) - 1, 10, 128, plane != 0, false);
        print_case(DIM_QCAP1, 1 << 20, (1 << 24) - 1, 10, 128, plane != 0, false);
        print_case(512, 1 << 20, (1 << 24) - 1, 10, 129, plane != 0, false);
    }
}

// ---- anchors: computed by hand from the expressions of ivf_search_lists before the plan moved out of it ------------------------------
static IvfPlan plan_of(int dim, int nlist, int64_t nq, int k, int nprobe, bool plane) {
    IvfFacts s;
    s.dim = dim; s.nlist = nlist; s.rows = 1000000; s.plane = plane;
    return ivf_plan_search(s, nq, k, nprobe, false);
}
static void anchors() {
    for (int dim : {64, 96, 128, 512, 1024}) CHECK(plan_of(dim, 4096, 1024, 15, 32, false).qcap == 16);
    CHECK(plan_of(5376, 4096, 1024, 15, 32, false).qcap == 5);
    CHECK(plan_of(DIM_QCAP1, 4096, 1024, 15, 32, false).qcap == 1);
    CHECK(plan_of(512, 4096, 1024, 15, 32, true).scan_lds == 37376 && plan_of(5376, 4096, 1024, 15, 32, true).scan_lds == 74576);
    CHECK(plan_of(512, 4096, 1024, 15, 32, false).scan_lds == 45568 && plan_of(5376, 4096, 1024, 15, 32, false).scan_lds == 120144);
    CHECK(plan_of(512, 4096, 1024, 15, 26, true).cmargin == 6 && plan_of(512, 4096, 1024, 15, 27, true).cmargin == 5);
    CHECK(plan_of(512, 4096, 1024, 15, 32, true).cmargin == 0 && plan_of(512, 4096, 1024, 15, 64, true).cmargin == 0);
    {   // the benchmark shape
        const IvfPlan p = plan_of(512, 4096, 1024, 15, 32, true);
        CHECK(p.status == IVF_PLAN_OK && p.hi_route);
        CHECK(p.npairs == 32768 && p.T == 6145 && !p.group_small && p.ccap == 2048 && p.split == 1 && p.tasks.bytes == 368656);
        CHECK(p.cap == 512 && p.refine_lds == 27904);
        CHECK(p.nslots == 1024 && p.xgrid == 4096 && p.xlds == 4096 && p.xlaunches == 1);
    }
    {   // ... with one query
        const IvfPlan p = plan_of(512, 4096, 1, 15, 32, true);
        CHECK(p.status == IVF_PLAN_OK && p.T == 35 && p.group_small && p.ccap == 8192 && p.split == 5);
    }
    {   // the exact scan's launch boundary
        CHECK(plan_of(64, 256, 1300, 26, 256, true).nslots == 1260);
        CHECK(plan_of(64, 256, 1260, 26, 256, true).xlaunches == 1);
        CHECK(plan_of(64, 256, 1261, 26, 256, true).xlaunches == 2);
        CHECK(plan_of(64, 256, 1300, 26, 256, false).xlaunches == 2);
    }
    // the refusals.  fp32 list scan: 4 (dim + 4) + 12 544 B of LDS at qcap 1, over 160 KB from dim 37 821 on
    CHECK(plan_of(37792, 4096, 1, 1, 1, false).status == IVF_PLAN_OK && plan_of(37824, 4096, 1, 1, 1, false).status == IVF_PLAN_DIM_TOO_LARGE);
    // f16 list scan: 2 (dim + 8) + 20 736 B, over 160 KB from dim 71 545 on: the search falls to the fp32 scan, which refuses it
    CHECK(plan_of(71552, 4096, 1, 1, 1, true).status == IVF_PLAN_DIM_TOO_LARGE && !plan_of(71552, 4096, 1, 1, 1, true).hi_route);
    // exact list scan at dim 40 000, k 26: 160 000 + 3328 + 4 nprobe B, over 160 KB from nprobe 129 on
    CHECK(plan_of(40000, 4096, 1, 26, 128, true).status == IVF_PLAN_OK && plan_of(40000, 4096, 1, 26, 129, true).status == IVF_PLAN_NPROBE_TOO_LARGE);
    CHECK(plan_of(71488, 4096, 1, 1, 1, true).hi_route);
    // pairs: 2^31 - 128 of them pass (T = 2^20 + 2^27 - 8 + 1), unless every pair is a task of its own; 2^31 + 2^24 - 129 do not
    CHECK(plan_of(512, 1 << 20, (1 << 24) - 1, 10, 128, true).status == IVF_PLAN_OK);
    CHECK(plan_of(DIM_QCAP1, 1 << 20, (1 << 24) - 1, 10, 128, true).status == IVF_PLAN_TOO_MANY_PAIRS);
    CHECK(plan_of(512, 1 << 20, (1 << 24) - 1, 10, 129, true).status == IVF_PLAN_TOO_MANY_PAIRS);
}

int main() {
    grid();
    extras();
    anchors();
    if (failures) { printf("ivf_plan_check: %d checks FAILED\n", failures); return 1; }
    printf("ivf_plan_check: ok\n");
    return 0;
}
