// ivf_plan_pq_check.cpp -- the per-query width of the IVF planner (csrc/ivf_plan.h: ivf_plan_search's trailing pq_m), without a GPU.
//   1. over the sweep of tests/ivf_plan_check.cpp, the plan with width 0 equals the plan of the five-argument call field for field;
//   2. with width m the suspect bitmap is sized as the admission bitmap, the hash bitset is the documented power of two, the tag block
//      is the documented [qcap][m] int64 + [qcap] int in 16-byte units, added to scan_lds of either route and to nothing else; every
//      other field is that of the batch-wide plan unless the tag block moved the route or refused the search, which the 160 KB checks
//      decide;
//   3. anchors computed by hand.
// Exit status 0 = every check passed.
#include "ivf_plan.h"

#include <math.h>
#include <stdio.h>

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static const size_t LDS_MAX = 160 * 1024;

// every field but the four of the per-query width
static bool same_but_pq(const IvfPlan& a, const IvfPlan& b) {
    return a.status == b.status && a.nq == b.nq && a.k == b.k && a.ksel == b.ksel && a.nprobe == b.nprobe && a.npairs == b.npairs &&
           a.cmargin == b.cmargin && a.qcap == b.qcap && a.T == b.T && a.group_small == b.group_small && a.group_lds == b.group_lds &&
           a.hi_route == b.hi_route && a.ccap == b.ccap && a.split == b.split && a.scan_grid == b.scan_grid && a.scan_lds == b.scan_lds &&
           a.cap == b.cap && a.refine_lds == b.refine_lds && a.xlds == b.xlds && a.nslots == b.nslots && a.xgrid == b.xgrid &&
           a.xlaunches == b.xlaunches && a.tasks.cnt == b.tasks.cnt && a.tasks.cur == b.tasks.cur && a.tasks.nt == b.tasks.nt &&
           a.tasks.tl == b.tasks.tl && a.tasks.tp == b.tasks.tp && a.tasks.tc == b.tasks.tc && a.tasks.pq == b.tasks.pq &&
           a.tasks.ps == b.tasks.ps && a.tasks.bytes == b.tasks.bytes && a.qbuf.qh == b.qbuf.qh && a.qbuf.qscale == b.qbuf.qscale &&
           a.qbuf.qconst == b.qbuf.qconst && a.qbuf.eps == b.qbuf.eps && a.qbuf.cand_cnt == b.qbuf.cand_cnt && a.qbuf.gbound == b.qbuf.gbound &&
           a.qbuf.fsel == b.qbuf.fsel && a.qbuf.fcount == b.qbuf.fcount && a.qbuf.bytes == b.qbuf.bytes && a.ws_a == b.ws_a && a.ws_b == b.ws_b &&
           a.part_s == b.part_s && a.part_i == b.part_i && a.cand_s == b.cand_s && a.cand_i == b.cand_i && a.xkey == b.xkey && a.xid == b.xid &&
           a.xarrive == b.xarrive && a.admit == b.admit && a.admit_words == b.admit_words;
}

static long cases = 0;
static void check_case(int dim, int nlist, int64_t nq, int k, int nprobe, bool plane) {
    IvfFacts s;
    s.dim = dim; s.nlist = nlist; s.rows = (int64_t)nlist * 100 + 37; s.plane = plane;
    for (int admit = 0; admit < 2; ++admit) {
        const IvfPlan base = ivf_plan_search(s, nq, k, nprobe, admit != 0);
        const IvfPlan zero = ivf_plan_search(s, nq, k, nprobe, admit != 0, 0);
        CHECK(same_but_pq(base, zero));
        CHECK(zero.pq_m == 0 && zero.pq_lds == 0 && zero.pq_bits == 0 && zero.pq_bitset == 0);
        // without a bitmap there is no per-query rule: the width is ignored
        if (!admit) { const IvfPlan p = ivf_plan_search(s, nq, k, nprobe, false, 7); CHECK(same_but_pq(base, p) && p.pq_m == 0 && p.pq_lds == 0 && p.pq_bitset == 0); }
    }
    const IvfPlan base = ivf_plan_search(s, nq, k, nprobe, true);
    for (int m : {1, 2, 7, 40, 64}) {
        ++cases;
        const IvfPlan p = ivf_plan_search(s, nq, k, nprobe, true, m);
        CHECK(p.pq_m == m);
        // the suspect bitmap: one bit per row and the spare word, as the admission bitmap
        CHECK(p.admit_words == (s.rows + 63) / 64 + 1 && p.admit == (size_t)p.admit_words * 8 && p.admit == base.admit);
        // the hash bitset: the power of two >= 32 nq m within [2^12, 2^30] bits; expected share of false suspects below 1 %
        CHECK(p.pq_bits >= IVF_PQ_MIN_BITS && p.pq_bits <= IVF_PQ_MAX_BITS && (p.pq_bits & (p.pq_bits - 1)) == 0 && p.pq_bitset == (size_t)p.pq_bits / 8);
        CHECK(p.pq_bits >= 32 * nq * m || p.pq_bits == IVF_PQ_MAX_BITS);
        CHECK(p.pq_bits == IVF_PQ_MIN_BITS || p.pq_bits / 2 < 32 * nq * m);
        if (p.pq_bits < IVF_PQ_MAX_BITS) { const double f = 1.0 - exp(-2.0 * (double)(nq * m) / (double)p.pq_bits); CHECK(f * f < 0.01); }
        if (p.status == IVF_PLAN_TOO_MANY_PAIRS) { CHECK(base.status == IVF_PLAN_TOO_MANY_PAIRS); continue; }      // (refused before any LDS is sized)
        // the tag block
        const size_t tag = (size_t)p.qcap * m * 8 + (size_t)p.qcap * 4;
        CHECK(p.pq_lds >= tag && p.pq_lds < tag + 16 && p.pq_lds % 16 == 0 && p.pq_lds == ivf_pq_lds_bytes(p.qcap, m));
        if (p.status == IVF_PLAN_DIM_TOO_LARGE) { CHECK(!p.hi_route && p.scan_lds > LDS_MAX && p.scan_lds == knn_sq_lds_f32(p.qcap, s.dim) + p.pq_lds); continue; }
        CHECK(p.scan_lds == (p.hi_route ? ivf_hi_lds_bytes(p.qcap, s.dim) : knn_sq_lds_f32(p.qcap, s.dim)) + p.pq_lds);
        CHECK(p.scan_lds <= LDS_MAX && (p.scan_lds - p.pq_lds) % 16 == 0);
        CHECK(p.hi_route == (plane && ivf_hi_lds_bytes(p.qcap, s.dim) + p.pq_lds <= LDS_MAX));
        CHECK(p.xlds == ivf_exact_lds_bytes(s.dim, k, p.nprobe));      // (the exact list scan holds the tags in registers)
        if (p.status == IVF_PLAN_NPROBE_TOO_LARGE) { CHECK(p.xlds > LDS_MAX); continue; }
        CHECK(p.status == IVF_PLAN_OK && p.xlds <= LDS_MAX && p.refine_lds <= LDS_MAX);
        if (p.hi_route == base.hi_route && base.status == IVF_PLAN_OK) {      // the same route: the batch-wide plan + the tag block
            IvfPlan q = p;
            q.scan_lds -= p.pq_lds;
            CHECK(same_but_pq(q, base));
        }
    }
}

static void anchors() {
    IvfFacts s;
    s.dim = 512; s.nlist = 4096; s.rows = 1000000; s.plane = true;
    {   // the benchmark shape, leave-one-out: 1024 tags -> 2^15 bits; 16 x 8 + 64 = 192 B of tags behind 37 376 B
        const IvfPlan p = ivf_plan_search(s, 1024, 15, 32, true, 1);
        CHECK(p.status == IVF_PLAN_OK && p.hi_route && p.pq_bits == 32768 && p.pq_bitset == 4096 && p.pq_lds == 192 && p.scan_lds == 37376 + 192);
        CHECK(p.admit_words == 15626 && p.admit == 125008);
    }
    {   // ... 64 tags per query: 2^21 bits, 16 x 64 x 8 + 64 = 8256 B
        const IvfPlan p = ivf_plan_search(s, 1024, 15, 32, true, 64);
        CHECK(p.pq_bits == 2097152 && p.pq_bitset == 262144 && p.pq_lds == 8256 && p.scan_lds == 37376 + 8256);
        s.plane = false;
        CHECK(ivf_plan_search(s, 1024, 15, 32, true, 64).scan_lds == 45568 + 8256);
        s.plane = true;
    }
    CHECK(ivf_plan_search(s, 1, 15, 32, true, 1).pq_bits == 4096);             // the floor
    CHECK(ivf_plan_search(s, 128, 15, 32, true, 1).pq_bits == 4096 && ivf_plan_search(s, 129, 15, 32, true, 1).pq_bits == 8192);
    CHECK(ivf_plan_search(s, (1 << 24) - 1, 15, 1, true, 64).pq_bits == IVF_PQ_MAX_BITS);      // the cap
    CHECK(ivf_pq_lds_bytes(5, 3) == 144 && ivf_pq_lds_bytes(1, 1) == 16 && ivf_pq_lds_bytes(16, 0) == 0);
    // the tag block moves a search off the f16 route: 2 (dim + 8) + 20 736 B reaches 160 KB at dim 71 544, qcap 1; with 64 tags (528 B)
    // the f16 scan no longer fits from dim 71 296 on, and the fp32 scan refuses such rows
    s.dim = 71488;
    CHECK(ivf_plan_search(s, 1, 1, 1, true).hi_route && !ivf_plan_search(s, 1, 1, 1, true, 64).hi_route);
    CHECK(ivf_plan_search(s, 1, 1, 1, true, 64).status == IVF_PLAN_DIM_TOO_LARGE);
    s.dim = 71232;
    CHECK(ivf_plan_search(s, 1, 1, 1, true, 64).hi_route);      // (163 216 + 528 B; the exact list scan refuses rows this wide afterwards)
    // fp32 scan: 4 (dim + 4) + 12 544 B at qcap 1 is 163 728 B at dim 37 792: it fits without tags and not with 528 B of them
    s.plane = false; s.dim = 37792;
    CHECK(ivf_plan_search(s, 1, 1, 1, true).status == IVF_PLAN_OK);
    CHECK(ivf_plan_search(s, 1, 1, 1, true, 64).status == IVF_PLAN_DIM_TOO_LARGE);
}

int main() {
    const int dims[] = {64, 96, 128, 512, 1024, 5376, 16384, 37792, 71488};
    const int nlists[] = {8, 64, 4096, 8193};
    const int64_t nqs[] = {1, 16, 17, 128, 129, 1024, 6000};
    const int ks[] = {1, 10, 11, 15, 26};
    for (int dim : dims)
        for (int nlist : nlists)
            for (int64_t nq : nqs)
                for (int k : ks)
                    for (int nprobe : {1, 8, 26, 27, 32, nlist})
                        for (int plane = 0; plane < 2; ++plane) check_case(dim, nlist, nq, k, nprobe, plane != 0);
    for (int plane = 0; plane < 2; ++plane) check_case(512, 1 << 20, (1 << 24) - 1, 10, 129, plane != 0);
    anchors();
    if (failures) { printf("ivf_plan_pq_check: %d checks FAILED\n", failures); return 1; }
    printf("ivf_plan_pq_check: ok %ld plans\n", cases);
    return 0;
}
