// ivf_range_plan_check.cpp -- the host-only planner of a range search over the probed lists (csrc/ivf_plan.h: ivf_plan_range), without
// a GPU.  For every case of a grid of indexes and searches it checks
//   * the route: IVF_RANGE_HI exactly when ivf_plan_search of the same index would take hi_route, IVF_RANGE_EXACT otherwise;
//   * that the coarse and grouping section (ws_a / ws_b, tasks, qcap, T, cmargin, group_small) is ivf_plan_search's, field for field;
//   * that the sub-arrays of `tasks` and `qbuf` (the floors among them) neither overlap nor leave their totals, and that every buffer
//     covers what the kernels index: 4096 positions per query, nslots x nprobe x M x 16 bytes of partial lists within the budget;
//   * the split (from the task count alone), the grids, every LDS size and the refusals;
//   * that ivf_plan_search still answers a fixed table of inputs as it did before ivf_plan_range was called (compared with its own
//     output, not with literals), its new trailing fields untouched.
// Prints one line per case; exit status 0 = every check passed, a failed check prints its line and the run ends with status 1.
#include "ivf_plan.h"

#include <stdio.h>

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static const size_t LDS_MAX = 160 * 1024;

static void check_carved(const size_t* off, const size_t* size, int n, size_t bytes) {
    for (int i = 0; i < n; ++i) {
        const size_t end = i + 1 < n ? off[i + 1] : bytes;
        CHECK(end >= off[i] && end - off[i] >= size[i]);
    }
}

// every field ivf_plan_search sets
static bool same_plan(const IvfPlan& a, const IvfPlan& b) {
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
           a.xarrive == b.xarrive && a.admit == b.admit && a.admit_words == b.admit_words && a.pq_m == b.pq_m && a.pq_lds == b.pq_lds &&
           a.pq_bits == b.pq_bits && a.pq_bitset == b.pq_bitset;
}

static void check_range(const IvfFacts& s, int64_t nq, int m, int nprobe_asked) {
    const IvfPlan ref = ivf_plan_search(s, nq, 10, nprobe_asked, false);
    const IvfPlan p = ivf_plan_range(s, nq, m, nprobe_asked);
    const int nprobe = p.nprobe;
    printf("case dim %d nlist %d plane %d nq %lld m %d nprobe %d: status %d route %d qcap %d T %lld split %d grid %lld scan_lds %zu xlds %zu nslots %lld "
           "xgrid %lld xlaunches %lld cand_i %zu\n", s.dim, s.nlist, (int)s.plane, (long long)nq, m, nprobe, (int)p.status, p.range_route, p.qcap,
           (long long)p.T, p.split, (long long)p.scan_grid, p.scan_lds, p.xlds, (long long)p.nslots, (long long)p.xgrid, (long long)p.xlaunches, p.cand_i);
    CHECK(nprobe >= 1 && nprobe <= s.nlist && (nprobe == nprobe_asked || nprobe == s.nlist));
    CHECK(p.nq == nq && p.k == m && p.ksel == 0 && p.npairs == nq * nprobe);
    // the coarse and grouping section is the top-k plan's
    CHECK(p.nprobe == ref.nprobe && p.npairs == ref.npairs && p.cmargin == ref.cmargin && p.qcap == ref.qcap && p.T == ref.T);
    CHECK(p.ws_a == ref.ws_a && p.ws_b == ref.ws_b && p.group_small == ref.group_small && p.group_lds == ref.group_lds);
    if (p.status == IVF_PLAN_TOO_MANY_PAIRS) { CHECK(ref.status == IVF_PLAN_TOO_MANY_PAIRS); return; }
    CHECK(ref.status != IVF_PLAN_TOO_MANY_PAIRS);
    CHECK(p.tasks.cnt == ref.tasks.cnt && p.tasks.cur == ref.tasks.cur && p.tasks.nt == ref.tasks.nt && p.tasks.tl == ref.tasks.tl &&
          p.tasks.tp == ref.tasks.tp && p.tasks.tc == ref.tasks.tc && p.tasks.pq == ref.tasks.pq && p.tasks.ps == ref.tasks.ps &&
          p.tasks.bytes == ref.tasks.bytes);
    // no per-pair partial lists, no scores, no admission bitmap, no tags
    CHECK(p.part_s == 0 && p.part_i == 0 && p.cand_s == 0 && p.admit == 0 && p.admit_words == 0 && p.pq_m == 0 && p.pq_lds == 0 && p.pq_bitset == 0);
    // the route: the top-k plan's own choice (a plane and the top-k scan's LDS within a CU's)
    const bool want_hi = s.plane && ivf_hi_lds_bytes(p.qcap, s.dim) <= LDS_MAX;
    CHECK(ref.hi_route == want_hi);
    CHECK(p.hi_route == ref.hi_route && p.range_route == (ref.hi_route ? IVF_RANGE_HI : IVF_RANGE_EXACT));
    {
        const size_t nlist = (size_t)s.nlist, T = (size_t)p.T, I = sizeof(int), npairs = (size_t)p.npairs;
        const size_t off[] = {p.tasks.cnt, p.tasks.cur, p.tasks.nt, p.tasks.tl, p.tasks.tp, p.tasks.tc, p.tasks.pq, p.tasks.ps};
        const size_t size[] = {nlist * I, nlist * I, I, T * I, T * I, T * I, npairs * I, npairs * I};
        check_carved(off, size, 8, p.tasks.bytes);
    }
    {
        const size_t vec = (size_t)nq * 4;
        const size_t off[] = {p.qbuf.qh, p.qbuf.qscale, p.qbuf.qconst, p.qbuf.eps, p.qbuf.cand_cnt, p.qbuf_thr, p.qbuf.fsel, p.qbuf.fcount};
        const size_t size[] = {p.hi_route ? (size_t)nq * s.dim * 2 : 0, vec, vec, vec, vec, vec, vec, 8 * sizeof(int)};
        check_carved(off, size, 8, p.qbuf.bytes);
        for (size_t o : off) CHECK(o % 256 == 0);
    }
    if (p.hi_route) {
        CHECK(p.ccap == IVF_RANGE_CAP && p.ccap == 4096 && p.cap == IVF_RANGE_CAP);
        CHECK(p.cand_i == (size_t)nq * 4096 * sizeof(int));
        CHECK(p.split == (p.T <= 64 ? 8 : p.T <= 128 ? 4 : p.T <= 256 ? 2 : 1));      // the task count alone: neither m nor nprobe
        CHECK(p.scan_grid == p.T * p.split);
        CHECK(p.scan_lds == (size_t)p.qcap * (s.dim + 8) * 2 && p.scan_lds <= ivf_hi_lds_bytes(p.qcap, s.dim) && p.scan_lds <= LDS_MAX);
        CHECK(p.refine_lds == (size_t)4096 * 12 + 64 && p.refine_lds <= LDS_MAX);
    } else {
        CHECK(p.ccap == 0 && p.cand_i == 0 && p.scan_grid == 0 && p.scan_lds == 0 && p.refine_lds == 0 && p.split == 1);
    }
    CHECK(p.xlds == (size_t)s.dim * 4 + (size_t)IVX_WAVES * m * 16 + IVX_WAVES * 4 + (size_t)nprobe * 4);
    if (p.status == IVF_PLAN_NPROBE_TOO_LARGE) { CHECK(p.xlds > LDS_MAX); return; }
    CHECK(p.status == IVF_PLAN_OK && p.xlds <= LDS_MAX);
    CHECK(p.nslots >= 1 && p.nslots <= nq);
    CHECK((size_t)p.nslots * nprobe * m * 16 <= IVX_PART_BUDGET || p.nslots == 1);
    CHECK(p.xkey == (size_t)p.nslots * nprobe * m * sizeof(double) && p.xid == (size_t)p.nslots * nprobe * m * sizeof(int64_t));
    CHECK(p.xarrive == (size_t)p.nslots * sizeof(int));
    CHECK(p.xgrid >= 1 && p.xgrid <= IVX_MAX_GRID && p.xgrid <= p.nslots * nprobe);
    CHECK(p.xlaunches * p.nslots >= nq && (p.xlaunches - 1) * p.nslots < nq);
}

int main() {
    const int dims[] = {32, 64, 96, 512, 1056, 5376};
    const int64_t nqs[] = {1, 16, 17, 1024};
    const int ms[] = {1, 128};
    const int nlists[] = {64, 4096};

    // the fixed table of top-k plans, before anything else is planned
    struct In { int dim, nlist; bool plane; int64_t nq; int k, nprobe; bool admit; int pq_m; };
    const In table[] = {{64, 64, true, 100, 5, 8, false, 0},    {512, 128, true, 300, 15, 32, false, 0}, {512, 4096, true, 1, 10, 32, false, 0},
                        {512, 4096, true, 1024, 10, 32, true, 0}, {96, 64, false, 3, 10, 64, false, 0},    {5376, 64, true, 20, 15, 4, false, 0},
                        {1056, 64, false, 20, 26, 16, true, 8}, {64, 64, true, 16, 26, 64, true, 64},    {32, 64, false, 17, 1, 1, false, 0}};
    const int n_table = (int)(sizeof(table) / sizeof(table[0]));
    IvfPlan before[sizeof(table) / sizeof(table[0])];
    for (int i = 0; i < n_table; ++i) {
        IvfFacts s; s.dim = table[i].dim; s.nlist = table[i].nlist; s.rows = 100000; s.plane = table[i].plane;
        before[i] = ivf_plan_search(s, table[i].nq, table[i].k, table[i].nprobe, table[i].admit, table[i].pq_m);
        CHECK(before[i].range_route == -1 && before[i].qbuf_thr == 0);          // the range plan's fields: not the top-k plan's to set
    }

    int cases = 0, hi = 0, exact = 0;
    for (int dim : dims)
        for (int nlist : nlists)
            for (int plane = 0; plane < 2; ++plane) {
                if (plane && dim % 64 != 0) continue;                            // (no plane at such a width: ivf_ensure_plane)
                IvfFacts s; s.dim = dim; s.nlist = nlist; s.rows = 1000000; s.plane = plane != 0;
                for (int64_t nq : nqs)
                    for (int m : ms)
                        for (int nprobe : {1, nlist}) {
                            check_range(s, nq, m, nprobe);
                            ++cases;
                            const IvfPlan p = ivf_plan_range(s, nq, m, nprobe);
                            if (p.status == IVF_PLAN_OK) (p.range_route == IVF_RANGE_HI ? hi : exact) += 1;
                        }
            }
    CHECK(hi > 0 && exact > 0);
    // a request beyond nlist is clamped; the refusals are reached
    {
        IvfFacts s; s.dim = 64; s.nlist = 64; s.rows = 1000; s.plane = true;
        CHECK(ivf_plan_range(s, 5, 128, 1000).nprobe == 64);
        CHECK(ivf_plan_range(s, 5, 128, 0).nprobe == 1);
        s.nlist = 1 << 20;
        CHECK(ivf_plan_range(s, (1 << 24) - 1, 128, 1 << 20).status == IVF_PLAN_TOO_MANY_PAIRS);
        CHECK(ivf_plan_range(s, 4, 128, 1 << 20).status == IVF_PLAN_NPROBE_TOO_LARGE);
        CHECK(ivf_plan_range(s, 4, 1, 1 << 20).status == IVF_PLAN_NPROBE_TOO_LARGE);
    }
    // dim 5376 has a plane and the top-k scan's LDS does not fit 16 queries of it beside the score tile?  whatever the answer, it is the top-k plan's
    {
        IvfFacts s; s.dim = 5376; s.nlist = 64; s.rows = 8000; s.plane = true;
        CHECK(ivf_plan_range(s, 20, 128, 4).hi_route == ivf_plan_search(s, 20, 15, 4, false).hi_route);
    }

    for (int i = 0; i < n_table; ++i) {
        IvfFacts s; s.dim = table[i].dim; s.nlist = table[i].nlist; s.rows = 100000; s.plane = table[i].plane;
        const IvfPlan after = ivf_plan_search(s, table[i].nq, table[i].k, table[i].nprobe, table[i].admit, table[i].pq_m);
        CHECK(same_plan(before[i], after));
        CHECK(after.range_route == -1 && after.qbuf_thr == 0);
    }
    printf("cases %d hi %d exact %d\n", cases, hi, exact);
    if (failures) { printf("ivf_range_plan_check: %d FAILED\n", failures); return 1; }
    printf("ivf_range_plan_check: ok\n");
    return 0;
}
