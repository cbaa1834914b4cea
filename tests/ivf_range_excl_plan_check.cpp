// ivf_range_excl_plan_check.cpp -- ivf_plan_range (csrc/ivf_plan.h) with its two exclusion parameters, without a GPU: has_admit (one
// exclusion set for the batch: the admission bitmap) and pq_m (one set of pq_m tags per query: the tag block in the scan's LDS).
// For every case of the grid it checks
//   * with both at their defaults (and with pq_m given but has_admit false, which means the same): the plan equals the 4-argument
//     plan field by field;
//   * has_admit alone: admit_words = ceil(rows / 64) + 1 (the spare word), admit = 8 bytes per word, no tag block;
//   * pq_m > 0: pq_m, pq_lds = ivf_pq_lds_bytes(qcap, pq_m), scan_lds = ivf_range_hi_lds_bytes + pq_lds, and NO bitmap and no hash
//     bitset (admit_words = admit = pq_bits = pq_bitset = 0);
//   * the route: that of ivf_plan_search(facts, nq, 1, nprobe, has_admit, pq_m); IVF_RANGE_HI only with scan_lds <= 160 KB;
//   * that everything the exclusion does not touch (coarse section, tasks, qbuf, the exact pass) is the 4-argument plan's;
//   * that the carved sub-arrays of `tasks`, `qbuf` and of the scan's LDS (f16 queries | tags | counts) do not overlap.
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

// what the exclusion parameters must leave alone
static bool same_outside(const IvfPlan& a, const IvfPlan& b) {
    return a.nq == b.nq && a.k == b.k && a.ksel == b.ksel && a.nprobe == b.nprobe && a.npairs == b.npairs && a.cmargin == b.cmargin &&
           a.qcap == b.qcap && a.T == b.T && a.group_small == b.group_small && a.group_lds == b.group_lds && a.xlds == b.xlds &&
           a.nslots == b.nslots && a.xgrid == b.xgrid && a.xlaunches == b.xlaunches && a.tasks.cnt == b.tasks.cnt && a.tasks.cur == b.tasks.cur &&
           a.tasks.nt == b.tasks.nt && a.tasks.tl == b.tasks.tl && a.tasks.tp == b.tasks.tp && a.tasks.tc == b.tasks.tc &&
           a.tasks.pq == b.tasks.pq && a.tasks.ps == b.tasks.ps && a.tasks.bytes == b.tasks.bytes && a.ws_a == b.ws_a && a.ws_b == b.ws_b &&
           a.part_s == b.part_s && a.part_i == b.part_i && a.cand_s == b.cand_s && a.xkey == b.xkey && a.xid == b.xid && a.xarrive == b.xarrive;
}
// ... and what follows the route (equal when the route is)
static bool same_route_fields(const IvfPlan& a, const IvfPlan& b) {
    return a.status == b.status && a.hi_route == b.hi_route && a.range_route == b.range_route && a.ccap == b.ccap && a.split == b.split &&
           a.scan_grid == b.scan_grid && a.cap == b.cap && a.refine_lds == b.refine_lds && a.cand_i == b.cand_i && a.qbuf.qh == b.qbuf.qh &&
           a.qbuf.qscale == b.qbuf.qscale && a.qbuf.qconst == b.qbuf.qconst && a.qbuf.eps == b.qbuf.eps && a.qbuf.cand_cnt == b.qbuf.cand_cnt &&
           a.qbuf.gbound == b.qbuf.gbound && a.qbuf.fsel == b.qbuf.fsel && a.qbuf.fcount == b.qbuf.fcount && a.qbuf.bytes == b.qbuf.bytes &&
           a.qbuf_thr == b.qbuf_thr;
}
static bool same_exclusion_fields(const IvfPlan& a, const IvfPlan& b) {
    return a.scan_lds == b.scan_lds && a.admit == b.admit && a.admit_words == b.admit_words && a.pq_m == b.pq_m && a.pq_lds == b.pq_lds &&
           a.pq_bits == b.pq_bits && a.pq_bitset == b.pq_bitset;
}

static void check_case(const IvfFacts& s, int64_t nq, int m, int nprobe_asked, bool has_admit, int pq_m) {
    const IvfPlan plain = ivf_plan_range(s, nq, m, nprobe_asked);
    const IvfPlan p = ivf_plan_range(s, nq, m, nprobe_asked, has_admit, pq_m);
    const IvfPlan topk = ivf_plan_search(s, nq, 1, nprobe_asked, has_admit, pq_m);
    const int eff_m = has_admit ? pq_m : 0;                                  // per-query tags mean something only in an exclusion-aware call
    printf("case dim %d nlist %d plane %d nq %lld m %d nprobe %d admit %d pq_m %d: status %d route %d qcap %d scan_lds %zu pq_lds %zu admit_words %lld\n",
           s.dim, s.nlist, (int)s.plane, (long long)nq, m, p.nprobe, (int)has_admit, pq_m, (int)p.status, p.range_route, p.qcap, p.scan_lds,
           p.pq_lds, (long long)p.admit_words);
    CHECK(same_outside(p, plain));
    if (plain.status == IVF_PLAN_TOO_MANY_PAIRS) { CHECK(p.status == IVF_PLAN_TOO_MANY_PAIRS); return; }
    // both off: today's plan, field by field
    if (!has_admit) {
        CHECK(same_route_fields(p, plain) && same_exclusion_fields(p, plain));
        CHECK(p.admit == 0 && p.admit_words == 0 && p.pq_m == 0 && p.pq_lds == 0 && p.pq_bits == 0 && p.pq_bitset == 0);
        return;
    }
    // the route is the top-k plan's, tag block included, and the hi route implies an LDS that fits
    const size_t want_pq_lds = ivf_pq_lds_bytes(p.qcap, eff_m);
    const bool want_hi = s.plane && ivf_hi_lds_bytes(p.qcap, s.dim) + want_pq_lds <= LDS_MAX;
    CHECK(topk.hi_route == want_hi && p.hi_route == want_hi);
    CHECK(p.range_route == (want_hi ? IVF_RANGE_HI : IVF_RANGE_EXACT));
    if (p.hi_route == plain.hi_route) CHECK(same_route_fields(p, plain));
    CHECK(p.pq_m == eff_m && p.pq_lds == want_pq_lds);
    CHECK(p.pq_bits == 0 && p.pq_bitset == 0);                               // no suspect pre-pass, whatever pq_m is
    if (eff_m == 0) {
        const int64_t words = (s.rows + 63) / 64 + 1;
        CHECK(p.admit_words == words && p.admit == (size_t)words * 8);
        CHECK(p.admit_words == topk.admit_words && p.admit == topk.admit);
        CHECK((int64_t)(p.admit_words - 1) * 64 >= s.rows);                  // a bit for every position, and the spare word behind them
    } else {
        CHECK(p.admit_words == 0 && p.admit == 0);
        CHECK(want_pq_lds >= (size_t)p.qcap * eff_m * 8 + (size_t)p.qcap * 4 && want_pq_lds % 16 == 0);
    }
    if (p.hi_route) {
        const size_t qbytes = ivf_range_hi_lds_bytes(p.qcap, s.dim);
        CHECK(p.scan_lds == qbytes + want_pq_lds && p.scan_lds <= LDS_MAX);
        // f16 queries | tags [qcap][m] int64 | counts [qcap] int32: the tag block begins where the queries end, 8-byte aligned
        const size_t tag_off = p.scan_lds - p.pq_lds;
        CHECK(tag_off == qbytes && tag_off % 8 == 0);
        const size_t off[] = {0, tag_off, tag_off + (size_t)p.qcap * eff_m * 8};
        const size_t size[] = {(size_t)p.qcap * (s.dim + 8) * 2, (size_t)p.qcap * eff_m * 8, eff_m ? (size_t)p.qcap * 4 : 0};
        check_carved(off, size, 3, p.scan_lds);
        CHECK(p.ccap == IVF_RANGE_CAP && p.cand_i == (size_t)nq * IVF_RANGE_CAP * sizeof(int) && p.scan_grid == p.T * p.split);
    } else {
        CHECK(p.scan_lds == 0 && p.cand_i == 0 && p.scan_grid == 0);
    }
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
    }
    CHECK(p.status == plain.status || p.hi_route != plain.hi_route);
}

int main() {
    const int dims[] = {32, 64, 96, 512, 5376};
    const int64_t nqs[] = {1, 16, 17, 300, 1024};
    const int nprobes[] = {1, 8, 32};
    const int ms[] = {1, 65, 128};
    const int pq_ms[] = {0, 1, 64};
    const int nlists[] = {64, 4096};
    int cases = 0, hi = 0, exact = 0;
    for (int dim : dims)
        for (int nlist : nlists)
            for (int plane = 0; plane < 2; ++plane) {
                if (plane && dim % 64 != 0) continue;                            // (no plane at such a width: ivf_ensure_plane)
                IvfFacts s; s.dim = dim; s.nlist = nlist; s.rows = plane ? 1000000 : 999937; s.plane = plane != 0;
                for (int64_t nq : nqs)
                    for (int nprobe : nprobes)
                        for (int m : ms)
                            for (int pq_m : pq_ms)
                                for (int admit = 0; admit < 2; ++admit) {
                                    check_case(s, nq, m, nprobe, admit != 0, pq_m);
                                    ++cases;
                                    const IvfPlan p = ivf_plan_range(s, nq, m, nprobe, admit != 0, pq_m);
                                    if (p.status == IVF_PLAN_OK) (p.range_route == IVF_RANGE_HI ? hi : exact) += 1;
                                }
            }
    CHECK(hi > 0 && exact > 0);
    // every width with a plane up to 8192: the route is the top-k plan's, and where the tag block takes a shape off the f16 scan (qcap
    // shrinks with the width, so today no width does: the count is printed) the range plan follows with an empty hi section
    {
        int found = 0;
        for (int dim = 64; dim <= 8192; dim += 64) {
            IvfFacts s; s.dim = dim; s.nlist = 64; s.rows = 5000; s.plane = true;
            const IvfPlan a = ivf_plan_range(s, 20, 128, 8), b = ivf_plan_range(s, 20, 128, 8, true, 64);
            CHECK(b.hi_route == ivf_plan_search(s, 20, 1, 8, true, 64).hi_route);
            if (b.hi_route) CHECK(b.scan_lds <= LDS_MAX);
            if (a.hi_route && !b.hi_route) { ++found; CHECK(b.range_route == IVF_RANGE_EXACT && b.scan_lds == 0 && b.cand_i == 0); }
        }
        printf("widths at which the tag block changes the route: %d\n", found);
    }
    // a store whose row count is a multiple of 64, and one row more: the spare word is there in both
    for (int64_t rows : {(int64_t)64, (int64_t)65, (int64_t)1, (int64_t)128 * 64}) {
        IvfFacts s; s.dim = 64; s.nlist = 64; s.rows = rows; s.plane = true;
        CHECK(ivf_plan_range(s, 3, 128, 8, true, 0).admit_words == (rows + 63) / 64 + 1);
    }
    printf("cases %d hi %d exact %d\n", cases, hi, exact);
    if (failures) { printf("ivf_range_excl_plan_check: %d FAILED\n", failures); return 1; }
    printf("ivf_range_excl_plan_check: ok\n");
    return 0;
}
