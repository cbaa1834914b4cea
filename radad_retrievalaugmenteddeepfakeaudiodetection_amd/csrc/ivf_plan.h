// ivf_plan.h -- the host side of an IVF list-scan search that needs no GPU: the task bound, which grouping kernels and which list
// scan run, every LDS size, the launches of the exact list scan, the byte count of every buffer the search sizes, and where the
// sub-arrays of the two carved buffers (`tasks`, `qbuf`) lie (the PLAN).
//
// Plain C++17 over knn_plan.h: no HIP header, no handle, no stream.  ivf.inc supplies the facts (IvfFacts), sizes the buffers the plan
// names, forms its pointers from the plan's offsets and launches what the plan says.  tests/ivf_plan_check.cpp drives this header alone.
#pragma once
#include "knn_plan.h"

// ---- constants the plan reads (the kernels of ivf.inc are written against the same ones) ------------------------------------------
constexpr int IVF_MAX_K = 128;           // largest k of radad_ivf_search (HipIVFFlatIndex.MAX_K); flat searches take any k <= RADAD_KNN_MAX_K
constexpr int IVF_TASK_THREADS = 1024;   // k_ivf_tasks, k_ivf_group_small: one workgroup
// grouping of a SMALL batch in one launch (k_ivf_group_small)
constexpr int IVG_MAX_PAIRS = 4096;
constexpr int IVG_MAX_LISTS = 8192;
// certified f16 list scan (k_ivf_scan_hi)
constexpr int IVH_CHUNK = 256;                 // rows per chunk: 4 waves x 4 steps of 16
constexpr int IVH_SLD = IVH_CHUNK + 4;         // score row (floats)
constexpr int IVH_CAND_CAP = 2048;             // candidate buffer per query ...
constexpr int IVH_CAND_CAP_SMALLQ = 8192;      // ... of a batch of <= 16 queries (its lists are split over several workgroups, each
                                               // of which emits against the k-th best of its own few rows)
constexpr size_t ivf_hi_lds_bytes(int qcap, int dim) {
    return (size_t)qcap * (dim + 8) * 2 + (size_t)SQ_NQ * IVH_SLD * 4 + (size_t)SQ_NQ * 32 * 8;
}
// exact float64 list scan (k_ivf_exact)
constexpr int IVX_THREADS = 512;
constexpr int IVX_WAVES = IVX_THREADS / 64;
constexpr int IVX_MAX_GRID = 4096;
constexpr size_t IVX_PART_BUDGET = (size_t)128 << 20;    // partial lists of one launch (nprobe x k x 16 B per query)
constexpr size_t ivf_exact_lds_bytes(int dim, int k, int nprobe) {
    return (size_t)dim * 4 + (size_t)IVX_WAVES * k * 16 + (size_t)nprobe * 4;
}
// per-query exclusion sets (radad_ivf_search_excl_pq), m tags per query
constexpr int IVF_PQ_MAX_TAGS = 64;            // RADAD_EXCL_PQ_MAX_TAGS: one wave compares a row's tag with a query's set in one ballot
// the tag block both list scans append to their LDS: [qcap][m] int64 tags of the task's queries, then [qcap] clamped counts, whole
// 16-byte units (k_ivf_exact has one query per pair and holds its tags in registers, lane t tag t: no LDS)
constexpr size_t ivf_pq_lds_bytes(int qcap, int m) {
    return m > 0 ? (((size_t)qcap * m * 8 + (size_t)qcap * 4 + 15) & ~(size_t)15) : 0;
}
// The hash bitset of the pre-pass (k_ivf_pq_hash, k_ivf_pq_suspect): every live tag of the batch sets two bits of a bitset of B bits; a
// stored row is SUSPECT when both bits of its tag are set.  With n = nq m tags (an upper bound on the live ones) a row no query excludes
// is suspect with probability (1 - exp(-2 n / B))^2; B = the power of two >= 32 n gives 2 n / B <= 1/16 and a share below
// (1 - exp(-1/16))^2 = 0.37 % -- under 1 % with room for the hash not being ideal.  At least 2^12 bits (one 512-byte clear), at most
// 2^30 (128 MB, reached by 2^25 tags: beyond that the share of false suspects grows, the result stays exact -- the list kernels decide).
constexpr int64_t IVF_PQ_MIN_BITS = (int64_t)1 << 12, IVF_PQ_MAX_BITS = (int64_t)1 << 30;
constexpr int64_t ivf_pq_bitset_bits(int64_t nq, int m) {
    int64_t b = IVF_PQ_MIN_BITS;
    while (b < IVF_PQ_MAX_BITS && b < 32 * nq * m) b <<= 1;
    return b;
}

// what the plan reads of an index
struct IvfFacts {
    int dim = 0, nlist = 0;
    int64_t rows = 0;            // rows the index holds (> 0: an empty index is answered without a plan)
    bool plane = false;          // the list-major f16 plane is available (ivf_ensure_plane)
};

// why a search is refused (ivf.inc: RADAD_EINVAL with the message of each)
enum IvfPlanStatus { IVF_PLAN_OK = 0, IVF_PLAN_TOO_MANY_PAIRS, IVF_PLAN_DIM_TOO_LARGE, IVF_PLAN_NPROBE_TOO_LARGE };

struct IvfPlan {
    IvfPlanStatus status = IVF_PLAN_OK;      // anything else: the fields behind the refused step are not set
    int64_t nq = 0;
    int k = 0, ksel = 0;
    int nprobe = 0;                  // as searched: within [1, nlist]
    int64_t npairs = 0;              // (query, probe) pairs
    // coarse search + grouping
    int cmargin = 0;                 // spare entries of the coarse search's lists
    int qcap = 0;                    // queries per task: query rows that fit in LDS (16 unless dim is very large)
    int64_t T = 0;                   // upper bound on the number of tasks
    bool group_small = false;        // k_ivf_group_small (one launch); else k_ivf_count, k_ivf_tasks, k_ivf_scatter
    size_t group_lds = 0;            // k_ivf_group_small: the per-list counters
    // the list scan and its re-rank
    bool hi_route = false;           // the certified f16 list scan; else the fp32 list scan
    int ccap = 0;                    // f16 route: entries of a query's candidate buffer
    int split = 1;                   // f16 route: workgroups per task
    int64_t scan_grid = 0;           // workgroups of the list scan
    size_t scan_lds = 0;             // LDS of the list scan
    int cap = 0;                     // candidates the re-rank can take per query
    size_t refine_lds = 0;           // LDS of k_merge_refine
    // exact list scan: launch i of xlaunches takes the slots i nslots .. (i + 1) nslots of the rejected queries
    size_t xlds = 0;
    int64_t nslots = 0;
    int64_t xgrid = 0;
    int64_t xlaunches = 0;
    // `tasks` (ints; the per-list counters FIRST: k_ivf_tasks leaves them zero for the next search, whatever that one's sizes are)
    struct { size_t cnt = 0, cur = 0, nt = 0, tl = 0, tp = 0, tc = 0, pq = 0, ps = 0, bytes = 0; } tasks;
    // `qbuf`: the queries' f16 side, per-query scratch of either route, the certificate's list of rejected queries, the search's 8 counters
    struct { size_t qh = 0, qscale = 0, qconst = 0, eps = 0, cand_cnt = 0, gbound = 0, fsel = 0, fcount = 0, bytes = 0; } qbuf;
    // bytes of every other buffer the search sizes (0: not used by this search)
    size_t ws_a = 0, ws_b = 0, part_s = 0, part_i = 0, cand_s = 0, cand_i = 0, xkey = 0, xid = 0, xarrive = 0, admit = 0;
    int64_t admit_words = 0;         // words of the admission bitmap, the spare one included
    // per-query exclusion sets (pq_m > 0): `admit` is then the SUSPECT bitmap (same size, same spare word)
    int pq_m = 0;                    // tags per query
    size_t pq_lds = 0;               // the tag block, part of scan_lds on both routes (at offset scan_lds - pq_lds)
    int64_t pq_bits = 0;             // bits of the pre-pass's hash bitset (a power of two)
    size_t pq_bitset = 0;            // its bytes
    // ivf_plan_range only (ivf_plan_search leaves both as they are): the route and where the floors thr[q] lie in `qbuf`
    int range_route = -1;            // IVF_RANGE_HI / IVF_RANGE_EXACT
    size_t qbuf_thr = 0;
};

// The plan of radad_ivf_search / radad_ivf_search_excl / radad_ivf_search_excl_pq on the probed lists (k + KNN_MARGIN <= 32).
// has_admit: the search reads an admission bitmap (exclusion-aware with a set that is not empty).  pq_m > 0 (with has_admit): one set
// of pq_m tags per query -- the bitmap is the suspect bitmap, the pre-pass needs its hash bitset and both list scans the tag block in
// LDS; with pq_m == 0 the plan is field for field what it was (tests/ivf_plan_pq_check.cpp).
static IvfPlan ivf_plan_search(const IvfFacts& s, int64_t nq, int k, int nprobe, bool has_admit, int pq_m = 0) {
    IvfPlan p;
    nprobe = std::max(1, std::min(nprobe, s.nlist));
    const int64_t n = s.rows;
    const int ksel = k + KNN_MARGIN;
    const int64_t npairs = nq * nprobe;
    p.nq = nq; p.k = k; p.ksel = ksel; p.nprobe = nprobe; p.npairs = npairs;
    if (has_admit) {
        const int64_t n_words = ((n + 63) >> 6) + 1;             // (+ 1: the spare word, all zero)
        p.admit_words = n_words;
        p.admit = (size_t)n_words * sizeof(unsigned long long);
    }
    if (!has_admit) pq_m = 0;
    p.pq_m = pq_m;
    if (pq_m > 0) {
        p.pq_bits = ivf_pq_bitset_bits(nq, pq_m);
        p.pq_bitset = (size_t)(p.pq_bits >> 3);
    }

    // 1) coarse quantiser: the nprobe nearest centroids of every query
    p.ws_a = (size_t)npairs * sizeof(float);
    p.ws_b = (size_t)npairs * sizeof(int64_t);
    const int cmargin = nprobe + KNN_MARGIN <= 32 ? KNN_MARGIN : std::max(0, 32 - nprobe);   // keep the register-list kernels
    // 2) group the (query, probe) pairs by list on the device; <= qcap queries per task (LDS holds qcap query rows)
    const int qcap = (int)std::max<size_t>(1, std::min<size_t>(SQ_NQ, (size_t)(112 * 1024) / ((size_t)(s.dim + 4) * sizeof(float))));
    const int64_t T = std::min<int64_t>(s.nlist, npairs) + npairs / qcap + 1;      // upper bound on the number of tasks
    p.cmargin = cmargin; p.qcap = qcap; p.T = T;
    if (!(npairs < (int64_t)1 << 31 && T < (int64_t)1 << 31)) { p.status = IVF_PLAN_TOO_MANY_PAIRS; return p; }
    {   // cnt [nlist] | cur [nlist] | nt [1] | tl [T] | tp [T] | tc [T] | pq [npairs] | ps [npairs]: 3 T + 2 npairs + 2 nlist + 1 ints
        size_t off = 0;
        auto take = [&](int64_t ints) { const size_t o = off; off += (size_t)ints * sizeof(int); return o; };
        p.tasks.cnt = take(s.nlist); p.tasks.cur = take(s.nlist); p.tasks.nt = take(1);
        p.tasks.tl = take(T); p.tasks.tp = take(T); p.tasks.tc = take(T); p.tasks.pq = take(npairs); p.tasks.ps = take(npairs);
        p.tasks.bytes = off;
    }
    p.part_s = (size_t)npairs * ksel * sizeof(float);
    p.part_i = (size_t)npairs * ksel * sizeof(int);
    p.group_small = npairs <= IVG_MAX_PAIRS && s.nlist <= IVG_MAX_LISTS;
    p.group_lds = p.group_small ? (size_t)s.nlist * sizeof(int) : 0;

    // per-query scratch of either route: eps, the certificate's list of rejected queries, the search's counters
    const size_t pq_lds = ivf_pq_lds_bytes(qcap, pq_m);
    p.pq_lds = pq_lds;
    const bool hi_route = s.plane && ivf_hi_lds_bytes(qcap, s.dim) + pq_lds <= 160 * 1024;
    const size_t b_qh = hi_route ? al256((size_t)nq * s.dim * 2) : 0, b_vec = al256((size_t)nq * sizeof(float));
    p.hi_route = hi_route;
    {   // qh | qscale | qconst | eps | cand_cnt | gbound | fsel | fcount [8]: [0] rejected, [1] answered by the exact scan
        size_t off = 0;
        auto take = [&](size_t bytes) { const size_t o = off; off += bytes; return o; };
        p.qbuf.qh = take(b_qh); p.qbuf.qscale = take(b_vec); p.qbuf.qconst = take(b_vec); p.qbuf.eps = take(b_vec);
        p.qbuf.cand_cnt = take(b_vec); p.qbuf.gbound = take(b_vec); p.qbuf.fsel = take(b_vec); p.qbuf.fcount = take(256);
        p.qbuf.bytes = off;
    }

    if (hi_route) {
        // 3a) the certified f16 list scan
        // (the tasks hold <= qcap queries, sized for the fp32 kernel's query block: the f16 block is half of it and fits beside the score tile)
        const int ccap = nq <= SQ_NQ ? IVH_CAND_CAP_SMALLQ : IVH_CAND_CAP;
        p.ccap = ccap;
        p.cand_s = (size_t)nq * ccap * sizeof(float);
        p.cand_i = (size_t)nq * ccap * sizeof(int);
        // few tasks (a one-query search has nprobe): several workgroups per list, as many as fill the chip -- but each emits ~k + 8 rows
        // against its own bound, and all of a query's must fit half its buffer
        p.split = (int)std::max<int64_t>(1, std::min<int64_t>(T <= 64 ? 8 : (T <= 128 ? 4 : (T <= 256 ? 2 : 1)), (ccap / 2) / ((int64_t)nprobe * (k + 8))));
        p.scan_grid = T * p.split;
        p.scan_lds = ivf_hi_lds_bytes(qcap, s.dim) + pq_lds;
        p.cap = std::max(k + KNN_CERT_EXTRA, KNN_CERT_CAP);
        p.refine_lds = refine_lds_bytes(p.cap) + (size_t)ccap * 8 + 1024;
    } else {
        // 3b) the fp32 list scan (no f16 plane: dim % 64 != 0, RADAD_IVF_OPT_HI_SCAN 0)
        p.scan_grid = T;
        const size_t lds = knn_sq_lds_f32(qcap, s.dim) + pq_lds;
        p.scan_lds = lds;
        if (!(lds <= 160 * 1024)) { p.status = IVF_PLAN_DIM_TOO_LARGE; return p; }
        p.cap = std::max(k + KNN_CERT_EXTRA, (int)std::min<int64_t>((int64_t)nprobe * ksel, KNN_CERT_CAP));
        p.refine_lds = refine_lds_bytes(p.cap);
    }

    // 4) the queries the route's certificate rejected: exact float64 scan of their probed lists
    const size_t xlds = ivf_exact_lds_bytes(s.dim, k, nprobe);
    p.xlds = xlds;
    if (!(xlds <= 160 * 1024)) { p.status = IVF_PLAN_NPROBE_TOO_LARGE; return p; }
    const int64_t per_q = (int64_t)nprobe * k * 16;
    const int64_t slots = std::min<int64_t>(nq, std::max<int64_t>(1, (int64_t)IVX_PART_BUDGET / per_q));
    p.nslots = slots;
    p.xkey = (size_t)slots * nprobe * k * sizeof(double);
    p.xid = (size_t)slots * nprobe * k * sizeof(int64_t);
    p.xarrive = (size_t)slots * sizeof(int);
    p.xgrid = std::min<int64_t>(slots * nprobe, IVX_MAX_GRID);
    p.xlaunches = ceil_div64(nq, slots);      // (one launch unless the batch's partial lists exceed IVX_PART_BUDGET)
    return p;
}

// ---- range search over the probed lists (radad_ivf_range_search) --------------------------------------------------------------------
// The routes (radad_hip.h: RADAD_IVF_RANGE_HI / RADAD_IVF_RANGE_EXACT; ivf.inc asserts the values)
constexpr int IVF_RANGE_HI = 0, IVF_RANGE_EXACT = 1;
constexpr int IVF_RANGE_CAP = 4096;              // positions of a query's candidate buffer = RG_MAX_CAP, what the re-rank's LDS sort is sized for
constexpr size_t ivf_range_hi_lds_bytes(int qcap, int dim) { return (size_t)qcap * (dim + 8) * 2; }      // the task's f16 queries: no score tile
constexpr size_t ivf_range_refine_lds_bytes() { return (size_t)IVF_RANGE_CAP * 12 + 64; }                // float64 key + id per entry, 4 wave counts
constexpr size_t ivf_range_exact_lds_bytes(int dim, int m, int nprobe) {                                  // query | 8 waves x m (key, id) | 8 lengths | nprobe heads
    return (size_t)dim * 4 + (size_t)IVX_WAVES * m * 16 + (size_t)IVX_WAVES * 4 + (size_t)nprobe * 4;
}

// The plan of radad_ivf_range_search: every member (float64 key < radius) of the nprobe probed lists, the best m <= IVF_MAX_K of them
// listed.  An IvfPlan whose coarse and grouping section (ws_a / ws_b, tasks, qcap, T, group_small) is ivf_plan_search's; k = m and
// ksel = 0 (no per-pair partial lists: part_s = part_i = 0, and the grouping kernels write nothing for a pair without a list).
//   IVF_RANGE_HI    exactly when ivf_plan_search takes hi_route (the plane is there and ivf_hi_lds_bytes <= 160 KB): k_hi_rows, the floors
//                   thr[q] (qbuf_thr), k_ivf_range_hi into buffers of IVF_RANGE_CAP POSITIONS per query (cand_i; no scores: cand_s = 0),
//                   k_ivf_range_refine; a query that emitted more goes to the exact pass.  split comes from the task count alone: no
//                   workgroup has a bound of its own, so the (ccap / 2) / (nprobe (k + 8)) clause of the top-k plan has no meaning here.
//   IVF_RANGE_EXACT k_ivf_range_exact for every query.
// The exact pass keeps nprobe x m x 16 B of partial lists per query, in launches of nslots queries within IVX_PART_BUDGET.
// has_admit / pq_m (radad_ivf_range_search_excl / _excl_pq) mean what they mean to ivf_plan_search, which picks the route with them:
// the tag block of pq_m tags per query counts towards its 160 KB, so IVF_RANGE_HI implies scan_lds = the f16 queries + the tag block
// <= 160 KB.  With both at their defaults the plan is field for field what it was (tests/ivf_range_excl_plan_check.cpp).
static IvfPlan ivf_plan_range(const IvfFacts& s, int64_t nq, int m, int nprobe, bool has_admit = false, int pq_m = 0) {
    // the coarse and grouping section is the top-k plan's own (k plays no part in it; the plan's later, k-dependent fields are not read)
    const IvfPlan b = ivf_plan_search(s, nq, 1, nprobe, has_admit, pq_m);
    IvfPlan p;
    nprobe = b.nprobe;
    const int64_t npairs = b.npairs, T = b.T;
    const int qcap = b.qcap;
    p.nq = nq; p.k = m; p.ksel = 0; p.nprobe = nprobe; p.npairs = npairs;
    p.ws_a = b.ws_a; p.ws_b = b.ws_b;
    p.cmargin = b.cmargin; p.qcap = qcap; p.T = T;
    if (b.status == IVF_PLAN_TOO_MANY_PAIRS) { p.status = IVF_PLAN_TOO_MANY_PAIRS; return p; }
    p.tasks = b.tasks;
    p.group_small = b.group_small; p.group_lds = b.group_lds;

    // the route is the top-k plan's choice, and so is the layout of `qbuf`: a range search has no running bound, so its floors thr[q]
    // stand where gbound does; fcount [8]: [0] queries left to the exact pass, [1] answered by it, [2] the largest cand_cnt
    const bool hi = b.hi_route;
    p.hi_route = hi;
    p.range_route = hi ? IVF_RANGE_HI : IVF_RANGE_EXACT;
    p.qbuf = b.qbuf;
    p.qbuf_thr = b.qbuf.gbound;
    // exclusion: one set for the batch reads the admission bitmap (the top-k plan's, spare word included); one set per query reads no
    // bitmap at all -- a pair is decided against the query's tags once it has passed the floor, so neither a suspect bitmap nor the
    // pre-pass's hash bitset exists (admit_words = pq_bits = pq_bitset = 0), only the tag block behind the f16 queries in LDS
    p.pq_m = b.pq_m;
    p.pq_lds = b.pq_lds;
    if (p.pq_m == 0) { p.admit_words = b.admit_words; p.admit = b.admit; }
    if (hi) {
        p.ccap = IVF_RANGE_CAP;
        p.cand_i = (size_t)nq * IVF_RANGE_CAP * sizeof(int);
        p.split = T <= 64 ? 8 : (T <= 128 ? 4 : (T <= 256 ? 2 : 1));
        p.scan_grid = T * p.split;
        p.scan_lds = ivf_range_hi_lds_bytes(qcap, s.dim) + p.pq_lds;
        p.cap = IVF_RANGE_CAP;
        p.refine_lds = ivf_range_refine_lds_bytes();
    }
    const size_t xlds = ivf_range_exact_lds_bytes(s.dim, m, nprobe);
    p.xlds = xlds;
    if (!(xlds <= 160 * 1024)) { p.status = IVF_PLAN_NPROBE_TOO_LARGE; return p; }
    const int64_t per_q = (int64_t)nprobe * m * 16;
    const int64_t slots = std::min<int64_t>(nq, std::max<int64_t>(1, (int64_t)IVX_PART_BUDGET / per_q));
    p.nslots = slots;
    p.xkey = (size_t)slots * nprobe * m * sizeof(double);
    p.xid = (size_t)slots * nprobe * m * sizeof(int64_t);
    p.xarrive = (size_t)slots * sizeof(int);
    p.xgrid = std::min<int64_t>(slots * nprobe, IVX_MAX_GRID);
    p.xlaunches = ceil_div64(nq, slots);
    return p;
}
