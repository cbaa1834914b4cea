// knn_plan.h -- the host side of a flat search that needs no GPU: which scan runs, with what geometry, lists, buffers and
// workspace layout (the PLAN), and when a handle retunes after the certificate rejected most of a batch (KnnTuning).
//
// Plain C++17: no HIP header, no handle, no stream.  Everything here is integer arithmetic on what a store is (StoreFacts) and what a
// search asks for (nq, k, margin); knn.hip supplies the facts, does the device work and launches what the plan says.
// tests/knn_plan_check.cpp drives this header alone.
#pragma once
#include <algorithm>
#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "../../include/radad_hip.h"
#include "ceil_div.h"

// ---- constants the plan reads (the kernels of knn.hip / knn_hi.inc are written against the same ones) ---------------------------
// fp32 tile kernels (k_knn_f32, k_knn_f32_reg)
constexpr int KT_M = 128;       // store rows per tile (MFMA A rows)
constexpr int KT_N = 128;       // queries per tile (MFMA B columns)
constexpr int KNN_THREADS = 256;
// certified f16 tile scan (knn_hi.inc)
constexpr int KW_M = 256;                          // store rows per tile
constexpr int KW_N = 256;                          // queries per tile
constexpr int KW_WAVES = 8;
constexpr int KW_THREADS = KW_WAVES * 64;
constexpr int KW_SAMPLE_LIST = 16;                 // sample pre-pass: entries per (query, tile): 8 holders x 2
constexpr int KW_SAMPLE_SPLITS = 64;     // one-tile splits of the threshold pre-pass (<= 16384 rows)
// small-batch streaming kernels
constexpr int SQ_THREADS = 256;
constexpr int SQ_NQ = 16;
constexpr int SQ_SLOTS = 16;
constexpr size_t SQ_LDS_BUDGET = 160 * 1024;      // the query block [nq][dim + pad] + slot buffers must fit one CU's LDS
// re-rank (k_merge_refine)
constexpr int KNN_MARGIN = 6;            // spare entries of a (query, chunk) list on the fp32 tile kernels
constexpr int KNN_CERT_EXTRA = 32;       // candidates beyond k the certified re-rank can take before it gives up, at least ...
constexpr int KNN_CERT_CAP = 512;        // ... and this many in all: stores of near-duplicates (the benchmark plants 2048 rows
                                         // within 2e-2 of every query) put hundreds of rows within 2 eps of the k-th
constexpr int KNN_F16_MAX_K = 128;       // largest k the certified f16 scans take; beyond it the fp32 tile kernels filter (certified too)
constexpr int RF_STAGE_MAX = 6144;       // list entries per query that k_merge_refine<true> stages in LDS (48 KB + candidates)
constexpr int RF_STAGE_MAX_SMALLQ = 16384;   // ... for batches of <= 16 queries (128 KB: occupancy does not matter there)
constexpr size_t refine_lds_bytes(int cap) { return (size_t)cap * 20 + 256; }      // candidates + per-wave scratch of k_merge_refine
// exact float64 kernel (k_exact_scan)
constexpr int KX_THREADS = 512;
constexpr int KX_WAVES = KX_THREADS / 64;
constexpr int KX_SLICES = 64;
constexpr size_t KX_LDS_MAX = 160 * 1024;              // LDS of a CU: the group's queries + KX_WAVES sorted lists of k per query
constexpr size_t KX_PART_BUDGET = (size_t)128 << 20;   // workspace of one launch's partial lists (KX_SLICES x k x 12 B per query)

static inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

// what the plan reads of a store and of its handle's options
struct StoreFacts {
    int64_t ntotal = 0;
    int dim = 0, metric = 0, f16 = 0;
    int hi_off = 0;              // 1: no f16 plane (switched off, or its allocation failed)
    int opt_centre = -1, opt_smallq_hi = 1, opt_wide_min_q = SQ_NQ + 1, opt_dense = 1;     // radad_knn_set_option
    int cap_boost = 1;           // KnnTuning::cap_boost
    int opt_range_smallq = 0;    // RADAD_KNN_OPT_RANGE_SMALLQ: range searches of <= 16 queries may stream the plane (knn_range_plan)
};

// ---- the exact kernel's grouping --------------------------------------------------------------------------------------------------
// rejected queries one launch of k_exact_scan takes: as many as KX_PART_BUDGET holds partial lists for, a whole group at least.
// (k = 1024: 170 per launch, 128 MiB -- instead of 64 x 1024 x 12 B = 768 KiB for EVERY query of the batch, 805 MB at nq = 1024;
// k <= 128 with batches of up to 1365 queries: one launch, as before)
static int64_t knn_exact_slots(int64_t nq, int k, int group) {
    const int64_t per_q = (int64_t)KX_SLICES * k * (int64_t)(sizeof(double) + sizeof(int));
    return std::min<int64_t>(nq, std::max<int64_t>(group, (int64_t)(KX_PART_BUDGET / per_q) / group * group));
}

// queries per workgroup of the exact kernel: the group's queries (<= 64 KB) and its KX_WAVES lists of k per query share the LDS
// (the lists shrink it at large k: k = 1024 takes one query per workgroup, 98 KB of lists)
static int knn_exact_group(int dim, int k) {
    return (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(8, (size_t)(64 * 1024) / ((size_t)dim * 4)),
                                                     (KX_LDS_MAX - 16) / ((size_t)dim * 4 + (size_t)KX_WAVES * k * 12)));
}

// LDS of one workgroup of the exact kernel.  Dynamic: the group's fp32 queries and KX_WAVES sorted lists of k (key, id) per query --
// what the kernel indexes and what a launch asks for.  Static: the kernel's arrival flag, 16 bytes with its alignment.  HIP adds
// the two and refuses a launch (and hipFuncSetAttribute) whose sum exceeds the 160 KB of a CU.
static size_t knn_exact_dyn_lds_bytes(int dim, int k) {
    const size_t group = (size_t)knn_exact_group(dim, k);
    return group * (size_t)dim * 4 + (size_t)KX_WAVES * group * (size_t)k * 12;
}
static size_t knn_exact_lds_bytes(int dim, int k) { return knn_exact_dyn_lds_bytes(dim, k) + 16; }
// The width x k limit of every flat search (radad_hip.h, radad_knn_create): one query and its lists must fit the LDS of a CU,
// dim * 4 + 96 k + 16 <= 160 KB -- dim <= 16380 at k = 1024, dim <= 40932 at k = 1.  Any search may need the exact kernel (whether a
// query is rejected is only known on the device), so the entry points refuse (dim, k) beyond it before anything is enqueued.
static bool knn_exact_fits(int dim, int k) { return knn_exact_lds_bytes(dim, k) <= KX_LDS_MAX; }

// ---- launch geometry --------------------------------------------------------------------------------------------------------------
// choose the launch geometry: enough equal splits to put >= 2 workgroups on each of the 256 CUs
static void knn_geometry(int64_t n, int64_t nq, int* n_qtiles, int* n_splits, int64_t* chunk_rows) {
    const int qt = (int)ceil_div64(nq, KT_N);
    const int64_t tiles = ceil_div64(n, KT_M);
    int64_t want = ceil_div64(512, qt);            // splits so that qt*splits ~ 512 workgroups
    want = std::min<int64_t>(want, tiles);
    want = std::max<int64_t>(8, ceil_div64(want, 8) * 8);
    want = std::min<int64_t>(want, 1024);
    const int64_t tiles_per = ceil_div64(tiles, want);
    *n_qtiles = qt;
    *n_splits = (int)want;
    *chunk_rows = tiles_per * KT_M;
}

// wide kernel: 256-query tiles, one workgroup per CU; two rounds of workgroups keep the tail short.  (The list-based scan of
// rounds 1-2 also needed >= 64 chunks so that no 16-entry list was used up; the emit-mode scan has no lists: a sharded batch of
// 32 query tiles now runs 16 chunks of 31 tiles instead of 64 chunks of 8, i.e. a quarter of the per-workgroup start-up cost.)
static void knn_geometry_wide(int64_t n, int64_t nq, int* n_qtiles, int* n_splits, int64_t* chunk_rows) {
    const int qt = (int)ceil_div64(nq, KW_N);
    const int64_t tiles = ceil_div64(n, KW_M);
    int64_t want = ceil_div64(512, qt);
    want = std::min<int64_t>(want, tiles);
    want = std::max<int64_t>(8, ceil_div64(want, 8) * 8);
    want = std::min<int64_t>(want, 1024);
    int64_t tiles_per = ceil_div64(tiles, want);
    // A launch takes (rounds of 256 workgroups) x (tiles per chunk) tile times, and both factors round up.  Round 4 always took
    // ceil(512 / query tiles) chunks ("two rounds keep the tail short"): right for 4 query tiles x 1 M rows (2 x 31 = 1 x 62), wrong
    // where the rounding bites -- BASELINE config 2's 100 k rows = 391 tiles x 4 query tiles: 128 chunks of 4 tiles = 392 workgroups =
    // 2 rounds x 4 = 8 tile times, 64 chunks of 7 = 224 workgroups = ONE round of 7; configs 4 / 5 at full size, 40 query tiles: 16
    // chunks = 640 workgroups = 2.5 -> 3 rounds x 2442 tiles, 32 chunks = 1280 = exactly 5 rounds x 1221 (-17 %).  So: the cheapest by
    // that count among one round's worth of chunks and `want`, `want` + 8, ... 4 x `want`, when it saves 3 % or more.
    if (qt <= 256) {
        auto cost = [&](int64_t per) { return ceil_div64((int64_t)qt * ceil_div64(tiles, per), 256) * per; };
        int64_t best = want, best_per = tiles_per, best_cost = cost(tiles_per);
        auto consider = [&](int64_t splits) {
            splits = std::min<int64_t>(std::max<int64_t>(8, splits / 8 * 8), std::min<int64_t>(1024, std::max<int64_t>(8, ceil_div64(tiles, 8) * 8)));
            const int64_t per = ceil_div64(tiles, splits);
            const int64_t c = cost(per);
            if (c * 100 < best_cost * 97) { best = splits; best_per = per; best_cost = c; }      // (a gain under 3 % is not worth leaving two rounds)
        };
        consider(256 / qt);
        for (int64_t sp = want + 8; sp <= 4 * want; sp += 8) consider(sp);
        want = best; tiles_per = best_per;
    }
    *n_qtiles = qt;
    *n_splits = (int)want;
    *chunk_rows = tiles_per * KW_M;
}

// ---- the plan ---------------------------------------------------------------------------------------------------------------------
// what one search scans with: the kind of scan, its launch layout, its list / buffer sizes and how its queries are prepared
struct ScanPlan {
    int kind = RADAD_SCAN_F32_TILE;  // RADAD_SCAN_*
    int64_t nq = 0;
    int k = 0, l2 = 0;
    int n_qtiles = 0, n_splits = 0;  // workgroups: query tiles x row splits (the streaming kernels: 1 x n_splits)
    int64_t chunk_rows = 0;
    int ksel = 0;                    // list length of the fp32 tile kernels: k + margin
    int ksel_sq = 0;                 // ... of the small-batch kernels
    int s_splits = 0;                // tile scan: tiles of the sample pre-pass
    int emit_cap = 0;                // tile scan: entries of a query's candidate buffer
    int cap = 0;                     // candidates the re-rank can take per query
    int plen = 0, n_parts = 0;       // entries of a partial list / candidate buffer, lists per query
    int sq_rows_per_wave = 0;        // small batches: rows per wave (per workgroup in the K-split form)
    bool sq_ksplit = false;          // small batch over a small store of wide rows: k_knn_hi_smallq_ksplit
    size_t sq_lds = 0;               // small batches: LDS of the streaming kernel
    int dense_plen = 0;
    int xgroup = 1;                  // queries per workgroup of the exact kernel
    int reported_qtiles = 0;         // radad_knn_last_launch: query tiles (the dense kernel's own are not reported) ...
    int block_threads = KNN_THREADS; // ... and threads per workgroup of the scan
    bool hi_q = false;               // f16 queries with a per-query scale (the certified f16 kernels)
    bool biased = false;             // the scale + bias variant of the f16 kernels (RSC 2, 3)
    const float* mu = nullptr;       // centred plane: the queries are centred the same way
    bool f16_queries() const { return kind == RADAD_SCAN_HI_TILE || kind == RADAD_SCAN_HI_SMALLQ || kind == RADAD_SCAN_F16_TILE; }
};

// small batches (<= 16 queries: the online predict() search, pipeline.py:1038-1054, is ONE query of dim 5376 / 3584) stream the
// store; the kernels park only the nq queries handed over in LDS, so any dim goes as long as that block fits beside the slots
// (16 queries of dim 5376 do not: such a batch takes the tile kernels like a large one)
// (slots: float2 x 4 x SQ_NQ x SQ_SLOTS, or the u64 triples of 32-entry lists, + 4 ints per query.  This header knows no device types:
// sizeof(float2), sizeof(u64) and sizeof(_Float16) are the literals 8, 8 and 2 here, and knn.hip static_asserts that they are)
constexpr size_t SQ_SLOT_BYTES = std::max<size_t>((size_t)8 * 4 * SQ_NQ * SQ_SLOTS, (size_t)8 * 3 * SQ_NQ * 32) + sizeof(int) * 4 * SQ_NQ;
static size_t knn_sq_lds_hi(int64_t nq, int dim) { return 2 * (size_t)nq * (dim + 8) + SQ_SLOT_BYTES; }                  // f16 queries
static size_t knn_sq_lds_f32(int64_t nq, int dim) { return sizeof(float) * (size_t)nq * (dim + 4) + SQ_SLOT_BYTES; }

// Whether a search may take the certified f16 TILE scan, and the sample pre-pass it would run.
// the certified f16 scans take k <= KNN_F16_MAX_K: their candidate buffers (emit_cap <= RF_STAGE_MAX) and phase sizes are
// tuned for ~8 (k + margin) admissions per launch.  Larger k is filtered by the fp32 tile kernels (lists of k + margin per
// split), certified the same way.
struct TileEligibility {
    bool eligible = false;
    int s_splits = 0;                // tiles of the sample pre-pass (set whenever the store and the batch qualify at all)
    int n_qtiles = 0;                // query tiles of the tile scan
};
static TileEligibility knn_tile_eligibility(const StoreFacts& s, int64_t nq, int k, int margin) {
    TileEligibility t;
    const int ksel = k + margin;
    const size_t sq_lds_hi = knn_sq_lds_hi(nq, s.dim), sq_lds_f32 = knn_sq_lds_f32(nq, s.dim);
    const bool sq_fits = nq <= SQ_NQ && ksel <= 32 &&
                         ((!s.hi_off && s.dim % 64 == 0 && sq_lds_hi <= SQ_LDS_BUDGET) || (!s.f16 && s.dim % 32 == 0 && sq_lds_f32 <= SQ_LDS_BUDGET));
    const bool f16_k = k <= KNN_F16_MAX_K;
    // the certified tile scan: its candidate buffers are sized from k; the floor's rank k + margin must exist in the sample (16
    // entries per sample tile)
    if (f16_k && (nq >= s.opt_wide_min_q || !sq_fits) && s.ntotal > 0 && s.dim % 64 == 0 && !s.hi_off) {
        int wq, ws; int64_t wc;
        knn_geometry_wide(s.ntotal, nq, &wq, &ws, &wc);
        // the sample pre-pass: one tile per workgroup, at most KW_SAMPLE_SPLITS tiles and 1/8 of the store (whatever the number of
        // query tiles: every phase of the scan is sized from the sample, a small sample means more phases)
        // ... and about 3 % of it: the pre-pass multiplies every query tile with its rows, so on a shard of a row-sharded store -- 1/G of
        // the rows against G times the queries -- a fixed 16 384-row sample was 12 % of the scan's own work at G = 8 (0.16 of 1.7 ms);
        // large enough, though, for the floor's rank to exist twice over (16 entries per sample tile)
        const int64_t tiles = s.ntotal / KW_M;
        int64_t want = (tiles * 3 / 100 + 4) / 8 * 8;
        const int64_t need = ((int64_t)(2 * ksel + KW_SAMPLE_LIST - 1) / KW_SAMPLE_LIST + 7) / 8 * 8;
        want = std::max<int64_t>(std::max<int64_t>(want, need), 8);
        // ... but never fewer tiles than fill ONE round of the chip: the pre-pass is one tile per workgroup, its time is that one
        // tile's latency whether 32 or 256 workgroups run it, and a larger sample is a tighter first floor (BASELINE config 2's
        // 100 k rows took 8 tiles = 2048 rows: every tile of the scan's first layer then admitted ~2 rows per query -- 512 returning
        // atomics per workgroup and tile; with 48 tiles the whole store is one launch behind the sample's floor alone)
        want = std::max<int64_t>(want, std::min<int64_t>(KW_SAMPLE_SPLITS, (256 / std::max(1, std::min(wq, 256))) / 8 * 8));
        t.s_splits = (int)std::min<int64_t>(std::min<int64_t>(KW_SAMPLE_SPLITS, want), tiles / 8 / 8 * 8);
        t.n_qtiles = wq;
        t.eligible = t.s_splits >= 8 && t.s_splits * KW_SAMPLE_LIST >= 2 * ksel;
    }
    return t;
}

// Whether a search that did not take the tile scan (`use_hi`) may stream the f16 plane as a small batch (certified like the tile
// scan): stores the plane is kept for, or fp16 stores.  A search whose tile scan was skipped by the tuning state does not ask again.
static bool knn_smallq_hi_eligible(const StoreFacts& s, int64_t nq, int k, int margin, bool use_hi, bool skipped_hi) {
    const bool smallq_geom = !use_hi && nq <= SQ_NQ && k + margin <= 32 && s.ntotal > 0;
    return smallq_geom && k <= KNN_F16_MAX_K && s.opt_smallq_hi && s.dim % 64 == 0 && s.ntotal >= 16384 && !s.hi_off && !skipped_hi &&
           knn_sq_lds_hi(nq, s.dim) <= SQ_LDS_BUDGET;
}

// The launch geometry of a streaming kernel with one wave per row slice (not the K-split form): rows per wave, workgroups of 4 waves.
// a wave streams >= 128 KB (128 rows at dim 512) so that its lists' hand-over stays small beside the stream, but no more
// rows than leave 8 waves for every CU; the lists of a query (one per workgroup, `list_len` entries each; 0: the kernel keeps no
// lists) should fit the re-rank's staged form
// one full round of resident waves: 1024 SIMDs x `waves_per_simd`, the waves per SIMD the kernel's registers allow.  (Measured: no
// difference against 2048 waves on the 1 M x 512 store -- 0.2075 vs 0.208 ms, 4.93 TB/s either way: the stream is not limited by
// the number of waves in flight.)
struct SqStream {
    int rows_per_wave = 0, n_splits = 0;
};
static SqStream knn_sq_stream_geometry(int64_t ntotal, size_t row_bytes, int waves_per_simd, int list_len) {
    const int64_t waves_wanted = 1024 * waves_per_simd;
    const int64_t rows_min = std::max<int64_t>(16, std::min<int64_t>(128, ceil_div64(ceil_div64(128 * 1024, (int64_t)row_bytes), 16) * 16));
    int64_t rpw = std::max<int64_t>(ceil_div64(ceil_div64(ntotal, waves_wanted), 16) * 16, rows_min);
    while (rpw < 128 && ceil_div64(ceil_div64(ntotal, rpw), 4) * list_len > RF_STAGE_MAX_SMALLQ) rpw += 16;
    SqStream g;
    g.rows_per_wave = (int)rpw;
    g.n_splits = (int)ceil_div64(ceil_div64(ntotal, rpw), 4);
    return g;
}

// The rest of the plan, once it is settled which certified f16 scan (if any) the search takes: `use_hi` the tile scan, `smallq_hi`
// the small-batch stream of the plane.  (ScanPlan::mu / ::biased depend on the plane's centring: the caller fills them in.)
static ScanPlan knn_finish_plan(const StoreFacts& s, int64_t nq, int k, int margin, const TileEligibility& t, bool use_hi, bool smallq_hi) {
    ScanPlan p;
    p.nq = nq; p.k = k; p.l2 = s.metric == RADAD_METRIC_L2 ? 1 : 0;
    p.ksel = k + margin;
    knn_geometry(std::max<int64_t>(s.ntotal, 1), nq, &p.n_qtiles, &p.n_splits, &p.chunk_rows);
    const int ksel = p.ksel;
    p.s_splits = t.s_splits;
    if (use_hi) p.n_qtiles = t.n_qtiles;
    const size_t sq_lds_hi = knn_sq_lds_hi(nq, s.dim), sq_lds_f32 = knn_sq_lds_f32(nq, s.dim);
    const bool smallq_geom = !use_hi && nq <= SQ_NQ && ksel <= 32 && s.ntotal > 0;
    // a small fp32 store (the IVF index's centroids; a database of a few thousand files): every score + select on the staged copy
    p.dense_plen = (int)((std::max<int64_t>(s.ntotal, 1) + 3) / 4 * 4);
    const bool dense = !use_hi && !smallq_hi && !s.f16 && s.opt_dense && s.ntotal >= 1 &&
                       s.ntotal <= (nq <= SQ_NQ ? RF_STAGE_MAX_SMALLQ : RF_STAGE_MAX) && s.dim % 16 == 0 && nq * (int64_t)p.dense_plen <= ((int64_t)1 << 24);
    const bool smallq = smallq_geom && !dense && !smallq_hi && !s.f16 && s.dim % 32 == 0 && sq_lds_f32 <= SQ_LDS_BUDGET;
    // a small store of wide rows (the reference's own: 25 423 x 5376) has too few 16-row steps to occupy the chip with one wave per
    // row slice: the K-split form puts four waves on every step
    p.sq_ksplit = smallq_hi && s.dim >= 1024 && ceil_div64(s.ntotal, 16) < 4096;
    // (its lists are 16 entries for k <= 16 -- the reference's k = 15 included -- instead of k + 6 <= 32: half the list registers,
    // twice the waves per SIMD to hide the HBM latency behind.  A workgroup whose 16-entry list is used up by rows within the
    // threshold rejects the query; the exact kernel over so small a store costs ~0.3 ms)
    // (the same 16-entry lists on every f16 small-batch scan since round 4: k_knn_hi_smallq<32> streams the 1 M x 512 store in 0.40 ms,
    // <16> in 0.20 -- 155 VGPRs against the 32-entry lists' panel of half the loads in flight)
    p.ksel_sq = (smallq_hi && k <= 16) ? 16 : ksel;
    if (p.sq_ksplit) {
        int64_t rpg = 16;
        while (ceil_div64(s.ntotal, rpg) * p.ksel_sq > RF_STAGE_MAX_SMALLQ) rpg += 16;
        p.sq_rows_per_wave = (int)rpg;                // (rows per WORKGROUP in this form)
        p.n_splits = (int)ceil_div64(s.ntotal, rpg);
        p.n_qtiles = 1;
    } else if (smallq || smallq_hi) {
        // (waves per SIMD the kernel's registers allow: k_knn_hi_smallq<16>: 155 VGPRs = 3; the 32-entry and fp32 variants: 2)
        const SqStream g = knn_sq_stream_geometry(s.ntotal, smallq_hi ? (size_t)s.dim * 2 : (size_t)s.dim * 4,
                                                  (smallq_hi && p.ksel_sq <= 16) ? 3 : 2, p.ksel_sq);
        p.sq_rows_per_wave = g.rows_per_wave;
        p.n_splits = g.n_splits;                                                 // workgroups of 4 waves = lists per query
        p.n_qtiles = 1;
    }
    p.sq_lds = smallq_hi ? sq_lds_hi : sq_lds_f32;
    const bool f16_tile = !use_hi && !smallq_hi && s.f16 && ksel <= 32 && s.dim % 64 == 0;
    p.kind = use_hi ? RADAD_SCAN_HI_TILE : dense ? RADAD_SCAN_F32_DENSE : smallq_hi ? RADAD_SCAN_HI_SMALLQ : smallq ? RADAD_SCAN_F32_SMALLQ
           : f16_tile ? RADAD_SCAN_F16_TILE : RADAD_SCAN_F32_TILE;
    p.emit_cap = use_hi ? std::min(RF_STAGE_MAX, std::max(1024 * s.cap_boost, 32 * ksel)) : 0;
    p.reported_qtiles = p.n_qtiles;                    // (the dense kernel's own query tiles are not reported)
    if (dense) { p.n_qtiles = (int)ceil_div64(nq, 16); p.n_splits = 1; }
    p.block_threads = use_hi ? KW_THREADS : ((smallq || smallq_hi || dense) ? SQ_THREADS : KNN_THREADS);
    p.plen = use_hi ? p.emit_cap : dense ? p.dense_plen : p.ksel_sq;   // entries of a partial list / of the candidate buffer
    p.n_parts = (use_hi || dense) ? 1 : p.n_splits;
    // (dense: eps of exact fp32 products is ~1e-6 of |q||y| -- hardly a row beyond the k best is within 2 eps; k + 32 candidates keep
    // the re-rank's workgroup at 34 KB of LDS for 4096 staged scores, four per CU instead of three: the IVF coarse step's 1024
    // workgroups in one round.  More near-ties than that reject the query: exact kernel.)
    // (a handle that has widened its candidate buffers -- cap_boost: a store whose rows crowd within 2 eps of the k-th best -- also
    // re-ranks four times as many: the fp32 funnel in front of the float64 re-score takes them at ~2 KB of row reads each)
    p.cap = dense ? k + KNN_CERT_EXTRA : std::max(k + KNN_CERT_EXTRA, KNN_CERT_CAP * (use_hi ? s.cap_boost : 1));
    p.xgroup = knn_exact_group(s.dim, k);
    p.hi_q = use_hi || smallq_hi;
    return p;
}

// ---- the certified f16 tile scan's launches ---------------------------------------------------------------------------------------
// `one_go`: the sample's floor alone filters the store to a third of the buffer (~(k + margin) N / sample rows): one launch
static bool knn_hi_one_go(const ScanPlan& p, int64_t ntotal) { return (int64_t)p.ksel * ntotal <= (int64_t)(p.emit_cap / 3) * p.s_splits * KW_M; }
// rows between the sample pre-pass's tiles: every (tiles / s_splits)-th tile of the store
static int64_t knn_hi_sample_stride(int64_t ntotal, int s_splits) { return std::max<int64_t>(1, (ntotal / KW_M) / s_splits) * KW_M; }
// query tiles of a launch's grid: more than 8 run as whole groups of 8 (see the kernel)
static int knn_hi_qtile_grid(int n_qtiles) { return n_qtiles <= 8 ? n_qtiles : (n_qtiles + 7) / 8 * 8; }

// The phases of the scan, as row boundaries 0 = r[0] < r[1] < ... = n: a floor taken from m rows admits ~(rank / m) of what it is
// applied to, so every launch covers at most 8 x the rows its floor was taken from -- the first 8 x the sample (phase0 rows) with the
// sample's floor, the next 8 x that with the floor the candidates so far give (k_kth_floor), and so on: 2 launches up to 1.2 M rows,
// 3 up to 9.5 M.  Each admits ~8 (k + margin) rows per query; the candidate buffer holds 32 (k + margin) (>= 1024): more (stores of
// near-duplicates) rejects the query.  (One launch with the floors raised inside it was measured slower and removed: DESIGN §4.1.)
static std::vector<int64_t> knn_hi_phases(int64_t n, int64_t nq, int64_t phase0, bool one_go) {
    std::vector<int64_t> r{0};
    for (int64_t r0 = 0, span = phase0; r0 < n; span *= 8) {
        // (a last phase of less than a quarter of its predecessor is not worth a launch of its own: it joins it.  The quarter is taken
        // HERE, before the balancing below: that may then move up to a quarter of this phase's tiles out of the last one, which can
        // end up shorter)
        int64_t r1 = std::min<int64_t>(n, r0 + span);
        if (n - r1 < span / 4) r1 = n;
        if (r0 == 0 && one_go) r1 = n;
        // A launch deals whole tiles to its row splits, ceil(tiles / splits) each: what decides its time is that quotient, and a
        // remainder of a few tiles costs a whole extra tile per workgroup (64 + 260 tiles over 128 splits = 1 + 3 tile times, the last
        // round of the second launch nearly empty; 68 + 256 tiles = 1 + 2).  When the LAST launch follows this one, up to a quarter
        // more tiles move into this one if that lowers the sum of the two quotients.  (BASELINE config 2 -- 100 k rows = 64 + 327
        // tiles -- gains nothing from it: 1 + 3 either way; its scan stays at 0.27 of the MFMA peak, 1 564 tile tasks over 256 CUs.)
        if (r1 < n && (n - r1 <= span * 8 || n - r1 - span * 8 < span * 2)) {
            auto tile_time = [&](int64_t rows) {
                int gq, gs; int64_t gc;
                knn_geometry_wide(rows, nq, &gq, &gs, &gc);
                return gc / KW_M;
            };
            const int64_t t_this = ceil_div64(r1 - r0, KW_M), t_rest = ceil_div64(n - r1, KW_M);
            int64_t best = tile_time(r1 - r0) + tile_time(n - r1), best_s = 0;
            for (int64_t sft = 1; sft <= std::min<int64_t>(t_this / 4, t_rest - 1); ++sft) {
                const int64_t c = tile_time(r1 - r0 + sft * KW_M) + tile_time(n - r1 - sft * KW_M);
                if (c < best) { best = c; best_s = sft; }
            }
            r1 += best_s * KW_M;
        }
        r.push_back(r1);
        r0 = r1;
    }
    return r;
}

// ---- early abandon of scan tiles (knn_hi.inc, ABANDON) ----------------------------------------------------------------------------
// After `c` of a tile's K stages (64 elements each) the rest of every dot product is at most |qh[64c:]| |yh[64c:]| (Cauchy-Schwarz):
// a tile none of whose 256 x 256 partial scores can still reach its query's admission floor is left there.  The checkpoint c per
// row width, 0 = the scan never tests: an eighth of the stages, at least one, and none on rows of a single stage.  An early
// checkpoint saves more of a skipped tile and succeeds less often: with flat energy the suffix norms have shrunk to
// (1 - c / stages) of |q||y|, so the test can succeed only against floors above that -- 0.875 |q||y| at an eighth.
// (dim 512: c = 1 of 8.  Measured against c = 2 on the benchmark, three alternations on one box: 1.197-1.201 against 1.242-1.246 ms
// per step, the skipped fraction 0.488 either way: profiles/abandon_ab.txt.)
static int knn_abandon_checkpoint(int dim) {
    if (dim < 128 || dim % 64 != 0) return 0;
    return std::max(1, dim / 64 / 8);
}
// first element of the suffix whose norms the store keeps per row tile and a search keeps per query
static int knn_abandon_suffix_from(int dim) { return 64 * knn_abandon_checkpoint(dim); }

// What one launch of the tile scan needs to take the ABANDON instantiation; everything else launches the parent's kernel.
struct AbandonFacts {
    int opt_abandon = 1;         // RADAD_KNN_OPT_ABANDON
    int rsc = 0;                 // the launch's RSC (knn_hi.inc): one scale for all rows (0, 3) is covered, per-row scales (1, 2) are not
    bool sample = false;         // the threshold pre-pass: it has no floor to test against
    int ksplit = 1;              // K split over two workgroups: neither holds a whole partial score
    bool floors = false;         // the launch admits from per-query floors (thr_init)
    bool per_call_bias = false;  // radad_knn_search_excl_scan's bias array (NaN rows): not covered
    bool terms_current = false;  // the store's per-tile suffix norms cover every row and were taken at this dim's checkpoint
    int dim = 0;
};
// -> the checkpoint the launch runs with, 0 = the plain instantiation
static int knn_abandon_launch(const AbandonFacts& f) {
    if (!f.opt_abandon || f.sample || f.ksplit != 1 || !f.floors || f.per_call_bias || !f.terms_current) return 0;
    if (f.rsc != 0 && f.rsc != 3) return 0;
    return knn_abandon_checkpoint(f.dim);
}

// The abandon's per-query terms live in a small buffer of the handle's own beside the search workspace (SearchLayout and its byte
// counts stay what every other scan was planned and pinned with): rq [nq] suffix norms | slack [nq] accumulation slack.
struct AbandonLayout {
    size_t rq = 0, slack = 0, bytes = 0;
};
static AbandonLayout knn_abandon_layout(int64_t nq) {
    AbandonLayout L;
    const size_t b_vec = al256((size_t)nq * sizeof(float));
    L.rq = 0; L.slack = b_vec; L.bytes = 2 * b_vec;
    return L;
}
// the store's per-tile terms (largest suffix norm, largest accumulator start): two floats per aligned KW_M-row tile of the capacity
static int64_t knn_abandon_tiles(int64_t rows) { return ceil_div64(rows, KW_M); }
// ints of the search's counter block (SearchLayout::fcount, 64 ints: flag_count + 6 statistics first) the abandon counts in
constexpr int KNN_AB_COUNTER0 = 8;       // [8] tile tasks tested, [9] tile tasks abandoned

// ---- the abandoning scan's tiles, dealt by ticket (knn_hi.inc, k_knn_hi_abandon_deal) ---------------------------------------------
// A static chunk of an abandoning launch holds as many tiles that cannot be skipped as the store happens to put there, and the launch
// ends with its slowest workgroup.  The scan keeps no per-chunk state (candidates go to per-query buffers by atomics, the re-rank does
// not depend on their order), so which workgroup multiplies a tile is free: in a DEALT launch a workgroup keeps its query tile and its
// XCD slot (bid & 7: knn_hi_task) and draws GRANULES of `granule` consecutive row tiles from a counter of its (slot, query tile) until
// the slot's share is used up.  The launch's granules go to the eight slots round-robin -- granule g belongs to slot g % 8, ticket t of
// slot s is granule 8 t + s -- so a store filled cluster by cluster spreads over all slots, and the query tiles of a slot walk the
// same sequence of row tiles (they share them through the XCD's L2, as the static chunks did).  Nothing depends on which physical
// XCD a workgroup runs on: the slot is a number, the counter is device-wide.
// The grid stays the one knn_geometry_wide gives: a launch whose gate is closed for a query tile (knn_hi.inc) runs that query tile's
// static chunks exactly as before, and of an open one the workgroups beyond the resident ones find their counter used up.
constexpr int KNN_DEAL_SLOTS = 8;            // XCD slots: bid & 7
constexpr int KNN_DEAL_MAX_QTILES = 8;       // the first branch of knn_hi_task
constexpr int KNN_DEAL_SETS = 4;             // counter sets of a search, one per launch (the phases of <= 9.5 M rows are three)
constexpr int KNN_DEAL_COUNTERS = KNN_DEAL_SETS * KNN_DEAL_SLOTS * KNN_DEAL_MAX_QTILES;      // ints the query preparation zeroes
#ifndef KNN_DEAL_GRANULE
#define KNN_DEAL_GRANULE 4                   // (measured against 1 and 2: profiles/abandon_deal_ab.txt; 8 granules within 40 tiles)
#endif
constexpr int knn_deal_counter(int set, int slot, int qt) { return (set * KNN_DEAL_SLOTS + slot) * KNN_DEAL_MAX_QTILES + qt; }

// ticket -> row tiles [tile0, tile0 + tiles) of the launch; tiles == 0: the slot's share is used up (every later ticket too).
// Host and device read this same text (constexpr: callable from both sides).  granule: a power of two.
struct DealRange {
    int tile0 = 0, tiles = 0;
};
constexpr int64_t knn_deal_granules(int64_t row_tiles, int granule) { return (row_tiles + granule - 1) / granule; }
constexpr DealRange knn_deal_ticket(int slot, int64_t ticket, int64_t row_tiles, int granule) {
    DealRange r;
    const int64_t first = (ticket * KNN_DEAL_SLOTS + slot) * granule;      // (no division: the kernel runs this once per granule)
    if (ticket < 0 || first >= row_tiles) return r;
    r.tile0 = (int)first;
    r.tiles = (int)(row_tiles - first < granule ? row_tiles - first : granule);
    return r;
}

// Whether a launch is dealt.  Only where it can help: the launch takes the ABANDON instantiation (ab_ck > 0: knn_abandon_launch), its
// query tiles are at most 8 (knn_hi_task's first branch: one stream of row tiles per (slot, query tile)), it is one of the search's
// first KNN_DEAL_SETS launches, and a resident workgroup -- one per CU, the CUs shared out over 8 slots x the query tiles, no more than
// the grid has -- would draw at least two granules of the smallest slot's share; the granule halves until that holds.  Everything else
// launches exactly what it launched before: the 20 000-row stores of the tests, K-split launches and the sample pre-pass (ab_ck 0),
// sharded batches of more than 8 query tiles.
struct DealFacts {
    int opt_deal = 1;            // RADAD_KNN_OPT_ABANDON_DEAL
    int ab_ck = 0;               // knn_abandon_launch of this launch
    int launch = 0;              // the launch's number in its search
    int64_t row_tiles = 0;       // KW_M-row tiles of the launch
    int n_qtiles = 0, n_splits = 0;      // knn_geometry_wide of the launch: the grid is n_qtiles x n_splits workgroups
    int cus = 0;                 // compute units of the device
};
struct DealPlan {
    bool dealt = false;
    int workgroups = 0;          // the launch's grid (unchanged)
    int resident = 0;            // workgroups of one (slot, query tile) that run at once and draw
    int granule = 0;
};
static DealPlan knn_abandon_deal(const DealFacts& f) {
    DealPlan d;
    if (!f.opt_deal || f.ab_ck <= 0 || f.launch < 0 || f.launch >= KNN_DEAL_SETS || f.row_tiles <= 0 || f.cus <= 0) return d;
    if (f.n_qtiles < 1 || f.n_qtiles > KNN_DEAL_MAX_QTILES || f.n_splits < KNN_DEAL_SLOTS || f.n_splits % KNN_DEAL_SLOTS != 0) return d;
    const int resident = std::min(f.n_splits / KNN_DEAL_SLOTS, std::max(1, f.cus / (KNN_DEAL_SLOTS * f.n_qtiles)));
    for (int g = KNN_DEAL_GRANULE; g >= 1; g /= 2) {
        if (knn_deal_granules(f.row_tiles, g) / KNN_DEAL_SLOTS >= 2 * (int64_t)resident) {
            d.dealt = true; d.workgroups = f.n_qtiles * f.n_splits; d.resident = resident; d.granule = g;
            return d;
        }
    }
    return d;
}

// ---- a vetoed tile's few live rows, deferred to a dense tail (knn_hi.inc, k_knn_hi_abandon_defer / k_knn_hi_tail) --------------------
// A tile task one wave vetoes is usually kept alive by a handful of its 256 rows.  In a DEFERRING launch the vetoing waves also find
// WHICH rows fail the abandon's inequality; a tile with 1 ... KNN_DEFER_MAX_ROWS of them appends those rows (launch-relative numbers)
// to the list of its QUERY TILE and is left exactly as a skipped tile is.  Behind the launch, on the same stream and in front of
// everything that reads the candidate buffers, the tail kernel scores each list's rows in full against that query tile alone, with the
// launch's floors and the scan's own stage loop and emit: a pair's accumulator does not depend on where its row sits in a tile, so the
// candidates are the parent's.  The tail fetches the listed rows straight from the plane by per-lane 32-bit offsets (no copy, no
// compact buffer of `capacity` rows), which is why a launch must address its rows in 32 bits.
constexpr int KNN_DEFER_MAX_ROWS = 16;       // live rows a deferred tile task may list
constexpr int KNN_DEFER_MAX_QTILES = 8;      // the first branch of knn_hi_task: one list per query tile
// A launch is dealt or defers, never both, and the query preparation zeroes every launch's set of deal counters anyway: a deferring
// launch counts in ITS set -- the entries of query tile qt's list where slot 0's ticket counters would be, the tile tasks deferred in
// slot 1's first.
constexpr int KNN_DEFER_SETS = KNN_DEAL_SETS;
static_assert(KNN_DEFER_MAX_QTILES <= KNN_DEAL_MAX_QTILES && KNN_DEAL_SLOTS >= 2, "the deferral counts inside a deal counter set");
constexpr int knn_defer_counter(int set, int qt) { return knn_deal_counter(set, 0, qt); }
constexpr int knn_defer_tasks_counter(int set) { return knn_deal_counter(set, 1, 0); }
constexpr int64_t KNN_DEFER_MAX_BYTES = ((int64_t)1 << 32) - ((int64_t)1 << 16);     // plane bytes of a launch the tail's offsets reach

struct DeferFacts {
    int opt_defer = 1;           // RADAD_KNN_OPT_ABANDON_DEFER
    int ab_ck = 0;               // knn_abandon_launch of this launch (0: the sample, a K split, a per-call bias, the abandon off ...)
    bool dealt = false;          // knn_abandon_deal of this launch
    int launch = 0;              // the launch's number in its search
    int64_t rows = 0;            // rows of the launch
    int row_bytes = 0;
    int n_qtiles = 0;            // knn_geometry_wide of the launch
    int cus = 0;                 // compute units of the device
};
struct DeferPlan {
    bool defer = false;
    int64_t list_cap = 0;        // entries of one query tile's list: it cannot overflow
    int tail_tiles = 0;          // KW_M-row tiles of a full list
    int tail_splits = 0;         // the tail's grid is n_qtiles x tail_splits workgroups (a multiple of 8: knn_hi_task) ...
    int tail_rounds = 0;         // ... and workgroup `split` takes tiles split, split + tail_splits, ...: at most this many
};
// entries of one query tile's list for a store of `rows` rows: every tile task lists at most KNN_DEFER_MAX_ROWS
static int64_t knn_defer_list_cap(int64_t rows) { return ceil_div64(rows, KW_M) * KNN_DEFER_MAX_ROWS; }
static DeferPlan knn_abandon_defer(const DeferFacts& f) {
    DeferPlan d;
    if (!f.opt_defer || f.ab_ck <= 0 || f.dealt || f.launch < 0 || f.launch >= KNN_DEFER_SETS || f.rows <= 0 || f.cus <= 0) return d;
    if (f.n_qtiles < 1 || f.n_qtiles > KNN_DEFER_MAX_QTILES) return d;
    if (f.row_bytes <= 0 || f.rows * f.row_bytes > KNN_DEFER_MAX_BYTES) return d;
    d.defer = true;
    d.list_cap = knn_defer_list_cap(f.rows);
    d.tail_tiles = (int)ceil_div64(d.list_cap, KW_M);
    // about one workgroup per CU over all query tiles, in eights, and no more than a full list has tiles
    const int per_qt = std::max(8, f.cus / f.n_qtiles / 8 * 8);
    d.tail_splits = std::min(per_qt, (d.tail_tiles + 7) / 8 * 8);
    d.tail_rounds = (d.tail_tiles + d.tail_splits - 1) / d.tail_splits;
    return d;
}

// ---- the row tail: short lists scored in 16-row groups on every CU (knn_hi.inc, k_knn_hi_rowtail) ------------------------------------
// Behind a deferring launch BOTH tails are launched; each reads its query tile's count and leaves unless the list is on its side of
// KNN_ROWTAIL_MAX_ENTRIES (device-side: the host never sees a count).  The row tail's unit is a GROUP of KNN_ROWTAIL_GROUP consecutive
// entries of one query tile's list against that query tile; its grid is n_qtiles x n_splits workgroups of KNN_ROWTAIL_THREADS, workgroup
// `split` walks groups split, split + n_splits, ... until the list ends (knn_rowtail_span: the text kernel and host check both read).
constexpr int KNN_ROWTAIL_GROUP = 16;        // one MFMA's rows
constexpr int KNN_ROWTAIL_THREADS = 256;     // 4 waves x 64 queries
constexpr int KNN_ROWTAIL_WG_PER_CU = 2;     // workgroups per CU the grid is cut for (4 fit: the kernel leaves room for 4 waves per SIMD; the
                                             // benchmark's lists are one round either way, and half the workgroups of an empty tail leave sooner)
// A list of more entries than this goes to the tile tail: every group re-reads its query tile from L2, a 256-row tile reads it once.
// Measured at 1 M x 512, 4 query tiles, one launch (tools/bench_row_tail.py; profiles/row_tail_ab.txt, section 3): with 2960 entries a
// query tile the row tail is 0.016 ms faster than the tile tail, with 8720 it is 0.052 ms slower, with 62 496 0.50 ms slower; the
// two lines cross at about 4300 entries.
constexpr int KNN_ROWTAIL_MAX_ENTRIES = 4096;
constexpr bool knn_rowtail_takes(int count) { return count <= KNN_ROWTAIL_MAX_ENTRIES; }
struct RowTailSpan { int first, n; };        // entries [first, first + n) of the list; n == 0: the workgroup is done
constexpr RowTailSpan knn_rowtail_span(int split, int round, int n_splits, int count) {
    const long long first = ((long long)round * n_splits + split) * KNN_ROWTAIL_GROUP;
    if (first >= count) return RowTailSpan{0, 0};
    return RowTailSpan{(int)first, count - first < KNN_ROWTAIL_GROUP ? (int)(count - first) : KNN_ROWTAIL_GROUP};
}
struct RowTailPlan {
    int groups = 0;              // groups of a full list
    int n_splits = 0;            // workgroups per query tile (a multiple of 8: knn_hi_task)
    int rounds = 0;              // groups a workgroup takes at most
};
// KNN_ROWTAIL_WG_PER_CU workgroups per CU over all query tiles, in eights, and no more than a full list has groups
static RowTailPlan knn_defer_rowtail(int64_t list_cap, int n_qtiles, int cus) {
    RowTailPlan r;
    if (list_cap <= 0 || n_qtiles < 1 || cus <= 0) return r;
    r.groups = (int)ceil_div64(list_cap, KNN_ROWTAIL_GROUP);
    const int per_qt = std::max(8, KNN_ROWTAIL_WG_PER_CU * cus / n_qtiles / 8 * 8);
    r.n_splits = std::min(per_qt, (r.groups + 7) / 8 * 8);
    r.rounds = (r.groups + r.n_splits - 1) / r.n_splits;
    return r;
}

// ---- the next tile's head, fetched at the abandon checkpoint (knn_hi.inc, ahead_on) ------------------------------------------------
// A tile that leaves at its checkpoint (skipped or deferred) has no use for its own next stage.  With RADAD_KNN_OPT_ABANDON_AHEAD the
// checkpoint stage of a TESTED tile that has a next tile and is predicted to leave fetches the next tile's stage 0 instead.  The
// prediction is one scalar per workgroup; kernel and host model read this same text (constexpr: callable from both sides).
//   initial state: "leaves" -- the workgroup's gate is open, which is already evidence;
//   after a tested tile: what that tile did.  An untested tile (its own gate shut) neither consults nor updates it.
constexpr bool knn_ahead_initial() { return true; }
constexpr bool knn_ahead_next(bool /*pred*/, bool left) { return left; }
constexpr bool knn_ahead_speculate(bool pred, bool has_next) { return pred && has_next; }
// The walk of one workgroup's tiles, as the kernel makes it: what happens at each tile (host only; tests/knn_abandon_ahead_check.cpp
// and the GPU test's expectations).
enum AheadOutcome { KNN_AHEAD_UNTESTED = 0, KNN_AHEAD_LEAVE = 1, KNN_AHEAD_STAY = 2 };
struct AheadCounts {
    int64_t used = 0;            // tile tasks that left into a head already fetched: one barrier
    int64_t wasted = 0;          // tile tasks that stayed and threw a fetched head away: one barrier more than without the option
    int64_t bubbles = 0;         // barriers that wait for a DMA nothing overlaps: a leaving tile that did not speculate and has a next
                                 // tile, and every wasted head
};
static AheadCounts knn_ahead_walk(const int* outcome, int tiles, bool ahead_on) {
    AheadCounts c;
    bool pred = knn_ahead_initial();
    for (int t = 0; t < tiles; ++t) {
        if (outcome[t] == KNN_AHEAD_UNTESTED) continue;
        const bool has_next = t + 1 < tiles;
        const bool spec = ahead_on && knn_ahead_speculate(pred, has_next);
        const bool left = outcome[t] == KNN_AHEAD_LEAVE;
        if (left) { if (spec) ++c.used; else if (has_next) ++c.bubbles; }
        else if (spec) { ++c.wasted; ++c.bubbles; }
        pred = knn_ahead_next(pred, left);
    }
    return c;
}
// the two counters of a launch live in its own set of the deal counters (zeroed with them): slot 2's first two ints.  A launch that
// prefetches heads is never dealt, and a deferring launch counts in slots 0 and 1 (knn_defer_counter).
static_assert(KNN_DEAL_SLOTS >= 3 && KNN_DEAL_MAX_QTILES >= 2, "the head prefetch counts inside a deal counter set");
constexpr int knn_ahead_counter(int set) { return knn_deal_counter(set, 2, 0); }
// Whether a launch prefetches heads: an abandoning launch that is not dealt, one of the search's first KNN_DEAL_SETS (its counters).
static bool knn_abandon_ahead(int opt_ahead, int ab_ck, bool dealt, int launch) {
    return opt_ahead != 0 && ab_ck > 0 && !dealt && launch >= 0 && launch < KNN_DEAL_SETS;
}

// ---- workspace layouts ------------------------------------------------------------------------------------------------------------
// byte offsets of a search's buffers in the handle's workspace (knn_search_layout)
struct SearchLayout {
    size_t qf = 0, qn = 0, qh = 0, qscale = 0, qconst = 0, eps = 0, thr = 0, ak = 0, cnt = 0, fcount = 0, fsel = 0, ps = 0, pi = 0, xk = 0, xi = 0;
    size_t cand_elems = 0;     // entries of the candidate buffers / partial lists in ps, pi: the sample pre-pass's lists follow them
    size_t bytes = 0;
};

// The search's workspace: qf (decoded bf16) | qn (normalised) | qh (f16 queries) | qscale | qconst | eps | thr_init | a_k | cand_cnt |
// flag_count + statistics | flag_sel | part_score | part_idx | exact partial keys | ids.  Byte offsets into the handle's workspace.
static SearchLayout knn_search_layout(const StoreFacts& s, const ScanPlan& p, int q_dtype) {
    const int64_t nq = p.nq;
    const size_t qrow_f32 = al256((size_t)nq * s.dim * sizeof(float));
    const size_t b_vec = al256((size_t)nq * sizeof(float));
    SearchLayout L;
    // (the sample pre-pass's lists live BEHIND the candidate buffers, not in them: k_floor_from_sample writes a query's floor while
    // other queries' sample lists are still being read)
    L.cand_elems = (size_t)nq * (size_t)p.n_parts * p.plen;
    const size_t part_elems = L.cand_elems + (p.kind == RADAD_SCAN_HI_TILE ? (size_t)nq * KW_SAMPLE_SPLITS * KW_SAMPLE_LIST : 0);
    const size_t b_part = al256(part_elems * sizeof(float));
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += bytes; return o; };
    L.qf = take(q_dtype == RADAD_Q_BF16 ? qrow_f32 : 0);
    L.qn = take(s.metric == RADAD_METRIC_COSINE ? qrow_f32 : 0);
    L.qh = take(p.f16_queries() ? al256((size_t)nq * s.dim * 2) : 0);
    L.qscale = take(b_vec);
    L.qconst = take(b_vec);
    L.eps = take(b_vec);
    L.thr = take(b_vec);
    L.ak = take(b_vec);            // a_k of the candidates (two-half searches: k_kth_floor -> k_merge_refine)
    L.cnt = take(b_vec);           // cand_cnt [nq] int (zeroed by k_hi_rows with the counters)
    L.fcount = take(256);          // flag_count + statistics
    L.fsel = take(b_vec);
    L.ps = take(b_part);
    L.pi = take(b_part);
    const int64_t xslots = knn_exact_slots(nq, p.k, p.xgroup);
    L.xk = take(al256((size_t)xslots * KX_SLICES * p.k * sizeof(double)));
    L.xi = take(al256((size_t)xslots * KX_SLICES * p.k * sizeof(int)));
    L.bytes = off;
    return L;
}

// byte offsets in the handle's exclusion workspace
struct ExclLayout {
    size_t fd = 0, fi = 0, fk = 0;          // the fast pass's k_fetch lists (dist, id, key)
    size_t count = 0, sel = 0;              // listed-query counter, listed queries
    size_t admit = 0, xk = 0, xi = 0;       // admission bitmap, the filtered exact pass's partial lists
    size_t bd = 0, bi = 0, bk = 0, own = 0; // begun form only: the shard's lists as _begin left them, and its own short-list flags
    size_t bytes = 0;
    int kf = 0, whole = 0, xgroup = 1;
    int64_t xslots = 0, n_words = 0;
};

// per_query (radad_knn_search_excl_pq): n_excl is the tags per query, m; the exact pass of that rule reads no bitmap
static ExclLayout knn_excl_layout(const StoreFacts& s, int64_t nq, int k, int k_fetch, int64_t n_excl, bool begun, bool per_query = false) {
    ExclLayout L;
    L.kf = (int)std::min<int64_t>(k_fetch, s.ntotal);
    L.whole = k_fetch > s.ntotal ? 1 : 0;          // the list was cut to the store: it is all there is (an unfilled slot, had it not been cut)
    L.xgroup = knn_exact_group(s.dim, k);
    L.xslots = knn_exact_slots(nq, k, L.xgroup);
    L.n_words = ceil_div64(s.ntotal, 64);
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += al256(bytes); return o; };
    L.fd = take((size_t)nq * L.kf * sizeof(float)); L.fi = take((size_t)nq * L.kf * sizeof(int64_t));
    L.fk = take((size_t)nq * L.kf * sizeof(double));
    L.count = take(256); L.sel = take((size_t)nq * sizeof(int));
    L.admit = take(n_excl > 0 && !per_query ? (size_t)L.n_words * sizeof(unsigned long long) : 0);
    L.xk = take(n_excl > 0 ? (size_t)L.xslots * KX_SLICES * k * sizeof(double) : 0);
    L.xi = take(n_excl > 0 ? (size_t)L.xslots * KX_SLICES * k * sizeof(int) : 0);
    if (begun) {
        L.bd = take((size_t)nq * k * sizeof(float)); L.bi = take((size_t)nq * k * sizeof(int64_t));
        L.bk = take((size_t)nq * k * sizeof(double)); L.own = take((size_t)nq * sizeof(int));
    }
    L.bytes = off;
    return L;
}

// ---- exclusion inside the certified tile scan (radad_knn_search_excl_scan) --------------------------------------------------------
// Which route a batch takes: the tile scan with the per-call bias array exactly when the plain search of this batch would take
// RADAD_SCAN_HI_TILE -- knn_tile_eligibility at the user searches' margin, and the tuning state not on its fp32 fallback
// (`fp32_searches_left`, KnnTuning::hi_skip: read, never counted down here) -- else the row-filtered float64 exact pass for every
// query.  (A plane that cannot be allocated sends the batch to the exact route as well: knn.hip.)
static int knn_excl_scan_route(const StoreFacts& s, int64_t nq, int k, int fp32_searches_left) {
    return (fp32_searches_left == 0 && knn_tile_eligibility(s, nq, k, KNN_MARGIN).eligible) ? RADAD_EXCL_SCAN_TILE : RADAD_EXCL_SCAN_EXACT;
}

// byte offsets in the handle's exclusion workspace: the admission bitmap (one bit per row), and on the tile route the per-call bias
// array (one float per row: the plane's bias or 0 where the row is admitted, NaN where it is not)
struct ExclScanLayout {
    size_t admit = 0, bias = 0, bytes = 0;
    int64_t n_words = 0;
};
static ExclScanLayout knn_excl_scan_layout(const StoreFacts& s, int route) {
    ExclScanLayout L;
    L.n_words = ceil_div64(s.ntotal, 64);
    L.admit = 0;
    L.bias = al256((size_t)L.n_words * sizeof(unsigned long long));
    L.bytes = L.bias + (route == RADAD_EXCL_SCAN_TILE ? al256((size_t)s.ntotal * sizeof(float)) : 0);
    return L;
}

// ---- per-query exclusion sets on the certified tile scan (radad_knn_search_excl_scan_pq) ------------------------------------------
// The routes are knn_excl_scan_route's.  The tile route runs the PLAIN plan -- no per-call bias, the plain search's RSC -- from a copy
// of the store's facts with the candidate buffers widened (cap_boost 4 whatever the handle's tuning state says: the scan emits a
// query's excluded rows too, they occupy slots until the scrub clears them, and a speaker of 1500 rows must fit), and between the
// scan's launches k_excl_pq_scrub clears every query's excluded entries out of the buffers the floors and the re-rank read:
//   1 launch on the sample pre-pass's entries (before k_floor_from_sample), 1 before each k_kth_floor between two phases, 1 before
//   the re-rank: 1 + (phases - 1) + 1; none on the exact route, none when m == 0.  One workgroup per query.
constexpr int KNN_EXCL_SCAN_PQ_CAP_BOOST = 4;
struct ExclScanPqPlan {
    int route = RADAD_EXCL_SCAN_EXACT;
    StoreFacts facts;            // what `plan` and the workspace layout are made from: the caller's with the forced cap_boost
    ScanPlan plan;               // tile route: the plain search's plan over `facts` (mu / biased: the caller's, as for any plan);
                                 // exact route: the plan the queries are prepared and the workspace laid out with
    int phases = 0;              // tile route: launches of the scan proper (knn_hi_phases)
    int scrub_launches = 0;
    int64_t scrub_grid = 0;      // workgroups of each scrub launch
};
static ExclScanPqPlan knn_excl_scan_pq_plan(const StoreFacts& s, int64_t nq, int k, int m, int fp32_searches_left) {
    ExclScanPqPlan x;
    x.route = knn_excl_scan_route(s, nq, k, fp32_searches_left);
    x.facts = s;
    x.facts.cap_boost = KNN_EXCL_SCAN_PQ_CAP_BOOST;
    const bool tile = x.route == RADAD_EXCL_SCAN_TILE;
    const TileEligibility t = knn_tile_eligibility(x.facts, nq, k, KNN_MARGIN);
    x.plan = knn_finish_plan(x.facts, nq, k, KNN_MARGIN, t, tile, false);
    if (tile) {
        x.phases = (int)knn_hi_phases(s.ntotal, nq, (int64_t)8 * x.plan.s_splits * KW_M, knn_hi_one_go(x.plan, s.ntotal)).size() - 1;
        if (m > 0) { x.scrub_launches = 1 + (x.phases - 1) + 1; x.scrub_grid = nq; }
    }
    return x;
}

// ---- certified range search (radad_knn_range_search) ------------------------------------------------------------------------------
// Every row within a radius instead of the k nearest.  The tile scan is a threshold filter already; a range search hands it the
// floor (threshold - eps(q), k_range_floor) instead of deriving one from rows, so there is no sample pre-pass, no floor kernel and
// nothing to phase: ONE scan launch over the whole store (knn_hi_phases, one_go).
// Route: the tile scan exactly when knn_excl_scan_route says so at k = 1, whatever max_per_query is -- the candidate buffers hold
// what the scan emits, not what the caller wants back.  That keeps the plain search's store-size precondition (a store large enough
// for a sample pre-pass that never runs) on purpose: every kernel precondition the tile scan has been tested under stays in force.
// Facts: the caller's with the widened candidate buffers (cap_boost 4: 4096 entries per query, whatever the handle's tuning state).
// The plan is the plain search's at k = 1 (mu / biased: the caller's, as for any plan); on the exact route it is the plan the queries
// are prepared and the workspace laid out with.
//
// Batches of <= 16 queries (RADAD_RANGE_STREAM; only with StoreFacts::opt_range_smallq, off by default): the one-query question "does
// a copy of THIS clip sit in the store" streams the f16 plane once (k_range_hi_smallq) instead of the fp32 rows in float64.  Chosen
// exactly when the option is set, the tuning state is not on its fp32 fallback, the tile route is not taken and the plain search of
// this batch at k = 1 could stream the plane (knn_smallq_hi_eligible: <= 16 queries, dim % 64 == 0, >= 16 384 rows, the plane on,
// opt_smallq_hi, the query block within SQ_LDS_BUDGET).  A batch of <= 16 queries too wide for the LDS takes the tile route as before.
// The plan: the plain small-batch search's (kind RADAD_SCAN_HI_SMALLQ, f16 queries with a scale) with ONE candidate buffer of
// KNN_RANGE_STREAM_CAP entries per query in place of the per-workgroup lists, one launch, and the one-wave-per-slice geometry whatever
// the store: the K-split form (small stores of wide rows) has no range kernel, such a store streams with one wave per slice here.
constexpr int KNN_RANGE_STREAM_CAP = 4096;       // = RG_MAX_CAP, what k_range_refine's sort is sized for (knn.hip asserts it)
static size_t knn_sq_lds_range(int64_t nq, int dim) { return 2 * (size_t)nq * (dim + 8); }     // the f16 query block alone: no slots, no lists
struct RangePlan {
    int route = RADAD_RANGE_EXACT;
    StoreFacts facts;
    ScanPlan plan;
    int launches = 0;            // tile and stream routes: launches of the scan (1); exact route: 0
};
static RangePlan knn_range_plan(const StoreFacts& s, int64_t nq, int max_per_query, int fp32_searches_left) {
    (void)max_per_query;
    RangePlan x;
    const bool tile = knn_excl_scan_route(s, nq, 1, fp32_searches_left) == RADAD_EXCL_SCAN_TILE;
    const bool stream = !tile && s.opt_range_smallq && fp32_searches_left == 0 && knn_smallq_hi_eligible(s, nq, 1, KNN_MARGIN, false, false);
    x.route = tile ? RADAD_RANGE_TILE : stream ? RADAD_RANGE_STREAM : RADAD_RANGE_EXACT;
    x.facts = s;
    x.facts.cap_boost = KNN_EXCL_SCAN_PQ_CAP_BOOST;
    const TileEligibility t = knn_tile_eligibility(x.facts, nq, 1, KNN_MARGIN);
    x.plan = knn_finish_plan(x.facts, nq, 1, KNN_MARGIN, t, tile, stream);
    if (tile) x.launches = (int)knn_hi_phases(s.ntotal, nq, (int64_t)8 * x.plan.s_splits * KW_M, true).size() - 1;
    if (stream) {
        ScanPlan& p = x.plan;                      // (kind, hi_q, block_threads, n_qtiles: the small-batch search's, from knn_finish_plan)
        // (k_range_hi_smallq keeps no lists: 120 VGPRs, 4 waves per SIMD by registers.  The geometry asks for the plain small-batch
        // kernel's 3 all the same, so that the two streams are cut alike: the stream is not limited by the waves in flight, above)
        const SqStream g = knn_sq_stream_geometry(s.ntotal, (size_t)s.dim * 2, 3, 0);
        p.sq_ksplit = false;
        p.sq_rows_per_wave = g.rows_per_wave;
        p.n_splits = g.n_splits;
        p.n_qtiles = p.reported_qtiles = 1;
        p.sq_lds = knn_sq_lds_range(nq, s.dim);
        p.emit_cap = p.plen = KNN_RANGE_STREAM_CAP;
        p.n_parts = 1;
        x.launches = 1;
    }
    return x;
}
// The exact range pass keeps lists of max_per_query entries, not of the plan's k = 1: its partial lists live in the handle's exclusion
// workspace (xk | xi), grouped and sized as any exact pass at k = max_per_query.
struct RangeLayout {
    size_t xk = 0, xi = 0, bytes = 0;
    int xgroup = 1;
    int64_t xslots = 0;
};
static RangeLayout knn_range_layout(const StoreFacts& s, int64_t nq, int max_per_query) {
    RangeLayout L;
    L.xgroup = knn_exact_group(s.dim, max_per_query);
    L.xslots = knn_exact_slots(nq, max_per_query, L.xgroup);
    L.xk = 0;
    L.xi = al256((size_t)L.xslots * KX_SLICES * max_per_query * sizeof(double));
    L.bytes = L.xi + al256((size_t)L.xslots * KX_SLICES * max_per_query * sizeof(int));
    return L;
}

// ---- certified range search among the rows a query does not exclude (radad_knn_range_search_excl / _excl_pq) ----------------------
// Route, facts (4096-entry buffers) and the ONE scan launch are knn_range_plan's, whatever the mode and whatever is excluded.
//   KNN_RANGE_EXCL_BATCH      one set for the batch: the pre-pass (k_excl_scan_bias, 1 launch on the tile and stream routes) writes a per-call bias
//                             that is NaN for the excluded rows, so the plan carries the BIASED instantiation whatever the plane, as
//                             radad_knn_search_excl_scan's does (RSC 2 / 3; mu is the caller's: without a centre the query constant is 0);
//   KNN_RANGE_EXCL_PER_QUERY  <= 64 tags per query: the plain range search's own plan, member for member -- the scan emits excluded rows
//                             like any others and the re-rank (k_range_refine<true>) drops them while it compacts: no bias, no scrub
//                             launch (k_excl_pq_scrub serves k_kth_floor, which a range search never runs).
// m (tags per query) changes nothing of the plan: m == 0 is answered by the plain range path outright (knn.hip).
constexpr int KNN_RANGE_EXCL_BATCH = 0;
constexpr int KNN_RANGE_EXCL_PER_QUERY = 1;
struct RangeExclPlan {
    int mode = KNN_RANGE_EXCL_BATCH;
    int route = RADAD_RANGE_EXACT;
    StoreFacts facts;
    ScanPlan plan;
    int launches = 0;            // tile and stream routes: launches of the scan (1); exact route: 0
    int prepass_launches = 0;    // batch mode, tile and stream routes: the bias pre-pass (1)
    int scrub_launches = 0;      // always 0
};
static RangeExclPlan knn_range_excl_plan(const StoreFacts& s, int64_t nq, int max_per_query, int mode, int m, int fp32_searches_left) {
    (void)m;
    const RangePlan r = knn_range_plan(s, nq, max_per_query, fp32_searches_left);
    RangeExclPlan x;
    x.mode = mode; x.route = r.route; x.facts = r.facts; x.plan = r.plan; x.launches = r.launches;
    if (mode == KNN_RANGE_EXCL_BATCH) {
        x.plan.biased = x.plan.hi_q;
        x.prepass_launches = r.route != RADAD_RANGE_EXACT ? 1 : 0;
    }
    return x;
}
// The exclusion workspace of the batch mode: the exact pass's partial lists (RangeLayout, unchanged) | the admission bitmap | on the
// tile and stream routes the per-call bias array (ExclScanLayout's two arrays, moved behind the lists).
struct RangeExclLayout {
    RangeLayout lists;
    size_t admit = 0, bias = 0, bytes = 0;
    int64_t n_words = 0;
};
static RangeExclLayout knn_range_excl_layout(const StoreFacts& s, int64_t nq, int max_per_query, int route) {
    RangeExclLayout L;
    L.lists = knn_range_layout(s, nq, max_per_query);
    const ExclScanLayout e = knn_excl_scan_layout(s, route != RADAD_RANGE_EXACT ? RADAD_EXCL_SCAN_TILE : RADAD_EXCL_SCAN_EXACT);
    L.n_words = e.n_words;
    L.admit = L.lists.bytes + e.admit;
    L.bias = L.lists.bytes + e.bias;
    L.bytes = L.lists.bytes + e.bytes;
    return L;
}

// ---- adaptive tuning --------------------------------------------------------------------------------------------------------------
// What a handle does when the certificate rejects more than a quarter of a batch of >= 64 queries: re-decide the plane if rows were
// appended since it was decided, else widen the candidate buffers once (cap_boost 1 -> 4), else leave the certified f16 kernels for
// hi_skip searches (8, doubling to 512).  It learns of a rejection from the reports k_exact_scan stamps into two pinned slots, or by
// looking at a large tile-scan search's certificate before its exact pass (verify_next).  Why, with the measurements: DESIGN.md §4.1,
// "Adaptive tuning"; the rules themselves are the methods below, and tests/knn_plan_check.cpp states each with its numbers.
struct KnnTuning {
    int stamp_seen[2] = {0, 0};      // stamp of the last report consumed from each slot
    bool verify_next = true;         // the next large tile-scan search looks at its certificate before the exact pass
    int hi_fail_streak = 0;          // consecutive returns from the fp32 kernels that were rejected again
    int64_t verified_retries = 0;    // searches run again after a look
    int64_t reports_consumed = 0;    // (radad_knn_tuning_info)
    uint64_t search_seq = 0;         // certified searches so far
    int hi_skip = 0;                 // searches left on the fp32 kernels
    int64_t plane_decided_rows = 0;  // rows the store held when the plane's centre and scale were decided
    float plane_stat[2] = {0.f, 0.f};     // max |y'|, max |y' - yh| right after the plane was built
    bool replan = false;             // decide the plane again at the next search that wants it
    int plane_rebuilds = 0;          // (radad_knn_plane_rebuilds)
    uint64_t tuned_at = 0;           // search_seq at the last change of the plane / of cap_boost / of hi_skip
    int cap_boost = 1;               // candidate buffers of the tile scan: 1024 entries per query x this (1 or 4)

    // -- the sequence of certified searches: search i reports into slot i % 2 under stamp (i mod 2^30) + 1
    int slot() const { return (int)(search_seq & 1); }
    int last_slot() const { return (int)((search_seq + 1) & 1); }       // slot of the most recent certified search
    int stamp() const { return (int)(search_seq & 0x3fffffff) + 1; }
    void search_issued() { ++search_seq; }

    bool appended_since_plane(bool have_plane, int64_t ntotal) const { return have_plane && ntotal > plane_decided_rows; }

    // a batch was mostly rejected by the certificate: re-decide the plane if rows were appended since it was decided, else widen the
    // candidate buffers, else leave the f16 kernels for a while (8 searches, doubling while every return is rejected again)
    void mass_rejection(bool appended) {
        if (appended) replan = true;
        else if (cap_boost == 1) cap_boost = 4;
        else { hi_skip = 8 << std::min(hi_fail_streak, 6); ++hi_fail_streak; }
        tuned_at = search_seq;
        verify_next = true;
    }

    // A search eligible for the certified tile scan: true = take it, false = this search was counted off the skip (the search after
    // the last skipped one looks before its exact pass).
    bool take_tile_turn() {
        if (hi_skip == 0) return true;
        if (--hi_skip == 0) verify_next = true;
        return false;
    }
    // ... for the small-batch stream of the plane (every search that would take a certified f16 kernel counts the skip down: a handle
    // that only sees small batches after a mass rejection used to stay on the fp32 kernel for ever)
    bool take_smallq_turn() {
        if (hi_skip == 0) return true;
        --hi_skip;
        return false;
    }
    void clear_skip() { hi_skip = 0; }

    // a slot holds a report (stamp != 0) that was not consumed yet
    bool report_is_new(int slot, int stamp) const { return stamp != 0 && stamp != stamp_seen[slot]; }
    // One report (slot, stamp, rejected queries, batch size), read consistently by the caller.  Returns whether it retuned: only
    // off a skip, for batches of >= 64 with more than a quarter rejected, and only for a search issued since the last tuning change
    // (a report from before the last change of the plane or of the buffers says nothing about them).
    bool consume_report(int slot, int stamp, int rejected, int batch, bool appended) {
        if (!report_is_new(slot, stamp)) return false;
        stamp_seen[slot] = stamp;
        ++reports_consumed;
        // the report's own search: the one search at or below search_seq with that stamp's low 30 bits
        const uint64_t rep_seq = report_search(stamp);
        if (hi_skip == 0 && batch >= 64 && (int64_t)rejected * 4 > batch && rep_seq >= tuned_at) { mass_rejection(appended); return true; }
        return false;
    }
    uint64_t report_search(int stamp) const {
        const uint64_t cur30 = search_seq & 0x3fffffff, rep30 = (uint64_t)(stamp - 1);
        return search_seq - ((cur30 - rep30) & 0x3fffffff);
    }

    // looking before the exact pass: only the tile scan, only when something changed, only where the exact pass would be expensive
    bool looks_before_exact(bool hi_tile, int64_t nq, int64_t ntotal, int dim) const {
        return hi_tile && verify_next && nq >= 64 && (double)nq * (double)ntotal * (double)dim >= 4e11;
    }
    // what the look saw.  true: retuned, run the search again (`may_retry`: not the last attempt)
    bool look_outcome(int rejected, int64_t nq, bool may_retry, bool appended) {
        if ((int64_t)rejected * 4 > nq && may_retry) {
            mass_rejection(appended);
            ++verified_retries;
            return true;
        }
        if ((int64_t)rejected * 4 <= nq) { verify_next = false; hi_fail_streak = 0; }
        return false;
    }

    // -- the plane.  `current`: a plane exists and was built for the store's present capacity (another capacity rebuilds it anyway)
    bool plane_rebuild_due(bool current, int64_t ntotal) const {
        return current && ntotal > plane_decided_rows && (replan || ntotal >= 2 * plane_decided_rows);
    }
    void plane_dropped_for_rebuild() { ++plane_rebuilds; tuned_at = search_seq; }
    void plane_wanted() { replan = false; }          // whatever asked for a new decision is being served now
    void plane_is_new() { verify_next = true; }
    void plane_decided(float max_abs, float max_residual, int64_t ntotal) { plane_stat[0] = max_abs; plane_stat[1] = max_residual; plane_decided_rows = ntotal; }
    // rows were removed (radad_knn_remove_ids) and the store now holds `ntotal_after`.  The comparisons above assume a store that only
    // grows: without this step a store cut from 1000 rows to 600 and refilled to 700 would not count as appended to.  The plane's
    // decision now stands for at most the rows that are left: rows appended from here on are noticed, and the plane re-decided at twice
    // that count, exactly as after a decision taken at `ntotal_after` rows.  A removal that leaves more rows than the plane was decided
    // at (rows appended since, not yet seen by a search) changes nothing.
    void rows_removed(int64_t ntotal_after) { plane_decided_rows = std::min(plane_decided_rows, std::max<int64_t>(ntotal_after, 0)); }
    // what the plane's operands measure after an append.  true: rows beyond what the scale was chosen for -- decide again, now
    bool plane_outgrown(float max_abs, float max_residual) {
        if ((plane_stat[0] > 0.f && max_abs > 8.f * plane_stat[0]) || (plane_stat[1] > 0.f && max_residual > 8.f * plane_stat[1])) { replan = true; return true; }
        return false;
    }
};

// ---- removing rows in place (knn_remove.inc, radad_knn_remove_ids) -------------------------------------------------------------------
// A removal marks the rows to drop (one byte each), takes the exclusive prefix sum of the marks (excl[i] = rows dropped in front of
// row i: per-block counts, a scan of the counts, in-block offsets -- integers only) and then moves every kept row i to i - excl[i].
// Destinations never exceed sources, but a launch whose workgroups read and write the same row range would still race, so the moves
// are planned here such that NO ROW IS WRITTEN WHILE ANY WORKGROUP OF THE SAME LAUNCH MAY STILL READ IT; what orders two launches is
// the stream.  The store is walked in ascending SLABS of S rows from the slab that holds the first removed row r0 (nothing in front
// of r0 moves):
//   - a slab with at least S removed rows in front of it is DIRECT: its kept rows land in [a - d, b - d') with d, d' >= S >= b - a,
//     i.e. wholly below its own start a.  Consecutive direct slabs share one launch while the launch's span b - a stays <= the rows
//     removed in front of a (the same argument with the launch for the slab);
//   - any other slab is STAGED: one launch gathers its kept rows into a staging buffer of S rows (reads the store, writes staging),
//     the next launch on the stream copies them to their destination (reads staging, writes the store).
// Every launch reads only rows at or above its own start that no earlier step of the SAME launch writes, and everything below a
// launch's start is final before it runs.  tests/knn_remove_plan_check.cpp executes plans on integer arrays and checks both.
constexpr int64_t KNN_REMOVE_MIN_STAGE_ROWS = 64;               // RADAD_KNN_OPT_REMOVE_STAGE_ROWS is clamped to this minimum
constexpr size_t KNN_REMOVE_STAGE_BYTES = (size_t)64 << 20;     // default staging buffer: 64 MiB of rows, whatever the store holds
constexpr int KNN_REMOVE_SCAN_ROWS = 2048;                      // rows per workgroup of the count / offset kernels (256 threads x 8)
enum { KNN_REMOVE_GATHER = 0, KNN_REMOVE_SCATTER = 1, KNN_REMOVE_DIRECT = 2 };

// slab size in rows: the option when set (> 0), else what the default staging bytes hold; never below the minimum
static int64_t knn_remove_stage_rows(size_t row_bytes, int64_t opt_stage_rows) {
    const int64_t s = opt_stage_rows > 0 ? opt_stage_rows : (int64_t)(KNN_REMOVE_STAGE_BYTES / std::max<size_t>(row_bytes, 1));
    return std::max<int64_t>(KNN_REMOVE_MIN_STAGE_ROWS, s);
}

// byte offsets in the handle's workspace: flags [ntotal] bytes | block counts [n_blocks + 1] int | excl [ntotal] int |
// slab counts [max_slabs + 1] int | head: first removed row, removed count (2 x int64) | staged rows [S] | staged norms [S] (L2)
struct RemoveLayout {
    size_t flags = 0, blk = 0, excl = 0, slab_rb = 0, head = 0, stage = 0, stage_norm = 0, bytes = 0;
    int64_t n_blocks = 0, max_slabs = 0;
};
static RemoveLayout knn_remove_layout(int64_t ntotal, size_t row_bytes, int64_t stage_rows, bool l2) {
    RemoveLayout L;
    L.n_blocks = ceil_div64(std::max<int64_t>(ntotal, 1), KNN_REMOVE_SCAN_ROWS);
    L.max_slabs = ceil_div64(std::max<int64_t>(ntotal, 1), stage_rows);
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += al256(bytes); return o; };
    // (the count kernel reads the flags eight at a time: the array is padded to whole blocks)
    L.flags = take((size_t)L.n_blocks * KNN_REMOVE_SCAN_ROWS);
    L.blk = take((size_t)(L.n_blocks + 1) * sizeof(int));
    L.excl = take((size_t)std::max<int64_t>(ntotal, 1) * sizeof(int));
    L.slab_rb = take((size_t)(L.max_slabs + 1) * sizeof(int));
    L.head = take(2 * sizeof(int64_t));
    L.stage = take((size_t)stage_rows * row_bytes);
    L.stage_norm = take(l2 ? (size_t)stage_rows * sizeof(float) : 0);
    L.bytes = off;
    return L;
}

struct RemoveSlab {
    int64_t row0 = 0, rows = 0;
    int64_t removed_before = 0;      // rows removed in front of row0
    int64_t kept = 0;                // rows of the slab that stay
    bool direct = false;
};
// one kernel launch: rows [row0, row0 + rows) of the store (GATHER, DIRECT) or `rows` staged rows (SCATTER); dst0 = where the first
// kept row of the range lands (row0 minus the rows removed in front of it)
struct RemoveLaunch {
    int kind = KNN_REMOVE_DIRECT;
    int64_t row0 = 0, rows = 0, dst0 = 0;
};
struct RemovePlan {
    int64_t stage_rows = 0;          // S
    int64_t slab0 = 0;               // first row of the first slab: r0 / S * S
    std::vector<RemoveSlab> slabs;
    std::vector<RemoveLaunch> launches;
    int64_t rows_moved = 0;          // kept rows that change position
    size_t bytes_moved = 0;          // bytes read + written by the launches (a staged row is read and written twice)
    RemoveLayout layout;
};
// the slabs of a removal whose first removed row is r0: [slab0, ntotal) in steps of S
static int64_t knn_remove_slab0(int64_t first_removed_row, int64_t stage_rows) { return first_removed_row / stage_rows * stage_rows; }
static int64_t knn_remove_n_slabs(int64_t ntotal, int64_t first_removed_row, int64_t stage_rows) {
    if (first_removed_row < 0 || first_removed_row >= ntotal) return 0;
    return ceil_div64(ntotal - knn_remove_slab0(first_removed_row, stage_rows), stage_rows);
}
// removed_before: [n_slabs + 1] rows removed in front of every slab's first row, then the removed count of the whole store (what the
// device's prefix sum says at those rows).  opt_stage_rows: RADAD_KNN_OPT_REMOVE_STAGE_ROWS, 0 = default.
static RemovePlan knn_remove_plan(int64_t ntotal, size_t row_bytes, int64_t first_removed_row, int64_t opt_stage_rows, bool l2,
                                  const int* removed_before) {
    RemovePlan p;
    const int64_t S = p.stage_rows = knn_remove_stage_rows(row_bytes, opt_stage_rows);
    p.layout = knn_remove_layout(ntotal, row_bytes, S, l2);
    const int64_t n_slabs = knn_remove_n_slabs(ntotal, first_removed_row, S);
    p.slab0 = n_slabs ? knn_remove_slab0(first_removed_row, S) : ntotal;
    const size_t moved_row = row_bytes + (l2 ? sizeof(float) : 0);
    for (int64_t j = 0; j < n_slabs; ++j) {
        RemoveSlab s;
        s.row0 = p.slab0 + j * S;
        s.rows = std::min<int64_t>(S, ntotal - s.row0);
        s.removed_before = removed_before[j];
        s.kept = s.rows - (removed_before[j + 1] - removed_before[j]);
        s.direct = s.removed_before >= S;
        p.slabs.push_back(s);
    }
    for (size_t j = 0; j < p.slabs.size(); ++j) {
        const RemoveSlab& s = p.slabs[j];
        if (s.direct) {
            // this slab and the direct ones behind it, while the launch's span stays within the rows removed in front of it
            RemoveLaunch l;
            l.kind = KNN_REMOVE_DIRECT; l.row0 = s.row0; l.rows = s.rows; l.dst0 = s.row0 - s.removed_before;
            int64_t kept = s.kept;
            while (j + 1 < p.slabs.size() && l.rows + p.slabs[j + 1].rows <= s.removed_before) {
                ++j;
                l.rows += p.slabs[j].rows; kept += p.slabs[j].kept;
            }
            if (kept > 0) { p.launches.push_back(l); p.rows_moved += kept; p.bytes_moved += 2 * (size_t)kept * moved_row; }
            continue;
        }
        // staged.  The first slab's rows in front of r0 stay where they are: its range starts at r0 (nothing is removed in front of it)
        RemoveLaunch g;
        g.kind = KNN_REMOVE_GATHER;
        g.row0 = j == 0 ? first_removed_row : s.row0;
        g.rows = s.row0 + s.rows - g.row0;
        g.dst0 = g.row0 - s.removed_before;
        const int64_t kept = s.kept - (g.row0 - s.row0);
        if (kept <= 0) continue;
        RemoveLaunch c;
        c.kind = KNN_REMOVE_SCATTER; c.row0 = 0; c.rows = kept; c.dst0 = g.dst0;
        p.launches.push_back(g);
        p.launches.push_back(c);
        p.rows_moved += kept; p.bytes_moved += 4 * (size_t)kept * moved_row;
    }
    return p;
}
