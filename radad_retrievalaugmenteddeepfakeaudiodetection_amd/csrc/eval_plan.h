// eval_plan.h -- host-only plan of radad_eval_metrics (csrc/eval_metrics.inc): which launches run with which grids, how many
// merge passes each sort takes and how the workspace is carved, as a function of the sample count and of whether group ids are
// present.  No HIP in here: tests/eval_plan_check.cpp compiles it with a plain C++ compiler.  eval_metrics.inc launches exactly
// what the plan says and radad_eval_metrics_workspace_bytes returns its `total`.
//
// One sort = one LDS bitonic sort per tile of EVAL_TILE keys, then ceil(log2(tiles)) merge-path passes that ping-pong between
// two key buffers; run r of a pass is `run` keys long (the last one shorter, an unpaired last run is copied).  Every per-tile
// kernel (tile sort, merge, count, scan, candidates, segment EER) has one workgroup of EVAL_THREADS threads per tile, each thread
// EVAL_ITEMS keys.  The pooled section always runs; the group section is launched only with group ids (and its kernels leave at
// once when the device finds that all ids are equal).
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr int EVAL_THREADS = 256;
constexpr int EVAL_ITEMS = 8;
constexpr int EVAL_TILE = EVAL_THREADS * EVAL_ITEMS;      // 2048 keys, 16 KiB of LDS in the tile sort
constexpr int64_t EVAL_MAX_N = 1ll << 24;                 // RADAD_EVAL_MAX_N
constexpr size_t EVAL_WS_HEAD = 256;                      // EvalHead: the scalars the kernels hand to one another
constexpr int EVAL_POOLED_FIXED_LAUNCHES = 6;             // tile sort, count, scan, candidates x2, finish
constexpr int EVAL_GROUP_FIXED_LAUNCHES = 8;              // the same with the scored-segment count and the per-segment EER in front of the finish

struct EvalPlan {
    bool ok = false;
    int64_t n = 0;
    int groups = 0;
    int tiles = 0;            // the grid of every per-tile launch
    int merge_passes = 0;     // per sort; pass p merges runs of EVAL_TILE << p keys
    int sorted_buf = 0;       // which of the two key buffers holds a finished sort: merge_passes & 1
    int sorts = 0;            // 1 pooled, + 1 by group
    int launches = 0;         // kernel launches of one radad_eval_metrics call (the one memset of the head not counted)
    // byte offsets into the workspace, each a multiple of 256
    size_t off_buf[2] = {0, 0};   // uint64[n] each: the sort's ping-pong buffers (buf[0] receives the tile sort)
    size_t off_cnt = 0;           // uint64[n + 1]: positives (high word) and run heads (low word) in front of each sorted key
    size_t off_best = 0;          // uint64[n]: per segment start the least |fnr - fpr|, later that segment's EER
    size_t off_idx = 0;           // uint32[n]: per segment start the first candidate that attains it
    size_t total = 0;
};

inline size_t eval_al256(size_t b) { return (b + 255) & ~(size_t)255; }

inline EvalPlan eval_plan(int64_t n, int groups) {
    EvalPlan p;
    if (n < 1 || n > EVAL_MAX_N) return p;
    p.ok = true;
    p.n = n;
    p.groups = groups != 0;
    p.tiles = (int)((n + EVAL_TILE - 1) / EVAL_TILE);
    while (((int64_t)1 << p.merge_passes) < p.tiles) ++p.merge_passes;
    p.sorted_buf = p.merge_passes & 1;
    p.sorts = 1 + p.groups;
    p.launches = EVAL_POOLED_FIXED_LAUNCHES + p.merge_passes + (p.groups ? EVAL_GROUP_FIXED_LAUNCHES + p.merge_passes : 0);
    size_t off = EVAL_WS_HEAD;
    p.off_buf[0] = off; off += eval_al256((size_t)n * 8);
    p.off_buf[1] = off; off += eval_al256((size_t)n * 8);
    p.off_cnt = off;    off += eval_al256((size_t)(n + 1) * 8);
    p.off_best = off;   off += eval_al256((size_t)n * 8);
    p.off_idx = off;    off += eval_al256((size_t)n * 4);
    p.total = off;
    return p;
}

#ifdef __HIPCC__
#define EVAL_HD __host__ __device__
#else
#define EVAL_HD
#endif

// where output position o of a merge pass over runs of `run` keys comes from: the pair's first key p0, the lengths of its two
// runs (the second may be short or empty), and o's diagonal d = o - p0 < nA + nB.  The kernel and the plan check share it.
struct EvalMergeSplit { int p0, nA, nB, d; };
EVAL_HD inline EvalMergeSplit eval_merge_split(int o, int n, int run) {
    EvalMergeSplit m;
    m.p0 = (int)(((int64_t)o / (2 * (int64_t)run)) * (2 * (int64_t)run));
    m.nA = n - m.p0 < run ? n - m.p0 : run;
    m.nB = n - m.p0 - m.nA < run ? n - m.p0 - m.nA : run;
    m.d = o - m.p0;
    return m;
}

// keys of one merge pass's runs, and how many runs it reads
inline int64_t eval_pass_run(int pass) { return (int64_t)EVAL_TILE << pass; }
inline int64_t eval_pass_runs(int64_t n, int pass) { return (n + eval_pass_run(pass) - 1) / eval_pass_run(pass); }
