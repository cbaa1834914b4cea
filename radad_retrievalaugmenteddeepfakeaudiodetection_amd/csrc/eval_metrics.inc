// eval_metrics.inc -- what RADAD's validation pass reads back and computes on the host (pipeline.py:725-733, 152-234, 277-326,
// 868-872), on gfx950.  Included at the end of proj.hip after optim_step.inc.
//
// radad_eval_append, one launch per validation batch: one workgroup writes a 64-bit sort key per sample and adds the batch's
// BCE-with-logits sum (fp64 terms, fp64 sum in k_bce_logits' order), correct count, sample count and non-finite count into four
// accumulators with plain read-add-write by one thread (appends on one stream are ordered).
//
// radad_eval_metrics, no host round trip.  The plan (eval_plan.h) fixes grids, passes and the workspace.  Per sort:
//   k_eval_tile_sort  bitonic sort of one tile of keys in LDS (the pooled sort clears the group field on the way in and looks
//                     for a second group id and for non-finite scores)
//   k_eval_merge      one merge-path pass: every thread finds its diagonal by binary search and merges EVAL_ITEMS keys
//   k_eval_count      positives and run heads per tile; resets the per-segment minima
//   k_eval_scan       exclusive scan of both counts in front of every sorted key (tile offsets summed by each workgroup itself)
//   k_eval_cand<1>    at every run head (= distinct score of a segment): fnr, fpr from the counts, the least |fnr - fpr| per
//                     segment by integer atomicMin on the fp64 bit pattern; pooled also t-DCF, the AUC sum, the ROC points
//   k_eval_cand<2>    among the candidates that attain the minimum, the first one (atomicMin on the index)
//   pooled: k_eval_finish_pooled     by group: k_eval_seg_count, k_eval_seg_eer (the scored groups' EERs compacted in ascending
//                     group id), k_eval_finish_groups (their fp64 sum, one by one in that order)
// Everything that is combined across threads is an integer (counts, bit patterns of non-negative doubles, indices), so atomics do
// not make the result depend on arrival order; the only fp64 sum (macro EER) has one order.  Two runs give the same bits.
//
// Key: group id (31 bits) << 33 | order-preserving image of the float32 score << 1 | label.  Ascending keys are ascending
// (group, score, label); -0.0 has the image of +0.0.  Inside a run of equal (group, score) the negatives come first.
#include "eval_plan.h"

namespace {

static_assert(EVAL_MAX_N == RADAD_EVAL_MAX_N, "the plan and the header agree on the cap");
static_assert(EVAL_THREADS % 64 == 0 && EVAL_TILE == EVAL_THREADS * EVAL_ITEMS && (EVAL_TILE & (EVAL_TILE - 1)) == 0,
              "a tile is a power of two of keys, EVAL_ITEMS per thread");

typedef unsigned long long u64;
constexpr int EVAL_GROUP_SHIFT = 33;
constexpr u64 EVAL_POOLED_MASK = ((u64)1 << EVAL_GROUP_SHIFT) - 1;
constexpr int EVAL_WAVES = EVAL_THREADS / 64;

struct EvalAcc {                 // acc_dev
    double loss_sum;
    int64_t correct, count, nonfinite;
};
static_assert(sizeof(EvalAcc) == RADAD_EVAL_ACC_BYTES, "acc_dev is four 8-byte slots");

struct EvalHead {                // head of the workspace, zeroed by the one memset in front of the launches
    u64 auc2;                    // sum over positives of 2 #{neg below} + #{neg equal}
    u64 tdcf_best;               // ordered image of the least t-DCF among the run heads
    uint32_t tdcf_idx;           // first run head that attains it
    uint32_t multi_group;        // some key's group id differs from key 0's
    uint32_t nonfinite;          // scores that are inf or NaN
    uint32_t pad;
};
static_assert(sizeof(EvalHead) <= EVAL_WS_HEAD, "the workspace head holds EvalHead");

__device__ __forceinline__ uint32_t eval_score_image(float x) {
    uint32_t b = __float_as_uint(x);
    if (b == 0x80000000u) b = 0u;                       // -0.0 is the threshold +0.0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ uint32_t eval_image_bits(uint32_t img) { return (img & 0x80000000u) ? (img ^ 0x80000000u) : ~img; }
__device__ __forceinline__ double eval_key_score(u64 key) { return (double)__uint_as_float(eval_image_bits((uint32_t)(key >> 1))); }
__device__ __forceinline__ int eval_key_group(u64 key) { return (int)(key >> EVAL_GROUP_SHIFT); }
__device__ __forceinline__ u64 eval_f64_image(double v) {
    const u64 b = (u64)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | ((u64)1 << 63));
}
__device__ __forceinline__ int eval_cnt_pos(u64 c) { return (int)(c >> 32); }
__device__ __forceinline__ int eval_cnt_heads(u64 c) { return (int)(c & 0xffffffffu); }

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// per-sample BCE-with-logits terms as k_bce_logits forms them; thread i takes elements i, i + 256, ...; the butterfly; the four
// waves in order; then thread 0 adds the batch to the accumulators
__global__ __launch_bounds__(EVAL_THREADS) void k_eval_append(const float* __restrict__ x, const float* __restrict__ y,
                                                              const int32_t* __restrict__ gid, int n, float pos_weight,
                                                              u64* __restrict__ keys, EvalAcc* __restrict__ acc) {
    __shared__ double s_sum[EVAL_WAVES];
    __shared__ int s_cnt[EVAL_WAVES], s_bad[EVAL_WAVES];
    const double pw1 = (double)pos_weight - 1.0;
    double sum = 0.0;
    int cnt = 0, bad = 0;
    for (int i = threadIdx.x; i < n; i += EVAL_THREADS) {
        const float xf = x[i], yf = y[i];
        const double xi = (double)xf, yi = (double)yf;
        const double w = 1.0 + pw1 * yi;
        const double e = exp(-fabs(xi));
        sum += (1.0 - yi) * xi + w * (log1p(e) + fmax(-xi, 0.0));
        cnt += (xf > 0.f) == (yf == 1.f);
        bad += !__builtin_isfinite(xf);
        const u64 g = gid ? (u64)((uint32_t)gid[i] & 0x7fffffffu) : 0;
        keys[i] = (g << EVAL_GROUP_SHIFT) | ((u64)eval_score_image(xf) << 1) | (u64)(yf == 1.f);
    }
    sum = wave_sum_f64(sum);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o, 64);
        bad += __shfl_xor(bad, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        s_sum[threadIdx.x >> 6] = sum;
        s_cnt[threadIdx.x >> 6] = cnt;
        s_bad[threadIdx.x >> 6] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = s_sum[0];
        int c = s_cnt[0], b = s_bad[0];
        for (int w = 1; w < EVAL_WAVES; ++w) { t += s_sum[w]; c += s_cnt[w]; b += s_bad[w]; }
        acc->loss_sum += t;
        acc->correct += c;
        acc->count += n;
        acc->nonfinite += b;
    }
}

// one tile of keys & mask, sorted ascending, into out.  pooled: mask clears the group field, and the same read finds out whether
// a second group id exists and counts the non-finite scores.  by group: leaves at once when there is one group only.
__global__ __launch_bounds__(EVAL_THREADS) void k_eval_tile_sort(const u64* __restrict__ keys, int n, u64 mask, int pooled,
                                                                 EvalHead* __restrict__ head, u64* __restrict__ out) {
    __shared__ u64 s[EVAL_TILE];
    if (!pooled && !head->multi_group) return;
    const int base = blockIdx.x * EVAL_TILE;
    const int g0 = eval_key_group(keys[0]);
    int bad = 0, other = 0;
#pragma unroll
    for (int j = 0; j < EVAL_ITEMS; ++j) {
        const int e = (int)threadIdx.x + j * EVAL_THREADS;
        const int i = base + e;
        u64 k = ~(u64)0;                                   // past the end: sorts behind every key of the tile
        if (i < n) {
            k = keys[i];
            bad += (eval_image_bits((uint32_t)(k >> 1)) & 0x7f800000u) == 0x7f800000u;
            other |= eval_key_group(k) != g0;
            k &= mask;
        }
        s[e] = k;
    }
    if (pooled) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, 64);
        if ((threadIdx.x & 63) == 0 && bad) atomicAdd(&head->nonfinite, (uint32_t)bad);
        if (other) head->multi_group = 1u;
    }
    for (int k = 2; k <= EVAL_TILE; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
#pragma unroll
            for (int q = 0; q < EVAL_ITEMS / 2; ++q) {
                const int t = (int)threadIdx.x + q * EVAL_THREADS;      // pair number, 0 .. EVAL_TILE / 2 - 1
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));   // its lower element: bit j clear
                const u64 a = s[i], b = s[i + j];
                if ((a > b) == ((i & k) == 0)) {
                    s[i] = b;
                    s[i + j] = a;
                }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < EVAL_ITEMS; ++j) {
        const int e = (int)threadIdx.x + j * EVAL_THREADS;
        if (base + e < n) out[base + e] = s[e];
    }
}

// one merge pass: runs of `run` sorted keys, (2r, 2r + 1) -> one run of 2 run.  A thread writes EVAL_ITEMS consecutive keys of
// the output: its diagonal's split by binary search (merge path), then a serial merge.  The last pair may have a short or an
// empty second run.
__global__ __launch_bounds__(EVAL_THREADS) void k_eval_merge(const u64* __restrict__ src, u64* __restrict__ dst, int n, int run,
                                                             int pooled, const EvalHead* __restrict__ head) {
    if (!pooled && !head->multi_group) return;
    const int o = ((int)blockIdx.x * EVAL_THREADS + (int)threadIdx.x) * EVAL_ITEMS;
    if (o >= n) return;
    const EvalMergeSplit m = eval_merge_split(o, n, run);
    const int nA = m.nA, nB = m.nB, d = m.d;                // d < nA + nB
    const u64* A = src + m.p0;
    const u64* B = A + nA;
    int lo = max(0, d - nB), hi = min(d, nA);
    while (lo < hi) {                                       // mid in [0, nA), d - 1 - mid in [0, nB)
        const int mid = (lo + hi) >> 1;
        if (A[mid] <= B[d - 1 - mid]) lo = mid + 1; else hi = mid;
    }
    int a = lo, b = d - lo;
    const int cnt = min(EVAL_ITEMS, nA + nB - d);
    u64 ka = a < nA ? A[a] : ~(u64)0, kb = b < nB ? B[b] : ~(u64)0;
    for (int i = 0; i < cnt; ++i) {
        if (b >= nB || (a < nA && ka <= kb)) {
            dst[o + i] = ka;
            ++a;
            ka = a < nA ? A[a] : ~(u64)0;
        } else {
            dst[o + i] = kb;
            ++b;
            kb = b < nB ? B[b] : ~(u64)0;
        }
    }
}

// a run head is the first key of a run of equal (group, score)
__device__ __forceinline__ bool eval_is_head(const u64* keys, int i, u64 key) { return i == 0 || (keys[i - 1] >> 1) != (key >> 1); }

// per tile: positives << 32 | run heads; resets the segment minima of the tile's positions
__global__ __launch_bounds__(EVAL_THREADS) void k_eval_count(const u64* __restrict__ keys, int n, int pooled,
                                                             EvalHead* __restrict__ head, u64* __restrict__ tile_tot,
                                                             u64* __restrict__ best, uint32_t* __restrict__ idx) {
    __shared__ u64 s_tot[EVAL_WAVES];
    if (!pooled && !head->multi_group) return;
    if (pooled && blockIdx.x == 0 && threadIdx.x == 0) {
        head->tdcf_best = ~(u64)0;
        head->tdcf_idx = ~0u;
    }
    const int base = blockIdx.x * EVAL_TILE;
    u64 tot = 0;
#pragma unroll
    for (int j = 0; j < EVAL_ITEMS; ++j) {
        const int i = base + (int)threadIdx.x + j * EVAL_THREADS;
        if (i < n) {
            const u64 k = keys[i];
            tot += ((k & 1) << 32) + (u64)eval_is_head(keys, i, k);
            best[i] = ~(u64)0;
            idx[i] = ~0u;
        }
    }
    tot = wave_sum_u64(tot);
    if ((threadIdx.x & 63) == 0) s_tot[threadIdx.x >> 6] = tot;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 t = s_tot[0];
        for (int w = 1; w < EVAL_WAVES; ++w) t += s_tot[w];
        tile_tot[blockIdx.x] = t;
    }
}

// cnt[i] = positives << 32 | run heads among sorted keys [0, i), for i = 0 .. n.  A workgroup adds up the totals of the tiles
// in front of its own (integers: any order), then scans its tile; a thread owns EVAL_ITEMS consecutive keys.
__global__ __launch_bounds__(EVAL_THREADS) void k_eval_scan(const u64* __restrict__ keys, int n, int pooled,
                                                            const EvalHead* __restrict__ head, const u64* __restrict__ tile_tot,
                                                            u64* __restrict__ cnt) {
    __shared__ u64 s_off[EVAL_WAVES], s_wave[EVAL_WAVES];
    if (!pooled && !head->multi_group) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 off = 0;
    for (int t = threadIdx.x; t < (int)blockIdx.x; t += EVAL_THREADS) off += tile_tot[t];
    off = wave_sum_u64(off);
    const int i0 = (int)blockIdx.x * EVAL_TILE + (int)threadIdx.x * EVAL_ITEMS;
    u64 mine[EVAL_ITEMS];
    u64 tot = 0;
#pragma unroll
    for (int j = 0; j < EVAL_ITEMS; ++j) {
        mine[j] = 0;
        if (i0 + j < n) {
            const u64 k = keys[i0 + j];
            mine[j] = ((k & 1) << 32) + (u64)eval_is_head(keys, i0 + j, k);
        }
        tot += mine[j];
    }
    u64 incl = tot;                                          // inclusive scan of the threads' totals inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    if (lane == 0) s_off[wave] = off;
    __syncthreads();
    u64 before = incl - tot;
    for (int w = 0; w < EVAL_WAVES; ++w) {
        before += s_off[w];
        if (w < wave) before += s_wave[w];
    }
#pragma unroll
    for (int j = 0; j < EVAL_ITEMS; ++j) {
        if (i0 + j < n) cnt[i0 + j] = before;
        before += mine[j];
        if (i0 + j == n - 1) cnt[n] = before;
    }
}

// first index in [lo, hi) whose key is >= v, or hi
__device__ __forceinline__ int eval_lower_bound(const u64* keys, int lo, int hi, u64 v) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// first index in [lo, hi) whose group id is > g, or hi
__device__ __forceinline__ int eval_group_end(const u64* keys, int lo, int hi, int g) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (eval_key_group(keys[mid]) <= g) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct EvalRates { double fnr, fpr; };
// fnr = #{positives below t} / P and fpr = #{negatives at or above t} / N: two IEEE divisions of integers
__device__ __forceinline__ EvalRates eval_rates(int cp, int cn, int P, int N) {
    EvalRates r;
    r.fnr = (double)cp / (double)P;
    r.fpr = (double)(N - cn) / (double)N;
    return r;
}

// pipeline.py:318-323 with c0, c1, c2 formed on the host; no contraction, so that near-tied thresholds keep their order
__device__ __forceinline__ double eval_tdcf(const radad_tdcf_consts& c, double pmiss) {
#pragma clang fp contract(off)
    const double t3 = (c.c1 * (1.0 - pmiss)) * c.p_fa_spoof_asv;
    const double t4 = c.c2 * pmiss;
    return ((c.c0 + t3) + t4) / c.c_def;
}

// the least v among the wave's candidates into arr[slot]: one atomic for the wave where all its candidates share a slot
template <typename T>
__device__ __forceinline__ void eval_wave_min(bool cand, int slot, T v, T* arr) {
    const u64 m = __ballot(cand);
    if (m == 0) return;
    const int s0 = __shfl(slot, __ffsll((long long)m) - 1, 64);
    if (__ballot(cand && slot != s0) == 0) {
        T r = cand ? v : ~(T)0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const T q = __shfl_xor(r, o, 64);
            r = q < r ? q : r;
        }
        if ((threadIdx.x & 63) == 0) atomicMin(&arr[s0], r);
    } else if (cand) {
        atomicMin(&arr[slot], v);
    }
}

struct EvalCandArgs {
    const u64* keys;
    int n;
    const u64* cnt;
    u64* best;
    uint32_t* idx;
    EvalHead* head;
    radad_tdcf_consts tc;
    int has_tc;
    double* roc;             // pooled only, or nullptr
    double* geer;            // the scored groups' EERs in ascending group id: the caller's array, or the free best[]
};

// PHASE 1: every run head of a segment with both classes offers |fnr - fpr| (bit pattern of a non-negative double: integer
// order is numeric order) to its segment's slot; pooled: also its t-DCF, its ROC point, and every positive its AUC term.
// PHASE 2: the heads whose value is the slot's minimum offer their index.  The slot is the segment's first position (pooled: 0).
template <int PHASE, bool POOLED>
__global__ __launch_bounds__(EVAL_THREADS) void k_eval_cand(EvalCandArgs p) {
    __shared__ int s_seg[4];
    const u64* keys = p.keys;
    const int n = p.n;
    const int base = blockIdx.x * EVAL_TILE;
    const int end = min(base + EVAL_TILE, n);
    int g_first = 0, g_last = 0;
    if (!POOLED) {
        if (!p.head->multi_group) return;
        g_first = eval_key_group(keys[base]);
        g_last = eval_key_group(keys[end - 1]);
        if (threadIdx.x == 0) {
            s_seg[0] = eval_lower_bound(keys, 0, base, (u64)g_first << EVAL_GROUP_SHIFT);
            s_seg[1] = eval_group_end(keys, base, n, g_first);
        }
        if (threadIdx.x == 64) {
            s_seg[2] = eval_lower_bound(keys, 0, end - 1, (u64)g_last << EVAL_GROUP_SHIFT);
            s_seg[3] = eval_group_end(keys, end - 1, n, g_last);
        }
        __syncthreads();
    }
    const u64 c_n = p.cnt[n];
    u64 auc = 0;
#pragma unroll 1
    for (int j = 0; j < EVAL_ITEMS; ++j) {
        const int i = base + (int)threadIdx.x + j * EVAL_THREADS;
        const bool valid = i < n;
        const u64 key = valid ? keys[i] : 0;
        const bool is_head = valid && eval_is_head(keys, i, key);
        bool cand = false;
        int slot = 0;
        u64 bits = 0, tbits = 0;
        if (is_head) {
            int s = 0, e = n;
            if (!POOLED) {
                const int g = eval_key_group(key);
                if (g == g_first) { s = s_seg[0]; e = s_seg[1]; }
                else if (g == g_last) { s = s_seg[2]; e = s_seg[3]; }
                else {                                       // a group that begins and ends inside this tile
                    s = eval_lower_bound(keys, base, i, (u64)g << EVAL_GROUP_SHIFT);
                    e = eval_group_end(keys, i, end, g);
                }
            }
            const u64 c_s = p.cnt[s], c_i = p.cnt[i];
            const int P = eval_cnt_pos(p.cnt[e]) - eval_cnt_pos(c_s), N = (e - s) - P;
            const int cp = eval_cnt_pos(c_i) - eval_cnt_pos(c_s), cn = (i - s) - cp;
            if (P > 0 && N > 0) {
                cand = true;
                slot = s;
                const EvalRates r = eval_rates(cp, cn, P, N);
                bits = (u64)__double_as_longlong(fabs(r.fnr - r.fpr));
                if (POOLED && p.has_tc) tbits = eval_f64_image(eval_tdcf(p.tc, r.fnr));
            }
            if (POOLED && PHASE == 1 && p.roc) {             // point 1 + (D - 1 - rank), in 1 .. D <= n
                const size_t stride = (size_t)n + 2;
                const size_t at = (size_t)(1 + (eval_cnt_heads(c_n) - 1 - eval_cnt_heads(c_i)));
                p.roc[at] = (double)(N - cn) / (double)N;
                p.roc[stride + at] = (double)(P - cp) / (double)P;
                p.roc[2 * stride + at] = eval_key_score(key);
            }
        }
        if (POOLED && PHASE == 1 && valid && (key & 1)) {
            // negatives below this positive's score are those in front of its run; the run's own negatives lie between
            const int from = (keys[base] >> 1) == (key >> 1) ? 0 : base;
            const int a = is_head ? i : eval_lower_bound(keys, from, i, key & ~(u64)1);
            auc += (u64)(a - eval_cnt_pos(p.cnt[a])) + (u64)(i - eval_cnt_pos(p.cnt[i]));
        }
        if (PHASE == 1) {
            eval_wave_min<u64>(cand, slot, bits, p.best);
            if (POOLED && p.has_tc) eval_wave_min<u64>(cand, 0, tbits, &p.head->tdcf_best);
        } else {
            eval_wave_min<uint32_t>(cand && bits == p.best[slot], slot, (uint32_t)i, p.idx);
            if (POOLED && p.has_tc) eval_wave_min<uint32_t>(cand && tbits == p.head->tdcf_best, 0, (uint32_t)i, &p.head->tdcf_idx);
        }
    }
    if (POOLED && PHASE == 1) {
        auc = wave_sum_u64(auc);
        if ((threadIdx.x & 63) == 0 && auc) atomicAdd(&p.head->auc2, auc);
    }
}

// pooled results.  Candidate -inf has the rates of the first run head and comes first, so a winning first head reports -inf;
// candidate +inf (fnr 1, fpr 0) never has the least |fnr - fpr| alone, and takes the t-DCF only when it is strictly lower.
__global__ __launch_bounds__(64) void k_eval_finish_pooled(EvalCandArgs p, double* __restrict__ out) {
    if (threadIdx.x != 0) return;
    const double nan = __longlong_as_double(0x7ff8000000000000ll), inf = __longlong_as_double(0x7ff0000000000000ll);
    const int n = p.n;
    const u64 c_n = p.cnt[n];
    const int P = eval_cnt_pos(c_n), N = n - P, D = eval_cnt_heads(c_n);
    const uint32_t bad = p.head->nonfinite;
    double auc = nan, eer = nan, eer_thr = nan, tdcf = nan, tdcf_thr = nan;
    int roc_n = 0;
    const size_t stride = (size_t)n + 2;
    if (bad == 0 && (P == 0 || N == 0)) {
        auc = 0.5;
        roc_n = 2;
        if (p.roc) {
            p.roc[0] = 0.0; p.roc[stride] = 0.0; p.roc[2 * stride] = inf;
            p.roc[1] = 1.0; p.roc[stride + 1] = 1.0; p.roc[2 * stride + 1] = -inf;
        }
    } else if (bad == 0) {
        const int k = (int)p.idx[0];
        const int cp = eval_cnt_pos(p.cnt[k]);
        const EvalRates r = eval_rates(cp, k - cp, P, N);
        eer = (r.fnr + r.fpr) / 2.0 * 100.0;
        eer_thr = k == 0 ? -inf : eval_key_score(p.keys[k]);
        if (p.has_tc) {
            const double at_inf = eval_tdcf(p.tc, (double)P / (double)P);
            if (eval_f64_image(at_inf) < p.head->tdcf_best) {
                tdcf = at_inf;
                tdcf_thr = inf;
            } else {
                const int t = (int)p.head->tdcf_idx;
                tdcf = eval_tdcf(p.tc, (double)eval_cnt_pos(p.cnt[t]) / (double)P);
                tdcf_thr = t == 0 ? -inf : eval_key_score(p.keys[t]);
            }
        }
        auc = (double)p.head->auc2 / (double)(2ll * (int64_t)P * (int64_t)N);
        roc_n = D + 2;
        if (p.roc) {
            p.roc[0] = 0.0; p.roc[stride] = 0.0; p.roc[2 * stride] = eval_key_score(p.keys[n - 1]) + 1e-6;
            p.roc[D + 1] = 1.0; p.roc[stride + D + 1] = 1.0; p.roc[2 * stride + D + 1] = eval_key_score(p.keys[0]) - 1e-6;
        }
    }
    out[RADAD_EVAL_AUC] = auc;
    out[RADAD_EVAL_EER] = eer;
    out[RADAD_EVAL_EER_THRESHOLD] = eer_thr;
    out[RADAD_EVAL_MACRO_EER] = eer;                         // one group: the mean over groups is the pooled EER
    p.geer[0] = eer;
    out[RADAD_EVAL_GROUPS_SCORED] = eer == eer ? 1.0 : 0.0;
    out[RADAD_EVAL_MIN_TDCF] = tdcf;
    out[RADAD_EVAL_MIN_TDCF_THRESHOLD] = tdcf_thr;
    out[RADAD_EVAL_NONFINITE] = (double)bad;
    out[RADAD_EVAL_POSITIVES] = (double)P;
    out[RADAD_EVAL_NEGATIVES] = (double)N;
    out[RADAD_EVAL_ROC_POINTS] = (double)roc_n;
    out[RADAD_EVAL_DISTINCT] = (double)D;
    for (int i = RADAD_EVAL_DISTINCT + 1; i < RADAD_EVAL_OUT_DOUBLES; ++i) out[i] = 0.0;
}

// a scored segment start: the first key of a group that holds both classes (cand<2> left it a candidate index)
__device__ __forceinline__ bool eval_is_scored_start(const EvalCandArgs& p, int i) {
    if (i >= p.n || p.idx[i] == ~0u) return false;
    return i == 0 || eval_key_group(p.keys[i - 1]) != eval_key_group(p.keys[i]);
}

// by group, per tile: how many scored segments start in it
__global__ __launch_bounds__(EVAL_THREADS) void k_eval_seg_count(EvalCandArgs p, u64* __restrict__ tile_tot) {
    __shared__ int s_tot[EVAL_WAVES];
    if (!p.head->multi_group) return;
    const int base = blockIdx.x * EVAL_TILE;
    int tot = 0;
#pragma unroll
    for (int j = 0; j < EVAL_ITEMS; ++j) tot += eval_is_scored_start(p, base + (int)threadIdx.x + j * EVAL_THREADS);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o, 64);
    if ((threadIdx.x & 63) == 0) s_tot[threadIdx.x >> 6] = tot;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = s_tot[0];
        for (int w = 1; w < EVAL_WAVES; ++w) t += s_tot[w];
        tile_tot[blockIdx.x] = (u64)t;
    }
}

// by group: geer[r] <- the EER of the r-th scored segment, segments in sorted order, i.e. ascending group id.  A thread owns
// EVAL_ITEMS consecutive positions; ranks by the scan of k_eval_scan's form over the scored-start flags.
__global__ __launch_bounds__(EVAL_THREADS) void k_eval_seg_eer(EvalCandArgs p, const u64* __restrict__ tile_tot) {
    __shared__ int s_off[EVAL_WAVES], s_wave[EVAL_WAVES];
    if (!p.head->multi_group) return;
    const u64* keys = p.keys;
    const int n = p.n;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int off = 0;
    for (int t = threadIdx.x; t < (int)blockIdx.x; t += EVAL_THREADS) off += (int)tile_tot[t];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) off += __shfl_xor(off, o, 64);
    const int i0 = (int)blockIdx.x * EVAL_TILE + (int)threadIdx.x * EVAL_ITEMS;
    bool mine[EVAL_ITEMS];
    int tot = 0;
#pragma unroll
    for (int j = 0; j < EVAL_ITEMS; ++j) {
        mine[j] = eval_is_scored_start(p, i0 + j);
        tot += mine[j];
    }
    int incl = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    if (lane == 0) s_off[wave] = off;
    __syncthreads();
    int rank = incl - tot;
    for (int w = 0; w < EVAL_WAVES; ++w) {
        rank += s_off[w];
        if (w < wave) rank += s_wave[w];
    }
#pragma unroll
    for (int j = 0; j < EVAL_ITEMS; ++j) {
        if (!mine[j]) continue;
        const int i = i0 + j;
        const int k = (int)p.idx[i];
        const int e = eval_group_end(keys, i, n, eval_key_group(keys[i]));
        const u64 c_s = p.cnt[i];
        const int P = eval_cnt_pos(p.cnt[e]) - eval_cnt_pos(c_s), N = (e - i) - P;
        const int cp = eval_cnt_pos(p.cnt[k]) - eval_cnt_pos(c_s);
        const EvalRates r = eval_rates(cp, (k - i) - cp, P, N);
        p.geer[rank++] = (r.fnr + r.fpr) / 2.0 * 100.0;     // rank < scored segments <= n
    }
}

// the mean of the groups' EERs, added one by one in ascending group id: the workgroup stages 256 of them in LDS, thread 0 adds
__global__ __launch_bounds__(EVAL_THREADS) void k_eval_finish_groups(EvalCandArgs p, const u64* __restrict__ tile_tot, int tiles,
                                                                     double* __restrict__ out) {
    __shared__ int s_tot[EVAL_WAVES];
    __shared__ double s_v[EVAL_THREADS];
    if (!p.head->multi_group) return;
    int G = 0;
    for (int t = threadIdx.x; t < tiles; t += EVAL_THREADS) G += (int)tile_tot[t];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) G += __shfl_xor(G, o, 64);
    if ((threadIdx.x & 63) == 0) s_tot[threadIdx.x >> 6] = G;
    __syncthreads();
    G = 0;
    for (int w = 0; w < EVAL_WAVES; ++w) G += s_tot[w];
    double sum = 0.0;
    for (int c0 = 0; c0 < G; c0 += EVAL_THREADS) {
        const int r = c0 + (int)threadIdx.x;
        s_v[threadIdx.x] = r < G ? p.geer[r] : 0.0;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = min(EVAL_THREADS, G - c0);
            for (int k = 0; k < m; ++k) sum += s_v[k];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const bool ok = G > 0 && p.head->nonfinite == 0;
        out[RADAD_EVAL_MACRO_EER] = ok ? sum / (double)G : __longlong_as_double(0x7ff8000000000000ll);
        out[RADAD_EVAL_GROUPS_SCORED] = p.head->nonfinite == 0 ? (double)G : 0.0;
    }
}

}  // namespace

extern "C" {

int64_t radad_eval_metrics_workspace_bytes(int64_t n, int has_groups) {
    const EvalPlan p = eval_plan(n, has_groups);
    return p.ok ? (int64_t)p.total : -1;
}

int radad_eval_append(const float* logits_dev, const float* labels_dev, const int32_t* group_ids_dev, int64_t n, float pos_weight,
                      int64_t offset, uint64_t* keys_dev, void* acc_dev, int device, void* stream) {
    const char* who = "radad_eval_append";
    RADAD_REQUIRE(n > 0, "%s: n must be at least 1, got %lld", who, (long long)n);
    RADAD_REQUIRE(offset >= 0, "%s: offset %lld is negative", who, (long long)offset);
    RADAD_REQUIRE(n <= RADAD_EVAL_MAX_N && offset <= RADAD_EVAL_MAX_N - n, "%s: offset %lld + n %lld is above the cap of %lld samples",
                  who, (long long)offset, (long long)n, (long long)RADAD_EVAL_MAX_N);
    RADAD_REQUIRE(pos_weight > 0.f, "%s: pos_weight must be positive, got %g", who, (double)pos_weight);
    RADAD_REQUIRE(logits_dev && labels_dev && keys_dev && acc_dev, "%s: NULL buffer", who);
    DeviceGuard g(device);
    hipLaunchKernelGGL(k_eval_append, dim3(1), dim3(EVAL_THREADS), 0, (hipStream_t)stream, logits_dev, labels_dev, group_ids_dev,
                       (int)n, pos_weight, reinterpret_cast<u64*>(keys_dev) + offset, reinterpret_cast<EvalAcc*>(acc_dev));
    RADAD_HIP_CHECK(hipGetLastError());
    return RADAD_OK;
}

int radad_eval_metrics(const uint64_t* keys_dev, int64_t n, int has_groups, const radad_tdcf_consts* consts, double* out_dev,
                       double* roc_dev, double* group_eer_dev, void* ws_dev, int64_t ws_bytes, int device, void* stream) {
    const char* who = "radad_eval_metrics";
    const EvalPlan pl = eval_plan(n, has_groups);
    RADAD_REQUIRE(pl.ok, "%s: n %lld outside 1..%lld", who, (long long)n, (long long)RADAD_EVAL_MAX_N);
    RADAD_REQUIRE(keys_dev && out_dev, "%s: NULL buffer", who);
    RADAD_REQUIRE(ws_dev, "%s: NULL workspace", who);
    RADAD_REQUIRE((reinterpret_cast<uintptr_t>(ws_dev) & 15) == 0, "%s: the workspace must start on a 16-byte boundary", who);
    RADAD_REQUIRE(ws_bytes >= (int64_t)pl.total, "%s: workspace too small (%lld < %lld bytes)", who, (long long)ws_bytes,
                  (long long)pl.total);
    DeviceGuard guard(device);
    hipStream_t st = (hipStream_t)stream;
    char* ws = reinterpret_cast<char*>(ws_dev);
    EvalHead* head = reinterpret_cast<EvalHead*>(ws);
    u64* buf[2] = {reinterpret_cast<u64*>(ws + pl.off_buf[0]), reinterpret_cast<u64*>(ws + pl.off_buf[1])};
    u64* cnt = reinterpret_cast<u64*>(ws + pl.off_cnt);
    u64* best = reinterpret_cast<u64*>(ws + pl.off_best);
    uint32_t* idx = reinterpret_cast<uint32_t*>(ws + pl.off_idx);
    const u64* keys = reinterpret_cast<const u64*>(keys_dev);
    const int ni = (int)n;
    const dim3 grid((unsigned)pl.tiles), block(EVAL_THREADS);
    RADAD_HIP_CHECK(hipMemsetAsync(head, 0, EVAL_WS_HEAD, st));
    for (int sort = 0; sort < pl.sorts; ++sort) {
        const int pooled = sort == 0;
        hipLaunchKernelGGL(k_eval_tile_sort, grid, block, 0, st, keys, ni, pooled ? EVAL_POOLED_MASK : ~(u64)0, pooled, head, buf[0]);
        RADAD_HIP_CHECK(hipGetLastError());
        for (int pass = 0; pass < pl.merge_passes; ++pass) {
            hipLaunchKernelGGL(k_eval_merge, grid, block, 0, st, (const u64*)buf[pass & 1], buf[(pass + 1) & 1], ni,
                               (int)eval_pass_run(pass), pooled, (const EvalHead*)head);
            RADAD_HIP_CHECK(hipGetLastError());
        }
        const u64* sorted = buf[pl.sorted_buf];
        u64* tile_tot = buf[pl.sorted_buf ^ 1];              // the other key buffer is free once the sort is done
        hipLaunchKernelGGL(k_eval_count, grid, block, 0, st, sorted, ni, pooled, head, tile_tot, best, idx);
        RADAD_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_eval_scan, grid, block, 0, st, sorted, ni, pooled, (const EvalHead*)head, (const u64*)tile_tot, cnt);
        RADAD_HIP_CHECK(hipGetLastError());
        EvalCandArgs a{};
        a.keys = sorted; a.n = ni; a.cnt = cnt; a.best = best; a.idx = idx; a.head = head;
        a.has_tc = consts != nullptr;
        if (consts) a.tc = *consts;
        a.roc = pooled ? roc_dev : nullptr;
        a.geer = group_eer_dev ? group_eer_dev : reinterpret_cast<double*>(best);     // best[] is free behind cand<2>
        if (pooled) {
            hipLaunchKernelGGL((k_eval_cand<1, true>), grid, block, 0, st, a);
            RADAD_HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL((k_eval_cand<2, true>), grid, block, 0, st, a);
            RADAD_HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL(k_eval_finish_pooled, dim3(1), dim3(64), 0, st, a, out_dev);
            RADAD_HIP_CHECK(hipGetLastError());
        } else {
            hipLaunchKernelGGL((k_eval_cand<1, false>), grid, block, 0, st, a);
            RADAD_HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL((k_eval_cand<2, false>), grid, block, 0, st, a);
            RADAD_HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL(k_eval_seg_count, grid, block, 0, st, a, tile_tot);
            RADAD_HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL(k_eval_seg_eer, grid, block, 0, st, a, (const u64*)tile_tot);
            RADAD_HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL(k_eval_finish_groups, dim3(1), block, 0, st, a, (const u64*)tile_tot, pl.tiles, out_dev);
            RADAD_HIP_CHECK(hipGetLastError());
        }
    }
    return RADAD_OK;
}

}  // extern "C"
