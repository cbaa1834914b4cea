// ivf.inc -- inverted-file flat index (faiss.IndexIVFFlat with an L2 coarse quantiser, METRIC_L2), the optional
// index type of the reference (vector_database.py:65-70 create, :124-128 train on the first <= 50 000 rows,
// :174-179 nprobe, config.py:76).  Included at the end of knn.hip (same translation unit: it reuses the flat
// store, the register top-k lists and the float64 re-rank).
//
// Layout in HBM: rows in insertion order (reconstruct) + the same rows permuted list-major (`lrows`, with |y|^2 and
// the insertion id of every position) + list offsets.  A search is
//   1. coarse: top-nprobe centroids of every query                  (flat L2 scan over the nlist centroids)
//   2. group the (query, probe) pairs by list, <= qcap queries per task (host, a few thousand ints)
//   3. k_ivf_scan: one workgroup per task streams ITS list once against its queries -- the small-batch streaming
//      kernel (16 rows per step, whole rows in one burst, v_mfma_f32_16x16x4_f32, per-wave register lists);
//      HBM-bound: a batch that touches every list reads the store once
//   4. k_merge_refine over the nprobe lists of each query (float64 re-score, (distance, id) order, id map back to
//      insertion ids)
// The result equals an exact search restricted to the union of the probed lists.  That rests on three things: both list scans are
// FILTERS whose error is bounded per query (eps); k_merge_refine re-scores in float64 everything within 2 eps of the k-th best score
// and certifies the query only when no row the scan did not list can lie in that band; and the queries it cannot certify are
// answered by k_ivf_exact, a float64 scan of their probed lists.  (Until the adversarial tests of tests/test_gpu_ivf_adversarial.py the
// fp32 scan's k + 6 entries per list were merged and re-ranked unchecked: wrong ids wherever more than six rows of a list lie within
// the fp32 error of the k-th.)
//
// Round 4 (k <= 26, dim % 64 == 0): the list scan reads the f16 PLANE of the flat store, gathered list-major (half the bytes, 16x the
// MFMA rate of v_mfma_f32_16x16x4_f32), behind the flat scan's certificate restricted to the probed lists:
//   1. coarse: the centroids are a small fp32 store -- k_knn_dense writes every (query, centroid) score, k_merge_refine<true>
//      selects the nprobe best on its staged copy, re-scores in float64 and certifies (knn.hip)
//   2. grouping as before (one fused single-workgroup kernel for small batches)
//   3. k_ivf_scan_hi: one workgroup per task; the scores of a 256-row chunk against the task's <= 16 queries go to LDS
//      (v_mfma_f32_16x16x32_f16), then a wave per query keeps the k + 6 best of chunk + carry by a 32-step binary search on the
//      score bits (ballot counts; no sorted register lists: with ~250 rows per list nearly every row used to be an insertion)
//   4. k_merge_refine<true> over the nprobe lists of each query with eps(q) of the plane (k_hi_rows): float64 re-score of
//      everything within 2 eps of the k-th, certificate per query (a list whose k + 6 entries are all within the threshold may
//      hide more: rejected)
//   5. rejected queries only: k_ivf_exact -- launched always, its workgroups leave at once when nobody was rejected
// Without a plane (dim % 64 != 0, RADAD_IVF_OPT_HI_SCAN 0): k_ivf_f32_eps, k_ivf_scan, k_merge_refine<false> with that eps, k_ivf_exact.
// Exclusion-aware searches (radad_ivf_search_excl: one set for the batch; radad_ivf_search_excl_pq: one per query) run the same launches
// with the ADM instantiations of the three list kernels behind a bitmap pre-pass: "exclusion inside the list scans", below.
// What a search launches and allocates is decided by ivf_plan.h (host-only: tests/ivf_plan_check.cpp); ivf_search_lists is its glue.
// Range search over the probed lists (radad_ivf_range_search, and among the rows a query does not exclude: radad_ivf_range_search_excl /
// _excl_pq): ivf_plan_range, the k_ivf_range_* kernels and ivf_range_lists, below.
#include "ivf_plan.h"
namespace {

// The admission test of a list kernel (the template parameter ADM):
//   IVF_ADM_NONE    every row is admissible (radad_ivf_search)
//   IVF_ADM_BITMAP  one set for the batch: bit = the row is admissible (radad_ivf_search_excl)
//   IVF_ADM_PQ      one set per query: bit = NO query of the batch excludes the row; a clear bit is decided per (row, query) against
//                   the query's tags (radad_ivf_search_excl_pq, below)
constexpr int IVF_ADM_NONE = 0, IVF_ADM_BITMAP = 1, IVF_ADM_PQ = 2;

// what the IVF_ADM_PQ kernels read beside the suspect bitmap: row r is admissible for query j iff row_tags[r] is not among the first
// clamp(q_cnt[j], 0, m) entries of q_tags[j, :] (q_cnt nullptr = m for every query)
struct IvfPqRule {
    const int64_t* row_tags = nullptr;  // [ntotal] by insertion id
    const int64_t* lids = nullptr;      // [N] insertion id of every list-major position
    const int64_t* q_tags = nullptr;    // [nq, m]
    const int* q_cnt = nullptr;         // [nq] or nullptr
    int m = 0;
    int tag_off = 0;                    // list scans: byte offset of the tag block in LDS (IvfPlan: scan_lds - pq_lds)
};

struct IvfScanParams {
    const float* lrows = nullptr;       // [N, dim] list-major
    const float* lnorm = nullptr;       // [N]
    const int* loff = nullptr;          // [nlist + 1]
    const float* q = nullptr;           // [nq, dim]
    const int* task_list = nullptr;     // [T]
    const int* task_pbeg = nullptr;     // [T] first pair of the task in the list-sorted pair order
    const int* task_cnt = nullptr;      // [T] pairs (queries) of the task, <= qcap
    const int* n_tasks_dev = nullptr;   // [1] T, built on the device: the grid is an upper bound, workgroups beyond T leave
    const int* pair_q = nullptr;        // [nq * nprobe] query of each sorted pair
    const int* pair_slot = nullptr;     // [nq * nprobe] output slot q * nprobe + j of each sorted pair
    int dim = 0, k = 0, qcap = 0;       // qcap: query rows that fit in LDS (16 unless dim is very large)
    float* part_score = nullptr;        // [nq * nprobe, k]
    int* part_idx = nullptr;            // [nq * nprobe, k]  positions in lrows
    const unsigned long long* admit = nullptr;      // FILTERED kernels: the admission bitmap by list-major position (k_admit_bitmap<true>)
    IvfPqRule pq;                                   // IVF_ADM_PQ: the per-query rule (admit is then the suspect bitmap)
};
static_assert(std::is_trivially_copyable_v<IvfScanParams>, "kernel argument");

// ---- exclusion inside the list scans (radad_ivf_search_excl) ---------------------------------------------------------
// The admission bitmap by list-major position (k_admit_bitmap<true> in knn.hip; the rows are reached through lids: position ->
// insertion id).  The array ends with one spare zero word, so that a reader may fetch the word behind any valid position's.
// The FILTERED instantiations of the three list kernels below read it: an excluded row is not part of the universe -- it is never
// emitted, listed or inserted, and it never counts towards a bound.  Bits are indexed by ABSOLUTE position: a list does not start
// on a multiple of 64, nor does a workgroup's share of a split list.
__device__ __forceinline__ bool ivf_admitted(const unsigned long long* __restrict__ admit, int64_t pos) {
    return (admit[pos >> 6] >> (pos & 63)) & 1ull;
}
// bits 0 .. n - 1 (n <= 16) = the admission bits of the positions pos .. pos + n - 1, pos a valid position: they lie in one word or
// in two adjacent ones (the spare word makes the second fetch safe)
__device__ __forceinline__ unsigned ivf_admit_bits(const unsigned long long* __restrict__ admit, int64_t pos, int n) {
    const int sh = (int)(pos & 63);
    unsigned long long w = admit[pos >> 6] >> sh;
    if (sh > 64 - n) w |= admit[(pos >> 6) + 1] << (64 - sh);
    return (unsigned)w & ((1u << n) - 1u);
}
// the padding of the exclusion-aware searches (radad_filter_topk, radad_knn_search_excl): distance NaN where the id is -1
// (k_merge_refine and k_ivf_exact write +inf there)
__global__ __launch_bounds__(256) void k_ivf_pad_nan(float* __restrict__ dist, const int64_t* __restrict__ idx, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && idx[i] < 0) dist[i] = __int_as_float(0x7fc00000);
}

// ---- one exclusion set PER QUERY inside the list scans (radad_ivf_search_excl_pq) ----------------------------------------------------
// The list kernels keep ONE bit per list-major position in their inner loops, fetched where the admission bits are, with a weaker
// meaning: set = no query of the batch excludes the row, clear = SUSPECT, some query may.  A suspect row is decided exactly, per (row,
// query), in a branch: the row's tag (through lids) against the query's tags, staged in LDS per task (ivf_pq_stage) or held across a
// wave's lanes (k_ivf_exact).  Any superset of the truly excluded rows is a correct suspect set, so the pre-pass may err on that side:
//   k_ivf_pq_hash     every live tag (j, t < cnt_j) sets two bits of a power-of-two bitset (ivf_pq_bitset_bits: the size and why)
//   k_ivf_pq_suspect  shaped like k_admit_bitmap<true>: one position per thread, one ballot and one word per wave, the spare word kept;
//                     a position is suspect when both bits of its row's tag are set (positions past the last row come out clear:
//                     the kernels look only at positions inside their list)
// RADAD_IVF_OPT_PQ_FILTER 0 (tests) skips both and clears the bitmap: every position is suspect, every (row, query) decided exactly.
__device__ __forceinline__ unsigned long long ivf_pq_mix(int64_t tag) {      // splitmix64's finaliser: the two halves are the two hashes
    unsigned long long x = (unsigned long long)tag + 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
__global__ __launch_bounds__(256) void k_ivf_pq_hash(const int64_t* __restrict__ q_tags, const int* __restrict__ q_cnt, int64_t nq, int m,
                                                     unsigned* __restrict__ bits, unsigned mask) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nq * m) return;
    const int64_t j = i / m;
    const int cnt = min(max(q_cnt ? q_cnt[j] : m, 0), m);
    if ((int)(i - j * m) >= cnt) return;
    const unsigned long long h = ivf_pq_mix(q_tags[i]);
    const unsigned a = (unsigned)h & mask, b = (unsigned)(h >> 32) & mask;
    atomicOr(&bits[a >> 5], 1u << (a & 31));
    atomicOr(&bits[b >> 5], 1u << (b & 31));
}
__global__ __launch_bounds__(256) void k_ivf_pq_suspect(const int64_t* __restrict__ tags, const int64_t* __restrict__ lids, int64_t n,
                                                        const unsigned* __restrict__ bits, unsigned mask,
                                                        unsigned long long* __restrict__ admit, int64_t n_words) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;          // (whole waves: every lane ballots)
    bool clean = false;
    if (i < n) {
        const unsigned long long h = ivf_pq_mix(tags[lids[i]]);
        const unsigned a = (unsigned)h & mask, b = (unsigned)(h >> 32) & mask;
        clean = !(((bits[a >> 5] >> (a & 31)) & 1u) && ((bits[b >> 5] >> (b & 31)) & 1u));
    }
    const unsigned long long w = __ballot(clean);
    if ((threadIdx.x & 63) == 0 && (i >> 6) < n_words) admit[i >> 6] = w;
}
// the tag block of a list-scan task: [qcap][m] tags of the task's queries (pair_q[pbeg + qq]) and their clamped counts, 0 for the rows
// of the block past the task's count; the caller's __syncthreads makes it visible
__device__ __forceinline__ void ivf_pq_stage(const IvfPqRule& r, char* smem, int qcap, const int* __restrict__ pair_q, int pbeg, int cnt,
                                             int tid, int nthreads) {
    int64_t* sTag = reinterpret_cast<int64_t*>(smem + r.tag_off);
    int* sTc = reinterpret_cast<int*>(sTag + qcap * r.m);
    for (int i = tid; i < qcap * r.m; i += nthreads) {
        const int qq = i / r.m;
        sTag[i] = qq < cnt ? r.q_tags[(int64_t)pair_q[pbeg + qq] * r.m + (i - qq * r.m)] : 0;
    }
    for (int qq = tid; qq < qcap; qq += nthreads) {
        int c = 0;
        if (qq < cnt) { const int pq = pair_q[pbeg + qq]; c = min(max(r.q_cnt ? r.q_cnt[pq] : r.m, 0), r.m); }
        sTc[qq] = c;
    }
}
// a suspect row (list-major position pos, inside the list) against the tags of the task's query qq: true = the query excludes it
__device__ __forceinline__ bool ivf_pq_excludes(const IvfPqRule& r, const char* smem, int qcap, int qq, int64_t pos) {
    const int64_t* sTag = reinterpret_cast<const int64_t*>(smem + r.tag_off);
    const int* sTc = reinterpret_cast<const int*>(sTag + qcap * r.m);
    const int64_t tag = r.row_tags[r.lids[pos]];
    const int c = sTc[qq];
    bool hit = false;
    for (int t = 0; t < c; ++t) hit |= sTag[qq * r.m + t] == tag;
    return hit;
}

// ---- (query, probe) pairs grouped by list, on the device ------------------------------------------------------------
// k_ivf_count: pairs per list.  k_ivf_tasks (one workgroup): exclusive scan -> first sorted position of every list, the
// lists' task ranges (<= qcap pairs per task) and the task table; k_ivf_scatter: every pair takes the next free position of
// its list (the order inside a list varies from run to run; a pair's partial list does not depend on its neighbours in the
// task, so the results do not).  No host round trip: radad_ivf_search used to copy the probes to the host, sort them there
// and upload five tables, with two stream synchronisations per search.
// A probe outside [0, nlist) (the coarse search fills -1 when a query is not finite) takes part in nothing: it is not counted,
// and k_ivf_scatter writes its pair's partial list as empty.
__global__ __launch_bounds__(256) void k_ivf_count(const int64_t* __restrict__ probes, int64_t npairs, int nlist, int* __restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < npairs && (uint64_t)probes[i] < (uint64_t)nlist) atomicAdd(&cnt[(int)probes[i]], 1);
}

// (IVF_TASK_THREADS: ivf_plan.h)
__global__ __launch_bounds__(IVF_TASK_THREADS) void k_ivf_tasks(int* __restrict__ cnt, int nlist, int qcap, int* __restrict__ cursor,
                                                                 int* __restrict__ task_list, int* __restrict__ task_pbeg,
                                                                 int* __restrict__ task_cnt, int* __restrict__ n_tasks) {
    __shared__ int s_p[IVF_TASK_THREADS], s_t[IVF_TASK_THREADS];
    const int tid = threadIdx.x;
    const int per = (nlist + IVF_TASK_THREADS - 1) / IVF_TASK_THREADS;      // consecutive lists per thread
    const int l0 = min(nlist, tid * per), l1 = min(nlist, l0 + per);
    int np = 0, nt = 0;
    for (int l = l0; l < l1; ++l) { const int c = cnt[l]; np += c; nt += (c + qcap - 1) / qcap; }
    s_p[tid] = np; s_t[tid] = nt;
    __syncthreads();
    for (int o = 1; o < IVF_TASK_THREADS; o <<= 1) {                        // inclusive scans of both counts
        const int a = tid >= o ? s_p[tid - o] : 0, b = tid >= o ? s_t[tid - o] : 0;
        __syncthreads();
        s_p[tid] += a; s_t[tid] += b;
        __syncthreads();
    }
    int pb = s_p[tid] - np, tb = s_t[tid] - nt;
    if (tid == IVF_TASK_THREADS - 1) *n_tasks = s_t[tid];
    for (int l = l0; l < l1; ++l) {
        const int c = cnt[l];
        cursor[l] = pb;
        cnt[l] = 0;                      // the counters are zero between searches: no memset launch (three fill kernels, 14 us) in front of k_ivf_count
        for (int b = 0; b < c; b += qcap, ++tb) { task_list[tb] = l; task_pbeg[tb] = pb + b; task_cnt[tb] = min(qcap, c - b); }
        pb += c;
    }
}

__global__ __launch_bounds__(256) void k_ivf_scatter(const int64_t* __restrict__ probes, int64_t npairs, int nprobe, int nlist,
                                                     int* __restrict__ cursor, int* __restrict__ pair_q, int* __restrict__ pair_slot,
                                                     float* __restrict__ part_score, int* __restrict__ part_idx, int ksel) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npairs) return;
    if ((uint64_t)probes[i] < (uint64_t)nlist) {
        const int pos = atomicAdd(&cursor[(int)probes[i]], 1);
        pair_q[pos] = (int)(i / nprobe);
        pair_slot[pos] = (int)i;
    } else {
        for (int j = 0; j < ksel; ++j) { part_score[i * ksel + j] = -INFINITY; part_idx[i * ksel + j] = IDX_SENTINEL; }
    }
}

// ADM == IVF_ADM_PQ: the same four bits are fetched at the same place; a row that passed `sc >= thr` with its bit clear is decided
// there, lazily, by its lane against the tags of the lane's query (r16) -- where IVF_ADM_BITMAP tests the bit.  Only rows the query
// admits are listed and only listed rows set thr, so the per-(query, list) lists hold the best k + 6 rows the QUERY admits, and
// k_merge_refine's certificate (eps over all rows of the probed lists is an upper bound for the admitted ones) holds as it stands.
template <int KSEL, int ADM>
__device__ __forceinline__ void ivf_scan_task(const IvfScanParams& p, const int task, char* smem) {
    constexpr bool FILTERED = ADM != IVF_ADM_NONE;
    const int qld = p.dim + 4;
    float* sQ = reinterpret_cast<float*>(smem);                   // [qcap][dim + 4] (rows past the task's count are zero)
    float2* sCand = reinterpret_cast<float2*>(sQ + p.qcap * qld); // [4 waves][16][SQ_SLOTS]; later 3 x 16 x KSEL keys
    int* sCnt = reinterpret_cast<int*>(sCand + 4 * SQ_NQ * 24);   // [4 waves][16]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int list = p.task_list[task], pbeg = p.task_pbeg[task], cnt = p.task_cnt[task];
    for (int i = tid; i < p.qcap * (p.dim >> 2); i += SQ_THREADS) {
        const int qq = i / (p.dim >> 2), c4 = i % (p.dim >> 2);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (qq < cnt) v = *reinterpret_cast<const f32x4*>(p.q + (int64_t)p.pair_q[pbeg + qq] * p.dim + c4 * 4);
        *reinterpret_cast<f32x4*>(sQ + qq * qld + c4 * 4) = v;
    }
    if (tid < 4 * SQ_NQ) sCnt[tid] = 0;
    if constexpr (ADM == IVF_ADM_PQ) ivf_pq_stage(p.pq, smem, p.qcap, p.pair_q, pbeg, cnt, tid, SQ_THREADS);
    __syncthreads();

    const int64_t l_begin = p.loff[list], l_end = p.loff[list + 1];
    const int64_t per_wave = ((l_end - l_begin + 4 * 16 - 1) / (4 * 16)) * 16;      // 16-row steps, 4 waves
    const int64_t w_begin = l_begin + wave * per_wave;
    const int64_t w_end = min(w_begin + per_wave, l_end);
    float2* myCand = sCand + wave * SQ_NQ * SQ_SLOTS;
    int* myCnt = sCnt + wave * SQ_NQ;

    const u64 SENT = pack_key(-INFINITY, IDX_SENTINEL);
    u64 lst[KSEL];
#pragma unroll
    for (int j = 0; j < KSEL; ++j) lst[j] = SENT;
    float thr = -INFINITY;
    const float* qrow = sQ + min(r16, p.qcap - 1) * qld + 4 * g;      // columns >= cnt are ignored below
    const int nkb = p.dim >> 5;

    for (int64_t row0 = w_begin; row0 < w_end; row0 += 16) {
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        const int64_t ra = min(row0 + r16, l_end - 1);
        const float* pa = p.lrows + ra * p.dim + 4 * g;
        unsigned adm = 0xfu;                                            // FILTERED: bit e = row row0 + 4 g + e is admissible (read ahead of the products;
        if constexpr (FILTERED)                                         // rows past w_end are not emitted whatever their bit says)
            adm = row0 + 4 * g < w_end ? ivf_admit_bits(p.admit, row0 + 4 * g, 4) : 0u;
        constexpr int PKB = KSEL <= 16 ? 16 : 8;
        for (int kp = 0; kp < nkb; kp += PKB) {
            const int nb = min(PKB, nkb - kp);
            f32x4 v[2 * PKB];
#pragma unroll
            for (int kb = 0; kb < PKB; ++kb)
                if (kb < nb) {
                    v[2 * kb] = *reinterpret_cast<const f32x4*>(pa + (kp + kb) * 32);
                    v[2 * kb + 1] = *reinterpret_cast<const f32x4*>(pa + (kp + kb) * 32 + 16);
                }
#pragma unroll
            for (int kb = 0; kb < PKB; ++kb)
                if (kb < nb) {
                    const f32x4 q0 = *reinterpret_cast<const f32x4*>(qrow + (kp + kb) * 32);
                    const f32x4 q1 = *reinterpret_cast<const f32x4*>(qrow + (kp + kb) * 32 + 16);
                    if (kb & 1) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(v[2 * kb][j], q0[j], acc1, 0, 0, 0);
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(v[2 * kb + 1][j], q1[j], acc1, 0, 0, 0);
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(v[2 * kb][j], q0[j], acc0, 0, 0, 0);
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(v[2 * kb + 1][j], q1[j], acc0, 0, 0, 0);
                    }
                }
        }
        bool any = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t row = row0 + 4 * g + e;
            const float sc = 2.f * (acc0[e] + acc1[e]) - p.lnorm[min(row, l_end - 1)];     // L2: rank by 2 q.y - |y|^2
            // (FILTERED: admission is tested HERE, where rows enter the lists -- thr is -inf until a list is full, so a score of -inf
            // would still be inserted; and only listed rows set thr, so an excluded row never counts towards it)
            // (IVF_ADM_PQ: a clear bit is a suspect row -- decided here, for this lane's query, only when the row would enter its list)
            if (row < w_end && r16 < cnt && sc >= thr &&
                (!FILTERED || ((adm >> e) & 1u) || (ADM == IVF_ADM_PQ && !ivf_pq_excludes(p.pq, smem, p.qcap, r16, row)))) {
                const int sl = atomicAdd(&myCnt[r16], 1);
                myCand[r16 * SQ_SLOTS + sl] = make_float2(sc, __int_as_float((int)row));
                any = true;
            }
        }
        if (__any(any)) {
            if (lane < SQ_NQ) {
                const int c = myCnt[lane];
                for (int i = 0; i < c; ++i) {
                    const float2 cv = myCand[lane * SQ_SLOTS + i];
                    list_insert<KSEL>(lst, pack_key(cv.x, __float_as_int(cv.y)));
                }
                myCnt[lane] = 0;
            }
            thr = __shfl(key_score(lst[KSEL - 1]), r16, 64);
        }
    }
    __syncthreads();
    u64* sKeys = reinterpret_cast<u64*>(sCand);
    if (wave > 0 && lane < SQ_NQ) {
#pragma unroll
        for (int j = 0; j < KSEL; ++j) sKeys[((wave - 1) * SQ_NQ + lane) * KSEL + j] = lst[j];
    }
    __syncthreads();
    if (wave == 0 && lane < cnt) {
        for (int w = 0; w < 3; ++w)
            for (int j = 0; j < KSEL; ++j) list_insert<KSEL>(lst, sKeys[(w * SQ_NQ + lane) * KSEL + j]);
        const int slot = p.pair_slot[pbeg + lane];
        float* ls = p.part_score + (int64_t)slot * p.k;
        int* li = p.part_idx + (int64_t)slot * p.k;
#pragma unroll
        for (int j = 0; j < KSEL; ++j)
            if (j < p.k) { ls[j] = key_score(lst[j]); li[j] = key_id(lst[j]); }
    }
}

// One workgroup per task.
template <int KSEL, int ADM>
__global__ __launch_bounds__(SQ_THREADS, 2) void k_ivf_scan(IvfScanParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if ((int)blockIdx.x < *p.n_tasks_dev) ivf_scan_task<KSEL, ADM>(p, blockIdx.x, smem);
}

// ---- grouping of a SMALL batch in one launch (npairs <= IVG_MAX_PAIRS, nlist <= IVG_MAX_LISTS): count, scan, task table and
// scatter by one workgroup with the per-list counters in LDS (memset + k_ivf_count + k_ivf_tasks + k_ivf_scatter are four
// dependent launches of ~5 us each, most of a one-query search)
// (IVG_MAX_PAIRS, IVG_MAX_LISTS: ivf_plan.h)
__global__ __launch_bounds__(IVF_TASK_THREADS) void k_ivf_group_small(const int64_t* __restrict__ probes, int npairs, int nprobe, int nlist, int qcap,
                                                                     int* __restrict__ task_list, int* __restrict__ task_pbeg, int* __restrict__ task_cnt,
                                                                     int* __restrict__ n_tasks, int* __restrict__ pair_q, int* __restrict__ pair_slot,
                                                                     float* __restrict__ part_score, int* __restrict__ part_idx, int ksel) {
    extern __shared__ int s_cnt[];                                          // [nlist] counts, then cursors
    __shared__ int s_p[IVF_TASK_THREADS], s_t[IVF_TASK_THREADS];
    const int tid = threadIdx.x;
    for (int l = tid; l < nlist; l += IVF_TASK_THREADS) s_cnt[l] = 0;
    __syncthreads();
    for (int i = tid; i < npairs; i += IVF_TASK_THREADS)
        if ((uint64_t)probes[i] < (uint64_t)nlist) atomicAdd(&s_cnt[(int)probes[i]], 1);
    __syncthreads();
    const int per = (nlist + IVF_TASK_THREADS - 1) / IVF_TASK_THREADS;
    const int l0 = min(nlist, tid * per), l1 = min(nlist, l0 + per);
    int np = 0, nt = 0;
    for (int l = l0; l < l1; ++l) { const int c = s_cnt[l]; np += c; nt += (c + qcap - 1) / qcap; }
    s_p[tid] = np; s_t[tid] = nt;
    __syncthreads();
    for (int o = 1; o < IVF_TASK_THREADS; o <<= 1) {
        const int a = tid >= o ? s_p[tid - o] : 0, b = tid >= o ? s_t[tid - o] : 0;
        __syncthreads();
        s_p[tid] += a; s_t[tid] += b;
        __syncthreads();
    }
    int pb = s_p[tid] - np, tb = s_t[tid] - nt;
    if (tid == IVF_TASK_THREADS - 1) *n_tasks = s_t[tid];
    for (int l = l0; l < l1; ++l) {
        const int c = s_cnt[l];
        s_cnt[l] = pb;                                                       // (this thread's lists only: the cursor replaces the count)
        for (int b = 0; b < c; b += qcap, ++tb) { task_list[tb] = l; task_pbeg[tb] = pb + b; task_cnt[tb] = min(qcap, c - b); }
        pb += c;
    }
    __syncthreads();
    for (int i = tid; i < npairs; i += IVF_TASK_THREADS) {
        if ((uint64_t)probes[i] < (uint64_t)nlist) {
            const int pos = atomicAdd(&s_cnt[(int)probes[i]], 1);
            pair_q[pos] = i / nprobe;
            pair_slot[pos] = i;
        } else {
            for (int j = 0; j < ksel; ++j) { part_score[(int64_t)i * ksel + j] = -INFINITY; part_idx[(int64_t)i * ksel + j] = IDX_SENTINEL; }
        }
    }
}

// ---- the f16 plane of the flat store, list-major -------------------------------------------------------------------------------
// position pos of the list-major order holds insertion id ids[pos]: its plane row, per-row scale and bias travel with it
__global__ __launch_bounds__(256) void k_ivf_gather_plane(const _Float16* __restrict__ hi, const float* __restrict__ rscale, const float* __restrict__ rbias,
                                                          const int64_t* __restrict__ ids, int64_t n, int dim, _Float16* __restrict__ lhi,
                                                          float* __restrict__ lscale, float* __restrict__ lbias) {
    const int lane = threadIdx.x & 63;
    const int64_t pos = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pos >= n) return;
    const int64_t src = ids[pos];
    const f16x8* a = reinterpret_cast<const f16x8*>(hi + src * dim);
    f16x8* b = reinterpret_cast<f16x8*>(lhi + pos * dim);
    for (int i = lane; i < (dim >> 3); i += 64) b[i] = a[i];
    if (lane == 0) {
        if (lscale) lscale[pos] = rscale[src];
        lbias[pos] = rbias[src];
    }
}

struct IvfHiParams {
    const _Float16* lhi = nullptr; // [N][dim] list-major f16 plane
    const float* lscale = nullptr; // [N] per-row scale, or nullptr: uscale for every row
    float uscale = 1.f;
    const float* lbias = nullptr;  // [N] |y'|^2 of the plane's operand (y' = y - mu when the plane is centred)
    const int* loff = nullptr;     // [nlist + 1]
    const _Float16* qh = nullptr;  // [nq][dim] f16 queries (k_hi_rows: scaled per query, centred as the plane)
    const float* qscale = nullptr; // [nq]
    const float* qconst = nullptr; // [nq] -|q'|^2
    const float* eps = nullptr;    // [nq] error bound of the scores
    const int* task_list = nullptr; const int* task_pbeg = nullptr; const int* task_cnt = nullptr; const int* n_tasks_dev = nullptr; const int* pair_q = nullptr;
    int dim = 0, k = 0, qcap = 0;  // k: neighbours asked for (<= 26: the carry holds 32 entries)
    int split = 1;                 // workgroups per task: each takes 1/split of the list's rows (few tasks: a one-query search has nprobe of them)
    unsigned* gbound = nullptr;    // [nq] running lower bound of a_k (the k-th best score over the query's lists) as an ordered key, 0 at launch
    int* cand_cnt = nullptr;       // [nq] entries emitted, 0 at launch; more than cand_cap = overflow (k_merge_refine rejects the query)
    int cand_cap = 0;
    float* cand_score = nullptr;   // [nq][cand_cap]
    int* cand_idx = nullptr;       // [nq][cand_cap] positions in the list-major order
    const unsigned long long* admit = nullptr;      // FILTERED: the admission bitmap by list-major position (k_admit_bitmap<true>)
    IvfPqRule pq;                                   // IVF_ADM_PQ: the per-query rule (admit is then the suspect bitmap)
};
static_assert(std::is_trivially_copyable_v<IvfHiParams>, "kernel argument");

// (IVH_CHUNK, IVH_SLD, IVH_CAND_CAP, IVH_CAND_CAP_SMALLQ, ivf_hi_lds_bytes: ivf_plan.h)
static_assert(sizeof(_Float16) == 2, "ivf_plan.h sizes the f16 queries (ivf_hi_lds_bytes, the qbuf layout) with this as a literal");

// EMIT mode, as the certified tile scan of the flat store: what leaves the kernel is, per query, every row of its probed lists whose
// score is >= b - 2 eps for some lower bound b of a_k.  A per-(query, list) top-(k + 6) list -- the first version -- was rejected for
// half the queries of a clustered store: the ~250 rows of a query's own cluster lie within 2 eps of each other (eps is a
// Cauchy-Schwarz bound, |q'||y'| 2^-11: ~6 on scores whose neighbours differ by ~1), so all k + 6 entries were within the threshold and
// the list "may hide more".  b = max(the k-th best score of THIS list so far, the largest such value any workgroup of the query has
// published): both are reached by k rows of the probed lists, so b <= a_k and nothing the certificate needs is left out; a far
// list emits its own ~k + few best at most, nothing once the home list has published.
// FILTERED (radad_ivf_search_excl): the rows whose admission bit is clear do not exist.  Two things must hold, and a score of -inf
// gives neither: an excluded row is never EMITTED (while no bound is published the threshold is -inf and `score >= thr` passes
// everything; k_merge_refine would re-score the row from lrows and return it whenever fewer than k admissible rows are listed), and
// it never COUNTS towards a bound (it takes KEY_NONE in the selection, like a row past l_end: the K-th best key, the carry and the
// published gbound are reached by K admissible rows, so b <= a_k of the admissible rows and the certificate holds as it stands).
// A NaN score gives both (see the chunk loop).
// IVF_ADM_PQ (radad_ivf_search_excl_pq): both arguments hold PER QUERY.  The score tile is [query][row]; the NaN goes to the entries
// (row, query) whose query excludes the row and to no other, so for every query a row it excludes is never emitted and never counts
// towards its K-th best, its carry or gbound[q] -- each is reached by K rows that query q admits, b <= a_k of q's admissible rows.
// The 16 bits are fetched as before; when all are set nothing else happens, otherwise (wave-uniform branch) the lane speaking for
// (query r16, row 4 g + e) decides its suspect rows against the query's tags in LDS.  k_merge_refine needs no change: every emitted
// row is admissible for its query, and eps over all rows of the probed lists is an upper bound for the admitted ones.
template <int ADM>
__global__ __launch_bounds__(SQ_THREADS, 4) void k_ivf_scan_hi(IvfHiParams p) {
    constexpr bool FILTERED = ADM != IVF_ADM_NONE;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int qld = p.dim + 8;
    _Float16* sQ = reinterpret_cast<_Float16*>(smem);                          // [qcap][dim + 8]
    float* sS = reinterpret_cast<float*>(sQ + p.qcap * qld);                    // [16][IVH_SLD] scores of the chunk
    float* sCs = sS + SQ_NQ * IVH_SLD;                                          // [16][32] carry: the k best of the list so far ...
    int* sCi = reinterpret_cast<int*>(sCs + SQ_NQ * 32);                        // ... (positions; only the scores are used again)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int task0 = blockIdx.x / p.split, sub = blockIdx.x % p.split;
    const int n_tasks = *p.n_tasks_dev;
    if (task0 >= n_tasks) return;                                              // (uniform per workgroup)
    const int list = p.task_list[task0];
    // (a list probed by more than qcap queries has several tasks, one workgroup each: they re-read the list -- 1.2 GB streamed for
    // 0.92 GB of lists on the 1024-query benchmark -- but taking a list's tasks in turn in ONE workgroup serialises the benchmark's hub
    // lists, 64 tasks each: 0.98 ms instead of 0.29, 0.45 with four tasks per workgroup)
    int64_t l_begin = p.loff[list], l_end = p.loff[list + 1];
    if (p.split > 1) {                                                         // this workgroup's share of the list: whole 16-row steps
        const int64_t len = ((l_end - l_begin + p.split - 1) / p.split + 15) / 16 * 16;
        l_begin += sub * len;
        l_end = min(l_end, l_begin + len);
        if (l_begin >= l_end) return;
    }
  {
    const int task = task0;
    const int pbeg = p.task_pbeg[task], cnt = p.task_cnt[task];
    for (int i = tid; i < p.qcap * (p.dim >> 3); i += SQ_THREADS) {
        const int qq = i / (p.dim >> 3), c8 = i % (p.dim >> 3);
        f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (qq < cnt) v = *reinterpret_cast<const f16x8*>(p.qh + (int64_t)p.pair_q[pbeg + qq] * p.dim + c8 * 8);
        *reinterpret_cast<f16x8*>(sQ + qq * qld + c8 * 8) = v;
    }
    for (int i = tid; i < SQ_NQ * 32; i += SQ_THREADS) { sCs[i] = -INFINITY; sCi[i] = IDX_SENTINEL; }
    if constexpr (ADM == IVF_ADM_PQ) ivf_pq_stage(p.pq, smem, p.qcap, p.pair_q, pbeg, cnt, tid, SQ_THREADS);
    const int pq = r16 < cnt ? p.pair_q[pbeg + r16] : 0;
    const float qs = r16 < cnt ? p.qscale[pq] * 2.f : 0.f;
    const float qc = r16 < cnt ? p.qconst[pq] : 0.f;
    // lane i < 4 of a wave speaks for the wave's i-th query (wave + 4 i) in the selection below
    int my_qid = -1;
    float my_eps = 0.f;
    unsigned my_gb = 0;
    if (lane < 4 && wave + 4 * lane < cnt) {
        my_qid = p.pair_q[pbeg + wave + 4 * lane];
        my_eps = p.eps[my_qid];
        my_gb = __builtin_nontemporal_load(&p.gbound[my_qid]);
    }
    __syncthreads();

    const _Float16* qrow = sQ + min(r16, p.qcap - 1) * qld + 8 * g;
    const int nkb = p.dim >> 5;
    const int K = p.k;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const unsigned KEY_NONE = 0x007fffffu;                                      // key of -inf: "no such row"
    for (int64_t chunk0 = l_begin; chunk0 < l_end; chunk0 += IVH_CHUNK) {
#pragma unroll 1
        for (int s4 = 0; s4 < 4; ++s4) {
            const int64_t row0 = chunk0 + 16 * (4 * s4 + wave);                   // (steps dealt round-robin: a short range occupies all four waves)
            f32x4 out = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            if (row0 < l_end) {                                                  // (wave-uniform)
                f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
                const int64_t ra = min(row0 + r16, l_end - 1);
                const _Float16* pa = p.lhi + ra * p.dim + 8 * g;
                // FILTERED: bit r = row row0 + r of the step is admissible.  The 16 bits lie in one or two consecutive words at
                // wave-uniform addresses (ABSOLUTE positions: neither a list nor a workgroup's share of a split list starts on a multiple
                // of 64; the bitmap ends with a spare word).  They are fetched ahead of the products and used behind them.
                unsigned abits = 0xffffu;
                if constexpr (FILTERED) abits = ivf_admit_bits(p.admit, chunk0 + 16 * (4 * s4 + __builtin_amdgcn_readfirstlane(wave)), 16);
                float rs[4], yb[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int64_t row = min(row0 + 4 * g + e, l_end - 1);
                    rs[e] = p.lscale ? p.lscale[row] : p.uscale;
                    yb[e] = qc - p.lbias[row];
                }
                // (FILTERED: 8 row fragments in flight instead of 16.  The unfiltered kernel uses all of the 128 VGPRs that four
                // workgroups per CU leave; with the admission bits pending across the products the compiler's resource report for 16
                // fragments was 128 VGPRs + 4 spilled, 20 bytes of scratch per lane -- whether the bits were read here, behind the
                // products, or patched into the score tile behind a second barrier.  With 8 it is 104 VGPRs and no scratch.  What the
                // shallower prefetch costs at dim 512 is for tools/bench_ivf.py's excl_ms leg to say: profiles/README.md.)
                constexpr int HKB = FILTERED ? 8 : 16;
                for (int kp = 0; kp < nkb; kp += HKB) {
                    const int nb = min(HKB, nkb - kp);
                    f16x8 v[HKB];
#pragma unroll
                    for (int kb = 0; kb < HKB; ++kb)
                        if (kb < nb) v[kb] = *reinterpret_cast<const f16x8*>(pa + (kp + kb) * 32);
#pragma unroll
                    for (int kb = 0; kb < HKB; ++kb)
                        if (kb < nb) {
                            const f16x8 b = *reinterpret_cast<const f16x8*>(qrow + (kp + kb) * 32);
                            if (kb & 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(v[kb], b, acc1, 0, 0, 0);
                            else acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(v[kb], b, acc0, 0, 0, 0);
                        }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (row0 + 4 * g + e < l_end) {
                        out[e] = fmaf((acc0[e] + acc1[e]) * rs[e], qs, yb[e]);
                        // an excluded row's score is NaN, this kernel's "no such row" in both places that matter: the selection gives
                        // it KEY_NONE (it counts towards no K-th best, carry or gbound), and `score >= thr` is false for it whatever
                        // thr is, -inf included (it is never emitted)
                        if constexpr (ADM == IVF_ADM_BITMAP) { if (!((abits >> (4 * g + e)) & 1u)) out[e] = __int_as_float(0x7fc00000); }
                    }
                // IVF_ADM_PQ: a step without a suspect row is done.  Otherwise the same NaN, per (row, query): this lane's query
                // (r16; a query row past the task's count has no tags) against its suspect rows of the step.  The bits behind l_end
                // belong to the next list or to no row: they are not looked at.
                if constexpr (ADM == IVF_ADM_PQ) {
                    if (abits != 0xffffu) {                                       // (wave-uniform)
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (row0 + 4 * g + e < l_end && !((abits >> (4 * g + e)) & 1u) &&
                                ivf_pq_excludes(p.pq, smem, p.qcap, min(r16, p.qcap - 1), row0 + 4 * g + e))
                                out[e] = __int_as_float(0x7fc00000);
                    }
                }
            }
            *reinterpret_cast<f32x4*>(sS + r16 * IVH_SLD + 16 * (4 * s4 + wave) + 4 * g) = out;      // row 4 g + e of the step, query r16
        }
        __syncthreads();
        const bool more = chunk0 + IVH_CHUNK < l_end;                            // (uniform) the list goes on: keep its k best for the next chunk
        // One wave per query, four queries per wave (qq = wave + 4 i).  Everything that waits for global memory -- the bound's
        // atomicMax, the slot reservation's atomicAdd -- is issued ONCE per wave, lane i acting for query i: the first version
        // went to memory four times per query in turn (bound, eps, atomicMax, atomicAdd: ~15 us of round trips per chunk).
        unsigned my_t = 0;                                                       // lane i: the K-th best key of query i
#pragma unroll 1
        for (int i = 0; i < 4; ++i) {
            const int qq = wave + 4 * i;
            if (qq >= cnt) break;                                                // (uniform)
            const f32x4 sv = *reinterpret_cast<const f32x4*>(sS + qq * IVH_SLD + 4 * lane);
            float v[5];
            int id[5];
            unsigned u[5];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t row = chunk0 + 4 * lane + j;
                v[j] = sv[j];
                id[j] = row < l_end ? (int)row : IDX_SENTINEL;
            }
            v[4] = lane < 32 ? sCs[qq * 32 + lane] : -INFINITY;
            id[4] = lane < 32 ? sCi[qq * 32 + lane] : IDX_SENTINEL;
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const unsigned b = __float_as_uint(v[j]);
                u[j] = (b & 0x80000000u) ? ~b : (b | 0x80000000u);            // order-preserving image of the float
                if (id[j] == IDX_SENTINEL || v[j] != v[j]) u[j] = KEY_NONE;      // (no row; a NaN score is no candidate)
            }
            unsigned t = 0;                                                       // the K-th largest key: the largest t with |{u >= t}| >= K
#pragma unroll 1
            for (int bit = 31; bit >= 0; --bit) {
                const unsigned cand = t | (1u << bit);
                int c = 0;
#pragma unroll
                for (int j = 0; j < 5; ++j) c += __popcll(__ballot(u[j] >= cand));
                if (c >= K) t = cand;
            }
            if (lane == i) my_t = t;
            if (more) {                                                          // carry := the K best of chunk + carry (ties of the K-th up to K entries)
                int cb = 0;
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    const unsigned long long mm = __ballot(u[j] > t);
                    if (u[j] > t) { const int pos = cb + __popcll(mm & lt_mask); sCs[qq * 32 + pos] = v[j]; sCi[qq * 32 + pos] = id[j]; }
                    cb += __popcll(mm);
                }
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    const unsigned long long mm = __ballot(u[j] == t);
                    if (u[j] == t) { const int pos = cb + __popcll(mm & lt_mask); if (pos < K) { sCs[qq * 32 + pos] = v[j]; sCi[qq * 32 + pos] = id[j]; } }
                    cb += __popcll(mm);
                }
                // (what is left of the previous carry beyond the new one must go: a row counted twice would raise the bound above a_k)
                for (int pos = min(cb, K) + lane; pos < 32; pos += 64) { sCs[qq * 32 + pos] = -INFINITY; sCi[qq * 32 + pos] = IDX_SENTINEL; }
            }
        }
        // b = max(own K-th best, what the query's other workgroups had published when this task began); publish the own one
        float my_thr = -INFINITY;
        if (lane < 4 && my_qid >= 0) {
            const unsigned t = my_t;
            if (t > KEY_NONE) {
                if (t > my_gb) atomicMax(&p.gbound[my_qid], t);
                my_gb = max(my_gb, t);
            }
            if (my_gb > KEY_NONE) {
                const unsigned fb = (my_gb & 0x80000000u) ? (my_gb & 0x7fffffffu) : ~my_gb;
                my_thr = __uint_as_float(fb) - 2.f * my_eps;
            }
        }
        // the chunk's rows >= thr (the carry's were emitted with their own chunk): count, reserve the slots (lane i for query i), write
        int my_tot = 0;
#pragma unroll 1
        for (int i = 0; i < 4; ++i) {
            const int qq = wave + 4 * i;
            if (qq >= cnt) break;
            const float thr = __shfl(my_thr, i, 64);
            const f32x4 sv = *reinterpret_cast<const f32x4*>(sS + qq * IVH_SLD + 4 * lane);
            int tot = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) tot += __popcll(__ballot(chunk0 + 4 * lane + j < l_end && sv[j] >= thr));
            if (lane == i) my_tot = tot;
        }
        int my_base = 0;
        if (lane < 4 && my_qid >= 0 && my_tot > 0) my_base = atomicAdd(&p.cand_cnt[my_qid], my_tot);
#pragma unroll 1
        for (int i = 0; i < 4; ++i) {
            const int qq = wave + 4 * i;
            if (qq >= cnt) break;
            if (__shfl(my_tot, i, 64) == 0) continue;                            // (uniform)
            int base = __shfl(my_base, i, 64);
            const int qid = __shfl(my_qid, i, 64);
            const float thr = __shfl(my_thr, i, 64);
            const f32x4 sv = *reinterpret_cast<const f32x4*>(sS + qq * IVH_SLD + 4 * lane);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool on = chunk0 + 4 * lane + j < l_end && sv[j] >= thr;
                const unsigned long long mj = __ballot(on);
                if (on) {
                    const int slot = base + __popcll(mj & lt_mask);
                    if (slot < p.cand_cap) { p.cand_score[(int64_t)qid * p.cand_cap + slot] = sv[j]; p.cand_idx[(int64_t)qid * p.cand_cap + slot] = (int)(chunk0 + 4 * lane + j); }
                }
                base += __popcll(mj);
            }
        }
        __syncthreads();
    }
  }
}

// k-means update: centroid c = mean of the (list-sorted) training rows [off[c], off[c+1]); empty clusters keep theirs
__global__ __launch_bounds__(256) void k_centroid_update(const float* __restrict__ sorted_rows, const int* __restrict__ off, int dim,
                                                         float* __restrict__ centroids) {
    const int c = blockIdx.x;
    const int col = blockIdx.y * 256 + threadIdx.x;
    if (col >= dim) return;
    const int a = off[c], b = off[c + 1];
    if (b == a) return;
    float v = 0.f;
    for (int r = a; r < b; ++r) v += sorted_rows[(int64_t)r * dim + col];
    centroids[(int64_t)c * dim + col] = v / (float)(b - a);
}

// ---- the certificate of the fp32 list scan ---------------------------------------------------------------------------------------
// k_ivf_scan ranks by a = fl(2 fl(q.y) - fl(|y|^2)).  With S = sum |q_i y_i| <= |q||y|: the two MFMA accumulators sum dim products in
// dim / 8 steps of four each and are added once; |y|^2 is an fp32 sum of dim squares; one subtraction forms a.  Charging EVERY product
// and addition a relative error of 2^-23 (twice the unit roundoff: the matrix core's internal additions need not round to nearest), any
// order of summation gives |a - (2 q.y - |y|^2)| <= (dim + 16) 2^-23 (2 |q||y| + |y|^2).  eps(q) takes the largest |y| of the query's
// probed lists (lmax: per list, k_ivf_list_maxnorm at the layout's rebuild), so one huge row costs its own list's queries only.
__global__ __launch_bounds__(256) void k_ivf_list_maxnorm(const float* __restrict__ lnorm, const int* __restrict__ loff, float* __restrict__ lmax) {
    __shared__ float s_m[4];
    const int l = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float m = 0.f;
    for (int r = loff[l] + threadIdx.x; r < loff[l + 1]; r += 256) m = fmaxf(m, lnorm[r]);
    m = wave_max(m);
    if (lane == 0) s_m[wave] = m;
    __syncthreads();
    if (threadIdx.x == 0) lmax[l] = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
}

// one wave per query; the first thread also clears the search's 8 counters (k_hi_rows does that on the f16 route)
__global__ __launch_bounds__(256) void k_ivf_f32_eps(const float* __restrict__ q, int64_t nq, int dim, const int64_t* __restrict__ probes, int nprobe,
                                                     int nlist, const float* __restrict__ lmax, float* __restrict__ eps, int* __restrict__ counters) {
    const int lane = threadIdx.x & 63;
    const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (blockIdx.x == 0 && threadIdx.x == 0) { for (int i = 0; i < 8; ++i) counters[i] = 0; }
    if (qi >= nq) return;
    float ss = 0.f, ym = 0.f;
    for (int i = lane; i < dim; i += 64) { const float v = q[qi * dim + i]; ss = fmaf(v, v, ss); }
    for (int j = lane; j < nprobe; j += 64) {
        const int64_t l = probes[qi * nprobe + j];
        if ((uint64_t)l < (uint64_t)nlist) ym = fmaxf(ym, lmax[l]);
    }
    ss = wave_sum(ss); ym = wave_max(ym);
    if (lane == 0) eps[qi] = (float)(dim + 16) * 1.1920929e-07f * 1.01f * (2.f * sqrtf(ss) * sqrtf(ym) + ym);      // (1.01: ss, ym and this line are fp32 too)
}

// ---- exact float64 scan of the probed lists, for the queries a certificate rejected ------------------------------------------
// Driven from the device as k_exact_scan is: *count rejected queries, their indices in sel (nullptr: slot s is query s); nobody
// rejected = every workgroup leaves at once.  A workgroup takes (rejected query, probe) pairs in turn: its 8 waves walk the list four
// rows at a time, sum (q - y)^2 in float64 (lanes across the row, butterfly), and keep the k best by (distance, insertion id) as a
// sorted list ACROSS the wave's lanes (lane e holds entry e: k <= 26); the waves' lists are ranked into the pair's partial list, and
// the workgroup that arrives last for a query (device-scope counter) merges the nprobe partial lists and overwrites the query's
// output rows.  Keys are minus the squared distance: larger is better.
// (IVX_THREADS, IVX_WAVES, IVX_MAX_GRID, IVX_PART_BUDGET, ivf_exact_lds_bytes: ivf_plan.h)
constexpr int IVX_ROWS = 4;                              // rows of a wave in flight
constexpr int64_t IVX_NO_ID = INT64_MAX;

struct IvfExactParams {
    const float* lrows = nullptr;      // [N, dim] list-major
    const int64_t* lids = nullptr;     // [N] insertion id of every position
    const int* loff = nullptr;         // [nlist + 1]
    const float* q = nullptr;          // [nq, dim]
    const int64_t* probes = nullptr;   // [nq, nprobe] lists; outside [0, nlist) = none
    const int* sel = nullptr;
    const int* count = nullptr;
    int* done = nullptr;               // [1] queries answered here (statistics: radad_ivf_last_search_counts)
    int dim = 0, k = 0, nprobe = 0, nlist = 0;
    int slot0 = 0, nslots = 0;         // this launch's rejected queries: slots slot0 .. slot0 + nslots
    double* pkey = nullptr;            // [nslots][nprobe][k]
    int64_t* pid = nullptr;
    int* arrive = nullptr;             // [nslots] arrival counters (zero between launches: the last arrival resets its own)
    float* out_dist = nullptr; int64_t* out_idx = nullptr;
    const unsigned long long* admit = nullptr;      // FILTERED: the admission bitmap by list-major position (k_admit_bitmap<true>)
    IvfPqRule pq;                                   // IVF_ADM_PQ: the per-query rule (admit is then the suspect bitmap)
};
static_assert(std::is_trivially_copyable_v<IvfExactParams>, "kernel argument");

__device__ __forceinline__ bool ivx_better(double ka, int64_t ia, double kb, int64_t ib) { return ka > kb || (ka == kb && ia < ib); }

// FILTERED (radad_ivf_search_excl): a row whose admission bit is clear is skipped before the insertion test.
// IVF_ADM_PQ (radad_ivf_search_excl_pq): a pair has ONE query; lane t of every wave holds tag t of it (t < its clamped count), and a
// row whose bit is clear -- a suspect -- is skipped iff one ballot finds its tag among them: the rule of k_exact_scan_any<true, true>.
template <int ADM>
__global__ __launch_bounds__(IVX_THREADS) void k_ivf_exact(IvfExactParams p) {
    const int count = min(*p.count - p.slot0, p.nslots);
    if (count <= 0) return;
    extern __shared__ __attribute__((aligned(16))) char smem_e[];
    __shared__ int s_last;
    float* sQ = reinterpret_cast<float*>(smem_e);                                   // [dim]
    double* sKey = reinterpret_cast<double*>(sQ + p.dim);                           // [IVX_WAVES][k]
    long long* sId = reinterpret_cast<long long*>(sKey + IVX_WAVES * p.k);          // [IVX_WAVES][k]
    int* sPos = reinterpret_cast<int*>(sId + IVX_WAVES * p.k);                      // [nprobe] heads of the final merge
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nv = p.dim >> 2, K = p.k;
    const int64_t npairs = (int64_t)count * p.nprobe;
    for (int64_t pr = blockIdx.x; pr < npairs; pr += gridDim.x) {                    // (uniform)
        const int slot = (int)(pr / p.nprobe), j = (int)(pr % p.nprobe);
        const int64_t qi = p.sel ? (int64_t)p.sel[p.slot0 + slot] : (int64_t)(p.slot0 + slot);
        const int64_t list = p.probes[qi * p.nprobe + j];
        int64_t r0 = 0, r1 = 0;
        if ((uint64_t)list < (uint64_t)p.nlist) { r0 = p.loff[list]; r1 = p.loff[list + 1]; }
        __syncthreads();                                                             // (the previous pair's LDS is free)
        for (int i = tid; i < nv; i += IVX_THREADS)
            reinterpret_cast<f32x4*>(sQ)[i] = reinterpret_cast<const f32x4*>(p.q + qi * p.dim)[i];
        __syncthreads();
        double ek = -INFINITY;                                                       // lane e: entry e of the wave's sorted list
        long long ei = IVX_NO_ID;
        int64_t my_tag = 0;                                                          // (IVF_ADM_PQ) tag `lane` of the pair's query ...
        bool my_tag_on = false;                                                      // ... when the query's clamped count reaches it
        if constexpr (ADM == IVF_ADM_PQ) {
            my_tag_on = lane < min(max(p.pq.q_cnt ? p.pq.q_cnt[qi] : p.pq.m, 0), p.pq.m);
            if (my_tag_on) my_tag = p.pq.q_tags[qi * p.pq.m + lane];
        }
        for (int64_t row = r0 + wave * IVX_ROWS; row < r1; row += IVX_WAVES * IVX_ROWS) {
            double acc[IVX_ROWS];
#pragma unroll
            for (int u = 0; u < IVX_ROWS; ++u) acc[u] = 0.0;
            for (int i = lane; i < nv; i += 64) {
                f32x4 y[IVX_ROWS];
#pragma unroll
                for (int u = 0; u < IVX_ROWS; ++u) y[u] = reinterpret_cast<const f32x4*>(p.lrows + min(row + u, r1 - 1) * p.dim)[i];
                const f32x4 x = reinterpret_cast<const f32x4*>(sQ)[i];
#pragma unroll
                for (int u = 0; u < IVX_ROWS; ++u)
#pragma unroll
                    for (int e = 0; e < 4; ++e) { const double d = (double)x[e] - (double)y[u][e]; acc[u] -= d * d; }
            }
#pragma unroll
            for (int u = 0; u < IVX_ROWS; ++u) {
                if (row + u >= r1) break;                                            // (wave-uniform)
                if constexpr (ADM == IVF_ADM_BITMAP) { if (!ivf_admitted(p.admit, row + u)) continue; }      // (wave-uniform)
                if constexpr (ADM == IVF_ADM_PQ) {                                   // (wave-uniform: one row, one query)
                    if (!ivf_admitted(p.admit, row + u)) {
                        const int64_t t = p.pq.row_tags[p.pq.lids[row + u]];
                        if (__ballot(my_tag_on && my_tag == t) != 0ull) continue;
                    }
                }
                double v = acc[u];
#pragma unroll
                for (int ofs = 32; ofs > 0; ofs >>= 1) v += __shfl_xor(v, ofs, 64);
                const long long gid = p.lids[row + u];
                if (ivx_better(v, gid, __shfl(ek, K - 1, 64), __shfl(ei, K - 1, 64))) {      // (wave-uniform) beats the k-th entry
                    // the better entries are a prefix of the sorted list: the new one goes behind them, the rest moves one lane up
                    const int nb = __popcll(__ballot(lane < K && ivx_better(ek, ei, v, gid)));
                    const double pk = __shfl_up(ek, 1, 64);
                    const long long pi = __shfl_up(ei, 1, 64);
                    if (lane > nb) { ek = pk; ei = pi; }
                    else if (lane == nb) { ek = v; ei = gid; }
                }
            }
        }
        if (lane < K) { sKey[wave * K + lane] = ek; sId[wave * K + lane] = ei; }
        const int64_t ob = ((int64_t)slot * p.nprobe + j) * K;
        if (tid < K) { p.pkey[ob + tid] = -INFINITY; p.pid[ob + tid] = IVX_NO_ID; }
        __syncthreads();
        if (tid < IVX_WAVES * K && sId[tid] != IVX_NO_ID) {                           // rank of every listed row among the waves' entries
            const double kc = sKey[tid];
            const long long ic = sId[tid];
            int rank = 0;
            for (int e = 0; e < IVX_WAVES * K; ++e) rank += (int)ivx_better(sKey[e], sId[e], kc, ic);
            if (rank < K) { p.pkey[ob + rank] = kc; p.pid[ob + rank] = ic; }
        }
        __threadfence();                                 // release: this pair's list is visible device-wide before the counter moves
        __syncthreads();
        if (tid == 0) {
            const int old = atomicAdd(&p.arrive[slot], 1);
            s_last = old == p.nprobe - 1;
            if (s_last) p.arrive[slot] = 0;              // ready for the next launch
        }
        __syncthreads();
        if (s_last && wave == 0) {                       // the query's last pair: merge its nprobe partial lists (lane l owns lists l, l + 64, ...)
            __threadfence();                             // acquire
            for (int part = lane; part < p.nprobe; part += 64) sPos[part] = 0;
            const int64_t lb = (int64_t)slot * p.nprobe * K;
            for (int o = 0; o < K; ++o) {
                double bk = -INFINITY;
                long long bi = IVX_NO_ID;
                int bp = -1;
                for (int part = lane; part < p.nprobe; part += 64) {
                    const int pos = sPos[part];
                    if (pos >= K) continue;
                    const long long id = p.pid[lb + (int64_t)part * K + pos];
                    if (id == IVX_NO_ID) continue;
                    const double key = p.pkey[lb + (int64_t)part * K + pos];
                    if (bp < 0 || ivx_better(key, id, bk, bi)) { bk = key; bi = id; bp = part; }
                }
#pragma unroll
                for (int ofs = 32; ofs > 0; ofs >>= 1) {
                    const double ok = __shfl_xor(bk, ofs, 64);
                    const long long oi = __shfl_xor(bi, ofs, 64);
                    const int op = __shfl_xor(bp, ofs, 64);
                    if (op >= 0 && (bp < 0 || ivx_better(ok, oi, bk, bi))) { bk = ok; bi = oi; bp = op; }
                }
                if (bp >= 0 && (bp & 63) == lane) sPos[bp] += 1;
                if (lane == 0) {
                    p.out_dist[qi * K + o] = bp < 0 ? INFINITY : (float)(-bk);
                    p.out_idx[qi * K + o] = bp < 0 ? (int64_t)-1 : (int64_t)bi;
                }
            }
            if (lane == 0) atomicAdd(p.done, 1);
        }
    }
}

// ---- range search over the probed lists (radad_ivf_range_search) -------------------------------------------------------------------
// Every row of a query's probed lists whose float64 key sum (q - y)^2 is < radius, the best m listed, the count exact.  The f16 list
// scan is a FILTER with a measured error bound eps(q) (k_hi_rows, as for the top-k search): with T = -radius and the floor
// thr[q] = T - eps(q), two ulps lower (knn.hip's k_range_floor, as it is), exact score > T implies scan score >= thr, so every member is
// emitted.  What the top-k scan derives from rows -- the k-th best of a chunk, the carry, the published bound -- does not exist here.
//   k_ivf_range_hi      the task, split and step structure of k_ivf_scan_hi<IVF_ADM_NONE>; a (row, query) pair at or above the floor takes
//                       a slot of the query's position buffer
//   k_ivf_range_refine  one workgroup per query: float64 re-score of every emitted position, strict test, count, (key, insertion id)
//                       sort in LDS, the best m; a buffer that overflowed proves nothing -- the query is listed for the exact pass
//   k_ivf_range_exact   the listed queries (or all of them: IVF_RANGE_EXACT), float64 over their probed lists
// Integer atomics only (slot counters, counts, arrival counters); every result is written with plain vector stores.
static_assert(IVF_RANGE_CAP == RG_MAX_CAP, "the candidate buffers are what the re-rank's LDS sort is sized for");
static_assert(IVF_RANGE_HI == RADAD_IVF_RANGE_HI && IVF_RANGE_EXACT == RADAD_IVF_RANGE_EXACT, "ivf_plan.h's routes are the header's");
static_assert(ivf_range_refine_lds_bytes() == range_refine_lds_bytes(), "k_ivf_range_refine has k_range_refine's LDS layout");

struct IvfRangeHiParams {
    const _Float16* lhi = nullptr; // [N][dim] list-major f16 plane
    const float* lscale = nullptr; // [N] per-row scale, or nullptr: uscale for every row
    float uscale = 1.f;
    const float* lbias = nullptr;  // [N]
    const int* loff = nullptr;     // [nlist + 1]
    const _Float16* qh = nullptr;  // [nq][dim]
    const float* qscale = nullptr; // [nq]
    const float* qconst = nullptr; // [nq]
    const float* thr = nullptr;    // [nq] the floor: -radius - eps(q), two ulps lower
    const int* task_list = nullptr; const int* task_pbeg = nullptr; const int* task_cnt = nullptr; const int* n_tasks_dev = nullptr; const int* pair_q = nullptr;
    int dim = 0, qcap = 0, split = 1;
    int* cand_cnt = nullptr;       // [nq] positions emitted, 0 at launch; it keeps counting past cand_cap (overflow)
    int cand_cap = 0;
    int* cand_idx = nullptr;       // [nq][cand_cap] positions in the list-major order
    const unsigned long long* admit = nullptr;      // IVF_ADM_BITMAP: the admission bitmap by list-major position (k_admit_bitmap<true>)
    IvfPqRule pq;                                   // IVF_ADM_PQ: the per-query rule (no bitmap: see the kernel)
};
static_assert(std::is_trivially_copyable_v<IvfRangeHiParams>, "kernel argument");

// k_ivf_scan_hi<IVF_ADM_NONE> without its second half.  That kernel parks the scores of a 256-row chunk in LDS because a wave per
// query then SELECTS among them; with a floor fixed before the launch the lane that holds the score of (row 4 g + e, query r16) in
// its accumulator decides alone.  So there is no score tile (LDS = the task's f16 queries: 16.6 KB at dim 512 instead of 37 KB), no
// barrier inside the row loop, and the 16-row steps are dealt to the four waves as before (step i of the share to wave i % 4).
// A NaN score is never emitted (`sc >= thr` is false).  Rows past l_end and the query rows past the task's count emit nothing.
// ADM (radad_ivf_range_search_excl / _excl_pq): an excluded row never takes a slot.  The top-k scans must keep excluded rows out of
// their bounds, so they fetch admission bits for every step and need a suspect pre-pass for the per-query form.  Here the floor is
// fixed before the launch and no row sets a bound: admission is asked only of a (row, query) pair that has ALREADY passed `sc >= thr`,
// by the lane that holds the pair.
//   IVF_ADM_BITMAP  the pair's bit of the admission bitmap (absolute list-major position)
//   IVF_ADM_PQ      the row's tag (through lids) against the tags of the lane's query r16, staged per task behind the f16 queries
//                   (ivf_pq_stage at tag_off = scan_lds - pq_lds).  No suspect bitmap, no hash bitset, no pre-pass.
// Both cost a gather per pair at or above the floor and nothing per row below it; the loop stays free of barriers.
template <int ADM>
__global__ __launch_bounds__(SQ_THREADS, 4) void k_ivf_range_hi(IvfRangeHiParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem_rh[];
    const int qld = p.dim + 8;
    _Float16* sQ = reinterpret_cast<_Float16*>(smem_rh);                       // [qcap][dim + 8]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int task = blockIdx.x / p.split, sub = blockIdx.x % p.split;
    if (task >= *p.n_tasks_dev) return;                                        // (uniform per workgroup)
    const int list = p.task_list[task];
    int64_t l_begin = p.loff[list], l_end = p.loff[list + 1];
    if (p.split > 1) {                                                         // this workgroup's share of the list: whole 16-row steps
        const int64_t len = ((l_end - l_begin + p.split - 1) / p.split + 15) / 16 * 16;
        l_begin += sub * len;
        l_end = min(l_end, l_begin + len);
        if (l_begin >= l_end) return;
    }
    const int pbeg = p.task_pbeg[task], cnt = p.task_cnt[task];
    for (int i = tid; i < p.qcap * (p.dim >> 3); i += SQ_THREADS) {
        const int qq = i / (p.dim >> 3), c8 = i % (p.dim >> 3);
        f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (qq < cnt) v = *reinterpret_cast<const f16x8*>(p.qh + (int64_t)p.pair_q[pbeg + qq] * p.dim + c8 * 8);
        *reinterpret_cast<f16x8*>(sQ + qq * qld + c8 * 8) = v;
    }
    if constexpr (ADM == IVF_ADM_PQ) ivf_pq_stage(p.pq, smem_rh, p.qcap, p.pair_q, pbeg, cnt, tid, SQ_THREADS);
    const bool q_on = r16 < cnt;
    const int pq = q_on ? p.pair_q[pbeg + r16] : 0;
    const float qs = q_on ? p.qscale[pq] * 2.f : 0.f;
    const float qc = q_on ? p.qconst[pq] : 0.f;
    const float thr = q_on ? p.thr[pq] : 0.f;
    int* my_cnt = p.cand_cnt + pq;
    int* my_idx = p.cand_idx + (int64_t)pq * p.cand_cap;
    __syncthreads();

    const _Float16* qrow = sQ + min(r16, p.qcap - 1) * qld + 8 * g;
    const int nkb = p.dim >> 5;
    for (int64_t row0 = l_begin + 16 * wave; row0 < l_end; row0 += 4 * 16) {     // (wave-uniform)
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        const int64_t ra = min(row0 + r16, l_end - 1);
        const _Float16* pa = p.lhi + ra * p.dim + 8 * g;
        float rs[4], yb[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t row = min(row0 + 4 * g + e, l_end - 1);
            rs[e] = p.lscale ? p.lscale[row] : p.uscale;
            yb[e] = qc - p.lbias[row];
        }
        constexpr int HKB = 16;
        for (int kp = 0; kp < nkb; kp += HKB) {
            const int nb = min(HKB, nkb - kp);
            f16x8 v[HKB];
#pragma unroll
            for (int kb = 0; kb < HKB; ++kb)
                if (kb < nb) v[kb] = *reinterpret_cast<const f16x8*>(pa + (kp + kb) * 32);
#pragma unroll
            for (int kb = 0; kb < HKB; ++kb)
                if (kb < nb) {
                    const f16x8 b = *reinterpret_cast<const f16x8*>(qrow + (kp + kb) * 32);
                    if (kb & 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(v[kb], b, acc1, 0, 0, 0);
                    else acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(v[kb], b, acc0, 0, 0, 0);
                }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t row = row0 + 4 * g + e;
            const float sc = fmaf((acc0[e] + acc1[e]) * rs[e], qs, yb[e]);      // the top-k scan's score, operation for operation
            if (q_on && row < l_end && sc >= thr) {
                if constexpr (ADM == IVF_ADM_BITMAP) { if (!ivf_admitted(p.admit, row)) continue; }
                if constexpr (ADM == IVF_ADM_PQ) { if (ivf_pq_excludes(p.pq, smem_rh, p.qcap, r16, row)) continue; }      // (q_on: r16 < cnt <= qcap)
                const int slot = atomicAdd(my_cnt, 1);
                if (slot < p.cand_cap) my_idx[slot] = (int)row;
            }
        }
    }
}

struct IvfRangeRefineParams {
    const int* idx = nullptr;           // [nq][cap] positions the scan emitted
    const int* cnt = nullptr;           // [nq] positions emitted (> cap: overflow)
    int cap = 0, dim = 0, m = 0;
    const float* lrows = nullptr;       // [N, dim] list-major
    const int64_t* lids = nullptr;      // [N] insertion id of every position
    int64_t n_pos = 0;                  // N
    const float* q = nullptr;           // [nq, dim]
    double radius = 0.0;
    int* flag_count = nullptr;          // [8]: [0] queries left to the exact pass, [2] the largest cnt of the call
    int* flag_sel = nullptr;            // the queries left to the exact pass
    int* out_count = nullptr;           // [nq]
    float* out_dist = nullptr;          // [nq, m]
    int64_t* out_idx = nullptr;         // [nq, m]
    double* out_key = nullptr;          // optional [nq, m]
};
static_assert(std::is_trivially_copyable_v<IvfRangeRefineParams>, "kernel argument");

// k_range_refine's plain form (knn.hip) over list-major positions: the same compaction, the same float64 re-score (refine_rescore_f64's
// plain form, not its exact-order one: a key may differ from k_ivf_range_exact's in its last place or two, as between the flat range
// search's tile and exact routes), the same strict test and bitonic sort.  What differs: a row is read at its POSITION in lrows, and
// once it has its key the position is replaced by the row's insertion id (an index holds fewer than 2^31 rows: positions are ints,
// and so are the ids), which is what ties are broken by and what is written.
__global__ __launch_bounds__(RF_THREADS) void k_ivf_range_refine(IvfRangeRefineParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem_rr[];
    double* c_key = reinterpret_cast<double*>(smem_rr);                  // [RG_MAX_CAP]
    int* c_id = reinterpret_cast<int*>(c_key + RG_MAX_CAP);              // [RG_MAX_CAP]
    int* w_cnt = c_id + RG_MAX_CAP;                                      // [4]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q = blockIdx.x;
    const int filled = p.cnt[q];
    if (tid == 0) atomicMax(&p.flag_count[2], filled);
    if (filled > p.cap) {                                                // (workgroup-uniform)
        if (tid == 0) { p.flag_sel[atomicAdd(p.flag_count, 1)] = (int)q; p.out_count[q] = 0; }
        return;
    }
    // the emitted positions (every slot below cnt was written; one outside the layout is left out all the same)
    const int NE = max(filled, 0);
    const int* ebuf = p.idx + q * p.cap;
    auto taken = [&](int id) -> bool { return id >= 0 && id < p.n_pos; };
    int mine = 0;
    for (int i = tid; i < NE; i += RF_THREADS) mine += taken(ebuf[i]) ? 1 : 0;
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) w_cnt[wave] = incl;
    __syncthreads();
    int slot = incl - mine, nsel = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { if (w < wave) slot += w_cnt[w]; nsel += w_cnt[w]; }
    for (int i = tid; i < NE; i += RF_THREADS) { const int id = ebuf[i]; if (taken(id)) c_id[slot++] = id; }
    __syncthreads();
    refine_rescore_f64<false>(p.lrows, 0, p.q + q * p.dim, p.dim, 1, c_id, c_key, nsel);
    __syncthreads();
    // membership, "larger is better" keys for the ranking, insertion ids for the tie-break and the output
    int P = 1;
    while (P < nsel) P <<= 1;                                            // <= RG_MAX_CAP: nsel <= cap == RG_MAX_CAP
    int n_pass = 0;
    for (int i0 = 0; i0 < P; i0 += RF_THREADS) {
        const int i = i0 + tid;
        bool pass = false;
        if (i < nsel) {
            const double key = c_key[i];
            pass = key < p.radius;
            c_key[i] = pass ? -key : -(double)INFINITY;
            c_id[i] = pass ? (int)p.lids[c_id[i]] : IDX_SENTINEL;
        } else if (i < P) {
            c_key[i] = -(double)INFINITY;
            c_id[i] = IDX_SENTINEL;
        }
        n_pass += __syncthreads_count(pass);
    }
    for (int k2 = 2; k2 <= P; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += RF_THREADS) {
                const int o = i ^ j;
                if (o > i) {
                    const double ka = c_key[i], kb = c_key[o];
                    const int ia = c_id[i], ib = c_id[o];
                    const bool b_first = kb > ka || (kb == ka && ib < ia);
                    const bool a_first = ka > kb || (ka == kb && ia < ib);
                    if ((i & k2) == 0 ? b_first : a_first) { c_key[i] = kb; c_id[i] = ib; c_key[o] = ka; c_id[o] = ia; }
                }
            }
            __syncthreads();
        }
    if (tid == 0) p.out_count[q] = n_pass;
    const int n_out = min(n_pass, p.m);
    const float nan_f = __int_as_float(0x7fc00000);
    for (int o = tid; o < p.m; o += RF_THREADS) {
        const bool have = o < n_out;
        const double kd = have ? -c_key[o] : (double)nan_f;
        p.out_dist[q * p.m + o] = have ? (float)kd : nan_f;
        p.out_idx[q * p.m + o] = have ? (int64_t)c_id[o] : -1;
        if (p.out_key) p.out_key[q * p.m + o] = kd;
    }
}

struct IvfRangeExactParams {
    const float* lrows = nullptr;      // [N, dim] list-major
    const int64_t* lids = nullptr;     // [N] insertion id of every position
    const int* loff = nullptr;         // [nlist + 1]
    const float* q = nullptr;          // [nq, dim]
    const int64_t* probes = nullptr;   // [nq, nprobe] lists; outside [0, nlist) = none
    const int* sel = nullptr;          // the listed queries (IVF_RANGE_EXACT: all of them, ivf_launch_range_list_all)
    const int* count = nullptr;        // [1] how many
    int* done = nullptr;               // [1] queries answered here (radad_ivf_last_range)
    int dim = 0, m = 0, nprobe = 0, nlist = 0;
    int slot0 = 0, nslots = 0;         // this launch's queries: slots slot0 .. slot0 + nslots
    double radius = 0.0;
    double* pkey = nullptr;            // [nslots][nprobe][m]
    int64_t* pid = nullptr;
    int* arrive = nullptr;             // [nslots] arrival counters (zero between launches: the last arrival resets its own)
    int* out_count = nullptr;          // [nq], zero at launch for the queries answered here
    float* out_dist = nullptr; int64_t* out_idx = nullptr; double* out_key = nullptr;
    const unsigned long long* admit = nullptr;      // IVF_ADM_BITMAP: the admission bitmap by list-major position
    IvfPqRule pq;                                   // IVF_ADM_PQ: the per-query rule (row_tags, lids, q_tags, q_cnt, m; no bitmap)
};
static_assert(std::is_trivially_copyable_v<IvfRangeExactParams>, "kernel argument");

// k_ivf_exact<IVF_ADM_NONE> with a radius: the same pairs in turn, the same float64 sums (keys are minus the squared distance inside the
// kernel: larger is better).  A row that fails the strict test -(key) < radius is skipped BEFORE the list insertion; the rows that
// pass are counted per wave, and each wave adds its count of the pair to out_count once.  m reaches 128, so a wave's sorted list is
// TWO entries per lane (lane e holds entries e and e + 64); an insertion shifts both halves one lane up, entry 63 crossing over.
// Insertions are rare once a list is full.  The waves' lists are ranked into the pair's partial list (only the entries the waves
// hold are compared: sLen), and the pair that arrives last for a query merges the nprobe partial lists and writes the m slots,
// -1 / NaN / NaN where there is no member.
// ADM: the admission test sits behind the strict radius test and in front of the count and the insertion, so only members pay for a
// tag gather.  IVF_ADM_BITMAP: the row's bit.  IVF_ADM_PQ: a pair has ONE query; lane t of every wave holds tag t of it (t < its
// clamped count) and one ballot per member row finds the row's tag among them -- the rule and the shape of k_ivf_exact<IVF_ADM_PQ>
// without its bitmap short-cut (there is no suspect bitmap here).  Either decision is wave-uniform.
template <int ADM>
__global__ __launch_bounds__(IVX_THREADS) void k_ivf_range_exact(IvfRangeExactParams p) {
    const int count = min(*p.count - p.slot0, p.nslots);
    if (count <= 0) return;
    extern __shared__ __attribute__((aligned(16))) char smem_re[];
    __shared__ int s_last;
    float* sQ = reinterpret_cast<float*>(smem_re);                                  // [dim]
    double* sKey = reinterpret_cast<double*>(sQ + p.dim);                           // [IVX_WAVES][m]
    long long* sId = reinterpret_cast<long long*>(sKey + IVX_WAVES * p.m);          // [IVX_WAVES][m]
    int* sLen = reinterpret_cast<int*>(sId + IVX_WAVES * p.m);                      // [IVX_WAVES] entries of every wave's list
    int* sPos = sLen + IVX_WAVES;                                                   // [nprobe] heads of the final merge
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nv = p.dim >> 2, K = p.m;
    const float nan_f = __int_as_float(0x7fc00000);
    const int64_t npairs = (int64_t)count * p.nprobe;
    for (int64_t pr = blockIdx.x; pr < npairs; pr += gridDim.x) {                    // (uniform)
        const int slot = (int)(pr / p.nprobe), j = (int)(pr % p.nprobe);
        const int64_t qi = p.sel[p.slot0 + slot];
        const int64_t list = p.probes[qi * p.nprobe + j];
        int64_t r0 = 0, r1 = 0;
        if ((uint64_t)list < (uint64_t)p.nlist) { r0 = p.loff[list]; r1 = p.loff[list + 1]; }
        __syncthreads();                                                             // (the previous pair's LDS is free)
        for (int i = tid; i < nv; i += IVX_THREADS)
            reinterpret_cast<f32x4*>(sQ)[i] = reinterpret_cast<const f32x4*>(p.q + qi * p.dim)[i];
        __syncthreads();
        double ek0 = -INFINITY, ek1 = -INFINITY;                                     // lane e: entries e and e + 64 of the wave's sorted list
        long long ei0 = IVX_NO_ID, ei1 = IVX_NO_ID;
        int members = 0;                                                             // (wave-uniform) rows of this wave that passed
        int64_t my_tag = 0;                                                          // (IVF_ADM_PQ) tag `lane` of the pair's query ...
        bool my_tag_on = false;                                                      // ... when the query's clamped count reaches it
        if constexpr (ADM == IVF_ADM_PQ) {
            my_tag_on = lane < min(max(p.pq.q_cnt ? p.pq.q_cnt[qi] : p.pq.m, 0), p.pq.m);
            if (my_tag_on) my_tag = p.pq.q_tags[qi * p.pq.m + lane];
        }
        for (int64_t row = r0 + wave * IVX_ROWS; row < r1; row += IVX_WAVES * IVX_ROWS) {
            double acc[IVX_ROWS];
#pragma unroll
            for (int u = 0; u < IVX_ROWS; ++u) acc[u] = 0.0;
            for (int i = lane; i < nv; i += 64) {
                f32x4 y[IVX_ROWS];
#pragma unroll
                for (int u = 0; u < IVX_ROWS; ++u) y[u] = reinterpret_cast<const f32x4*>(p.lrows + min(row + u, r1 - 1) * p.dim)[i];
                const f32x4 x = reinterpret_cast<const f32x4*>(sQ)[i];
#pragma unroll
                for (int u = 0; u < IVX_ROWS; ++u)
#pragma unroll
                    for (int e = 0; e < 4; ++e) { const double d = (double)x[e] - (double)y[u][e]; acc[u] -= d * d; }
            }
#pragma unroll
            for (int u = 0; u < IVX_ROWS; ++u) {
                if (row + u >= r1) break;                                            // (wave-uniform)
                double v = acc[u];
#pragma unroll
                for (int ofs = 32; ofs > 0; ofs >>= 1) v += __shfl_xor(v, ofs, 64);
                if (!(-v < p.radius)) continue;                                      // (wave-uniform) the strict test; a NaN key fails it
                if constexpr (ADM == IVF_ADM_BITMAP) { if (!ivf_admitted(p.admit, row + u)) continue; }      // (wave-uniform)
                if constexpr (ADM == IVF_ADM_PQ) {                                   // (wave-uniform: one row, one query)
                    const int64_t t = p.pq.row_tags[p.pq.lids[row + u]];
                    if (__ballot(my_tag_on && my_tag == t) != 0ull) continue;
                }
                ++members;
                const long long gid = p.lids[row + u];
                const double lk = K <= 64 ? __shfl(ek0, K - 1, 64) : __shfl(ek1, K - 65, 64);
                const long long li = K <= 64 ? __shfl(ei0, K - 1, 64) : __shfl(ei1, K - 65, 64);
                if (ivx_better(v, gid, lk, li)) {                                    // (wave-uniform) beats the m-th entry
                    // the better entries are a prefix of the sorted list: the new one goes behind them, the rest moves one entry up
                    const int nb = __popcll(__ballot(lane < K && ivx_better(ek0, ei0, v, gid))) +
                                   __popcll(__ballot(lane + 64 < K && ivx_better(ek1, ei1, v, gid)));
                    const double t_k = __shfl(ek0, 63, 64);
                    const long long t_i = __shfl(ei0, 63, 64);
                    double pk0 = __shfl_up(ek0, 1, 64), pk1 = __shfl_up(ek1, 1, 64);
                    long long pi0 = __shfl_up(ei0, 1, 64), pi1 = __shfl_up(ei1, 1, 64);
                    if (lane == 0) { pk1 = t_k; pi1 = t_i; }
                    if (lane > nb) { ek0 = pk0; ei0 = pi0; }
                    else if (lane == nb) { ek0 = v; ei0 = gid; }
                    if (lane + 64 > nb) { ek1 = pk1; ei1 = pi1; }
                    else if (lane + 64 == nb) { ek1 = v; ei1 = gid; }
                }
            }
        }
        if (lane < K) { sKey[wave * K + lane] = ek0; sId[wave * K + lane] = ei0; }
        if (lane + 64 < K) { sKey[wave * K + lane + 64] = ek1; sId[wave * K + lane + 64] = ei1; }
        if (lane == 0) {
            sLen[wave] = min(members, K);
            if (members > 0) atomicAdd(&p.out_count[qi], members);
        }
        const int64_t ob = ((int64_t)slot * p.nprobe + j) * K;
        if (tid < K) { p.pkey[ob + tid] = -INFINITY; p.pid[ob + tid] = IVX_NO_ID; }
        __syncthreads();
        for (int i = tid; i < IVX_WAVES * K; i += IVX_THREADS) {                      // rank of every listed row among the waves' entries
            const int w = i / K, e = i - w * K;
            if (e >= sLen[w]) continue;
            const double kc = sKey[i];
            const long long ic = sId[i];
            int rank = 0;
            for (int w2 = 0; w2 < IVX_WAVES; ++w2) {
                const int n2 = sLen[w2];
                for (int e2 = 0; e2 < n2; ++e2) rank += (int)ivx_better(sKey[w2 * K + e2], sId[w2 * K + e2], kc, ic);
            }
            if (rank < K) { p.pkey[ob + rank] = kc; p.pid[ob + rank] = ic; }
        }
        __threadfence();                                 // release: this pair's list is visible device-wide before the counter moves
        __syncthreads();
        if (tid == 0) {
            const int old = atomicAdd(&p.arrive[slot], 1);
            s_last = old == p.nprobe - 1;
            if (s_last) p.arrive[slot] = 0;              // ready for the next launch
        }
        __syncthreads();
        if (s_last && wave == 0) {                       // the query's last pair: merge its nprobe partial lists (lane l owns lists l, l + 64, ...)
            __threadfence();                             // acquire
            for (int part = lane; part < p.nprobe; part += 64) sPos[part] = 0;
            const int64_t lb = (int64_t)slot * p.nprobe * K;
            for (int o = 0; o < K; ++o) {
                double bk = -INFINITY;
                long long bi = IVX_NO_ID;
                int bp = -1;
                for (int part = lane; part < p.nprobe; part += 64) {
                    const int pos = sPos[part];
                    if (pos >= K) continue;
                    const long long id = p.pid[lb + (int64_t)part * K + pos];
                    if (id == IVX_NO_ID) continue;
                    const double key = p.pkey[lb + (int64_t)part * K + pos];
                    if (bp < 0 || ivx_better(key, id, bk, bi)) { bk = key; bi = id; bp = part; }
                }
#pragma unroll
                for (int ofs = 32; ofs > 0; ofs >>= 1) {
                    const double ok = __shfl_xor(bk, ofs, 64);
                    const long long oi = __shfl_xor(bi, ofs, 64);
                    const int op = __shfl_xor(bp, ofs, 64);
                    if (op >= 0 && (bp < 0 || ivx_better(ok, oi, bk, bi))) { bk = ok; bi = oi; bp = op; }
                }
                if (bp >= 0 && (bp & 63) == lane) sPos[bp] += 1;
                if (lane == 0) {
                    const double kd = bp < 0 ? (double)nan_f : -bk;
                    p.out_dist[qi * K + o] = bp < 0 ? nan_f : (float)kd;
                    p.out_idx[qi * K + o] = bp < 0 ? (int64_t)-1 : (int64_t)bi;
                    if (p.out_key) p.out_key[qi * K + o] = kd;
                }
            }
            if (lane == 0) atomicAdd(p.done, 1);
        }
    }
}

struct DevMem {
    void* p = nullptr;
    size_t bytes = 0;
    int ensure(size_t need) {
        if (need <= bytes) return RADAD_OK;
        if (p) (void)hipFree(p);
        p = nullptr; bytes = 0;
        if (hipMalloc(&p, need + need / 8 + 256) != hipSuccess) { radad_set_error("hipMalloc of %zu bytes failed", need); return RADAD_ENOMEM; }
        bytes = need + need / 8 + 256;
        return RADAD_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
};

}  // namespace

struct radad_ivf_s {
    int dim = 0, nlist = 0, device = 0;
    bool trained = false, dirty = false;
    radad_knn_t quant = nullptr;        // flat L2 store over the centroids
    float* centroids = nullptr;         // [nlist, dim]
    radad_knn_t flat = nullptr;         // rows in insertion order (IP metric = plain copy; used for storage + reconstruct)
    std::vector<int> assign;            // list of every stored row (host)
    DevMem lrows, lnorm, lids, loff, ws_a, ws_b, ws_c, part_s, part_i, tasks;
    DevMem lmax, xkey, xid, xarrive;    // |y|^2 max of every list (the fp32 scan's error bound); partial lists + arrival counters of the exact list scan
    DevMem admit;                       // radad_ivf_search_excl: the admission bitmap by list-major position, rebuilt by every call
    DevMem pqset;                       // radad_ivf_search_excl_pq: the hash bitset of the suspect pre-pass (`admit` is the suspect bitmap)
    DevMem lhi, lscale, lbias, qbuf, cand_s, cand_i;    // the flat store's f16 plane gathered list-major (+ per-row scale, bias); the queries' f16 side
    bool have_hi = false;               // lhi is up to date with ...
    const void* hi_src = nullptr;       // ... this plane of the flat store (pointer, rows and rebuild count at the gather)
    int64_t hi_src_rows = 0;
    int hi_src_epoch = -1;
    int opt_hi = 1;                     // 0: every search on the fp32 list scan (A/B measurements; radad_ivf_set_option)
    int opt_pq_filter = 1;              // 0 (tests): the per-query search marks every position suspect (RADAD_IVF_OPT_PQ_FILTER)
    std::vector<int> loff_host;
    hipEvent_t ev_done = nullptr;       // end of the last search's device work: the next search (any stream) waits for it,
    bool last_hi = false;               // the most recent search went through the certified f16 list scan
    const int* last_fcount = nullptr;   // device counters of the most recent list-scan search: [0] queries its certificate rejected, [1] queries the
                                        // exact list scan answered
    bool last_exact = false;            // the most recent search was answered by the exact flat scan (k > 26): radad_ivf_last_search_exact
    bool last_range = false;            // the most recent search was a radad_ivf_range_search (radad_ivf_last_range describes it: last_fcount [1] the
    int64_t last_range_nq = 0;          // queries the exact pass answered, [2] the largest number of positions a query emitted)
    int last_range_route = IVF_RANGE_EXACT;
    bool have_last = false;             // since all searches share the workspaces below and nothing synchronises with the host: a search on
    hipStream_t last_stream = nullptr;  // ANOTHER stream than the last records the event behind that stream's work first (knn.hip does the same)
    std::mutex mu;
};

// calls that rebuild or reuse what a search reads wait for the last (asynchronous) search first
static void ivf_wait_searches(radad_ivf_t h) {
    if (!h->have_last) return;
    if (hipStreamSynchronize(h->last_stream) != hipSuccess) { (void)hipGetLastError(); (void)hipDeviceSynchronize(); }
    h->have_last = false;
}

// assignment of n rows to their nearest centroid (a flat k = 1 search of `quant`) -> host ints.  *bad_row = -1, or the first row
// the quantiser found no centroid for: id outside [0, nlist) (a non-finite query comes back with id -1) or a distance that is not
// finite (the float64 re-score of a row with a NaN or an infinity in it, whatever id the scan gave it).  The callers refuse the
// whole batch then: such a row has no list.
static int ivf_assign(radad_ivf_t h, radad_knn_t quant, const float* rows_dev, int64_t n, std::vector<int>& out, int64_t* bad_row, hipStream_t st) {
    int rc;
    if ((rc = h->ws_a.ensure((size_t)n * sizeof(float)))) return rc;
    if ((rc = h->ws_b.ensure((size_t)n * sizeof(int64_t)))) return rc;
    if ((rc = radad_knn_search(quant, rows_dev, n, 1, (float*)h->ws_a.p, (int64_t*)h->ws_b.p, st))) return rc;
    std::vector<int64_t> ids((size_t)n);
    std::vector<float> dist((size_t)n);
    RADAD_HIP_CHECK(hipMemcpyAsync(ids.data(), h->ws_b.p, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    RADAD_HIP_CHECK(hipMemcpyAsync(dist.data(), h->ws_a.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, st));
    RADAD_HIP_CHECK(hipStreamSynchronize(st));
    out.resize((size_t)n);
    *bad_row = -1;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t id = ids[(size_t)i];
        if (*bad_row < 0 && (id < 0 || id >= h->nlist || !std::isfinite(dist[(size_t)i]))) *bad_row = i;
        out[(size_t)i] = (int)id;
    }
    return RADAD_OK;
}

// a flat L2 store over the [nlist, dim] centroids at `cent`
static int ivf_make_quantizer(radad_ivf_t h, const float* cent, hipStream_t st, radad_knn_t* out) {
    radad_knn_t q = nullptr;
    int rc = radad_knn_create(h->dim, RADAD_METRIC_L2, h->device, 0, &q);
    if (rc) return rc;
    q->owned_serial = true;      // searched under this index's lock, in the stream order this index keeps: no event of its own per search
    if ((rc = radad_knn_add(q, cent, h->nlist, st))) { radad_knn_destroy(q); return rc; }
    *out = q;
    return RADAD_OK;
}

// (re)load the quantiser from h->centroids
static int ivf_load_quantizer(radad_ivf_t h, hipStream_t st) {
    if (h->quant) radad_knn_destroy(h->quant);
    h->quant = nullptr;
    return ivf_make_quantizer(h, h->centroids, st, &h->quant);
}

// stable counting sort of `assign` -> perm (position -> source index) and offsets.  false, with nothing indexed, when a list id lies
// outside [0, nlist): the callers refuse such rows before they get here, and an id that slipped through must not index cur / off.
static bool ivf_sort(const std::vector<int>& assign, int nlist, std::vector<int64_t>& perm, std::vector<int>& off) {
    for (int a : assign) if ((unsigned)a >= (unsigned)nlist) return false;
    off.assign((size_t)nlist + 1, 0);
    for (int a : assign) off[(size_t)a + 1]++;
    for (int l = 0; l < nlist; ++l) off[(size_t)l + 1] += off[(size_t)l];
    std::vector<int> cur(off.begin(), off.end() - 1);
    perm.resize(assign.size());
    for (size_t i = 0; i < assign.size(); ++i) perm[(size_t)cur[(size_t)assign[i]]++] = (int64_t)i;
    return true;
}

// rebuild the list-major layout after adds
static int ivf_prepare(radad_ivf_t h, hipStream_t st) {
    if (!h->dirty) return RADAD_OK;
    const int64_t n = (int64_t)h->assign.size();
    std::vector<int64_t> perm;
    if (!ivf_sort(h->assign, h->nlist, perm, h->loff_host)) { radad_set_error("the index holds a row without a list"); return RADAD_ESTATE; }
    int rc;
    if ((rc = h->lrows.ensure((size_t)n * h->dim * sizeof(float)))) return rc;
    if ((rc = h->lnorm.ensure((size_t)n * sizeof(float)))) return rc;
    if ((rc = h->lids.ensure((size_t)n * sizeof(int64_t)))) return rc;
    if ((rc = h->loff.ensure((size_t)(h->nlist + 1) * sizeof(int)))) return rc;
    if ((rc = h->lmax.ensure((size_t)h->nlist * sizeof(float)))) return rc;
    RADAD_HIP_CHECK(hipMemcpyAsync(h->lids.p, perm.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, st));
    RADAD_HIP_CHECK(hipMemcpyAsync(h->loff.p, h->loff_host.data(), (size_t)(h->nlist + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    if ((rc = radad_knn_reconstruct(h->flat, (const int64_t*)h->lids.p, n, (float*)h->lrows.p, st))) return rc;   // gather by insertion id
    hipLaunchKernelGGL(k_row_sqnorm<float>, dim3((unsigned)ceil_div64(n, 4)), dim3(256), 0, st, (const float*)h->lrows.p, n, h->dim,
                       (float*)h->lnorm.p);
    hipLaunchKernelGGL(k_ivf_list_maxnorm, dim3((unsigned)h->nlist), dim3(256), 0, st, (const float*)h->lnorm.p, (const int*)h->loff.p, (float*)h->lmax.p);
    RADAD_HIP_CHECK(hipGetLastError());
    RADAD_HIP_CHECK(hipStreamSynchronize(st));     // perm / loff_host are host vectors
    h->dirty = false;
    return RADAD_OK;
}

// the list-major copy of the flat store's f16 plane, (re)built when the layout or the plane changed.  false = no plane (dim % 64,
// RADAD_KNN_OPT_HI_PLANE off, no memory): the search stays on the fp32 list scan.
static bool ivf_ensure_plane(radad_ivf_t h, hipStream_t st) {
    radad_knn_t f = h->flat;
    if (!h->opt_hi || h->dim % 64 != 0 || f->ntotal == 0) return false;
    {
        std::lock_guard<std::mutex> lk(f->mu);
        if (!knn_ensure_hi(f, st, true) || !f->hi || f->hi_rows != f->ntotal) return false;
    }
    const int64_t n = (int64_t)h->assign.size();
    if (h->have_hi && h->hi_src == (const void*)f->hi && h->hi_src_rows == f->hi_rows && h->hi_src_epoch == f->tune.plane_rebuilds) return true;
    h->have_hi = false;
    if (h->lhi.ensure((size_t)n * h->dim * 2) || h->lbias.ensure((size_t)n * sizeof(float)) ||
        (f->rscale && h->lscale.ensure((size_t)n * sizeof(float)))) { (void)hipGetLastError(); return false; }
    hipLaunchKernelGGL(k_ivf_gather_plane, dim3((unsigned)ceil_div64(n, 4)), dim3(256), 0, st, (const _Float16*)f->hi, (const float*)f->rscale,
                       (const float*)(f->cmu ? f->rbias : f->ynorm), (const int64_t*)h->lids.p, n, h->dim, (_Float16*)h->lhi.p,
                       f->rscale ? (float*)h->lscale.p : (float*)nullptr, (float*)h->lbias.p);
    if (hipGetLastError() != hipSuccess) return false;
    h->have_hi = true; h->hi_src = f->hi; h->hi_src_rows = f->hi_rows; h->hi_src_epoch = f->tune.plane_rebuilds;
    return true;
}

// the counters of the most recent search (zero when the flat store answered it, or the index held no rows); synchronises with it
static int ivf_last_counts(radad_ivf_t h, int* rejected_out, int* exact_out) {
    int c[2] = {0, 0};
    if (!h->last_exact && h->last_fcount) {
        DeviceGuard g(h->device);
        ivf_wait_searches(h);
        RADAD_HIP_CHECK(hipMemcpy(c, h->last_fcount, sizeof(c), hipMemcpyDeviceToHost));
    }
    *rejected_out = c[0];
    if (exact_out) *exact_out = c[1];
    return RADAD_OK;
}

// ---- the list-scan search: ivf_plan.h decides, the functions below size the buffers and launch, one job each -------------------------
template <typename T>
static inline T* ivf_at(const DevMem& m, size_t off) { return reinterpret_cast<T*>((char*)m.p + off); }

// what the launches of one search share
struct IvfSearch {
    radad_ivf_t h;
    const IvfPlan& p;
    const float* q;                      // [nq, dim]
    float* out_dist; int64_t* out_idx;   // [nq, k]
    hipStream_t st;
    const unsigned long long* admit;     // the admission bitmap, or nullptr: every row is admissible (the unfiltered kernels run)
    IvfPqRule pq;                        // pq.m > 0: one set per query, `admit` is the suspect bitmap (the IVF_ADM_PQ kernels run)
    int adm() const { return !admit ? IVF_ADM_NONE : (pq.m > 0 ? IVF_ADM_PQ : IVF_ADM_BITMAP); }
    int* tasks(size_t off) const { return ivf_at<int>(h->tasks, off); }                            // a sub-array of `tasks` (p.tasks.*)
    template <typename T> T* qbuf(size_t off) const { return ivf_at<T>(h->qbuf, off); }            // ... of `qbuf` (p.qbuf.*)
    int* fcount() const { return qbuf<int>(p.qbuf.fcount); }
    const int64_t* probes() const { return (const int64_t*)h->ws_b.p; }
};

// the plan's three refusals, with the error code and messages they have always had
static int ivf_plan_refused(const char* fn, radad_ivf_t h, const IvfPlan& p) {
    RADAD_REQUIRE(p.status != IVF_PLAN_TOO_MANY_PAIRS, "%s: too many (query, probe) pairs", fn);
    RADAD_REQUIRE(p.status != IVF_PLAN_DIM_TOO_LARGE, "%s: dim %d too large for the list-scan kernel", fn, h->dim);
    RADAD_REQUIRE(p.status != IVF_PLAN_NPROBE_TOO_LARGE, "%s: nprobe %d too large for the exact list scan", fn, p.nprobe);
    return RADAD_OK;
}

// every buffer of the search at the plan's size.  `tasks` (its per-list counters start at zero) and `xarrive` (the arrival counters)
// are cleared when, and only when, they are new memory.
static int ivf_ensure_buffers(radad_ivf_t h, const IvfPlan& p, hipStream_t st) {
    int rc;
    if ((rc = h->admit.ensure(p.admit))) return rc;
    if ((rc = h->pqset.ensure(p.pq_bitset))) return rc;
    if ((rc = h->ws_a.ensure(p.ws_a))) return rc;
    if ((rc = h->ws_b.ensure(p.ws_b))) return rc;
    if ((rc = h->part_s.ensure(p.part_s))) return rc;
    if ((rc = h->part_i.ensure(p.part_i))) return rc;
    if ((rc = h->qbuf.ensure(p.qbuf.bytes))) return rc;
    if ((rc = h->cand_s.ensure(p.cand_s))) return rc;
    if ((rc = h->cand_i.ensure(p.cand_i))) return rc;
    if ((rc = h->xkey.ensure(p.xkey))) return rc;
    if ((rc = h->xid.ensure(p.xid))) return rc;
    // (a buffer that grew is new memory even when hipMalloc hands back the address hipFree just released: compare the sizes.  A grown
    // xarrive's new tail is not zero -- the arrival counters of the slots behind the old size would start anywhere, their queries be
    // merged early or never)
    const size_t tasks_before = h->tasks.bytes, xarrive_before = h->xarrive.bytes;
    if ((rc = h->tasks.ensure(p.tasks.bytes))) return rc;
    if (h->tasks.bytes != tasks_before) RADAD_HIP_CHECK(hipMemsetAsync(h->tasks.p, 0, h->tasks.bytes, st));
    if ((rc = h->xarrive.ensure(p.xarrive))) return rc;
    if (h->xarrive.bytes != xarrive_before) RADAD_HIP_CHECK(hipMemsetAsync(h->xarrive.p, 0, h->xarrive.bytes, st));
    return RADAD_OK;
}

// a trained index without rows: every slot unfilled (id -1, distance +inf; NaN for the exclusion-aware search)
static int ivf_answer_empty(int64_t nq, int k, bool filtered, float* out_dist_dev, int64_t* out_idx_dev, hipStream_t st) {
    hipLaunchKernelGGL(k_fill_f32, dim3((unsigned)ceil_div64(nq * k, 256)), dim3(256), 0, st, out_dist_dev, nq * k,
                       filtered ? __builtin_nanf("") : INFINITY);
    RADAD_HIP_CHECK(hipGetLastError());
    RADAD_HIP_CHECK(hipMemsetAsync(out_idx_dev, 0xff, (size_t)nq * k * sizeof(int64_t), st));
    return RADAD_OK;
}

// the admission bitmap: on the search's stream, behind ivf_prepare (lids changes with every add); the tags and the set are the
// caller's, so nothing of it is kept between calls
static int ivf_launch_admit(const IvfSearch& s, const int64_t* row_tags, const int64_t* excl_sorted, int64_t n_excl) {
    radad_ivf_t h = s.h;
    const int64_t n = (int64_t)h->assign.size(), n_words = s.p.admit_words;
    hipLaunchKernelGGL(k_admit_bitmap<true>, dim3((unsigned)ceil_div64(n_words * 64, 256)), dim3(256), 0, s.st, row_tags,
                       (const int64_t*)h->lids.p, n, excl_sorted, n_excl, (const int*)nullptr, (unsigned long long*)h->admit.p, n_words);
    RADAD_HIP_CHECK(hipGetLastError());
    return RADAD_OK;
}

// the suspect bitmap of the per-query search, where ivf_launch_admit sits for the batch-wide one: clear the hash bitset, hash the
// batch's live tags into it, test every position's tag (the kernels' comment, above).  RADAD_IVF_OPT_PQ_FILTER 0: no pre-pass, the
// bitmap all clear -- every position suspect.
static int ivf_launch_suspect(const IvfSearch& s) {
    radad_ivf_t h = s.h;
    const IvfPlan& p = s.p;
    const int64_t n = (int64_t)h->assign.size(), n_words = p.admit_words;
    if (!h->opt_pq_filter) {
        RADAD_HIP_CHECK(hipMemsetAsync(h->admit.p, 0, p.admit, s.st));
        return RADAD_OK;
    }
    const unsigned mask = (unsigned)(p.pq_bits - 1);
    RADAD_HIP_CHECK(hipMemsetAsync(h->pqset.p, 0, p.pq_bitset, s.st));
    hipLaunchKernelGGL(k_ivf_pq_hash, dim3((unsigned)ceil_div64(p.nq * p.pq_m, 256)), dim3(256), 0, s.st, s.pq.q_tags, s.pq.q_cnt, p.nq, p.pq_m,
                       (unsigned*)h->pqset.p, mask);
    hipLaunchKernelGGL(k_ivf_pq_suspect, dim3((unsigned)ceil_div64(n_words * 64, 256)), dim3(256), 0, s.st, s.pq.row_tags,
                       (const int64_t*)h->lids.p, n, (const unsigned*)h->pqset.p, mask, (unsigned long long*)h->admit.p, n_words);
    RADAD_HIP_CHECK(hipGetLastError());
    return RADAD_OK;
}

// 1) coarse quantiser: the nprobe nearest centroids of every query; 2) the (query, probe) pairs grouped by list on the device,
// <= qcap queries per task (LDS holds qcap query rows)
static int ivf_launch_coarse_group(const IvfSearch& s) {
    radad_ivf_t h = s.h;
    const IvfPlan& p = s.p;
    const hipStream_t st = s.st;
    int rc;
    if ((rc = knn_search_core(h->quant, s.q, RADAD_Q_F32, p.nq, p.nprobe, p.cmargin, (float*)h->ws_a.p, (int64_t*)h->ws_b.p, nullptr, st))) return rc;
    int* d_cnt = s.tasks(p.tasks.cnt); int* d_cur = s.tasks(p.tasks.cur); int* d_nt = s.tasks(p.tasks.nt);
    int* d_tl = s.tasks(p.tasks.tl); int* d_tp = s.tasks(p.tasks.tp); int* d_tc = s.tasks(p.tasks.tc);
    int* d_pq = s.tasks(p.tasks.pq); int* d_ps = s.tasks(p.tasks.ps);
    if (p.group_small) {
        hipLaunchKernelGGL(k_ivf_group_small, dim3(1), dim3(IVF_TASK_THREADS), p.group_lds, st, s.probes(), (int)p.npairs,
                           p.nprobe, h->nlist, p.qcap, d_tl, d_tp, d_tc, d_nt, d_pq, d_ps, (float*)h->part_s.p, (int*)h->part_i.p, p.ksel);
    } else {
        const unsigned pair_blocks = (unsigned)((p.npairs + 255) / 256);
        hipLaunchKernelGGL(k_ivf_count, dim3(pair_blocks), dim3(256), 0, st, s.probes(), p.npairs, h->nlist, d_cnt);
        hipLaunchKernelGGL(k_ivf_tasks, dim3(1), dim3(IVF_TASK_THREADS), 0, st, d_cnt, h->nlist, p.qcap, d_cur, d_tl, d_tp, d_tc, d_nt);
        hipLaunchKernelGGL(k_ivf_scatter, dim3(pair_blocks), dim3(256), 0, st, s.probes(), p.npairs, p.nprobe, h->nlist, d_cur, d_pq, d_ps,
                           (float*)h->part_s.p, (int*)h->part_i.p, p.ksel);
    }
    RADAD_HIP_CHECK(hipGetLastError());
    return RADAD_OK;
}

// what both routes' re-rank shares: the certificate's outputs, the float64 side, the search's outputs
static RefineParams ivf_refine_params(const IvfSearch& s) {
    radad_ivf_t h = s.h;
    const IvfPlan& p = s.p;
    RefineParams m;
    m.k = p.k; m.dim = h->dim; m.l2 = 1; m.cap = p.cap; m.eps = s.qbuf<float>(p.qbuf.eps);
    m.flag_count = s.fcount(); m.flag_sel = s.qbuf<int>(p.qbuf.fsel); m.nq = p.nq;
    m.db = h->lrows.p; m.q = s.q; m.id_map = (const int64_t*)h->lids.p;
    m.out_dist = s.out_dist; m.out_idx = s.out_idx;
    return m;
}

// 3a) the certified f16 list scan: k_hi_rows on the queries (f16 side, eps; it zeroes cand_cnt, gbound and the counters),
//     k_ivf_scan_hi (emit mode), k_merge_refine<true> with the certificate
static int ivf_launch_hi_route(const IvfSearch& s) {
    radad_ivf_t h = s.h;
    const IvfPlan& p = s.p;
    const hipStream_t st = s.st;
    radad_knn_t f = h->flat;
    _Float16* qh = s.qbuf<_Float16>(p.qbuf.qh);
    float* qscale = s.qbuf<float>(p.qbuf.qscale); float* qconst = s.qbuf<float>(p.qbuf.qconst);
    float* eps = s.qbuf<float>(p.qbuf.eps);
    int* cand_cnt = s.qbuf<int>(p.qbuf.cand_cnt); unsigned* gbound = s.qbuf<unsigned>(p.qbuf.gbound);
    HiRowsParams hp;
    hp.in = s.q; hp.hi = qh; hp.scale_out = qscale; hp.eps_out = eps; hp.ystat = f->stat;
    hp.n = p.nq; hp.dim = h->dim; hp.fixed_e = HI_E_PER_ROW; hp.l2 = 1;
    hp.zero_flags = cand_cnt; hp.zero_flags2 = (int*)gbound; hp.zero_counters = s.fcount();
    hp.mu = f->cmu; hp.mu_norm = f->cmu ? f->mu_norm : 0.f; hp.mu_sq = f->cmu ? f->mu_sq : 0.f; hp.biased = 1;
    hp.qconst_out = qconst;
    launch_hi_rows(hp, st);
    IvfHiParams ip;
    ip.lhi = (const _Float16*)h->lhi.p; ip.lscale = f->rscale ? (const float*)h->lscale.p : nullptr;
    ip.uscale = f->uniform_e != HI_E_PER_ROW ? ldexpf(1.0f, -f->uniform_e) : 1.0f;
    ip.lbias = (const float*)h->lbias.p; ip.loff = (const int*)h->loff.p; ip.qh = qh; ip.qscale = qscale; ip.qconst = qconst; ip.eps = eps;
    ip.task_list = s.tasks(p.tasks.tl); ip.task_pbeg = s.tasks(p.tasks.tp); ip.task_cnt = s.tasks(p.tasks.tc);
    ip.n_tasks_dev = s.tasks(p.tasks.nt); ip.pair_q = s.tasks(p.tasks.pq);
    ip.split = p.split;
    ip.dim = h->dim; ip.k = p.k; ip.qcap = p.qcap; ip.gbound = gbound; ip.cand_cnt = cand_cnt; ip.cand_cap = p.ccap;
    ip.cand_score = (float*)h->cand_s.p; ip.cand_idx = (int*)h->cand_i.p; ip.admit = s.admit; ip.pq = s.pq;
    auto scan = [&](auto kern) -> int {
        RADAD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.scan_lds));
        hipLaunchKernelGGL(kern, dim3((unsigned)p.scan_grid), dim3(SQ_THREADS), p.scan_lds, st, ip);
        return RADAD_OK;
    };
    int rc;
    switch (s.adm()) {
        case IVF_ADM_PQ: rc = scan(k_ivf_scan_hi<IVF_ADM_PQ>); break;
        case IVF_ADM_BITMAP: rc = scan(k_ivf_scan_hi<IVF_ADM_BITMAP>); break;
        default: rc = scan(k_ivf_scan_hi<IVF_ADM_NONE>);
    }
    if (rc) return rc;
    RefineParams m = ivf_refine_params(s);
    m.score = (const float*)h->cand_s.p; m.idx = (const int*)h->cand_i.p; m.n_parts = 1; m.part_len = p.ccap; m.part_cnt = cand_cnt;
    if (p.refine_lds > 48 * 1024)
        RADAD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_merge_refine<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.refine_lds));
    hipLaunchKernelGGL(k_merge_refine<true>, dim3((unsigned)p.nq), dim3(RF_THREADS), p.refine_lds, st, m);
    if (h->opt_hi == 2) {       // (tests) every query counts as rejected: the exact scan answers them all (ivf_launch_exact: slot s = query s)
        float all;
        const int in = (int)p.nq;
        memcpy(&all, &in, 4);
        hipLaunchKernelGGL(k_fill_f32, dim3(1), dim3(256), 0, st, (float*)s.fcount(), (int64_t)1, all);
    }
    RADAD_HIP_CHECK(hipGetLastError());
    return RADAD_OK;
}

// 3b) the fp32 list scan (no f16 plane: dim % 64 != 0, RADAD_IVF_OPT_HI_SCAN 0): k_ivf_f32_eps (it zeroes the counters), then every
//     touched list once, k + 6 entries per (query, list); k_merge_refine re-scores in float64 everything within 2 eps of the k-th best
//     fp32 score and certifies the query unless a full list lies entirely inside that band (it may hide more) or the band holds more
//     than `cap` rows
static int ivf_launch_f32_route(const IvfSearch& s) {
    radad_ivf_t h = s.h;
    const IvfPlan& p = s.p;
    const hipStream_t st = s.st;
    hipLaunchKernelGGL(k_ivf_f32_eps, dim3((unsigned)ceil_div64(p.nq, 4)), dim3(256), 0, st, s.q, p.nq, h->dim, s.probes(), p.nprobe, h->nlist,
                       (const float*)h->lmax.p, s.qbuf<float>(p.qbuf.eps), s.fcount());
    IvfScanParams sp;
    sp.lrows = (const float*)h->lrows.p; sp.lnorm = (const float*)h->lnorm.p; sp.loff = (const int*)h->loff.p; sp.q = s.q;
    sp.task_list = s.tasks(p.tasks.tl); sp.task_pbeg = s.tasks(p.tasks.tp); sp.task_cnt = s.tasks(p.tasks.tc);
    sp.n_tasks_dev = s.tasks(p.tasks.nt); sp.pair_q = s.tasks(p.tasks.pq); sp.pair_slot = s.tasks(p.tasks.ps);
    sp.dim = h->dim; sp.k = p.ksel; sp.qcap = p.qcap;
    sp.part_score = (float*)h->part_s.p; sp.part_idx = (int*)h->part_i.p; sp.admit = s.admit; sp.pq = s.pq;
    auto scan = [&](auto kern) -> int {
        RADAD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.scan_lds));
        hipLaunchKernelGGL(kern, dim3((unsigned)p.scan_grid), dim3(SQ_THREADS), p.scan_lds, st, sp);
        return RADAD_OK;
    };
    int rc;
    const int adm = s.adm();
    if (p.ksel <= 16) rc = adm == IVF_ADM_PQ ? scan(k_ivf_scan<16, IVF_ADM_PQ>) : (adm ? scan(k_ivf_scan<16, IVF_ADM_BITMAP>) : scan(k_ivf_scan<16, IVF_ADM_NONE>));
    else rc = adm == IVF_ADM_PQ ? scan(k_ivf_scan<32, IVF_ADM_PQ>) : (adm ? scan(k_ivf_scan<32, IVF_ADM_BITMAP>) : scan(k_ivf_scan<32, IVF_ADM_NONE>));
    if (rc) return rc;
    RefineParams m = ivf_refine_params(s);
    m.score = (const float*)h->part_s.p; m.idx = (const int*)h->part_i.p; m.n_parts = p.nprobe; m.part_len = p.ksel;
    hipLaunchKernelGGL(k_merge_refine<false>, dim3((unsigned)p.nq), dim3(RF_THREADS), p.refine_lds, st, m);
    RADAD_HIP_CHECK(hipGetLastError());
    return RADAD_OK;
}

// 4) the queries the route's certificate rejected: exact float64 scan of their probed lists (leaves at once when there are none);
//    one launch unless the batch's partial lists exceed IVX_PART_BUDGET
static int ivf_launch_exact(const IvfSearch& s) {
    radad_ivf_t h = s.h;
    const IvfPlan& p = s.p;
    IvfExactParams x;
    x.lrows = (const float*)h->lrows.p; x.lids = (const int64_t*)h->lids.p; x.loff = (const int*)h->loff.p; x.q = s.q;
    // the rejected queries: the certificate's list -- or, where the f16 route declared every query rejected (hi_scan 2), slot s = query s
    x.sel = p.hi_route && h->opt_hi == 2 ? nullptr : s.qbuf<int>(p.qbuf.fsel);
    x.probes = s.probes(); x.count = s.fcount(); x.done = s.fcount() + 1;
    x.dim = h->dim; x.k = p.k; x.nprobe = p.nprobe; x.nlist = h->nlist; x.nslots = (int)p.nslots;
    x.pkey = (double*)h->xkey.p; x.pid = (int64_t*)h->xid.p; x.arrive = (int*)h->xarrive.p;
    x.out_dist = s.out_dist; x.out_idx = s.out_idx; x.admit = s.admit; x.pq = s.pq;
    auto exact = [&](auto kern) -> int {
        RADAD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.xlds));
        for (int64_t i = 0; i < p.xlaunches; ++i) {
            x.slot0 = (int)(i * p.nslots);
            hipLaunchKernelGGL(kern, dim3((unsigned)p.xgrid), dim3(IVX_THREADS), p.xlds, s.st, x);
        }
        RADAD_HIP_CHECK(hipGetLastError());
        return RADAD_OK;
    };
    switch (s.adm()) {
        case IVF_ADM_PQ: return exact(k_ivf_exact<IVF_ADM_PQ>);
        case IVF_ADM_BITMAP: return exact(k_ivf_exact<IVF_ADM_BITMAP>);
        default: return exact(k_ivf_exact<IVF_ADM_NONE>);
    }
}

// unfilled slots of the exclusion-aware search: -1 / NaN, the padding of radad_filter_topk
static int ivf_launch_pad_nan(const IvfSearch& s) {
    hipLaunchKernelGGL(k_ivf_pad_nan, dim3((unsigned)ceil_div64(s.p.nq * s.p.k, 256)), dim3(256), 0, s.st, s.out_dist, (const int64_t*)s.out_idx, s.p.nq * s.p.k);
    RADAD_HIP_CHECK(hipGetLastError());
    return RADAD_OK;
}

// The list-scan search behind radad_ivf_search (filtered = false) and radad_ivf_search_excl (filtered = true).  The caller has
// checked the arguments (k + KNN_MARGIN <= 32); this takes the handle's lock.  filtered: the exact top-k among the rows of the
// probed lists whose tag (row_tags, by insertion id) is not in excl_sorted; unfilled slots -1 / NaN.  With n_excl == 0 every row is
// admissible: the unfiltered kernels run and only the padding differs.
// pq (radad_ivf_search_excl_pq; with filtered, instead of excl_sorted / n_excl): one set per query, pq->m > 0 tags wide (its row_tags,
// q_tags, q_cnt and m are the caller's; lids and tag_off are filled in here).
static int ivf_search_lists(const char* fn, radad_ivf_t h, const float* q_dev, int64_t nq, int k, int nprobe, bool filtered, const int64_t* row_tags,
                            const int64_t* excl_sorted, int64_t n_excl, float* out_dist_dev, int64_t* out_idx_dev, void* stream,
                            const IvfPqRule* pq = nullptr) {
    std::lock_guard<std::mutex> lk(h->mu);
    h->last_exact = false;
    h->last_range = false;
    DeviceGuard g(h->device);
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (!h->ev_done) RADAD_HIP_CHECK(hipEventCreateWithFlags(&h->ev_done, hipEventDisableTiming));
    if (h->have_last && st != h->last_stream) {
        if (hipEventRecord(h->ev_done, h->last_stream) == hipSuccess) RADAD_HIP_CHECK(hipStreamWaitEvent(st, h->ev_done, 0));
        else { (void)hipGetLastError(); RADAD_HIP_CHECK(hipDeviceSynchronize()); }
    }
    if ((rc = ivf_prepare(h, st))) return rc;
    IvfFacts facts;
    facts.dim = h->dim; facts.nlist = h->nlist; facts.rows = (int64_t)h->assign.size();
    if (facts.rows == 0) {
        if ((rc = ivf_answer_empty(nq, k, filtered, out_dist_dev, out_idx_dev, st))) return rc;
        h->last_hi = false; h->last_fcount = nullptr;
        h->last_stream = st; h->have_last = true;
        return RADAD_OK;
    }
    facts.plane = ivf_ensure_plane(h, st);
    const int pq_m = filtered && pq ? pq->m : 0;
    const IvfPlan p = ivf_plan_search(facts, nq, k, nprobe, filtered && (n_excl > 0 || pq_m > 0), pq_m);
    if ((rc = ivf_plan_refused(fn, h, p))) return rc;
    if ((rc = ivf_ensure_buffers(h, p, st))) return rc;

    IvfPqRule rule;
    if (p.pq_m > 0) { rule = *pq; rule.lids = (const int64_t*)h->lids.p; rule.tag_off = (int)(p.scan_lds - p.pq_lds); }
    const IvfSearch s{h, p, q_dev, out_dist_dev, out_idx_dev, st, p.admit_words ? (const unsigned long long*)h->admit.p : nullptr, rule};
    if (p.admit_words && (rc = p.pq_m > 0 ? ivf_launch_suspect(s) : ivf_launch_admit(s, row_tags, excl_sorted, n_excl))) return rc;
    if ((rc = ivf_launch_coarse_group(s))) return rc;
    if ((rc = p.hi_route ? ivf_launch_hi_route(s) : ivf_launch_f32_route(s))) return rc;
    h->last_hi = p.hi_route;
    h->last_fcount = s.fcount();
    if ((rc = ivf_launch_exact(s))) return rc;
    if (filtered && (rc = ivf_launch_pad_nan(s))) return rc;
    h->last_stream = st;
    h->have_last = true;
    return RADAD_OK;
}

// ---- the range search's launches (ivf_plan_range decides; an IvfPlan, so IvfSearch, ivf_ensure_buffers and ivf_launch_coarse_group serve
// as they are) ---------------------------------------------------------------------------------------------------------------------
struct IvfRangeOut { float radius; int32_t* count; float* dist; int64_t* idx; double* key; };

// the instantiation both range kernels run (the scan and the exact pass behind it always the same one).  Unlike IvfSearch::adm, the
// per-query form has no bitmap: pq.m > 0 alone selects it.
static int ivf_range_adm(const IvfSearch& s) { return s.pq.m > 0 ? IVF_ADM_PQ : (s.admit ? IVF_ADM_BITMAP : IVF_ADM_NONE); }

// IVF_RANGE_HI: the top-k hi route's query preparation (k_hi_rows: f16 side, eps; it zeroes cand_cnt and the 8 counters), the floors,
// the scan, the re-rank
static int ivf_launch_range_hi(const IvfSearch& s, const IvfRangeOut& o) {
    radad_ivf_t h = s.h;
    const IvfPlan& p = s.p;
    const hipStream_t st = s.st;
    radad_knn_t f = h->flat;
    _Float16* qh = s.qbuf<_Float16>(p.qbuf.qh);
    float* qscale = s.qbuf<float>(p.qbuf.qscale); float* qconst = s.qbuf<float>(p.qbuf.qconst);
    float* eps = s.qbuf<float>(p.qbuf.eps); float* thr = s.qbuf<float>(p.qbuf_thr);
    int* cand_cnt = s.qbuf<int>(p.qbuf.cand_cnt);
    HiRowsParams hp;
    hp.in = s.q; hp.hi = qh; hp.scale_out = qscale; hp.eps_out = eps; hp.ystat = f->stat;
    hp.n = p.nq; hp.dim = h->dim; hp.fixed_e = HI_E_PER_ROW; hp.l2 = 1;
    hp.zero_flags = cand_cnt; hp.zero_counters = s.fcount();
    hp.mu = f->cmu; hp.mu_norm = f->cmu ? f->mu_norm : 0.f; hp.mu_sq = f->cmu ? f->mu_sq : 0.f; hp.biased = 1;
    hp.qconst_out = qconst;
    launch_hi_rows(hp, st);
    hipLaunchKernelGGL(k_range_floor, dim3((unsigned)ceil_div64(p.nq, 256)), dim3(256), 0, st, (const float*)eps, -o.radius, thr, p.nq);
    IvfRangeHiParams ip;
    ip.lhi = (const _Float16*)h->lhi.p; ip.lscale = f->rscale ? (const float*)h->lscale.p : nullptr;
    ip.uscale = f->uniform_e != HI_E_PER_ROW ? ldexpf(1.0f, -f->uniform_e) : 1.0f;
    ip.lbias = (const float*)h->lbias.p; ip.loff = (const int*)h->loff.p; ip.qh = qh; ip.qscale = qscale; ip.qconst = qconst; ip.thr = thr;
    ip.task_list = s.tasks(p.tasks.tl); ip.task_pbeg = s.tasks(p.tasks.tp); ip.task_cnt = s.tasks(p.tasks.tc);
    ip.n_tasks_dev = s.tasks(p.tasks.nt); ip.pair_q = s.tasks(p.tasks.pq);
    ip.dim = h->dim; ip.qcap = p.qcap; ip.split = p.split;
    ip.cand_cnt = cand_cnt; ip.cand_cap = p.ccap; ip.cand_idx = (int*)h->cand_i.p; ip.admit = s.admit; ip.pq = s.pq;
    auto scan = [&](auto kern) -> int {
        RADAD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.scan_lds));
        hipLaunchKernelGGL(kern, dim3((unsigned)p.scan_grid), dim3(SQ_THREADS), p.scan_lds, st, ip);
        return RADAD_OK;
    };
    int rc;
    switch (ivf_range_adm(s)) {
        case IVF_ADM_PQ: rc = scan(k_ivf_range_hi<IVF_ADM_PQ>); break;
        case IVF_ADM_BITMAP: rc = scan(k_ivf_range_hi<IVF_ADM_BITMAP>); break;
        default: rc = scan(k_ivf_range_hi<IVF_ADM_NONE>);
    }
    if (rc) return rc;
    IvfRangeRefineParams g;
    g.idx = (const int*)h->cand_i.p; g.cnt = cand_cnt; g.cap = p.ccap; g.dim = h->dim; g.m = p.k;
    g.lrows = (const float*)h->lrows.p; g.lids = (const int64_t*)h->lids.p; g.n_pos = (int64_t)h->assign.size(); g.q = s.q;
    g.radius = (double)o.radius; g.flag_count = s.fcount(); g.flag_sel = s.qbuf<int>(p.qbuf.fsel);
    g.out_count = o.count; g.out_dist = o.dist; g.out_idx = o.idx; g.out_key = o.key;
    RADAD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ivf_range_refine), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.refine_lds));
    hipLaunchKernelGGL(k_ivf_range_refine, dim3((unsigned)p.nq), dim3(RF_THREADS), p.refine_lds, st, g);
    RADAD_HIP_CHECK(hipGetLastError());
    return RADAD_OK;
}

// every query of the batch listed for the exact pass, its count zero: IVF_RANGE_EXACT (fresh: the 8 counters are cleared here), or
// behind the hi route under RADAD_IVF_OPT_HI_SCAN 2 (the counters keep what the re-rank recorded)
static int ivf_launch_range_list_all(const IvfSearch& s, const IvfRangeOut& o, bool fresh) {
    if (fresh) RADAD_HIP_CHECK(hipMemsetAsync(s.fcount(), 0, 8 * sizeof(int), s.st));
    RADAD_HIP_CHECK(hipMemsetAsync(o.count, 0, (size_t)s.p.nq * sizeof(int32_t), s.st));
    knn_launch_list_all(s.qbuf<int>(s.p.qbuf.fsel), s.fcount(), s.p.nq, s.st);
    RADAD_HIP_CHECK(hipGetLastError());
    return RADAD_OK;
}

// the listed queries: k_ivf_range_exact, driven from the device (it leaves at once when nobody is listed); one launch unless the
// batch's partial lists exceed IVX_PART_BUDGET
static int ivf_launch_range_exact(const IvfSearch& s, const IvfRangeOut& o) {
    radad_ivf_t h = s.h;
    const IvfPlan& p = s.p;
    IvfRangeExactParams x;
    x.lrows = (const float*)h->lrows.p; x.lids = (const int64_t*)h->lids.p; x.loff = (const int*)h->loff.p; x.q = s.q;
    x.probes = s.probes(); x.sel = s.qbuf<int>(p.qbuf.fsel); x.count = s.fcount(); x.done = s.fcount() + 1;
    x.dim = h->dim; x.m = p.k; x.nprobe = p.nprobe; x.nlist = h->nlist; x.nslots = (int)p.nslots; x.radius = (double)o.radius;
    x.pkey = (double*)h->xkey.p; x.pid = (int64_t*)h->xid.p; x.arrive = (int*)h->xarrive.p;
    x.out_count = o.count; x.out_dist = o.dist; x.out_idx = o.idx; x.out_key = o.key; x.admit = s.admit; x.pq = s.pq;
    auto exact = [&](auto kern) -> int {
        RADAD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.xlds));
        for (int64_t i = 0; i < p.xlaunches; ++i) {
            x.slot0 = (int)(i * p.nslots);
            hipLaunchKernelGGL(kern, dim3((unsigned)p.xgrid), dim3(IVX_THREADS), p.xlds, s.st, x);
        }
        RADAD_HIP_CHECK(hipGetLastError());
        return RADAD_OK;
    };
    switch (ivf_range_adm(s)) {
        case IVF_ADM_PQ: return exact(k_ivf_range_exact<IVF_ADM_PQ>);
        case IVF_ADM_BITMAP: return exact(k_ivf_range_exact<IVF_ADM_BITMAP>);
        default: return exact(k_ivf_range_exact<IVF_ADM_NONE>);
    }
}

// The range search behind radad_ivf_range_search, beside ivf_search_lists: the same ordering, preparation, plane, buffers, coarse
// search and grouping; then the route's launches.  The caller has checked the arguments; this takes the handle's lock.
// The exclusion arguments are ivf_search_lists's: row_tags with excl_sorted / n_excl (radad_ivf_range_search_excl; n_excl == 0: every
// row is admissible, the IVF_ADM_NONE kernels run), or pq with pq->m > 0 (radad_ivf_range_search_excl_pq: its row_tags, q_tags, q_cnt
// and m are the caller's; lids and tag_off are filled in here).  The bitmap of the batch-wide form is built by ivf_launch_admit on the
// call's stream behind ivf_prepare; the per-query form has no pre-pass.
static int ivf_range_lists(const char* fn, radad_ivf_t h, const float* q_dev, int64_t nq, int nprobe, int m, const IvfRangeOut& o, void* stream,
                           const int64_t* row_tags = nullptr, const int64_t* excl_sorted = nullptr, int64_t n_excl = 0, const IvfPqRule* pq = nullptr) {
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (!h->ev_done) RADAD_HIP_CHECK(hipEventCreateWithFlags(&h->ev_done, hipEventDisableTiming));
    if (h->have_last && st != h->last_stream) {
        if (hipEventRecord(h->ev_done, h->last_stream) == hipSuccess) RADAD_HIP_CHECK(hipStreamWaitEvent(st, h->ev_done, 0));
        else { (void)hipGetLastError(); RADAD_HIP_CHECK(hipDeviceSynchronize()); }
    }
    if ((rc = ivf_prepare(h, st))) return rc;
    IvfFacts facts;
    facts.dim = h->dim; facts.nlist = h->nlist; facts.rows = (int64_t)h->assign.size();
    if (facts.rows == 0) {                               // count 0 and the padding (an all-ones float64 is a NaN too)
        RADAD_HIP_CHECK(hipMemsetAsync(o.count, 0, (size_t)nq * sizeof(int32_t), st));
        if ((rc = ivf_answer_empty(nq, m, true, o.dist, o.idx, st))) return rc;
        if (o.key) RADAD_HIP_CHECK(hipMemsetAsync(o.key, 0xff, (size_t)nq * m * sizeof(double), st));
        h->last_exact = false; h->last_hi = false; h->last_fcount = nullptr;
        h->last_range = true; h->last_range_nq = nq; h->last_range_route = IVF_RANGE_EXACT;
        h->last_stream = st; h->have_last = true;
        return RADAD_OK;
    }
    facts.plane = ivf_ensure_plane(h, st);
    const int pq_m = pq ? pq->m : 0;
    const IvfPlan p = ivf_plan_range(facts, nq, m, nprobe, n_excl > 0 || pq_m > 0, pq_m);
    if ((rc = ivf_plan_refused(fn, h, p))) return rc;
    if ((rc = ivf_ensure_buffers(h, p, st))) return rc;
    IvfPqRule rule;
    if (p.pq_m > 0) { rule = *pq; rule.lids = (const int64_t*)h->lids.p; rule.tag_off = (int)(p.scan_lds - p.pq_lds); }
    const IvfSearch s{h, p, q_dev, o.dist, o.idx, st, p.admit_words ? (const unsigned long long*)h->admit.p : nullptr, rule};
    if (p.admit_words && (rc = ivf_launch_admit(s, row_tags, excl_sorted, n_excl))) return rc;
    if ((rc = ivf_launch_coarse_group(s))) return rc;
    const bool hi = p.range_route == IVF_RANGE_HI;
    if (hi && (rc = ivf_launch_range_hi(s, o))) return rc;
    if ((!hi || h->opt_hi == 2) && (rc = ivf_launch_range_list_all(s, o, !hi))) return rc;
    if ((rc = ivf_launch_range_exact(s, o))) return rc;
    h->last_exact = false; h->last_hi = hi; h->last_fcount = s.fcount();
    h->last_range = true; h->last_range_nq = nq; h->last_range_route = p.range_route;
    h->last_stream = st;
    h->have_last = true;
    return RADAD_OK;
}

extern "C" {

int radad_ivf_range_search(radad_ivf_t h, const float* q_dev, int64_t nq, int nprobe, float radius, int max_per_query, int32_t* out_count_dev,
                           float* out_dist_dev, int64_t* out_idx_dev, double* out_key_dev, void* stream) {
    const char* fn = "radad_ivf_range_search";
    RADAD_REQUIRE(h, "%s: NULL handle", fn);
    if (!h->trained) { radad_set_error("%s: the index is not trained", fn); return RADAD_ESTATE; }
    RADAD_REQUIRE(max_per_query >= 1 && max_per_query <= IVF_MAX_K, "%s: max_per_query=%d outside [1,%d]", fn, max_per_query, IVF_MAX_K);
    RADAD_REQUIRE(radius == radius, "%s: the radius is NaN", fn);
    RADAD_REQUIRE(nq >= 0 && nq < (1 << 24), "%s: bad nq", fn);
    RADAD_REQUIRE(nprobe >= 1, "%s: nprobe=%d must be >= 1", fn, nprobe);
    if (nq == 0) return RADAD_OK;
    RADAD_REQUIRE(q_dev && out_count_dev && out_dist_dev && out_idx_dev, "%s: NULL buffer", fn);
    const IvfRangeOut o{radius, out_count_dev, out_dist_dev, out_idx_dev, out_key_dev};
    return ivf_range_lists(fn, h, q_dev, nq, nprobe, max_per_query, o, stream);
}

// The range search among the admissible rows of the probed lists (the header's contract): ivf_range_lists with one set for the batch.
int radad_ivf_range_search_excl(radad_ivf_t h, const float* q_dev, int64_t nq, int nprobe, float radius, int max_per_query,
                                const int64_t* row_tags_dev, const int64_t* excl_sorted_dev, int64_t n_excl, int32_t* out_count_dev,
                                float* out_dist_dev, int64_t* out_idx_dev, double* out_key_dev, void* stream) {
    const char* fn = "radad_ivf_range_search_excl";
    RADAD_REQUIRE(h, "%s: NULL handle", fn);
    if (!h->trained) { radad_set_error("%s: the index is not trained", fn); return RADAD_ESTATE; }
    RADAD_REQUIRE(max_per_query >= 1 && max_per_query <= IVF_MAX_K, "%s: max_per_query=%d outside [1,%d]", fn, max_per_query, IVF_MAX_K);
    RADAD_REQUIRE(radius == radius, "%s: the radius is NaN", fn);
    RADAD_REQUIRE(nq >= 0 && nq < (1 << 24), "%s: bad nq", fn);
    RADAD_REQUIRE(nprobe >= 1, "%s: nprobe=%d must be >= 1", fn, nprobe);
    RADAD_REQUIRE(n_excl >= 0, "%s: n_excl=%lld is negative", fn, (long long)n_excl);
    if (nq == 0) return RADAD_OK;
    RADAD_REQUIRE(q_dev && out_count_dev && out_dist_dev && out_idx_dev, "%s: NULL buffer", fn);
    RADAD_REQUIRE(n_excl == 0 || (row_tags_dev && excl_sorted_dev), "%s: row_tags_dev / excl_sorted_dev may be NULL only when n_excl == 0", fn);
    const IvfRangeOut o{radius, out_count_dev, out_dist_dev, out_idx_dev, out_key_dev};
    return ivf_range_lists(fn, h, q_dev, nq, nprobe, max_per_query, o, stream, row_tags_dev, excl_sorted_dev, n_excl);
}

// ... with one set per query: the IVF_ADM_PQ kernels, no pre-pass.  m == 0: nothing is excluded, the plain kernels run.
int radad_ivf_range_search_excl_pq(radad_ivf_t h, const float* q_dev, int64_t nq, int nprobe, float radius, int max_per_query,
                                   const int64_t* row_tags_dev, const int64_t* q_tags_dev, int m, const int32_t* q_tag_counts_dev,
                                   int32_t* out_count_dev, float* out_dist_dev, int64_t* out_idx_dev, double* out_key_dev, void* stream) {
    const char* fn = "radad_ivf_range_search_excl_pq";
    RADAD_REQUIRE(h, "%s: NULL handle", fn);
    if (!h->trained) { radad_set_error("%s: the index is not trained", fn); return RADAD_ESTATE; }
    RADAD_REQUIRE(max_per_query >= 1 && max_per_query <= IVF_MAX_K, "%s: max_per_query=%d outside [1,%d]", fn, max_per_query, IVF_MAX_K);
    RADAD_REQUIRE(radius == radius, "%s: the radius is NaN", fn);
    RADAD_REQUIRE(nq >= 0 && nq < (1 << 24), "%s: bad nq", fn);
    RADAD_REQUIRE(nprobe >= 1, "%s: nprobe=%d must be >= 1", fn, nprobe);
    RADAD_REQUIRE(m >= 0 && m <= RADAD_EXCL_PQ_MAX_TAGS, "%s: m=%d tags per query outside [0,%d] (RADAD_EXCL_PQ_MAX_TAGS)", fn, m, RADAD_EXCL_PQ_MAX_TAGS);
    if (nq == 0) return RADAD_OK;             // (an empty batch has no tags to point at)
    RADAD_REQUIRE(q_dev && out_count_dev && out_dist_dev && out_idx_dev, "%s: NULL buffer", fn);
    RADAD_REQUIRE(m == 0 || (q_tags_dev && row_tags_dev), "%s: %d tags per query need the query tags and the row tags", fn, m);
    const IvfRangeOut o{radius, out_count_dev, out_dist_dev, out_idx_dev, out_key_dev};
    IvfPqRule rule;
    rule.row_tags = row_tags_dev; rule.q_tags = q_tags_dev; rule.q_cnt = m > 0 ? (const int*)q_tag_counts_dev : nullptr; rule.m = m;
    return ivf_range_lists(fn, h, q_dev, nq, nprobe, max_per_query, o, stream, row_tags_dev, nullptr, 0, &rule);
}

int radad_ivf_last_range(radad_ivf_t h, int64_t* n_queries, int* route, int* n_exact, int* max_emitted) {
    RADAD_REQUIRE(h, "radad_ivf_last_range: NULL handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->last_range) { radad_set_error("radad_ivf_last_range: the most recent search of this index was not a range search"); return RADAD_ESTATE; }
    int c[3] = {0, 0, 0};
    if (h->last_fcount) {
        DeviceGuard g(h->device);
        ivf_wait_searches(h);
        RADAD_HIP_CHECK(hipMemcpy(c, h->last_fcount, sizeof(c), hipMemcpyDeviceToHost));
    }
    if (n_queries) *n_queries = h->last_range_nq;
    if (route) *route = h->last_range_route;
    if (n_exact) *n_exact = c[1];
    if (max_emitted) *max_emitted = c[2];
    return RADAD_OK;
}

int radad_ivf_create(int dim, int nlist, int device, radad_ivf_t* out) {
    RADAD_REQUIRE(out, "radad_ivf_create: out is NULL");
    RADAD_REQUIRE(dim > 0 && dim % 32 == 0, "radad_ivf_create: dim must be a positive multiple of 32 (got %d)", dim);
    RADAD_REQUIRE(nlist >= 1 && nlist <= (1 << 20), "radad_ivf_create: nlist out of range");
    radad_ivf_s* h = new (std::nothrow) radad_ivf_s();
    if (!h) { radad_set_error("out of host memory"); return RADAD_ENOMEM; }
    h->dim = dim; h->nlist = nlist; h->device = device;
    int rc = radad_knn_create(dim, RADAD_METRIC_L2, device, 0, &h->flat);      // L2: rows stored verbatim (+ |y|^2); also answers k > 26
    if (!rc) {
        DeviceGuard g(device);
        if (hipMalloc((void**)&h->centroids, (size_t)nlist * dim * sizeof(float)) != hipSuccess) { radad_set_error("hipMalloc failed"); rc = RADAD_ENOMEM; }
    }
    if (rc) { radad_ivf_destroy(h); return rc; }
    *out = h;
    return RADAD_OK;
}

int radad_ivf_destroy(radad_ivf_t h) {
    if (!h) return RADAD_OK;
    if (h->quant) radad_knn_destroy(h->quant);
    if (h->flat) radad_knn_destroy(h->flat);
    {
        DeviceGuard g(h->device);
        if (h->centroids) (void)hipFree(h->centroids);
        h->lrows.release(); h->lnorm.release(); h->lids.release(); h->loff.release();
        h->ws_a.release(); h->ws_b.release(); h->ws_c.release(); h->part_s.release(); h->part_i.release(); h->tasks.release();
        h->lmax.release(); h->xkey.release(); h->xid.release(); h->xarrive.release();
        h->lhi.release(); h->lscale.release(); h->lbias.release(); h->qbuf.release(); h->cand_s.release(); h->cand_i.release();
        h->admit.release(); h->pqset.release();
        if (h->ev_done) { (void)hipDeviceSynchronize(); (void)hipEventDestroy(h->ev_done); }
    }
    delete h;
    return RADAD_OK;
}

int radad_ivf_is_trained(radad_ivf_t h, int* trained) { RADAD_REQUIRE(h && trained, "NULL argument"); *trained = h->trained ? 1 : 0; return RADAD_OK; }
int radad_ivf_ntotal(radad_ivf_t h, int64_t* n) { RADAD_REQUIRE(h && n, "NULL argument"); *n = (int64_t)h->assign.size(); return RADAD_OK; }
int radad_ivf_nlist(radad_ivf_t h, int* nlist) { RADAD_REQUIRE(h && nlist, "NULL argument"); *nlist = h->nlist; return RADAD_OK; }

// Lloyd iterations on the device (assignment = flat L2 scan over the centroids, update = deterministic per-list mean of
// the list-sorted rows).  Initial centroids: n_train / nlist-strided rows.  Empty clusters keep their centroid.
// The iterations run on a centroid buffer and a quantiser of their own (`cent`, *quant_out); radad_ivf_train installs them when all
// of it went well, so a refused training set leaves the index as it was.
static int ivf_train_into(radad_ivf_t h, const float* rows_dev, int64_t n, int niter, hipStream_t st, float* cent, radad_knn_t* quant_out) {
    int rc;
    // initial centroids: row (c * n) / nlist (repeats when n < nlist, as good as any for a degenerate training set)
    {
        std::vector<int64_t> pick((size_t)h->nlist);
        for (int c = 0; c < h->nlist; ++c) pick[(size_t)c] = ((int64_t)c * n) / h->nlist;
        if ((rc = h->ws_b.ensure((size_t)std::max<int64_t>(n, h->nlist) * sizeof(int64_t)))) return rc;
        RADAD_HIP_CHECK(hipMemcpyAsync(h->ws_b.p, pick.data(), pick.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_gather_rows<float>, dim3((unsigned)ceil_div64(h->nlist, 4)), dim3(256), 0, st, rows_dev,
                           (const int64_t*)h->ws_b.p, (int64_t)h->nlist, n, (int64_t)0, h->dim, cent);
        RADAD_HIP_CHECK(hipGetLastError());
        // the picked rows must be finite whatever niter is: with niter = 0 they are the centroids, and no assignment looks at them
        std::vector<float> host((size_t)h->nlist * h->dim);
        RADAD_HIP_CHECK(hipMemcpyAsync(host.data(), cent, host.size() * sizeof(float), hipMemcpyDeviceToHost, st));
        RADAD_HIP_CHECK(hipStreamSynchronize(st));
        for (size_t i = 0; i < host.size(); ++i)
            RADAD_REQUIRE(std::isfinite(host[i]), "radad_ivf_train: training row %lld (the initial centroid of list %lld) is not finite",
                          (long long)pick[i / (size_t)h->dim], (long long)(i / (size_t)h->dim));
    }
    std::vector<int> assign, off;
    std::vector<int64_t> perm;
    for (int it = 0; it < niter; ++it) {
        if (*quant_out) { radad_knn_destroy(*quant_out); *quant_out = nullptr; }
        if ((rc = ivf_make_quantizer(h, cent, st, quant_out))) return rc;
        int64_t bad = -1;
        if ((rc = ivf_assign(h, *quant_out, rows_dev, n, assign, &bad, st))) return rc;
        RADAD_REQUIRE(bad < 0, "radad_ivf_train: training row %lld is not finite (no nearest centroid)", (long long)bad);
        RADAD_REQUIRE(ivf_sort(assign, h->nlist, perm, off), "radad_ivf_train: a training row has no list");
        if ((rc = h->ws_c.ensure((size_t)n * h->dim * sizeof(float)))) return rc;
        if ((rc = h->ws_b.ensure((size_t)n * sizeof(int64_t)))) return rc;
        if ((rc = h->loff.ensure((size_t)(h->nlist + 1) * sizeof(int)))) return rc;
        RADAD_HIP_CHECK(hipMemcpyAsync(h->ws_b.p, perm.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, st));
        RADAD_HIP_CHECK(hipMemcpyAsync(h->loff.p, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_gather_rows<float>, dim3((unsigned)ceil_div64(n, 4)), dim3(256), 0, st, rows_dev, (const int64_t*)h->ws_b.p,
                           n, n, (int64_t)0, h->dim, (float*)h->ws_c.p);
        hipLaunchKernelGGL(k_centroid_update, dim3((unsigned)h->nlist, (unsigned)((h->dim + 255) / 256)), dim3(256), 0, st,
                           (const float*)h->ws_c.p, (const int*)h->loff.p, h->dim, cent);
        RADAD_HIP_CHECK(hipGetLastError());
        RADAD_HIP_CHECK(hipStreamSynchronize(st));
    }
    if (*quant_out) { radad_knn_destroy(*quant_out); *quant_out = nullptr; }
    return ivf_make_quantizer(h, cent, st, quant_out);
}

int radad_ivf_train(radad_ivf_t h, const float* rows_dev, int64_t n, int niter, void* stream) {
    RADAD_REQUIRE(h && rows_dev, "radad_ivf_train: NULL argument");
    RADAD_REQUIRE(n >= 1 && niter >= 0, "radad_ivf_train: need at least one training row");
    std::lock_guard<std::mutex> lk(h->mu);
    ivf_wait_searches(h);
    DeviceGuard g(h->device);
    hipStream_t st = (hipStream_t)stream;
    const size_t cbytes = (size_t)h->nlist * h->dim * sizeof(float);
    float* cent = nullptr;
    if (hipMalloc((void**)&cent, cbytes) != hipSuccess) { (void)hipGetLastError(); radad_set_error("hipMalloc of %zu bytes failed", cbytes); return RADAD_ENOMEM; }
    radad_knn_t quant = nullptr;
    int rc = ivf_train_into(h, rows_dev, n, niter, st, cent, &quant);
    if (!rc && (hipMemcpyAsync(h->centroids, cent, cbytes, hipMemcpyDeviceToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)) {
        (void)hipGetLastError();
        radad_set_error("radad_ivf_train: copying the centroids failed");
        rc = RADAD_EHIP;
    }
    if (!rc) {
        if (h->quant) radad_knn_destroy(h->quant);
        h->quant = quant;
        quant = nullptr;
        h->trained = true;
    }
    if (quant) radad_knn_destroy(quant);
    (void)hipStreamSynchronize(st);
    (void)hipFree(cent);
    return rc;
}

int radad_ivf_set_centroids(radad_ivf_t h, const float* centroids_dev, void* stream) {
    RADAD_REQUIRE(h && centroids_dev, "radad_ivf_set_centroids: NULL argument");
    RADAD_REQUIRE(h->assign.empty(), "radad_ivf_set_centroids: index already holds rows");
    std::lock_guard<std::mutex> lk(h->mu);
    ivf_wait_searches(h);
    DeviceGuard g(h->device);
    hipStream_t st = (hipStream_t)stream;
    RADAD_HIP_CHECK(hipMemcpyAsync(h->centroids, centroids_dev, (size_t)h->nlist * h->dim * sizeof(float), hipMemcpyDeviceToDevice, st));
    int rc = ivf_load_quantizer(h, st);
    if (rc) return rc;
    h->trained = true;
    return RADAD_OK;
}

int radad_ivf_centroids(radad_ivf_t h, float* out_dev, void* stream) {
    RADAD_REQUIRE(h && out_dev, "radad_ivf_centroids: NULL argument");
    DeviceGuard g(h->device);
    RADAD_HIP_CHECK(hipMemcpyAsync(out_dev, h->centroids, (size_t)h->nlist * h->dim * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return RADAD_OK;
}

int radad_ivf_assignments_host(radad_ivf_t h, int32_t* out_host, int64_t cap) {
    RADAD_REQUIRE(h && out_host && cap >= (int64_t)h->assign.size(), "radad_ivf_assignments_host: buffer too small");
    memcpy(out_host, h->assign.data(), h->assign.size() * sizeof(int));
    return RADAD_OK;
}

int radad_ivf_add(radad_ivf_t h, const float* rows_dev, int64_t n, void* stream) {
    RADAD_REQUIRE(h, "NULL handle");
    if (n == 0) return RADAD_OK;
    RADAD_REQUIRE(rows_dev && n > 0, "radad_ivf_add: bad argument");
    RADAD_REQUIRE(h->trained, "radad_ivf_add: the index is not trained");
    std::lock_guard<std::mutex> lk(h->mu);
    ivf_wait_searches(h);
    DeviceGuard g(h->device);
    hipStream_t st = (hipStream_t)stream;
    // the assignment comes first: a batch that is refused has appended nothing
    std::vector<int> a;
    int64_t bad = -1;
    int rc = ivf_assign(h, h->quant, rows_dev, n, a, &bad, st);
    if (rc) return rc;
    RADAD_REQUIRE(bad < 0, "radad_ivf_add: row %lld of the batch is not finite (no nearest centroid); nothing was added", (long long)bad);
    if ((rc = radad_knn_add(h->flat, rows_dev, n, st))) return rc;
    h->assign.insert(h->assign.end(), a.begin(), a.end());
    h->dirty = true;
    return RADAD_OK;
}

int radad_ivf_last_search_exact(radad_ivf_t h, int* exact_out) {
    RADAD_REQUIRE(h && exact_out, "radad_ivf_last_search_exact: NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    *exact_out = h->last_exact ? 1 : 0;
    return RADAD_OK;
}

int radad_ivf_set_option(radad_ivf_t h, int option, int value) {
    RADAD_REQUIRE(h, "radad_ivf_set_option: NULL handle");
    std::lock_guard<std::mutex> lk(h->mu);
    RADAD_REQUIRE((option == RADAD_IVF_OPT_HI_SCAN && value >= 0 && value <= 2) || (option == RADAD_IVF_OPT_PQ_FILTER && value >= 0 && value <= 1),
                  "radad_ivf_set_option: unknown option %d or bad value %d", option, value);
    if (option == RADAD_IVF_OPT_HI_SCAN) h->opt_hi = value;
    else h->opt_pq_filter = value;
    return RADAD_OK;
}

int radad_ivf_last_search_info(radad_ivf_t h, int* kind_out, int* rejected_out) {
    RADAD_REQUIRE(h && kind_out && rejected_out, "radad_ivf_last_search_info: NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->last_range) { radad_set_error("radad_ivf_last_search_info: the most recent search of this index was a range search (radad_ivf_last_range)"); return RADAD_ESTATE; }
    *kind_out = h->last_exact ? RADAD_IVF_SCAN_EXACT_FLAT : (h->last_hi ? RADAD_IVF_SCAN_HI : RADAD_IVF_SCAN_F32);
    return ivf_last_counts(h, rejected_out, nullptr);
}

int radad_ivf_last_search_counts(radad_ivf_t h, int* rejected_out, int* exact_out) {
    RADAD_REQUIRE(h && rejected_out && exact_out, "radad_ivf_last_search_counts: NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->last_range) { radad_set_error("radad_ivf_last_search_counts: the most recent search of this index was a range search (radad_ivf_last_range)"); return RADAD_ESTATE; }
    return ivf_last_counts(h, rejected_out, exact_out);
}

int radad_ivf_reconstruct(radad_ivf_t h, const int64_t* idx_dev, int64_t n, float* out_dev, void* stream) {
    RADAD_REQUIRE(h, "NULL handle");
    return radad_knn_reconstruct(h->flat, idx_dev, n, out_dev, stream);
}

int radad_ivf_search(radad_ivf_t h, const float* q_dev, int64_t nq, int k, int nprobe, float* out_dist_dev, int64_t* out_idx_dev,
                     void* stream) {
    RADAD_REQUIRE(h, "NULL handle");
    RADAD_REQUIRE(h->trained, "radad_ivf_search: the index is not trained");
    RADAD_REQUIRE(k >= 1 && k <= IVF_MAX_K, "radad_ivf_search: k=%d outside [1,%d]", k, IVF_MAX_K);
    RADAD_REQUIRE(nq >= 0 && nq < (1 << 24), "radad_ivf_search: bad nq");
    if (nq == 0) return RADAD_OK;
    RADAD_REQUIRE(q_dev && out_dist_dev && out_idx_dev, "radad_ivf_search: NULL buffer");
    // The list scan keeps k + 6 <= 32 candidates per (query, list) pair in registers.  Larger k (faiss takes up to 2048,
    // vector_database.py:169-181) is answered by the EXACT search over the same rows in insertion order (the certified f16 scan of
    // the flat store behind this index): every neighbour an IVF search could return and the ones its probing would miss -- recall
    // 1.0 instead of the probed lists', at the flat scan's cost (~1 ms per 1024 queries x 1 M x 512).
    // faiss returns only rows of the nprobe lists (vector_database.py:174-179); this answer is a SUPERSET of that (and ignores nprobe):
    // the caller can tell from radad_ivf_last_search_exact.
    RADAD_REQUIRE(nprobe >= 1, "radad_ivf_search: nprobe=%d must be >= 1", nprobe);
    if (k + KNN_MARGIN > 32) {
        { std::lock_guard<std::mutex> lk(h->mu); h->last_exact = true; h->last_range = false; }
        return radad_knn_search(h->flat, q_dev, nq, k, out_dist_dev, out_idx_dev, stream);
    }
    return ivf_search_lists("radad_ivf_search", h, q_dev, nq, k, nprobe, false, nullptr, nullptr, 0, out_dist_dev, out_idx_dev, stream);
}

// The exclusion-aware search (pipeline.py:478,491-515 on the probed lists of vector_database.py:174-179): see ivf_search_lists and the
// FILTERED kernels.  k stops at 26, what the list scans hold: forwarding a larger k to the flat store as radad_ivf_search does would
// ignore nprobe and answer another question than the one specified.
int radad_ivf_search_excl(radad_ivf_t h, const float* q_dev, int64_t nq, int k, int nprobe, const int64_t* row_tags_dev,
                          const int64_t* excl_sorted_dev, int64_t n_excl, float* out_dist_dev, int64_t* out_idx_dev, void* stream) {
    RADAD_REQUIRE(h, "NULL handle");
    RADAD_REQUIRE(h->trained, "radad_ivf_search_excl: the index is not trained");
    RADAD_REQUIRE(k >= 1 && k + KNN_MARGIN <= 32, "radad_ivf_search_excl: k=%d outside [1,%d], the range the list scans hold", k, 32 - KNN_MARGIN);
    RADAD_REQUIRE(nq >= 0 && nq < (1 << 24), "radad_ivf_search_excl: bad nq");
    RADAD_REQUIRE(nprobe >= 1, "radad_ivf_search_excl: nprobe=%d must be >= 1", nprobe);
    RADAD_REQUIRE(n_excl >= 0 && (n_excl == 0 || (row_tags_dev && excl_sorted_dev)),
                  "radad_ivf_search_excl: row_tags_dev / excl_sorted_dev may be NULL only when n_excl == 0");
    if (nq == 0) return RADAD_OK;
    RADAD_REQUIRE(q_dev && out_dist_dev && out_idx_dev, "radad_ivf_search_excl: NULL buffer");
    return ivf_search_lists("radad_ivf_search_excl", h, q_dev, nq, k, nprobe, true, row_tags_dev, excl_sorted_dev, n_excl, out_dist_dev, out_idx_dev, stream);
}

// One exclusion set per query (the header's contract): ivf_search_lists with the per-query rule -- the suspect pre-pass where the
// admission bitmap is built, the IVF_ADM_PQ list kernels.  m == 0: nothing is excluded, the unfiltered kernels run.
int radad_ivf_search_excl_pq(radad_ivf_t h, const float* q_dev, int64_t nq, int k, int nprobe, const int64_t* row_tags_dev,
                             const int64_t* q_tags_dev, int m, const int32_t* q_tag_counts_dev, float* out_dist_dev, int64_t* out_idx_dev,
                             void* stream) {
    static_assert(RADAD_EXCL_PQ_MAX_TAGS == IVF_PQ_MAX_TAGS && RADAD_EXCL_PQ_MAX_TAGS <= 64, "lane t of a wave holds tag t (k_ivf_exact)");
    RADAD_REQUIRE(h, "NULL handle");
    RADAD_REQUIRE(h->trained, "radad_ivf_search_excl_pq: the index is not trained");
    RADAD_REQUIRE(k >= 1 && k + KNN_MARGIN <= 32, "radad_ivf_search_excl_pq: k=%d outside [1,%d], the range the list scans hold", k, 32 - KNN_MARGIN);
    RADAD_REQUIRE(nq >= 0 && nq < (1 << 24), "radad_ivf_search_excl_pq: bad nq");
    RADAD_REQUIRE(nprobe >= 1, "radad_ivf_search_excl_pq: nprobe=%d must be >= 1", nprobe);
    RADAD_REQUIRE(m >= 0 && m <= RADAD_EXCL_PQ_MAX_TAGS, "radad_ivf_search_excl_pq: m=%d tags per query outside [0,%d] (RADAD_EXCL_PQ_MAX_TAGS)", m,
                  RADAD_EXCL_PQ_MAX_TAGS);
    RADAD_REQUIRE(m == 0 || (q_tags_dev && row_tags_dev), "radad_ivf_search_excl_pq: %d tags per query need the query tags and the row tags", m);
    if (nq == 0) return RADAD_OK;
    RADAD_REQUIRE(q_dev && out_dist_dev && out_idx_dev, "radad_ivf_search_excl_pq: NULL buffer");
    IvfPqRule rule;
    rule.row_tags = row_tags_dev; rule.q_tags = q_tags_dev; rule.q_cnt = m > 0 ? (const int*)q_tag_counts_dev : nullptr; rule.m = m;
    return ivf_search_lists("radad_ivf_search_excl_pq", h, q_dev, nq, k, nprobe, true, row_tags_dev, nullptr, 0, out_dist_dev, out_idx_dev, stream, &rule);
}

}  // extern "C"
