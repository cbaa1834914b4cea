// knn_hi.inc -- the large-batch scan: ONE f16 MFMA product per element, certified (included by knn.hip inside its
// anonymous namespace).
//
// The scan is only a FILTER in front of the float64 re-rank (k_merge_refine), so it may compute the dot products from
// rounded operands as long as the rounding is BOUNDED and the bound is checked:
//     y -> yh = f16(y 2^ey) 2^-ey          (the "hi plane" of an fp32 store, built once per row; an fp16 store is its own plane)
//     q -> qh = f16(q 2^eq) 2^-eq          (per search)
//     a(q, y) = qh . yh                    (exact f16 products, fp32 accumulate on v_mfma_f32_16x16x32_f16)
//     |a - q.y| <= |q - qh| |y| + |qh| |y - yh| + D 2^-23 |qh| |yh|  =: eps(q)      (Cauchy-Schwarz; the norms are MEASURED:
//                                       |q - qh| per query, max |y|, max |y - yh| per store -- k_hi_rows)
// The scan EMITS every (query, row) whose score reaches the query's admission floor into that query's candidate buffer (one
// global atomic per candidate -- a few hundred per query over the whole scan); there are no per-chunk lists, no slot buffers and
// no drain, so nothing can be "used up" or dropped short of the buffer itself overflowing.  The floor is a score that at least
// k rows are KNOWN to reach, lowered by 2 eps: first the (k + 6)-th best of a sample (k_knn_hi_sample / k_floor_from_sample), then --
// after the first eighth of a large store has been scanned with that -- the k-th best score emitted so far (k_kth_floor).
// k_merge_refine then re-scores in float64 every emitted row with a >= a_k - 2 eps (a_k = the k-th best a; the floor is <= that
// by construction) and certifies the query when its buffer did not overflow.  Certified queries are exactly the float64 brute
// force; the others are counted and searched again by the exact float64 kernel (k_exact_scan), driven from the device.
// (Rounds 1-2 kept a sorted 16-entry list per (query, chunk) behind 8-slot LDS buffers: on unstructured queries the push / drain
// path cost 0.27 of 1.04 ms, a chunk holding more than 16 near-ties or a tile admitting more than 8 rows rejected the query, and
// at the reference's own shape -- 25 423 rows: one tile per chunk, every tile filtered by the sample's floor alone -- most
// queries lost a candidate to a full slot buffer.)
// One product instead of the three of a split-f16 fp32 emulation: 3x less matrix-pipe time and half the extra HBM
// (2 bytes per element beside the fp32 rows, not 4).
//
// Tile: 256 rows x 256 queries per workgroup (8 waves, each 128 rows x 64 queries = 32 accumulator tiles of 16 x 16),
// one workgroup per CU, K stepped 64 elements (128-byte LDS rows) through two 64 KB stages filled by LDS-DMA; XOR
// swizzle on the source side and on the reads (16-byte chunk c of row r lives at chunk c ^ ((r >> 1) & 7)).
// (KW_M x KW_N = 256 x 256, KW_WAVES = 8, KW_THREADS, KW_SAMPLE_LIST: knn_plan.h)
constexpr int KW_OP_BYTES = KW_M * 128;            // one operand of one stage: 256 rows x 128 B
constexpr int KW_STAGE_BYTES = 2 * KW_OP_BYTES;    // A + B



struct KnnHiParams {
    const void* db = nullptr;             // [n][dim] f16: hi plane of an fp32 store, or the rows of an fp16 store
    const float* rscale = nullptr;        // [n] 2^-ey of each row, or nullptr: every row uses `uscale`
    float uscale = 1.f;                   // 2^-ey shared by all rows when rscale == nullptr
    const float* rbias = nullptr;         // RSC 2: [n] per-row bias magnitude: |y'|^2 (L2, bias_sign -1) or mu.y (centred IP / cosine, bias_sign +1)
    float bias_sign = 1.f;
    float mult = 1.f;                     // RSC 2: 2 (L2: score = 2 a - |y'|^2 - |q'|^2 estimates -|q - y|^2) or 1 (IP: a + mu.y + q'.mu estimates q.y)
    const float* qconst = nullptr;        // RSC 2: [nq] per-query constant of the score (-|q'|^2 or q'.mu), or nullptr
    const void* q = nullptr;              // [nq][dim] f16 scaled queries (centred when the plane is)
    const float* qscale = nullptr;        // [nq] 2^-eq
    int64_t n = 0;
    int nq = 0;
    int row_bytes = 0;                    // dim * 2; multiple of 128
    int l2 = 0;
    int n_qtiles = 0;
    int n_splits = 0;                     // multiple of 8
    int64_t chunk_rows = 0;               // rows per split, multiple of KW_M
    int64_t chunk_stride = 0;             // rows between the starts of consecutive splits: chunk_rows, or more (the sample pre-pass spreads its tiles over the store)
    int64_t id_off = 0;                   // reported row = id_off + row inside [db, db + n): a launch may cover a row range of the store
    float* part_score = nullptr;          // sample pre-pass: [nq, n_splits, 16] as 8 holders x 2;  scan: [nq, cand_cap] candidate scores
    int* part_idx = nullptr;              //                                                         ... and rows
    int cand_cap = 0;                     // scan: entries of a query's candidate buffer
    int* cand_cnt = nullptr;              // scan: [nq] candidates emitted so far (may exceed cand_cap: the excess is not stored, the query is rejected)
    const float* thr_init = nullptr;      // [nq] admission floor, or nullptr (-inf)
    // K split over TWO workgroups per tile (small stores of wide rows: the reference's 25 423 x 5376 is 100 tiles of 84 K steps -- 100
    // workgroups on 256 CUs, each a chain of 84 dependent DMA round trips).  Workgroups 2j and 2j + 1 take the first / second half of
    // the K steps of tile j; each publishes its 256 x 256 partial sums; the one that arrives SECOND (device-scope counter) adds the
    // other's and runs the epilogue.  a + b == b + a in fp32: the result does not depend on who arrives first.
    int loose_floor = 0;                  // 1: the counting form of the emit (see the epilogue)
    int ksplit = 1;                       // 1 or 2 (2 only with one tile per workgroup)
    float* kacc = nullptr;                // ksplit 2: [tiles][2][32][512] f32x4 partial accumulators
    int* kflag = nullptr;                 // ksplit 2: [tiles] arrival counters (zero between launches: the second arrival resets its own)
    int debug = 0;                        // timing experiments, only in a -DRADAD_DEBUG_HOOKS build (RADAD_DEBUG_KNN): 1 skip the epilogue,
                                          // 2 skip the DMA issue
    unsigned long long* stamps = nullptr; // -DRADAD_DEBUG_HOOKS only: [2][4096] (tag << 56 | s_memtime) of waves 0 and 4 of workgroup 0
    // (floors raised inside one launch over the whole store were measured slower and removed: DESIGN §4.1)
    // EARLY ABANDON (the ABANDON instantiations only; which launches take them: knn_abandon_launch, knn_plan.h).  All norms are
    // those of the RAW f16 values, i.e. in the accumulators' units, inflated as hi_rows_body inflates its norms.
    int ab_ck = 0;                        // K stages multiplied before the test
    const float* ab_rq = nullptr;         // [nq] |qh_j[64 ck:]|
    const float* ab_slack = nullptr;      // [nq] 2 dim 2^-23 (|qh_j| max |yh| + |c0|max) in true units (x 1 / (2^-eq uscale) in the kernel)
    const float* ab_ry = nullptr;         // [tiles of this launch] max over the tile's rows of |yh_i[64 ck:]|
    const float* ab_b = nullptr;          // RSC 3: [tiles of this launch] max over the tile's rows of bias_sign x bias (what the accumulators start from, x s_qs)
    int* ab_count = nullptr;              // [2] tile tasks tested, tile tasks abandoned (one atomic each per workgroup)
    // DEALT launches (k_knn_hi_abandon_deal; which launches are: knn_abandon_deal, knn_plan.h): a workgroup draws granules of deal_g row
    // tiles from the counter of its (XCD slot, query tile) instead of walking a static chunk
    int deal_g = 0;                       // row tiles per granule (a power of two)
    int deal_tiles = 0;                   // row tiles of this launch
    int* deal_cnt = nullptr;              // [KNN_DEAL_SLOTS][KNN_DEAL_MAX_QTILES] this launch's ticket counters (zeroed once per search: k_hi_rows)
    // DEFERRING launches (k_knn_hi_abandon_defer; which launches are: knn_abandon_defer, knn_plan.h) append a vetoed tile's few live rows
    // to the list of their query tile; the launch's tails (k_knn_hi_rowtail for short lists, k_knn_hi_tail for long ones) read the same
    // three fields
    int* df_cnt = nullptr;                // [KNN_DEFER_MAX_QTILES] entries of each query tile's list, this launch (zeroed once per search: k_hi_rows)
    int* df_list = nullptr;               // [KNN_DEFER_MAX_QTILES][df_cap] launch-relative rows
    int df_cap = 0;                       // row tiles of the launch x KNN_DEFER_MAX_ROWS: a list cannot overflow
    int* df_tasks = nullptr;              // [1] tile tasks deferred (one atomic per workgroup)
    unsigned df_bytes = 0;                // the tails: bytes of the launch's rows (the plane is addressed through ONE 32-bit descriptor)
    // THE HEAD PREFETCH (ABANDON without DEAL; RADAD_KNN_OPT_ABANDON_AHEAD): the checkpoint stage of a tile predicted to leave
    // (knn_ahead_speculate, knn_plan.h) fetches the NEXT tile's stage 0 instead of its own stage ab_ck
    int ab_ahead = 0;
    int* ah_count = nullptr;              // [2] tile tasks that left into a head already fetched, tile tasks that stayed and threw one away
};
static_assert(std::is_trivially_copyable_v<KnnHiParams>, "kernel argument");

constexpr size_t knn_hi_lds_bytes(bool abandon = false, bool defer = false) {
    // (ABANDON: + three per-query arrays and the two veto words; DEFER: + the three 256-bit masks of live rows)
    return 2 * KW_STAGE_BYTES + sizeof(float) * KW_N * 4 + sizeof(float) * 2 * KW_M * 2 + 16 + (abandon ? sizeof(float) * KW_N * 3 + 16 : 0) +
           (defer ? 96 : 0);
}

// RSC: 0 = IP with one scale for all rows (un-centred cosine stores, fp16 stores): no per-score arithmetic at all;
//      1 = IP with per-row scales: one multiply;
//      2 = per-row scale AND per-row bias: L2 (score = 2 a - |y'|^2 - |q'|^2) and stores whose plane is CENTRED (y' = y - mu,
//          q' = q - mu: score = a' + mu.y + q'.mu = q.y).  The bias costs nothing in the epilogue: the accumulators of a tile
//          START at bias_row 2^eq / (mult 2^-ey) (exact: powers of two) instead of zero, the MFMAs add the products on top, and
//          the epilogue is RSC 1's single multiply.  The per-query constant moves to the threshold side of the compare.
//      3 = bias with ONE scale for all rows (the store's rows are of one magnitude: knn_ensure_hi decides): RSC 0's epilogue -- no
//          per-score arithmetic -- with RSC 2's accumulator start.  The reference's default index (L2 over clip embeddings) and
//          centred cosine stores run this one.
// SAMPLE: the threshold pre-pass.  No lists: every lane writes the best two scores it holds for each of its queries
// (8 holders x 2 = 16 entries per query and tile) and k_floor_from_sample picks the wanted rank over all of them.
#ifdef RADAD_DEBUG_HOOKS
#define KH_STAMP(tag)                                                                                              \
    do {                                                                                                           \
        if (!SAMPLE && p.stamps && blockIdx.x == 0 && (threadIdx.x & 63) == 0 && stamp_n < 4096) {               \
            p.stamps[(threadIdx.x >> 6) * 4096 + stamp_n] = ((unsigned long long)(tag) << 56) |                  \
                (__builtin_amdgcn_s_memtime() & 0x00ffffffffffffffull);                                            \
            ++stamp_n;                                                                                             \
        }                                                                                                          \
    } while (0)
#else
#define KH_STAMP(tag) do { } while (0)
#endif

// workgroup -> (query tile, chunk of the store); false: a workgroup of the grid's padding (block-uniform)
__device__ __forceinline__ bool knn_hi_task(const KnnHiParams& p, int bid, int& qt, int& split) {
    const int xcd = bid & 7;
    const int slot_b = bid >> 3;
    if (p.n_qtiles <= 8) {
        qt = slot_b % p.n_qtiles;
        split = (slot_b / p.n_qtiles) * 8 + xcd;
        return true;
    }
    const int per_group = p.n_splits;            // slots of one query group on this XCD: 8 query tiles x n_splits / 8 chunks
    const int r = slot_b % per_group;
    qt = (slot_b / per_group) * 8 + (r & 7);
    split = (r >> 3) * 8 + xcd;
    return qt < p.n_qtiles;                      // (the grid covers whole groups)
}

// The abandon's terms of one live query, in the accumulators' units (RSC 0, 3): `at` exactly the value the epilogue compares against
// ((s_thr - s_qc) s_qs, the same operations on the same values), rq = |qh_j[64 ck:]|, sl the accumulation slack; qi = 1 / s_qs.
template <int RSC>
__device__ __forceinline__ void knn_hi_ab_query(const KnnHiParams& p, int q, float& at, float& rq, float& sl, float& qi) {
    qi = p.qscale[q] * p.uscale;
    if (RSC == 3) qi *= p.mult;
    const float qs = 1.0f / qi;                  // powers of two: exact
    const float qc = (RSC >= 2 && p.qconst) ? p.qconst[q] : 0.f;
    at = (p.thr_init[q] - qc) * qs;
    rq = p.ab_rq[q];
    sl = p.ab_slack[q] * qs * (RSC == 3 ? p.mult : 1.f);
}
// THE GATE (scalars only; a heuristic: it decides whether the test RUNS, never what the test finds).  A tile can only be skipped if
// for every live query   at_j - sl_j - start_ij - RQ_j RY > 0   leaves room for the partial products; with the accumulators' start
// start_ij = b_i / qi_j (RSC 3: b = bias_sign x bias; RSC 0: 0) and everything multiplied by qi_j > 0:
//     amin - rmax RY - B > 0,    amin = min_j (at_j - sl_j) qi_j,  rmax = max_j RQ_j qi_j,  B = the tile's largest b
// (sufficient for none of the per-query conditions to fail on the suffix product alone; a NaN anywhere closes it).
__device__ __forceinline__ bool knn_hi_gate(float amin, float rmax, float ry, float b) { return amin - rmax * (ry * (1.0f + 0x1p-10f)) - b > 0.f; }

// ABANDON: after p.ab_ck K stages a tile whose partial scores provably cannot reach any query's floor is left (the test, its gate and
// the proof are at the checkpoint below).  Instantiations without it compile to the code they had before it existed.
// (ab_amin, ab_rmax: the gate's query side, from knn_hi_gate_open)
// DEAL (with ABANDON only): the tiles come by ticket.  deal_ticket: the first of the TWO tickets the gate pass drew for this workgroup.
// DEFER (with ABANDON only, not DEAL): a vetoed tile with 1 ... KNN_DEFER_MAX_ROWS live rows lists them and is left like a skipped one.
// MAPPED (the tail of a deferring launch, no ABANDON): ONE tile per call, rows map_tile * KW_M ... of this query tile's LIST; the A
// operand is fetched row by row from where the list says, everything else -- K order, accumulator start, emit -- is the scan's.
template <int RSC, bool SAMPLE, bool ABANDON = false, bool DEAL = false, bool DEFER = false, bool MAPPED = false>
__device__ __forceinline__ void knn_hi_body(const KnnHiParams& p, const float ab_amin = 0.f, const float ab_rmax = 0.f, const int deal_ticket = 0,
                                            const int map_tile = 0) {
    static_assert(!ABANDON || (!SAMPLE && (RSC == 0 || RSC == 3)), "the abandon covers the one-scale scans");
    static_assert(!DEAL || ABANDON, "only the abandoning scan is dealt");
    static_assert(!DEFER || (ABANDON && !DEAL), "only the abandoning scan over static chunks defers");
    static_assert(!MAPPED || (!SAMPLE && !ABANDON && (RSC == 0 || RSC == 3)), "the tail scores what an abandoning launch listed");
    int stamp_n = 0;
    (void)stamp_n;
    // acc[mt][nt][r] = row wm*128 + mt*16 + 4*lq + r, query wn*64 + nt*16 + l15   (l15 = lane & 15, lq = lane >> 4)
    static_assert(KW_WAVES == 8, "the body is laid out for 8 waves");
    constexpr int MT = 8, NT = 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* s_thr = reinterpret_cast<float*>(smem + 2 * KW_STAGE_BYTES);      // [KW_N] admission floor (true scale)
    float* s_qs = s_thr + KW_N;                                              // [KW_N] v-domain scale of each query
    float* s_qi = s_qs + KW_N;                                               // [KW_N] and its inverse
    float* s_qc = s_qi + KW_N;                                               // [KW_N] per-query constant of the score (RSC 2, 3)
    float* s_rs = s_qc + KW_N;                                               // [2][KW_M] row scale (x mult)
    float* s_rb = s_rs + 2 * KW_M;                                           // [2][KW_M] accumulator start of the row: bias / (mult scale)
    // ABANDON (behind the K split's flag, which such a launch never uses):
    float* s_at = s_rb + 2 * KW_M + 4;                                       // [KW_N] the epilogue's threshold of each query, +inf past nq
    float* s_arq = s_at + KW_N;                                              // [KW_N] |qh_j[64 ck:]|
    float* s_asl = s_arq + KW_N;                                             // [KW_N] accumulation slack, accumulator units
    int* s_veto = reinterpret_cast<int*>(s_asl + KW_N);                      // [2] by tile parity: the tile (row0 / KW_M) a wave vetoed last
    unsigned* s_live = reinterpret_cast<unsigned*>(s_veto + 4);              // DEFER: [3][8] by tile number mod 3: bit r of the 256 = row r is live
    int* s_map = reinterpret_cast<int*>(s_rs);                               // MAPPED: [KW_M] the tile's rows of the launch, -1 past the list's
                                                                             // end (s_rs: RSC 0 and 3 never use it)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave & 1, wn = wave >> 1;         // wave tile: rows wm*128.., queries wn*64..
    const int l15 = lane & 15, lq = lane >> 4;

    // XCD-aware: workgroups are dealt to the 8 XCDs round-robin and an XCD runs 32 of them at a time (one per CU).  Up to 8 query
    // tiles: the query tiles of one store chunk are consecutive on one XCD and share the chunk through its L2.  More (a sharded
    // search: every rank scores ALL ranks' queries, 32-40 tiles): 32 query tiles of 256 KB each would evict each other from a 4 MB
    // L2 and every stage would refetch its query tile from the Infinity Cache -- instead GROUPS of 8 query tiles (2 MB) stay on
    // an XCD while its share of the chunks passes, 4 chunks at a time (the 32 concurrent workgroups = 8 query tiles x 4 chunks).
    const int part = (!ABANDON && p.ksplit == 2) ? (int)(blockIdx.x & 1) : 0;
    const int bid = (!ABANDON && p.ksplit == 2) ? (int)(blockIdx.x >> 1) : (int)blockIdx.x;
    int qt, split;
    if (!knn_hi_task(p, bid, qt, split)) return;     // (block-uniform, before any barrier)
    const int q0 = qt * KW_N;
    // (DEAL: the "chunk" is the launch -- every tile but the launch's last is whole -- and `split` is not used)
    // (MAPPED: the "store" is the query tile's list, the chunk its tile map_tile)
    const int64_t chunk_begin = DEAL ? (int64_t)0 : MAPPED ? (int64_t)map_tile * KW_M : (int64_t)split * p.chunk_stride;
    const int64_t chunk_end = DEAL ? p.n : MAPPED ? min(chunk_begin + KW_M, (int64_t)min(p.df_cnt[qt], p.df_cap)) : min(chunk_begin + p.chunk_rows, p.n);
    if constexpr (MAPPED) { if (chunk_begin >= chunk_end) return; }          // (block-uniform, before any barrier)
    const bool owner = tid < KW_N && q0 + tid < p.nq;
    const int nk_all = p.row_bytes >> 7;             // 128-byte K steps per row
    const int k_lo = part * (nk_all >> 1);           // this workgroup's K steps [k_lo, k_lo + nk)
    const int nk = (!ABANDON && p.ksplit == 2) ? (part == 0 ? (nk_all >> 1) : nk_all - (nk_all >> 1)) : nk_all;

    if (tid < KW_N) {
        s_thr[tid] = (owner && p.thr_init) ? p.thr_init[q0 + tid] : -INFINITY;
        // v = a * s_qs: the accumulator domain (RSC 0, 3) or accumulator x row scale (RSC 1, 2)
        float qi = owner ? p.qscale[q0 + tid] : 1.f;
        if (RSC == 0) qi *= p.uscale;
        if (RSC == 3) qi *= p.uscale * p.mult;
        s_qi[tid] = qi;
        s_qs[tid] = 1.0f / qi;                       // powers of two: exact
        s_qc[tid] = (RSC >= 2 && owner && p.qconst) ? p.qconst[q0 + tid] : 0.f;
        if constexpr (ABANDON) {
            // a slot past nq counts as +inf (the epilogue's -inf would veto every skip of a partly filled query tile); a real query
            // whose floor is -inf vetoes
            float at = INFINITY, rq = 0.f, sl = 0.f, qi_ab;
            if (owner) knn_hi_ab_query<RSC>(p, q0 + tid, at, rq, sl, qi_ab);
            s_at[tid] = at; s_arq[tid] = rq; s_asl[tid] = sl;
        }
    }
    if constexpr (ABANDON) { if (tid < 2) s_veto[tid] = -1; }
    if constexpr (DEFER) { if (tid < 24) s_live[tid] = 0u; }
    if constexpr (MAPPED) {
        // the tile's rows, in LDS before the first fetch needs them (one tile per call: no parity)
        if (tid < KW_M) s_map[tid] = chunk_begin + tid < chunk_end ? p.df_list[(int64_t)qt * p.df_cap + chunk_begin + tid] : -1;
        __syncthreads();
    }

    // DMA plan.  One LDS-DMA instruction fills an 8-row group (1 KB, lane-linear) of an operand tile; 32 groups per operand
    // and stage.  Waves 0-3 fetch the A (store) tile, 8 groups each, right after the stage's barrier (it comes from HBM: the
    // longest trip first); waves 4-7 fetch the B (query) tile (L2-resident) after their first two pairs of row tiles: while one
    // half of the waves is busy issuing DMA (~55 cycles an instruction, no MFMA from that wave meanwhile) the other half -- its
    // partner on every SIMD -- has the matrix pipe, and both halves' DMA is under way in the first quarter of the stage: an
    // LDS-DMA takes ~1 us from issue to landing under load (about as long as the stage's MFMA work), and the next barrier waits
    // for it.
    // (Tried and dropped: four 32 KB stages of 64-byte row chunks with the DMA issued three k steps ahead behind a counted
    // vmcnt and a raw s_barrier -- it hides the landing latency, but 64-byte pieces of a row double the texture-addresser work
    // per byte and a barrier per k step costs more than it saves: 1.23 ms against 1.11 ms for this loop.)
    // Lane l of a group fetches logical 16-byte chunk (l & 7) ^ ((r >> 1) & 7) of row r = 8 g + (l >> 3) into physical chunk
    // l & 7: (r >> 1) & 7 = (4 (g & 1) + (l >> 4)) & 7, so two per-lane offsets (even / odd group) serve all 8 groups.
    const int grp_half = wave >> 2;                  // 0: A fetcher, 1: B fetcher
    const int g0 = (wave & 3) * 8;                   // first of this wave's 8 groups
    unsigned dma_vo[2];
#pragma unroll
    for (int par = 0; par < 2; ++par) {
        const int r = par * 8 + (lane >> 3);         // row inside a 16-row pair of groups
        const int lc = (lane & 7) ^ ((r >> 1) & 7);
        dma_vo[par] = (unsigned)(r * p.row_bytes + lc * 16);
    }
    const unsigned pair_bytes = (unsigned)(16 * p.row_bytes);
    const unsigned rd_a = (unsigned)((wm * 128 + l15) * 128);
    const unsigned rd_b = (unsigned)(KW_OP_BYTES + (wn * 64 + l15) * 128);
    const unsigned rd_x = (unsigned)((lq ^ (l15 >> 1)) << 4);      // 16-byte chunk lq of the row, swizzled

    const __amdgpu_buffer_rsrc_t q_desc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(p.q) + (int64_t)q0 * p.row_bytes), 0,
        min(KW_N, p.nq - q0) * p.row_bytes, 0x00020000);
    auto tile_desc = [&](int64_t r0) {
        // (MAPPED: the whole launch, whatever the tile: the per-lane offsets say which rows)
        if constexpr (MAPPED) return __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(p.db)), 0, (int)p.df_bytes, 0x00020000);
        const int rows = (int)max((int64_t)0, min((int64_t)KW_M, chunk_end - r0));
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(p.db) + r0 * p.row_bytes), 0,
                                                 rows * p.row_bytes, 0x00020000);
    };
    // this wave's 8 groups of ONE operand (rows past the end of the tile fall outside num_records and read as zero)
    auto dma_half = [&](__amdgpu_buffer_rsrc_t desc, int stage, int kc, int operand) {
        char* base = smem + stage * KW_STAGE_BYTES + operand * KW_OP_BYTES;
        const int soff = kc * 128;
        // (opaque copies: hipcc would otherwise keep all eight per-group offsets in registers across the K loop -- and spill them)
        unsigned vo_par[2] = {dma_vo[0], dma_vo[1]};
        asm volatile("" : "+v"(vo_par[0]), "+v"(vo_par[1]));
        if constexpr (MAPPED) {
            if (operand == 0) {
                // row 8 g + (lane >> 3) of the tile is row s_map[..] of the launch; a slot past the list's end points past the
                // descriptor's end and reads as a zero row
                int lane_m = lane;
                asm volatile("" : "+v"(lane_m));
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int g = g0 + i;
                    const int r = 8 * g + (lane_m >> 3);
                    const int m = s_map[r];
                    const unsigned lc = (unsigned)((lane_m & 7) ^ ((r >> 1) & 7));
                    const unsigned vo = m < 0 ? p.df_bytes : (unsigned)m * (unsigned)p.row_bytes + lc * 16u;
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(desc, (lds_ptr_t)(base + g * 1024), 16, vo, soff, 0, 0);
                }
                return;
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int g = g0 + i;
            const unsigned vo = vo_par[i & 1] + (unsigned)(g >> 1) * pair_bytes;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(desc, (lds_ptr_t)(base + g * 1024), 16, vo, soff, 0, 0);
        }
    };

    // per-row scale / accumulator start of a tile (RSC >= 1), parked in LDS one tile AHEAD: tile t's values are written after the first
    // barrier of tile t - 1's K loop (everyone has left the epilogue that read this parity), so neither the accumulator start at
    // the top of a tile nor the epilogue needs a barrier of its own
    auto park_row_terms = [&](int64_t r0, int par) {
        int t = tid;
        asm volatile("" : "+v"(t));                  // opaque: the addresses are formed here, not kept (or spilled) across the K loop
        if (RSC != 0 && t < KW_M) {
            const bool in = r0 + t < chunk_end;
            int64_t rb_row = r0 + t;
            if constexpr (MAPPED) { if (in) rb_row = p.df_list[(int64_t)qt * p.df_cap + r0 + t]; }
            float rs = (in && p.rscale) ? p.rscale[r0 + t] : p.uscale;
            if (RSC == 2) rs *= p.mult;
            if (RSC != 3) s_rs[par * KW_M + t] = in ? rs : 0.f;
            // RSC 2: bias / (row scale) (a power of two: exact); RSC 3: the bias itself (the one scale sits in the query's factor)
            // (K split: the bias starts the FIRST half's accumulators only)
            s_rb[par * KW_M + t] = (RSC >= 2 && in && part == 0) ? (RSC == 2 ? p.bias_sign * p.rbias[r0 + t] / rs : p.bias_sign * p.rbias[rb_row]) : 0.f;
        }
    };
    // ---- DEAL: which tile comes next ------------------------------------------------------------------------------------------------
    // Tickets map to granules of deal_g consecutive tiles (knn_deal_ticket, knn_plan.h: the text the host's check enumerates).  A
    // granule begins on a multiple of deal_g, so "first / last tile of its granule" is read off the tile's number, and the state that
    // lives across the tile loop is three scalars: the tile, the granule after this one (d_next) and the one after that (d_next2),
    // each as its first tile, d_tiles = none.  The next tile must be known at the top of a tile (a skip issues its stage 0 at the
    // checkpoint barrier, the last K stage prefetches it), so the draw runs a whole granule ahead: thread 0 issues the atomic in front
    // of the first stage of a granule's first tile, parks the ticket in s_veto[2] behind that stage's MFMAs, the stage's own barrier --
    // which waits vmcnt(0) anyway -- publishes it.  (The word is read right behind that barrier and written again a granule later:
    // at least one more barrier lies between.)
    const int d_tiles = DEAL ? p.deal_tiles : 0, d_mask = DEAL ? p.deal_g - 1 : 0;
    int d_next = 0, d_next2 = 0;
    int64_t row_first = chunk_begin, d_row_adv = 0;
    (void)d_mask; (void)d_next; (void)d_next2; (void)d_row_adv;
    auto deal_tile = [&](int ticket) {        // ticket -> the granule's first tile, or d_tiles
        const DealRange g = knn_deal_ticket(bid & 7, ticket, d_tiles, p.deal_g);
        return __builtin_amdgcn_readfirstlane(g.tiles > 0 ? g.tile0 : d_tiles);
    };
    if constexpr (DEAL) {
        const int d_first = deal_tile(deal_ticket);
        if (d_first >= d_tiles) return;              // a workgroup beyond the resident ones: its counter is used up (block-uniform, no barrier pending)
        d_next = d_next2 = deal_tile(deal_ticket + 1);
        row_first = (int64_t)d_first * KW_M;
    }
    int gbuf = 0;
    if (row_first < chunk_end) {
        if (grp_half == 0) dma_half(tile_desc(row_first), 0, k_lo, 0);
        else dma_half(q_desc, 0, k_lo, 1);
        park_row_terms(row_first, 0);
    }
    __syncthreads();

    // One stage = 128 bytes of every row = two 32-element MFMA steps.  Fragment registers: the B fragments of both steps
    // (2 x 4) and two PAIRS of A fragments: while the 8 MFMAs of one pair of row tiles run (128 cycles), the next pair's
    // two ds_read_b128 are in flight -- the LDS latency is hidden behind the wave's own MFMAs, not left to its partner.
    // sched_barrier(0) pins that order (hipcc otherwise keeps ONE A fragment and waits lgkmcnt(0) in front of every 4 MFMAs).
    // HOLD-BACK: the last pair of row tiles of a stage (8 MFMAs, 128 cycles) is NOT multiplied before the barrier but after it,
    // behind the next stage's first six ds_reads: its fragments (afr[1], both; bfr[1]) are in registers already, the first reads
    // go to afr[0] / bfr[0], so it costs no register -- and the ~400 cycles after a barrier in which both waves of a SIMD used
    // to wait for LDS now hold 2 x 128 cycles of matrix work.  Not across tiles (the epilogue needs the finished accumulators).
    // (Round 5: TWO held-back pairs -- 16 MFMAs per wave behind the first reads, a third A fragment buffer, 215 VGPRs, no spills, parity
    // green -- measured 0.913-0.921 against 0.898-0.909 ms per search, three alternations on one box (profiles/r5_ab_hold2.txt): the
    // window behind a barrier is not idle pipe time that more held-back work could fill; reverted.)
    // (the L2 variant used to be left out: its epilogue -- a multiply and an fma with |y|^2 per score -- needed the registers and hipcc
    // spilled INSIDE the K loop with the fragments live across the barrier; with the bias as the accumulators' start value its
    // epilogue is RSC 1's)
    constexpr bool HOLD = true;
    f32x4 acc[MT][NT];
    f16x8 bfr[2][NT], afr[2][2];
    // (ABANDON: the checkpoint stage holds nothing back -- the test needs the finished partial sums -- so the stage after it has no
    // held-back pair to finish: hold_in, wave-uniform; without ABANDON it is the constant true)
    auto stage_body = [&](const char* a_row, const char* b_row, auto first_c, const bool hold_out, const bool hold_in, const float* rb_t, auto&& dma_a, auto&& dma_b) {
        constexpr bool ZERO = decltype(first_c)::value;         // a tile's first stage: C = 0, or (RSC 2, 3) C = the row bias in the
                                                                // accumulator's units, bias_row 2^eq / (mult 2^-ey): exact (powers of two)
        constexpr bool HOLD_IN = HOLD && !ZERO;   // every stage but a tile's first finishes the previous stage's last pair first;
                                              // hold_out (wave-uniform): leave this stage's last pair to the next stage
        // (the start values are formed inside the stage that consumes them: as a block in front of the K loop the 128 of them were
        // live INTO the loop beside the fragments and hipcc spilled 100 registers per tile)
        f32x4 rb4[ZERO && RSC >= 2 ? MT : 1];
        float qs4[ZERO && RSC >= 2 ? NT : 1];
        if constexpr (ZERO && RSC >= 2) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) rb4[mt] = *reinterpret_cast<const f32x4*>(rb_t + mt * 16);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) qs4[nt] = s_qs[wn * 64 + nt * 16 + l15];
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bfr[0][nt] = *reinterpret_cast<const f16x8*>(b_row + nt * 2048 + rd_x);
        afr[0][0] = *reinterpret_cast<const f16x8*>(a_row + rd_x);
        afr[0][1] = *reinterpret_cast<const f16x8*>(a_row + 2048 + rd_x);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (HOLD_IN) {
            if (!ABANDON || hold_in) {
#pragma unroll
                for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[6 + h2][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(afr[1][h2], bfr[1][nt], acc[6 + h2][nt], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        KH_STAMP(1);
        dma_a();          // the database tile comes from HBM (~1 us from issue to landing): first thing after the barrier.  The stage
                          // length used to settle at "issue offset + that latency" with the A fetch issued ~1100 cycles in
        __builtin_amdgcn_sched_barrier(0);
        KH_STAMP(2);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const unsigned off = rd_x ^ (unsigned)(64 * s);   // chunk (4s + lq) ^ swizzle, in bytes
#pragma unroll
            for (int pr = 0; pr < 4; ++pr) {
                if (pr < 3) {                                 // next pair of row tiles of this step
                    afr[(pr + 1) & 1][0] = *reinterpret_cast<const f16x8*>(a_row + (2 * pr + 2) * 2048 + off);
                    afr[(pr + 1) & 1][1] = *reinterpret_cast<const f16x8*>(a_row + (2 * pr + 3) * 2048 + off);
                } else if (s == 0) {                          // first fragments of the second step
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) bfr[1][nt] = *reinterpret_cast<const f16x8*>(b_row + nt * 2048 + (rd_x ^ 64u));
                    afr[0][0] = *reinterpret_cast<const f16x8*>(a_row + (rd_x ^ 64u));
                    afr[0][1] = *reinterpret_cast<const f16x8*>(a_row + 2048 + (rd_x ^ 64u));
                }
                __builtin_amdgcn_sched_barrier(0);
                if (!(s == 1 && pr == 3) || !(HOLD && hold_out)) {
#pragma unroll
                    for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) {
                            const int mt = 2 * pr + h2;
                            if (ZERO && s == 0 && RSC >= 2)
                                acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(afr[pr & 1][h2], bfr[s][nt], rb4[ZERO && RSC >= 2 ? mt : 0] * qs4[ZERO && RSC >= 2 ? nt : 0], 0, 0, 0);
                            else if (ZERO && s == 0)
                                acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(afr[pr & 1][h2], bfr[s][nt], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                            else
                                acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(afr[pr & 1][h2], bfr[s][nt], acc[mt][nt], 0, 0, 0);
                        }
                }
                __builtin_amdgcn_sched_barrier(0);
                if (s == 0 && pr == 1) { KH_STAMP(3); dma_b(); __builtin_amdgcn_sched_barrier(0); KH_STAMP(4); }   // queries: L2-resident, shorter trip
            }
        }
        KH_STAMP(5);
    };
    static_assert(MT == 8, "the hold-back names row tiles 6 and 7");

    // ---- EARLY ABANDON ----------------------------------------------------------------------------------------------------------
    // After ck stages the accumulators hold acc_c = (bias start) + sum over the first 64 ck elements, and for every pair (row i, query j)
    //     acc_full <= acc_c + RQ_j RY (1 + 2^-10) + slack_j,    RQ_j = |qh_j[64 ck:]|, RY = max_i |yh_i[64 ck:]| over the tile's rows
    // (Cauchy-Schwarz on the exact rest of the dot product; both norms are fp32 sums of squares of the raw f16 values inflated by 2^-10
    // as hi_rows_body inflates its norms; slack_j = 2 dim 2^-23 (|qh_j| max |yh| + |c0|max) covers the fp32 accumulation error of any
    // summation order, of the part done and of the part to come).  The epilogue emits a pair iff acc_full >= at_j; so when
    //     acc_c + RQ_j RY (1 + 2^-10) + slack_j < at_j      for all 256 x 256 pairs (every comparison TRUE: a NaN vetoes),
    // the tile emits nothing and its remaining stages and its epilogue are left out.  The set of emitted candidates is the parent's.
    // Every lane takes the maximum of its 32 partial scores per query (4 queries); a wave that cannot agree writes the tile's number
    // into s_veto[parity]; the stage's own barrier publishes it; everyone reads it: the decision is workgroup-uniform, no spinning, no
    // communication between workgroups.  (The word holds a tile NUMBER and is never reset.  Tile t's word is read between t's checkpoint
    // barrier and the next barrier anyone reaches, which is at the latest the first barrier of tile t + 1 -- every tile has one, a
    // leaving tile exactly one since the head prefetch.  The next write to the same parity is in a stage of tile t + 2, behind that
    // barrier: one barrier per leaving tile is enough.)
    // THE HEAD PREFETCH (ahead_on; DESIGN §4.1).  A tile that leaves at its checkpoint used to have fetched its own stage ab_ck for nothing,
    // then issued the next tile's stage 0 over it and sat through a barrier that waited for nothing else.  With ahead_on the checkpoint
    // stage of a tested tile that has a next tile and is PREDICTED to leave (one scalar per workgroup: knn_ahead_speculate / knn_ahead_next,
    // knn_plan.h -- the text the host model walks) fetches the next tile's stage 0 instead.  A tile that leaves then goes straight into
    // the next tile's first stage: ONE barrier per leaving tile.  A tile that stays issues its own stage ab_ck over the head and waits one
    // barrier for it -- the bubble a leaving tile used to pay -- and the K loop goes on as it was; its last stage fetches the next tile's
    // head as ever.  What is fetched when changes no accumulator: the scores are the same bit for bit.
    // What relied on the second barrier of a leaving tile, with the argument for one:
    //   s_veto[parity]: above.
    //   s_live: three masks by tile number mod 3, below where they are cleared.
    //   s_rb (RSC 3): tile t + 1's accumulator starts used to be parked behind tile t's first barrier, and with the checkpoint at stage 0
    //     nothing would separate that store from tile t + 1's first stage, which reads them.  With ahead_on they are loaded in front of
    //     tile t's first stage and stored in front of its first barrier.  The parity they go to was last read by tile t - 1's FIRST stage
    //     (RSC 3's epilogue reads neither s_rs nor s_rb), which lies in front of tile t - 1's first barrier.
    //   the dealt kernel's s_veto[2]: a dealt launch does not prefetch heads (ahead_on is false for DEAL) and keeps its two barriers.
    //   the deferral's list append: carried to behind the next tile's first barrier (df_flush).
    int ab_ck = 0, ab_checked = 0, ab_skipped = 0, ab_deferred = 0;
    (void)ab_deferred;
    if constexpr (ABANDON) ab_ck = p.ab_ck;
    const bool ahead_on = ABANDON && !DEAL && p.ab_ahead != 0;      // (a kernel argument: uniform)
    bool ah_pred = knn_ahead_initial();
    int ah_used = 0, ah_wasted = 0;
    (void)ah_pred; (void)ah_used; (void)ah_wasted;
    // DEFER: a deferred tile's list entries, written behind the NEXT tile's first barrier (or behind the tile loop): lane 0 of wave 0
    // holds the returning atomic's slot, lane l the nibble of rows 4 l ... 4 l + 3 and their rank among the tile's live rows (rank << 4
    // | nibble); df_row = the tile's first row.  Nothing waits for the atomic in front of the next tile's stage: the barrier behind that
    // stage waits vmcnt(0) anyway.
    // (REGISTERS: df_slot and df_pack, and RSC 3's park_v below, are live across a whole stage.  With them the deferring kernels stand
    // at 246 (RSC 0) / 250 (RSC 3) VGPRs, no scratch -- 6 below the 256 at which hipcc starts to spill inside the K loop.  Anything
    // more carried across a stage here has to be paid for elsewhere: check -Rpass-analysis=kernel-resource-usage before a GPU run.)
    bool df_pend = false;
    int df_slot = 0, df_row = 0;
    unsigned df_pack = 0u;
    (void)df_pend; (void)df_slot; (void)df_row; (void)df_pack;
    auto df_flush = [&]() {
        if (wave == 0) {
            int* dst = p.df_list + (int64_t)qt * p.df_cap + __builtin_amdgcn_readfirstlane(df_slot) + (int)(df_pack >> 4);
            const int row_l = df_row + 4 * (lane & 63);
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if (df_pack & (1u << b)) { *dst = row_l + b; ++dst; }
            }
        }
        df_pend = false;
    };
    int tile_par = 0, live_slot = 0;
    (void)live_slot;
    for (int64_t row0 = row_first; row0 < chunk_end; row0 = DEAL ? d_row_adv : row0 + KW_M, tile_par ^= 1, live_slot = (live_slot == 2 ? 0 : live_slot + 1)) {
        int64_t row_next = row0 + KW_M;
        bool d_draw = false;
        if constexpr (DEAL) {
            const int t = __builtin_amdgcn_readfirstlane((int)(row0 >> 8));
            const bool first = (t & d_mask) == 0;
            if (first) d_next = d_next2;             // (a granule's first tile is only ever reached from the granule before it)
            const bool last = (t & d_mask) == d_mask || t + 1 >= d_tiles;
            row_next = (int64_t)(last ? d_next : t + 1) * KW_M;      // none = d_tiles: at or past chunk_end
            d_row_adv = row_next;
            d_draw = first && d_next < d_tiles;      // (a used-up counter stays used up: nothing more to ask)
        }
        (void)d_draw;
        const bool has_next = row_next < chunk_end;
        // THE GATE, tile side (scalars only): the test runs iff it can succeed
        float ab_ry = 0.f;
        bool ab_check = false, ab_skip = false, ab_defer = false, ab_spec = false;
        int df_ns = 0;
        (void)ab_defer; (void)df_ns; (void)ab_spec;
        if constexpr (ABANDON) {
            ab_ry = p.ab_ry[row0 >> 8] * (1.0f + 0x1p-10f);
            ab_check = knn_hi_gate(ab_amin, ab_rmax, p.ab_ry[row0 >> 8], RSC == 3 ? p.ab_b[row0 >> 8] : 0.f);
        }
        static_assert(KW_M == 256, "row0 >> 8 is the tile's number");
        const int rowlimit = (int)min((int64_t)KW_M, chunk_end - row0);
        const __amdgpu_buffer_rsrc_t cur_desc = tile_desc(row0);
        const __amdgpu_buffer_rsrc_t next_desc = tile_desc(row_next);
        for (int kc = 0; kc < nk; ++kc) {
            const int stage = gbuf & 1;
            const bool more_k = kc + 1 < nk;
            const bool fetch = (more_k || has_next) && !RADAD_DBG(p.debug, 2);
            const bool at_ck = ABANDON && ab_check && kc + 1 == ab_ck;      // the checkpoint stage (wave-uniform)
            const bool after_ck = ABANDON && ab_check && kc == ab_ck;
            // the head prefetch: this stage fetches what the tile's LAST stage would, the next tile's stage 0 (block-uniform)
            const bool spec = ABANDON && !DEAL && ahead_on && at_ck && more_k && knn_ahead_speculate(ah_pred, has_next);
            const bool own_k = more_k && !spec;
            const int nkc = k_lo + (own_k ? kc + 1 : 0);
            auto dma_a = [&]() { if (fetch && grp_half == 0) dma_half(own_k ? cur_desc : next_desc, stage ^ 1, nkc, 0); };
            auto dma_b = [&]() { if (fetch && grp_half == 1) dma_half(q_desc, stage ^ 1, nkc, 1); };
            const char* a_row = smem + stage * KW_STAGE_BYTES + rd_a;
            const char* b_row = smem + stage * KW_STAGE_BYTES + rd_b;
            const float* rb_t = s_rb + tile_par * KW_M + wm * 128 + 4 * lq;
            // (ahead_on, RSC 3: the next tile's accumulator starts, loaded here and stored in front of this stage's barrier: see above)
            const bool park_early = ABANDON && !DEAL && RSC == 3 && ahead_on && kc == 0 && has_next;
            float park_v = 0.f;
            if constexpr (ABANDON && !DEAL && RSC == 3) {
                if (park_early) {
                    int t = tid;
                    asm volatile("" : "+v"(t));
                    if (t < KW_M && row_next + t < chunk_end) park_v = p.bias_sign * p.rbias[row_next + t];
                }
            }
            int d_ticket = 0;
            if constexpr (DEAL) {
                // (the counter's address goes through an OPAQUE per-lane zero: with an address it can prove uniform hipcc rewrites the
                // atomic into its wave-aggregated form, which reads the result back -- s_waitcnt vmcnt(0) -- right behind the
                // instruction: wave 0 then sat through the atomic's round trip in front of every granule's first DMA, ~1 us per
                // granule for the whole workgroup.  As written the result is first touched at the LDS store behind the stage.)
                if (kc == 0 && d_draw && tid == 0) {
                    int z = 0;
                    asm volatile("" : "+v"(z));
                    d_ticket = atomicAdd(p.deal_cnt + (bid & 7) * KNN_DEAL_MAX_QTILES + qt + z, 1);
                }
            }
            if (kc == 0) stage_body(a_row, b_row, std::true_type{}, more_k && !at_ck, true, rb_t, dma_a, dma_b);      // first stage of a tile: C = 0 / the bias
            else stage_body(a_row, b_row, std::false_type{}, more_k && !at_ck, !after_ck, rb_t, dma_a, dma_b);       // (the last stage leaves nothing over)
            if constexpr (ABANDON) {
                if (at_ck) {
                    int lane_t = lane;
                    asm volatile("" : "+v"(lane_t));         // (opaque, as in the epilogue: no address of this block lives across the K loop)
                    bool ok = true;
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        const int ql = wn * 64 + nt * 16 + (lane_t & 15);
                        float gm = -INFINITY;
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt)
                            gm = fmaxf(gm, fmaxf(fmaxf(acc[mt][nt][0], acc[mt][nt][1]), fmaxf(acc[mt][nt][2], acc[mt][nt][3])));
                        // (fmaxf drops a NaN score: a NaN score is never emitted either.  Rows past the tile's end read as zero rows.)
                        ok = ok && (gm + fmaf(s_arq[ql], ab_ry, s_asl[ql]) < s_at[ql]);
                    }
                    if constexpr (!DEFER) {
                        if (!__all(ok) && (lane_t & 63) == 0) s_veto[tile_par] = (int)(row0 >> 8);
                    } else {
                        // DEFER: a wave that vetoes also says WHICH of its 128 rows are live: row i is live iff for some query j of the
                        // wave the same comparison, with the same terms, is not true (any NaN keeps the row live).  gm is the maximum of
                        // the column and the addition is monotonic, so a wave that does not veto has no live row.  Bit mt * 4 + r of
                        // `live` is row mt * 16 + 4 lq + r of the wave; word (mt >> 1) of the wave's four holds it at bit
                        // (mt & 1) * 16 + 4 lq + r.  The stage's barrier publishes the words with the veto.
                        if (!__all(ok)) {            // (wave-uniform)
                            if ((lane_t & 63) == 0) s_veto[tile_par] = (int)(row0 >> 8);
                            unsigned live = 0u;
                            float bd[NT], at[NT];
#pragma unroll
                            for (int nt = 0; nt < NT; ++nt) {
                                const int ql = wn * 64 + nt * 16 + (lane_t & 15);
                                bd[nt] = fmaf(s_arq[ql], ab_ry, s_asl[ql]);
                                at[nt] = s_at[ql];
                            }
                            // (shifted in from the top row down -- a select between 32 different one-bit constants had hipcc keep all
                            // 32 of them in registers across the tile loop, and spill)
#pragma unroll
                            for (int mt = MT - 1; mt >= 0; --mt)
#pragma unroll
                                for (int r = 3; r >= 0; --r) {
                                    bool all_true = true;
#pragma unroll
                                    for (int nt = 0; nt < NT; ++nt) all_true = all_true && (acc[mt][nt][r] + bd[nt] < at[nt]);
                                    live = (live << 1) | (all_true ? 0u : 1u);
                                }
                            const int sh = 4 * (lane_t >> 4);
#pragma unroll
                            for (int w = 0; w < 4; ++w) {
                                const unsigned v = (((live >> (8 * w)) & 15u) << sh) | (((live >> (8 * w + 4)) & 15u) << (16 + sh));
                                if (v) atomicOr(&s_live[live_slot * 8 + wm * 4 + w], v);
                            }
                        }
                    }
                }
            }
            if constexpr (DEFER) {
                // the mask the NEXT tile will write (tile number + 1 mod 3 -- the one tile t - 2 wrote) is cleared here, in front of this
                // tile's first barrier.  Its readers read it between tile t - 2's checkpoint barrier and the next barrier they reach, at
                // the latest tile t - 1's first; this store lies behind that one.  Its next writers are in a stage of tile t + 1, behind
                // this tile's first barrier.  (Two masks by parity needed the leaving tile's second barrier: with one, wave 0 clears tile
                // t - 1's mask here while another wave still counts its bits; cleared behind this tile's first barrier instead, the store
                // races with the next tile's atomicOr.)
                if (kc == 0 && tid < 8) s_live[(live_slot == 2 ? 0 : live_slot + 1) * 8 + tid] = 0u;
            }
            if constexpr (ABANDON && !DEAL && RSC == 3) {
                if (park_early) {
                    int t = tid;
                    asm volatile("" : "+v"(t));
                    if (t < KW_M) s_rb[(tile_par ^ 1) * KW_M + t] = park_v;
                }
            }
            if constexpr (DEAL) {
                if (kc == 0 && d_draw && tid == 0) s_veto[2] = d_ticket;
            }
#ifdef RADAD_DEBUG_HOOKS
            if (p.stamps) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); KH_STAMP(10); }   // own DMA landed (stamps only)
#endif
            __syncthreads();     // waits vmcnt(0): the stage issued above has landed for everyone
            KH_STAMP(6);
            ++gbuf;
            if (kc == 0 && has_next && !park_early) park_row_terms(row_next, tile_par ^ 1);
            if constexpr (DEFER) {
                if (kc == 0 && df_pend) df_flush();          // the tile before this one was deferred: its atomic has returned
            }
            if constexpr (DEAL) {
                if (kc == 0 && d_draw) d_next2 = deal_tile(__builtin_amdgcn_readfirstlane(s_veto[2]));
            }
            if constexpr (ABANDON) {
                if (at_ck) {
                    ++ab_checked;
                    ab_spec = spec;
                    if (__builtin_amdgcn_readfirstlane(s_veto[tile_par]) != (int)(row0 >> 8)) { ab_skip = true; break; }
                    if constexpr (DEFER) {
                        // vetoed: how many rows of the tile (positions < rowlimit) are live; everyone reads the same eight words
                        int ns = 0;
#pragma unroll
                        for (int w = 0; w < 8; ++w) {
                            const int valid = min(32, max(0, rowlimit - 32 * w));
                            const unsigned keep = valid >= 32 ? 0xffffffffu : ((1u << valid) - 1u);
                            ns += __popc((unsigned)__builtin_amdgcn_readfirstlane((int)s_live[live_slot * 8 + w]) & keep);
                        }
                        if (ns >= 1 && ns <= KNN_DEFER_MAX_ROWS) { ab_defer = true; df_ns = ns; break; }
                    }
                    // the tile STAYS
                    ah_pred = knn_ahead_next(ah_pred, false);
                    if (spec) {
                        // ... over a head fetched for nothing: its own stage ab_ck goes over it, and one barrier waits for that
                        ++ah_wasted;
                        if (grp_half == 0) dma_half(cur_desc, gbuf & 1, k_lo + kc + 1, 0);
                        else dma_half(q_desc, gbuf & 1, k_lo + kc + 1, 1);
                        __syncthreads();
                    }
                }
            }
        }
        if constexpr (ABANDON) {
            if (ab_skip || ab_defer) {
                ah_pred = knn_ahead_next(ah_pred, true);
                if (ab_spec) ++ah_used;
            }
        }
        if constexpr (DEFER) {
            if (ab_defer) {
                // DEFERRED: the tile's live rows go to this query tile's list and the workgroup leaves as a skip does.  Wave 0 appends:
                // lane l holds rows 4 l ... 4 l + 3 (a nibble of word l >> 3) and their rank among the tile's live rows; lane 0
                // reserves the ns entries with ONE returning atomic, issued here and first read behind the next tile's first barrier
                // (df_flush), which waits vmcnt(0) anyway.  (The counter's address goes through an opaque zero, as the dealt kernel's
                // does: a provably uniform address makes hipcc aggregate the atomic over the wave and wait for it on the spot.)
                // The list holds ns x row tiles entries at least: no decision depends on the slot.
                ++ab_deferred;
                if (wave == 0) {
                    int lane_d = lane;
                    asm volatile("" : "+v"(lane_d));
                    const int wd = lane_d >> 3;
                    unsigned df_nib = 0u;
                    int df_rank = 0;
#pragma unroll
                    for (int w = 0; w < 8; ++w) {
                        const int valid = min(32, max(0, rowlimit - 32 * w));
                        const unsigned keep = valid >= 32 ? 0xffffffffu : ((1u << valid) - 1u);
                        const unsigned word = s_live[live_slot * 8 + w] & keep;
                        if (w < wd) df_rank += __popc(word);
                        if (w == wd) {
                            const int sh = 4 * (lane_d & 7);
                            df_nib = (word >> sh) & 15u;
                            df_rank += __popc(word & ((1u << sh) - 1u));
                        }
                    }
                    df_pack = ((unsigned)df_rank << 4) | df_nib;
                    if (lane_d == 0) {
                        int z = 0;
                        asm volatile("" : "+v"(z));
                        df_slot = atomicAdd(p.df_cnt + qt + z, df_ns);
                    }
                }
                df_pend = true;
                df_row = (int)row0;
            }
        }
        if constexpr (ABANDON) {
            if (ab_skip || ab_defer) {
                // without a head fetched ahead: the stage fetched during the checkpoint stage (this tile's stage ck) has landed behind
                // the barrier and is not read; the next tile's stage 0 goes over it, and one barrier waits for it (the leaving tile's
                // DMA bubble)
                if (ab_skip) ++ab_skipped;
                if (has_next && !ab_spec) {
                    if (grp_half == 0) dma_half(next_desc, gbuf & 1, 0, 0);
                    else dma_half(q_desc, gbuf & 1, 0, 1);
                    __syncthreads();
                }
                continue;
            }
        }
        KH_STAMP(8);
        if (!ABANDON && p.ksplit == 2) {
            // publish this half's partial sums, lane-linear (vector v of thread t at [v][t]); the second arrival adds the other half's
            int* s_flag = reinterpret_cast<int*>(s_rb + 2 * KW_M);
            // (K split: one tile per workgroup pair -- the pair's index is the tile's.  Taken from blockIdx here: `split * n_qtiles + qt`
            // kept two more values alive across the tile loop, and hipcc went from 204 VGPRs and no scratch to 256 + 73 spilled
            // dwords per lane -- 80 MB of scratch writes per launch of the dominant kernel, for a branch the 1 M-row scan never takes)
            // (the tile's index in the store, also for the sample pre-pass's spread tiles: the host sizes the scratch for it.  NOT
            // `split * n_qtiles + qt` or `blockIdx.x >> 1`: with either, hipcc's allocation of this whole kernel went from 204 VGPRs and
            // no scratch to 256 + 73 spilled dwords per lane -- 80 MB of scratch writes per launch of the dominant kernel, found in
            // round 4's WRITE_SIZE counter -- for a branch the 1 M-row scan never takes)
            const int64_t tile_id = (row0 / KW_M) * p.n_qtiles + qt;
            f32x4* mine = reinterpret_cast<f32x4*>(p.kacc) + ((tile_id * 2 + part) * 32) * KW_THREADS + tid;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) mine[(mt * NT + nt) * KW_THREADS] = acc[mt][nt];
            __threadfence();                         // release: the partial sums are visible device-wide before the counter moves
            __syncthreads();
            if (tid == 0) s_flag[0] = atomicAdd(&p.kflag[tile_id], 1);
            __syncthreads();
            if (s_flag[0] == 0) return;              // first to arrive: the other half finishes the tile (one tile per workgroup)
            if (tid == 0) p.kflag[tile_id] = 0;      // ready for the next launch
            __threadfence();                         // acquire
            const f32x4* other = reinterpret_cast<const f32x4*>(p.kacc) + ((tile_id * 2 + (part ^ 1)) * 32) * KW_THREADS + tid;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[mt][nt] += other[(mt * NT + nt) * KW_THREADS];
        }
        // ---- epilogue: scores in the v domain (v = a * s_qs[query]) -----------------------------------------------
        // The lane-derived indices are re-derived here from an OPAQUE copy of the lane id: hipcc would otherwise hoist every
        // epilogue address out of the tile loop, run out of registers and reload the spills here -- and a scratch reload is a
        // VMEM load, which makes it wait vmcnt(0): the whole DMA ring would drain once per tile.
        int lane_e = lane;
        asm volatile("" : "+v"(lane_e));
        const int l15 = lane_e & 15, lq = lane_e >> 4;
        if constexpr (RSC == 1 || RSC == 2) {
            const float* rs_t = s_rs + tile_par * KW_M;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int rl = wm * 128 + mt * 16 + 4 * lq;                   // rows rl..rl+3 = registers 0..3
                const f32x4 rs4 = *reinterpret_cast<const f32x4*>(rs_t + rl);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) acc[mt][nt][i] *= rs4[i];
            }
        }
        if (!SAMPLE && RADAD_DBG(p.debug, 1)) {      // keep the accumulators alive, skip the filter
            float keep = 0.f;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) keep += acc[mt][nt][(mt + nt) & 3];
            if (keep == 12345.678f) s_thr[tid & 255] = 1.f;
            continue;
        }
        if constexpr (SAMPLE) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int ql = wn * 64 + nt * 16 + l15;
                float b1 = -INFINITY, b2 = -INFINITY;
                int i1 = IDX_SENTINEL, i2 = IDX_SENTINEL;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int rl = wm * 128 + mt * 16 + 4 * lq + r;
                        const float v = rl < rowlimit ? acc[mt][nt][r] : -INFINITY;
                        const bool first = v > b1;
                        const bool second = !first && v > b2;
                        b2 = first ? b1 : (second ? v : b2);
                        i2 = first ? i1 : (second ? (int)(p.id_off + row0 + rl) : i2);
                        b1 = first ? v : b1;
                        i1 = first ? (int)(p.id_off + row0 + rl) : i1;
                    }
                if (q0 + ql < p.nq) {
                    const float qi = s_qi[ql], qc = s_qc[ql];
                    const int64_t base = ((int64_t)(q0 + ql) * p.n_splits + split) * 16 + (wm * 4 + lq) * 2;
                    p.part_score[base] = fmaf(b1, qi, qc);
                    p.part_idx[base] = i1;
                    p.part_score[base + 1] = fmaf(b2, qi, qc);
                    p.part_idx[base + 1] = i2;
                }
            }
            continue;
        }
        // Two forms of the emit, chosen per launch (wave-uniform): with a TIGHT floor (every launch of a large store: the floor
        // comes from >= 16 384 rows) candidates are rare and a slot is reserved as each one is met; with a LOOSE floor (a small store
        // scanned in one go: the floor comes from a 2048-row sample and ~1 % of all scores pass) slot-by-slot reservation made a wave
        // sit through a ~1 us atomic round trip for every (row, query) position at which ANY lane had a candidate (~60 per tile), so
        // there a lane counts first and reserves all its slots of a query with ONE atomic, the four of a lane issued together.
        // (The counting form costs the large scan 3 %: 0.898 against 0.874 ms on the benchmark; the slot form costs the 25 k-row
        // scan 0.04 of 0.27 ms.)
        if (p.loose_floor) {
            // every lane filters its NT x 32 scores against its queries' floors and emits the survivors (rare: the floor is a score
            // that k rows are known to reach) straight into the queries' candidate buffers.  ONE returning atomic per (lane, query)
            // reserves all of the lane's slots for that query, and the four of a lane are issued together before anything waits for
            // them: the first form reserved slot by slot, and a wave then sat through one ~1 us round trip for every (row, query)
            // position at which ANY of its lanes had a candidate -- with a loose floor (the reference's 25 k-row store: the floor comes
            // from a 2048-row sample) that was ~60 round trips per tile, 0.16 ms of a 0.25 ms scan.
            float thr4[NT];
            int cnt4[NT];
    #pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int ql = wn * 64 + nt * 16 + l15;
                // (score = v qi + qc with qi > 0: "score >= s_thr" is tested as "v >= (s_thr - qc) qs"; the subtraction rounds, so the
                // test admits at most an ulp-wide band more or less than s_thr -- inside the slack eps carries for forming the score)
                thr4[nt] = (q0 + ql < p.nq && !RADAD_DBG(p.debug, 32)) ? (s_thr[ql] - s_qc[ql]) * s_qs[ql] : INFINITY;
                float gm = -INFINITY;                    // (the common case -- nothing of this lane reaches the floor -- costs 16 v_max3)
    #pragma unroll
                for (int mt = 0; mt < MT; ++mt)
                    gm = fmaxf(gm, fmaxf(fmaxf(acc[mt][nt][0], acc[mt][nt][1]), fmaxf(acc[mt][nt][2], acc[mt][nt][3])));
                int c = 0;
                if (gm >= thr4[nt]) {
    #pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
    #pragma unroll
                        for (int r = 0; r < 4; ++r)
                            c += (wm * 128 + mt * 16 + 4 * lq + r < rowlimit && acc[mt][nt][r] >= thr4[nt]) ? 1 : 0;
                }
                cnt4[nt] = c;
            }
            int base4[NT];
    #pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                base4[nt] = cnt4[nt] > 0 ? atomicAdd(p.cand_cnt + (q0 + wn * 64 + nt * 16 + l15), cnt4[nt]) : 0;
    #pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                if (cnt4[nt] > 0) {
                    const int ql = wn * 64 + nt * 16 + l15;
                    const float qi = s_qi[ql], qc = s_qc[ql];
                    const int64_t cbase = (int64_t)(q0 + ql) * p.cand_cap;
                    int sl = base4[nt];
    #pragma unroll
                    for (int mt = 0; mt < MT; ++mt) {
                        if (fmaxf(fmaxf(acc[mt][nt][0], acc[mt][nt][1]), fmaxf(acc[mt][nt][2], acc[mt][nt][3])) >= thr4[nt]) {
    #pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int rl = wm * 128 + mt * 16 + 4 * lq + r;
                                if (rl < rowlimit && acc[mt][nt][r] >= thr4[nt]) {
                                    if (sl < p.cand_cap) {
                                        p.part_score[cbase + sl] = fmaf(acc[mt][nt][r], qi, qc);
                                        p.part_idx[cbase + sl] = MAPPED ? (int)(p.id_off + s_map[rl]) : (int)(p.id_off + row0 + rl);
                                    }
                                    ++sl;
                                }
                            }
                        }
                    }
                }
            }
        } else {
            // every lane filters its NT x 32 scores against its queries' floors and emits the survivors (rare: the floor is a score
            // that k rows are known to reach) straight into the queries' candidate buffers
    #pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int ql = wn * 64 + nt * 16 + l15;
                // (score = v qi + qc with qi > 0: "score >= s_thr" is tested as "v >= (s_thr - qc) qs"; the subtraction rounds, so the
                // test admits at most an ulp-wide band more or less than s_thr -- inside the slack eps carries for forming the score)
                const float thr = (s_thr[ql] - s_qc[ql]) * s_qs[ql];
                float gm = -INFINITY;
    #pragma unroll
                for (int mt = 0; mt < MT; ++mt)
                    gm = fmaxf(gm, fmaxf(fmaxf(acc[mt][nt][0], acc[mt][nt][1]), fmaxf(acc[mt][nt][2], acc[mt][nt][3])));
                if (q0 + ql < p.nq && gm >= thr && !RADAD_DBG(p.debug, 32)) {
                    const float qi = s_qi[ql], qc = s_qc[ql];
                    int* cnt = p.cand_cnt + (q0 + ql);
                    const int64_t cbase = (int64_t)(q0 + ql) * p.cand_cap;
    #pragma unroll
                    for (int mt = 0; mt < MT; ++mt) {
                        if (fmaxf(fmaxf(acc[mt][nt][0], acc[mt][nt][1]), fmaxf(acc[mt][nt][2], acc[mt][nt][3])) >= thr) {
    #pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int rl = wm * 128 + mt * 16 + 4 * lq + r;
                                if (rl < rowlimit && acc[mt][nt][r] >= thr) {
                                    const int sl = atomicAdd(cnt, 1);
                                    if (sl < p.cand_cap) {
                                        p.part_score[cbase + sl] = fmaf(acc[mt][nt][r], qi, qc);
                                        p.part_idx[cbase + sl] = MAPPED ? (int)(p.id_off + s_map[rl]) : (int)(p.id_off + row0 + rl);
                                    }
                                }
                            }
                        }
                    }
                }
            }
        }
        KH_STAMP(9);
        if (nk < 2 && has_next) __syncthreads();     // one K step per tile: the next tile's only barrier comes after park_row_terms' reader
    }
    if constexpr (DEFER) {
        if (df_pend) df_flush();                     // the workgroup's last tile was deferred
    }
    if constexpr (ABANDON) {
        if (tid == 0 && ab_checked > 0) {
            atomicAdd(p.ab_count, ab_checked);
            if (ab_skipped > 0) atomicAdd(p.ab_count + 1, ab_skipped);
            if constexpr (DEFER) { if (ab_deferred > 0) atomicAdd(p.df_tasks, ab_deferred); }
            if constexpr (!DEAL) {
                if (ah_used > 0) atomicAdd(p.ah_count, ah_used);
                if (ah_wasted > 0) atomicAdd(p.ah_count + 1, ah_wasted);
            }
        }
    }
}

template <int RSC>
__global__ __launch_bounds__(KW_THREADS, 1) void k_knn_hi(KnnHiParams p) { knn_hi_body<RSC, false>(p); }

// Whether the gate can open for ANY tile of this workgroup's chunk, and its query side (amin, rmax: knn_hi_gate).  Decided once, in front
// of the body, so that a workgroup that can never test runs the plain body: the abandoning one carries a wave-uniform branch around
// every stage's held-back MFMAs, measured at 2.5 % of the scan on unstructured queries.
// WHOLE (a dealt launch): decided per QUERY TILE over all of the launch's tiles, so that every workgroup of a query tile reaches the same
// answer from the same inputs -- were some to draw tickets while others walked their static chunks, tiles would be multiplied twice or
// never.  The workgroup's first two tickets are drawn here, under the loads of the per-query terms (*ticket: the first of them; a query
// tile whose gate stays shut draws too, and nobody reads its counters).
template <int RSC, bool WHOLE = false>
__device__ __forceinline__ bool knn_hi_gate_open(const KnnHiParams& p, float& amin, float& rmax, int* ticket = nullptr) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* s_pre = reinterpret_cast<float*>(smem);           // [16] (+ the ticket): the stage buffers are not in use yet
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int qt, split;
    if (!knn_hi_task(p, (int)blockIdx.x, qt, split)) return false;       // (the plain body returns at the same test)
    if constexpr (WHOLE) {
        if (tid == 0) reinterpret_cast<int*>(s_pre)[16] = atomicAdd(p.deal_cnt + ((int)blockIdx.x & 7) * KNN_DEAL_MAX_QTILES + qt, 2);
    }
    const int q = qt * KW_N + tid;
    float a = INFINITY, r = 0.f;
    if (tid < KW_N && q < p.nq) {
        float at, rq, sl, qi;
        knn_hi_ab_query<RSC>(p, q, at, rq, sl, qi);
        a = (at - sl) * qi;
        r = rq * qi;
        if (!(a == a) || !(r == r)) a = -INFINITY;            // NaN: shut
    }
    a = -wave_max(-a); r = wave_max(r);
    if (lane == 0) { s_pre[wave] = a; s_pre[8 + wave] = r; }
    __syncthreads();
    amin = fminf(fminf(s_pre[0], s_pre[1]), fminf(s_pre[2], s_pre[3]));
    rmax = fmaxf(fmaxf(s_pre[8], s_pre[9]), fmaxf(s_pre[10], s_pre[11]));
    if constexpr (WHOLE) *ticket = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(s_pre)[16]);
    const int64_t chunk_begin = WHOLE ? (int64_t)0 : (int64_t)split * p.chunk_stride;
    const int64_t chunk_end = WHOLE ? p.n : min(chunk_begin + p.chunk_rows, p.n);
    int open = 0;
    for (int64_t r0 = chunk_begin + (int64_t)tid * KW_M; r0 < chunk_end; r0 += (int64_t)KW_THREADS * KW_M)
        open |= knn_hi_gate(amin, rmax, p.ab_ry[r0 >> 8], RSC == 3 ? p.ab_b[r0 >> 8] : 0.f) ? 1 : 0;
    __syncthreads();                                         // (everyone has read s_pre)
    if (__any(open) && lane == 0) s_pre[wave] = 1.f;
    else if (lane == 0) s_pre[wave] = 0.f;
    __syncthreads();
    float any = 0.f;
#pragma unroll
    for (int w = 0; w < KW_WAVES; ++w) any += s_pre[w];
    __syncthreads();                                         // (the body's first DMA overwrites s_pre)
    amin = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(amin)));
    rmax = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(rmax)));
    return __builtin_amdgcn_readfirstlane(any > 0.f ? 1 : 0) != 0;
}

// the same scan with the early abandon: own symbol (profiles keep the two apart)
template <int RSC>
__global__ __launch_bounds__(KW_THREADS, 1) void k_knn_hi_abandon(KnnHiParams p) {
    float amin, rmax;
    if (knn_hi_gate_open<RSC>(p, amin, rmax)) knn_hi_body<RSC, false, true>(p, amin, rmax);
    else knn_hi_body<RSC, false, false>(p);
}

// the abandoning scan of a DEALT launch (knn_abandon_deal, knn_plan.h): own symbol, so that a launch that is not dealt runs
// k_knn_hi_abandon as it was, instruction for instruction.  A query tile whose gate is shut runs the plain body over its static chunks,
// exactly as before: the grid is the one the static chunks are cut for.
template <int RSC>
__global__ __launch_bounds__(KW_THREADS, 1) void k_knn_hi_abandon_deal(KnnHiParams p) {
    float amin, rmax;
    int ticket = 0;
    if (knn_hi_gate_open<RSC, true>(p, amin, rmax, &ticket)) knn_hi_body<RSC, false, true, true>(p, amin, rmax, ticket);
    else knn_hi_body<RSC, false, false>(p);
}

// the abandoning scan of a DEFERRING launch (knn_abandon_defer, knn_plan.h): own symbol, so that every other launch runs the kernel it
// ran.  A workgroup whose gate is shut runs the plain body and lists nothing.
template <int RSC>
__global__ __launch_bounds__(KW_THREADS, 1) void k_knn_hi_abandon_defer(KnnHiParams p) {
    float amin, rmax;
    if (knn_hi_gate_open<RSC>(p, amin, rmax)) knn_hi_body<RSC, false, true, false, true>(p, amin, rmax);
    else knn_hi_body<RSC, false, false>(p);
}

// the TILE tail of a deferring launch, for lists too long for the row tail below (knn_rowtail_takes): every listed row against its query
// tile, in full, with the launch's floors.  The grid is
// n_qtiles x n_splits workgroups (knn_hi_task); workgroup `split` takes tiles split, split + n_splits, ... of its query tile's list and
// leaves before any barrier when the list ends in front of its first.
template <int RSC>
__global__ __launch_bounds__(KW_THREADS, 1) void k_knn_hi_tail(KnnHiParams p) {
    int qt, split;
    if (!knn_hi_task(p, (int)blockIdx.x, qt, split)) return;
    const int cnt_all = p.df_cnt[qt];
    if (knn_rowtail_takes(cnt_all)) return;                  // a short list: the row tail's (k_knn_hi_rowtail)
    const int cnt = min(cnt_all, p.df_cap);
    for (int t = split; (int64_t)t * KW_M < cnt; t += p.n_splits) {
        knn_hi_body<RSC, false, false, false, false, true>(p, 0.f, 0.f, 0, t);
        __syncthreads();                                     // (the next tile's map and per-query terms go over this one's)
    }
}

// THE ROW TAIL: the tail of a deferring launch whose lists are short (knn_rowtail_takes, knn_plan.h) -- on the benchmark 3 % of their
// capacity.  The tile tail above scores such a list as a handful of 256-row tiles, each a chain of K stages (DMA, barrier, MFMAs) alone
// on its CU: its time is latency, not work.  Here the unit is a GROUP of KNN_ROWTAIL_GROUP = 16 consecutive list entries against the
// query tile's <= 256 queries, on a workgroup of 4 waves; the grid is persistent and host-planned (knn_defer_rowtail): workgroup `split`
// of a query tile walks groups split, split + n_splits, ... (knn_rowtail_span) and one whose first group lies beyond the list's end
// leaves after the load of the count.  Wave w takes queries 64 w ... 64 w + 63 as four 16-query blocks (4 f32x4 accumulators).  Lane
// (l15, lq) fetches the 16-byte chunk 4 s + lq of K step s (32 elements) of listed row l15 straight from the plane into registers --
// KR_RING_A steps are requested before anything waits, a step's registers are requested again for step s + KR_RING_A right behind its
// MFMAs -- and the same chunk of its four queries KR_RING_B steps ahead (the query tile is L2-resident).  No LDS staging, no barrier
// in the K loop; the per-query terms are parked in LDS once per workgroup.
// THE SCORE IS THE SCAN'S, bit for bit: the accumulator of (row, query) starts at 0 (RSC 0) or (bias_sign rbias[row]) s_qs[query] (RSC
// 3: the one multiply `rb4 * qs4` of knn_hi_body), then takes v_mfma_f32_16x16x32_f16 with rows as A and queries as B over the K steps
// in ascending order, chunk lq of each 64-byte half stage in lane quarter lq -- knn_hi_body's chain; where a row sits among the 16 of
// an MFMA changes nothing.  The test (acc >= (s_thr - s_qc) s_qs, +inf past nq) and the value written (fmaf(acc, qi, qc), id_off + row)
// are the body's counting form.  An entry past the list's end is a zero row that never emits (its offset lies past the descriptor).
// THE EMIT: the four lane quarters of a wave hold rows 4 lq ... 4 lq + 3 of the SAME 16 queries, so their counts are added inside the
// wave and quarter 0 reserves the slots of all four with one returning atomic per (query block, query), the four of a lane issued
// together; the slots are dealt by lane quarter.  (Nearly every listed row is a candidate of most queries, and same-address atomics
// serialise at ~10 ns each: hi_rows_body.)
constexpr int KR_THREADS = KNN_ROWTAIL_THREADS;
constexpr int KR_RING_A = 16;            // K steps of the rows in flight: dim 512 whole (64 VGPRs)
constexpr int KR_RING_B = 2;             // K steps of the queries in flight (16 VGPRs each)
static_assert(KR_THREADS == 256 && KW_N == 256 && KNN_ROWTAIL_GROUP == 16, "4 waves x 64 queries, one 16-row MFMA operand");
static_assert(KR_RING_A % KR_RING_B == 0 && KR_RING_B == 2, "a ring slot is named by the step's position in its block");

template <int RSC>
__global__ __launch_bounds__(KR_THREADS, 4) void k_knn_hi_rowtail(KnnHiParams p) {
    static_assert(RSC == 0 || RSC == 3, "the tail scores what an abandoning launch listed");
    __shared__ float s_at[KW_N], s_qs[KW_N], s_qi[KW_N], s_qc[KW_N];
    int qt, split;
    if (!knn_hi_task(p, (int)blockIdx.x, qt, split)) return;
    const int cnt_all = p.df_cnt[qt];
    if (!knn_rowtail_takes(cnt_all)) return;                 // (the tile tail's: block-uniform, before any barrier)
    const int cnt = min(cnt_all, p.df_cap);
    if (knn_rowtail_span(split, 0, p.n_splits, cnt).n <= 0) return;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lq = lane >> 4;
    const int q0 = qt * KW_N;
    {
        // the per-query terms, as knn_hi_body forms them; s_at: what the epilogue compares against
        const bool owner = q0 + tid < p.nq;
        float qi = owner ? p.qscale[q0 + tid] : 1.f;
        if (RSC == 0) qi *= p.uscale;
        if (RSC == 3) qi *= p.uscale * p.mult;
        const float qs = 1.0f / qi;                          // powers of two: exact
        const float qc = (RSC >= 2 && owner && p.qconst) ? p.qconst[q0 + tid] : 0.f;
        const float thr = (owner && p.thr_init) ? p.thr_init[q0 + tid] : -INFINITY;
        s_qi[tid] = qi; s_qs[tid] = qs; s_qc[tid] = qc;
        s_at[tid] = (owner && !RADAD_DBG(p.debug, 32)) ? (thr - qc) * qs : INFINITY;         // (debug bit 32: no emit, as in the body)
    }
    __syncthreads();
    const int nk = p.row_bytes >> 6;                         // 64-byte K steps per row: EVEN and >= 2 = KR_RING_B, because row_bytes is a
                                                             // multiple of 128 (KnnHiParams; the tile scan's own condition, dim % 64 == 0)
    // rows: the launch's plane through one 32-bit descriptor (KNN_DEFER_MAX_BYTES); queries: this query tile's, the ones past nq read as zero
    const __amdgpu_buffer_rsrc_t a_desc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(p.db)), 0, (int)p.df_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t q_desc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(p.q) + (int64_t)q0 * p.row_bytes), 0, min(KW_N, p.nq - q0) * p.row_bytes, 0x00020000);
    const unsigned vb0 = (unsigned)((wave * 64 + l15) * p.row_bytes + lq * 16);
    const unsigned vb_nt = (unsigned)(16 * p.row_bytes);
    auto load_b = [&](f16x8 (&dst)[4], int s, bool in = true) {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
            dst[nt] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(q_desc, in ? vb0 + nt * vb_nt : 0x7FFF0000u, s * 64, 0));
    };
    const int* list = p.df_list + (int64_t)qt * p.df_cap;
    for (int round = 0;; ++round) {
        const RowTailSpan span = knn_rowtail_span(split, round, p.n_splits, cnt);
        if (span.n <= 0) break;
        f16x8 a[KR_RING_A], b[KR_RING_B][4];
#pragma unroll
        for (int j = 0; j < KR_RING_B; ++j) load_b(b[j], j);         // (nk >= 2 = KR_RING_B)
        const int row = l15 < span.n ? list[span.first + l15] : -1;
        float rb_own = 0.f;
        if (RSC == 3) rb_own = row >= 0 ? p.bias_sign * p.rbias[row] : 0.f;
        const unsigned va = row < 0 ? p.df_bytes : (unsigned)row * (unsigned)p.row_bytes + (unsigned)(lq * 16);
#pragma unroll
        for (int j = 0; j < KR_RING_A; ++j) {
            // (a step the row does not have is requested past the descriptor's end -- zeros, no memory access -- and never multiplied:
            // every ring register is DEFINED in every round, or hipcc carries the ring across the emit and spills around it)
            a[j] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(a_desc, j < nk ? va : p.df_bytes, j * 64, 0));
        }
        // acc[nt][r] = listed row 4 lq + r, query wave * 64 + nt * 16 + l15
        f32x4 acc[4];
        if (RSC == 3) {
            int lane_s = lane;
            asm volatile("" : "+v"(lane_s));             // (opaque, as in the emit below)
            f32x4 rb4;
#pragma unroll
            for (int r = 0; r < 4; ++r) rb4[r] = __shfl(rb_own, 4 * (lane_s >> 4) + r, 64);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[nt] = rb4 * s_qs[wave * 64 + nt * 16 + (lane_s & 15)];
        } else {
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        // whole blocks of KR_RING_A steps run as straight-line code (no branch around a load or an MFMA: hipcc counts the loads in flight
        // per path and, across branches, waits for ALL of them at every step).  A step past the row's end is requested past the
        // descriptor's end, as above.
        int s0 = 0;
        for (; s0 + KR_RING_A <= nk; s0 += KR_RING_A) {
#pragma unroll
            for (int j = 0; j < KR_RING_A; ++j) {
                const int s = s0 + j;
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[j], b[j % KR_RING_B][nt], acc[nt], 0, 0, 0);
                a[j] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(a_desc, s + KR_RING_A < nk ? va : p.df_bytes, (s + KR_RING_A) * 64, 0));
                load_b(b[j % KR_RING_B], s + KR_RING_B, s + KR_RING_B < nk);
                __builtin_amdgcn_sched_barrier(0);       // (pins the order: hipcc otherwise hoists the block's loads and spills)
            }
        }
        // the rest of the row, in pairs of steps (nk is even); its rows are in the ring already
#pragma unroll
        for (int j = 0; j < KR_RING_A; j += 2) {
            if (s0 + j < nk) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[j + h], b[h][nt], acc[nt], 0, 0, 0);
                }
                load_b(b[0], s0 + j + 2, s0 + j + 2 < nk);
                load_b(b[1], s0 + j + 3, s0 + j + 3 < nk);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // the emit: count per lane, add over the lane quarters, one atomic per (query block, query), slots dealt by quarter
        // (the lane-derived indices come from an OPAQUE copy of the lane id, as in knn_hi_body's epilogue: hipcc otherwise hoists every
        // address of the emit out of the group loop and spills them around the K loop)
        int lane_e = lane;
        asm volatile("" : "+v"(lane_e));
        const int e15 = lane_e & 15, eq = lane_e >> 4;
        const int ql0 = wave * 64 + e15;
        int tot4[4], off4[4], base4[4], row_e[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) row_e[r] = __shfl(row, 4 * eq + r, 64);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const float at = s_at[ql0 + nt * 16];
            int c = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) c += (row_e[r] >= 0 && acc[nt][r] >= at) ? 1 : 0;
            const int c0 = __shfl(c, e15, 64), c1 = __shfl(c, 16 + e15, 64), c2 = __shfl(c, 32 + e15, 64), c3 = __shfl(c, 48 + e15, 64);
            tot4[nt] = c0 + c1 + c2 + c3;
            off4[nt] = (eq > 0 ? c0 : 0) + (eq > 1 ? c1 : 0) + (eq > 2 ? c2 : 0);
        }
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
            base4[nt] = (eq == 0 && tot4[nt] > 0) ? atomicAdd(p.cand_cnt + (q0 + ql0 + nt * 16), tot4[nt]) : 0;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            int sl = __shfl(base4[nt], e15, 64) + off4[nt];
            if (tot4[nt] > 0) {
                const int ql = ql0 + nt * 16;
                const float at = s_at[ql], qi = s_qi[ql], qc = s_qc[ql];
                const int64_t cbase = (int64_t)(q0 + ql) * p.cand_cap;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (row_e[r] >= 0 && acc[nt][r] >= at) {
                        if (sl < p.cand_cap) {
                            p.part_score[cbase + sl] = fmaf(acc[nt][r], qi, qc);
                            p.part_idx[cbase + sl] = (int)(p.id_off + row_e[r]);
                        }
                        ++sl;
                    }
                }
            }
        }
    }
}

// the threshold pre-pass over the first rows of the store: same K loop, own symbol (profiles keep the two apart);
// one tile per workgroup
template <int RSC>
__global__ __launch_bounds__(KW_THREADS, 1) void k_knn_hi_sample(KnnHiParams p) { knn_hi_body<RSC, true>(p); }

// The abandon's per-tile terms, read off the values the scan multiplies: one workgroup per aligned KW_M-row tile, a wave per row.
struct TileTermsParams {
    const _Float16* plane = nullptr; // [n][dim] the f16 plane, or the rows of an fp16 store
    int dim = 0, suf_from = 0;
    int64_t n = 0, tile0 = 0;        // rows of the store; first tile to compute (the grid covers tile0 ... the last)
    const float* rbias = nullptr;    // [n] per-row bias of a biased scan (RSC 3), or nullptr
    float bias_sign = 1.f;
    float* ry = nullptr;             // [tiles] max_i |yh_i[suf_from:]|, fp32 sum of squares inflated like hi_rows_body's norms
    float* bmax = nullptr;           // [tiles] max_i bias_sign x bias_i (0 without a bias)
};
static_assert(std::is_trivially_copyable_v<TileTermsParams>, "kernel argument");

__global__ __launch_bounds__(256) void k_tile_terms(TileTermsParams p) {
    __shared__ float s_m[8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t tile = p.tile0 + blockIdx.x;
    const int64_t row_end = min((tile + 1) * (int64_t)KW_M, p.n);
    const int nv = (p.dim - p.suf_from) >> 3;                // f16x8 chunks of the suffix
    float m = 0.f;
    for (int64_t row = tile * KW_M + wave; row < row_end; row += 4) {
        const f16x8* src = reinterpret_cast<const f16x8*>(p.plane + row * p.dim + p.suf_from);
        float ss = 0.f;
        for (int i = lane; i < nv; i += 64) {
            const f16x8 v = src[i];
#pragma unroll
            for (int j = 0; j < 8; ++j) ss = fmaf((float)v[j], (float)v[j], ss);
        }
        const float nrm = sqrtf(wave_sum(ss)) * (1.0f + 0x1p-10f);
        m = (nrm == nrm) ? fmaxf(m, nrm) : INFINITY;         // (a NaN row can never let its tile be skipped)
    }
    float b = -INFINITY;
    if (p.rbias) {
        const int64_t row = tile * KW_M + threadIdx.x;
        if (row < row_end) { const float v = p.bias_sign * p.rbias[row]; b = (v == v) ? v : INFINITY; }
        b = wave_max(b);
    }
    if (lane == 0) { s_m[wave] = m; s_m[4 + wave] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        p.ry[tile] = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
        p.bmax[tile] = p.rbias ? fmaxf(fmaxf(s_m[4], s_m[5]), fmaxf(s_m[6], s_m[7])) : 0.f;
    }
}

// ---- operand preparation ---------------------------------------------------------------------------------------
// one wave per row: hi[row][:] = f16(in[row][:] * 2^e), scale_out[row] = 2^-e.
//   fixed_e == INT_MIN: e per row so that the row maximum lands in [2^13, 2^14) (any data range is safe);
//   otherwise e = fixed_e for every row (cosine stores: |x| <= 1, e = 14; un-scaled fp16 queries: e = 0).
// Measured on the way: |x| and |x - xh| (Euclidean, of the un-scaled row).
//   stat_max  (optional) [2] float bits: atomic max over rows of |x| and |x - xh|           (store side)
//   eps_out   (optional) [n]: the error bound eps(q) of this row used as a QUERY against a store with the given
//             max |y| = ystat[0], max |y - yh| = ystat[1] (read from device memory: no host round trip)
struct HiRowsParams {
    const void* in = nullptr;        // fp32 rows, or fp16 rows when in_f16 (statistics of an fp16 store)
    int in_f16 = 0;
    _Float16* hi = nullptr;          // [n][dim] or nullptr (statistics only)
    float* scale_out = nullptr;      // [n] or nullptr
    unsigned* stat_max = nullptr;    // [4] or nullptr: max |x'|, max |x' - xh|, max |x|, max |mu.x'| (x' = x - mu when centred)
    float* eps_out = nullptr;        // [n] or nullptr
    const unsigned* ystat = nullptr; // [4] store statistics (float bits) for eps_out
    int64_t n = 0;
    int dim = 0;
    int fixed_e = 0;
    int l2 = 0;                      // eps for the L2 ranking score 2 q.y - |y|^2
    int exact_ops = 0;               // 1: the scan multiplies the fp32 operands themselves (fp32 MFMA paths): rounding terms are 0
    float* norm_out = nullptr;       // optional [n][dim]: rows are first normalised x / (|x| + 1e-12) (cosine queries, the arithmetic of
                                     // k_rows_prepare mode 2) and written here; everything else is computed from the normalised row
    int* zero_flags2 = nullptr;      // optional [n]: a second per-row array to clear (the IVF list scan's running bounds)
    int* zero_flags = nullptr;       // optional [n]: set to 0 (the search's per-query flags) ...
    int* zero_counters = nullptr;    // ... and [8] counters, cleared by the first wave: saves the search a memset launch
    // CENTRED planes (knn_ensure_hi decides per store): the rounded operand is x' = x - mu, so that a common component of all
    // embeddings -- pooled encoder features share most of their mean -- does not eat the f16 mantissa: the Cauchy-Schwarz error
    // bound scales with |x'|, not |x|.  L2 is translation invariant; for IP / cosine q.y = q'.y' + mu.y + q'.mu.
    const float* mu = nullptr;       // [dim] or nullptr
    float mu_norm = 0.f;             // |mu|, rounded up (host-known: computed once, when the plane is built)
    float mu_sq = 0.f;               // |mu|^2 as the device summed it (a term of the per-query constant)
    int biased = 0;                  // 1: the scan runs the scale + bias variant (RSC 2): L2 always, IP / cosine when centred
    // IP / cosine: q.y = q'.y' + mu.y' + (q'.mu + |mu|^2) -- the row's share is mu.y' (small: the centred rows are nearly
    // orthogonal to their mean), the large |mu|^2 goes with the query's constant, so the accumulators never carry it
    float* bias_out = nullptr;       // store side, optional [n]: |x'|^2 (L2) or mu.x' (IP / cosine)
    float* qconst_out = nullptr;     // query side, optional [n]: -|x'|^2 (L2) or x'.mu + |mu|^2 (IP / cosine)
    // the tile scan's early abandon: norms of the RAW f16 values xh 2^e (the accumulators' units) from element suf_from on
    int suf_from = 0;                // a multiple of 64 (knn_abandon_suffix_from), 0 = none wanted
    float* suf_out = nullptr;        // query side, [n]: |xh[suf_from:]|, inflated like the other norms
    float* ab_slack_out = nullptr;   // query side, [n] (with eps_out): 2 dim 2^-23 (|qh| max |yh| + |c0|max), true units
    int* zero_ab = nullptr;          // optional [2]: the abandon's counters, cleared with zero_counters
    int* zero_deal = nullptr;        // optional [KNN_DEAL_COUNTERS]: the ticket counters of the search's dealt launches, cleared by row 0's team
};
static_assert(std::is_trivially_copyable_v<HiRowsParams>, "kernel argument");
constexpr int HI_E_PER_ROW = -0x7fffffff - 1;

// WPR = waves per row: 1 (a wave per row, four rows per workgroup: the plane's rows, batches of queries) or 4 (the whole workgroup on
// one row: the <= 16 queries of an online search -- ONE query of dim 5376 took a single wave 13 us of a 110 us search, three to four
// sequential sweeps of 21 loads each).  The two forms add their partial sums in different orders: the normalised query, the bound and
// the constants differ in their last bits between them, never within a batch size class; what a search returns is decided by
// the float64 re-rank either way.
template <int WPR>
__device__ __forceinline__ float hi_rows_sum(float v, float* scratch) {
    v = wave_sum(v);
    if (WPR == 1) return v;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    return (scratch[0] + scratch[1]) + (scratch[2] + scratch[3]);
}
template <int WPR>
__device__ __forceinline__ float hi_rows_max(float v, float* scratch) {
    v = wave_max(v);
    if (WPR == 1) return v;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(scratch[0], scratch[1]), fmaxf(scratch[2], scratch[3]));
}

template <int WPR>
__device__ __forceinline__ void hi_rows_body(const HiRowsParams& p) {
    static_assert(WPR == 1 || WPR == 4, "a wave or the whole workgroup per row");
    __shared__ float scratch[4];
    const int lane = WPR == 1 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;       // position inside the row's team
    constexpr int TEAM = 64 * WPR;
    const int64_t row = WPR == 1 ? (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6) : (int64_t)blockIdx.x;
    if (row >= p.n) return;                                                       // (WPR 4: uniform per workgroup)
    const int nv = p.dim >> 2;
    if (p.zero_deal && row == 0) { for (int i = lane; i < KNN_DEAL_COUNTERS; i += TEAM) p.zero_deal[i] = 0; }
    if (lane == 0) {
        if (p.zero_flags) p.zero_flags[row] = 0;
        if (p.zero_flags2) p.zero_flags2[row] = 0;
        if (p.zero_counters && row == 0) { for (int i = 0; i < 8; ++i) p.zero_counters[i] = 0; }
        if (p.zero_ab && row == 0) { p.zero_ab[0] = 0; p.zero_ab[1] = 0; }
    }
    float den = 1.f;
    if (p.norm_out) {                        // same arithmetic as k_rows_prepare<float> mode 2 (bit for bit)
        const f32x4* src = reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(p.in) + row * p.dim);
        float ss = 0.f;
        if (WPR == 1) {
            for (int i = lane; i < nv; i += 64) {
                const f32x4 v = src[i];
                ss += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
            }
            ss = wave_sum(ss);
        } else {
            // |x|^2 in the ONE-wave order whatever the team: the normalised query is part of the contract (radad_rownorm, the rows'
            // k_rows_prepare and both forms of this kernel give the same bits: tests/test_gpu_store_contents.py,
            // test_the_query_a_search_uses, reads the query a search used off unit-vector rows and compares it with radad_rownorm
            // bit for bit at 1, 16, 17 and 300 queries), the rest below is not
            if (threadIdx.x < 64) {
                for (int i = lane; i < nv; i += 64) {
                    const f32x4 v = src[i];
                    ss += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
                }
                ss = wave_sum(ss);
                if (threadIdx.x == 0) scratch[0] = ss;
            }
            __syncthreads();
            ss = scratch[0];
            __syncthreads();
        }
        den = sqrtf(ss) + 1e-12f;
        for (int i = lane; i < nv; i += TEAM) {
            f32x4 v = src[i];
            v[0] = v[0] / den; v[1] = v[1] / den; v[2] = v[2] / den; v[3] = v[3] / den;
            reinterpret_cast<f32x4*>(p.norm_out + row * (int64_t)p.dim)[i] = v;
        }
    }
    auto load4 = [&](int i) -> f32x4 {
        if (p.in_f16) {
            const f16x4 b = reinterpret_cast<const f16x4*>(reinterpret_cast<const _Float16*>(p.in) + row * p.dim)[i];
            return f32x4{(float)b[0], (float)b[1], (float)b[2], (float)b[3]};
        }
        f32x4 v = reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(p.in) + row * p.dim)[i];
        if (p.norm_out) { v[0] = v[0] / den; v[1] = v[1] / den; v[2] = v[2] / den; v[3] = v[3] / den; }   // == what was written above
        if (p.mu) {                                                   // x' = fl(x - mu): THE operand from here on
            const f32x4 m = reinterpret_cast<const f32x4*>(p.mu)[i];
            v[0] -= m[0]; v[1] -= m[1]; v[2] -= m[2]; v[3] -= m[3];
        }
        return v;
    };
    int e = p.fixed_e;
    if (e == HI_E_PER_ROW) {
        float mx = 0.f;
        for (int i = lane; i < nv; i += TEAM) {
            const f32x4 v = load4(i);
            mx = fmaxf(mx, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
        }
        mx = hi_rows_max<WPR>(mx, scratch);
        e = 0;
        if (mx > 0.f && mx < INFINITY) {
            int ex;
            (void)frexpf(mx, &ex);          // mx = m 2^ex, m in [0.5, 1)
            e = max(-100, min(100, 14 - ex));
        }
    }
    const float up = ldexpf(1.0f, e), down = ldexpf(1.0f, -e);
    float sx = 0.f, sd = 0.f, sh = 0.f, sm = 0.f, so = 0.f, ssuf = 0.f;
    const int suf_v = p.suf_from > 0 ? (p.suf_from >> 2) : nv;      // first 4-vector of the suffix
    for (int i = lane; i < nv; i += TEAM) {
        const f32x4 v = load4(i);
        f16x4 hi;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            hi[j] = (_Float16)fminf(fmaxf(v[j] * up, -65504.f), 65504.f);     // (a row far above the store's one scale saturates: its
                                                                              // residual is MEASURED below, the bound stays rigorous)
            const float back = (float)hi[j] * down;           // exact (power-of-two scaling of an f16 value)
            const float d = v[j] - back;
            sx = fmaf(v[j], v[j], sx);
            sd = fmaf(d, d, sd);
            sh = fmaf(back, back, sh);
            const float raw = (float)hi[j];
            if (i >= suf_v) ssuf = fmaf(raw, raw, ssuf);
        }
        if (p.mu) {                                           // mu.x'
            const f32x4 m = reinterpret_cast<const f32x4*>(p.mu)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sm = fmaf(m[j], v[j], sm);
                so = fmaf(v[j] + m[j], v[j] + m[j], so);          // |x|^2 of the un-centred row (to within rounding: inflated below)
            }
        }
        if (p.hi) reinterpret_cast<f16x4*>(p.hi + row * (int64_t)p.dim)[i] = hi;
    }
    sx = hi_rows_sum<WPR>(sx, scratch); sd = hi_rows_sum<WPR>(sd, scratch); sh = hi_rows_sum<WPR>(sh, scratch);
    sm = hi_rows_sum<WPR>(sm, scratch); so = hi_rows_sum<WPR>(so, scratch);
    if (p.suf_from > 0) ssuf = hi_rows_sum<WPR>(ssuf, scratch);       // (uniform: a kernel argument)
    if (lane != 0) return;
    if (p.bias_out) p.bias_out[row] = p.l2 ? sx : sm;
    if (p.qconst_out) p.qconst_out[row] = p.l2 ? -sx : sm + p.mu_sq;
    // the sums themselves carry fp32 rounding (relative <= (dim/64 + 8) 2^-24 each): inflate every norm by 2^-10
    const float infl = 1.0f + 0x1p-10f;
    const float nx = sqrtf(sx) * infl, nd = p.exact_ops ? 0.f : sqrtf(sd) * infl, nh = p.exact_ops ? nx : sqrtf(sh) * infl;
    if (p.scale_out) p.scale_out[row] = down;
    if (p.stat_max) {                        // non-negative floats order like their bit patterns
        // (an atomic only when the row raises the maximum it can see: a million rows hammering four addresses with atomicMax took
        // 45 ms -- same-address atomics serialise at ~10 ns each -- for a kernel that moves 3 GB)
        auto raise = [](unsigned* a, float v) {
            const unsigned u = __float_as_uint(v);
            if (u > *reinterpret_cast<volatile unsigned*>(a)) atomicMax(a, u);
        };
        raise(&p.stat_max[0], nx);
        raise(&p.stat_max[1], nd);
        raise(&p.stat_max[2], p.mu ? sqrtf(so) * infl * infl : nx);
        raise(&p.stat_max[3], fabsf(sm) * infl);       // |mu.x'|: what an IP row's accumulator starts from
    }
    if (p.suf_out) p.suf_out[row] = sqrtf(ssuf) * infl;     // (ssuf <= 16380 x 65504^2 = 7e13: finite)
    if (p.eps_out) {
        // (all norms are those of the CENTRED operands when the plane is centred: q' = fl(q - mu), y' = fl(y - mu))
        // (exact_ops: the fp32 kernels multiply the un-centred fp32 operands themselves: |y| is the un-centred maximum)
        const float ymax = __uint_as_float(p.ystat[p.exact_ops ? 2 : 0]), dymax = p.exact_ops ? 0.f : __uint_as_float(p.ystat[1]);
        // |a - q.y| <= |q - qh||y| + |qh||y - yh| + acc(|qh||yh| + |c0|);  acc = D 2^-23 covers any summation order of D exact
        // products in fp32 with round-to-nearest or truncation; c0 = the value the accumulator starts from (the biased variant:
        // |y|^2 / 2 for L2, mu.y for IP -- it takes part in every one of the accumulations)
        const float gamma = (float)p.dim * 0x1p-23f;
        const float gsum = (float)(p.dim / 64 + 16) * 0x1p-24f;        // relative error of an fp32 wave sum of `dim` terms
        const float yorig = ymax + p.mu_norm;                          // |y| <= |y'| + |mu|
        const float c0 = !p.biased ? 0.f : (p.l2 ? 0.5f * ymax * ymax : __uint_as_float(p.ystat[3]));
        float eps = nd * ymax + nh * dymax + gamma * (nh * (ymax + dymax) + c0);
        // the abandon's slack: the same accumulation term twice (the part of the sum done at the checkpoint and the part to come)
        if (p.ab_slack_out) p.ab_slack_out[row] = 2.f * gamma * (nh * (ymax + dymax) + c0) * infl;
        if (p.l2) {
            // the score 2 a - |y'|^2 - |q'|^2 estimates -|q - y|^2: |y'|^2 and |q'|^2 are fp32 wave sums, and the start value, the
            // epilogue's multiply and the constant's add each round once on a magnitude <= 2 |q'||y'| + |y'|^2 + |q'|^2
            eps = 2.f * eps + gsum * (ymax * ymax + nx * nx) + 0x1p-21f * (2.f * nx * ymax + ymax * ymax + nx * nx);
        } else if (p.mu) {
            // q.y = q'.y' + mu.y + q'.mu: two more fp32 wave sums (|mu.y| <= |mu||y|, |q'.mu| <= |q'||mu|), the roundings of forming
            // x' = fl(x - mu) on both sides (relative 2^-24 per element), and the adds
            eps += gsum * p.mu_norm * (yorig + nx + p.mu_norm) + 0x1p-21f * (nx * ymax + p.mu_norm * (yorig + nx + p.mu_norm));
        }
        p.eps_out[row] = eps * infl + 1e-30f;
    }
}

__global__ __launch_bounds__(256) void k_hi_rows(HiRowsParams p) { hi_rows_body<1>(p); }
__global__ __launch_bounds__(256) void k_hi_rows_wide(HiRowsParams p) { hi_rows_body<4>(p); }

// rows of a plane and batches of queries: a wave per row; the few queries of an online search: a workgroup per row
static inline void launch_hi_rows(const HiRowsParams& hp, hipStream_t st) {
    if (hp.n <= 16 && hp.stat_max == nullptr)
        hipLaunchKernelGGL(k_hi_rows_wide, dim3((unsigned)hp.n), dim3(256), 0, st, hp);
    else
        hipLaunchKernelGGL(k_hi_rows, dim3((unsigned)((hp.n + 3) / 4)), dim3(256), 0, st, hp);
}
