// knn_remove.inc -- radad_knn_remove_ids: remove rows from a flat store in place, on the device, keeping the order of the rest
// (faiss IndexFlat.remove_ids).  Included from knn.hip behind the handle and its entry points.
//
// Three steps (the plan, its slabs and the argument why no launch races with itself: knn_plan.h, knn_remove_plan):
//   mark    k_remove_mark scatters the id list into one byte per stored row (1 = drop) and takes the first removed row (atomicMin);
//   scan    k_remove_block_counts -> k_remove_scan_counts -> k_remove_offsets: excl[i] = rows dropped in front of row i, as per-block
//           counts, an exclusive scan of the counts by ONE workgroup, and in-block offsets.  Integers only, no atomics: the result does
//           not depend on the order anything ran in.  k_remove_offsets also writes the caller's old -> new id map;
//   move    k_remove_move, once per launch of the plan: one wave per row, 16-byte accesses.
// No kernel here waits for another workgroup: every dependence is a launch boundary on one stream.

namespace {

constexpr int RM_THREADS = 256;
static_assert(KNN_REMOVE_SCAN_ROWS == RM_THREADS * 8, "the count / offset kernels take eight flags per thread");

// flags[pos] = 1 for every id that names a stored row; anything else is skipped.  Several threads may store the same 1 to one byte
__global__ __launch_bounds__(RM_THREADS) void k_remove_mark(const int64_t* __restrict__ ids, int64_t n_ids, int64_t id_base, int64_t ntotal,
                                                            unsigned char* __restrict__ flags, long long* __restrict__ head /*[0] first removed row*/) {
    const int64_t i = (int64_t)blockIdx.x * RM_THREADS + threadIdx.x;
    if (i >= n_ids) return;
    const int64_t id = ids[i];
    if (id < id_base) return;                 // (negative ids included: id_base >= 0 is not assumed, the subtraction cannot overflow here)
    const int64_t pos = id - id_base;
    if (pos >= ntotal) return;
    flags[pos] = 1;
    if (pos < *reinterpret_cast<volatile long long*>(&head[0])) atomicMin(&head[0], (long long)pos);
}

// eight flags of one thread (the flag array is padded to whole blocks and zeroed: no bounds test) -> their sum
__device__ __forceinline__ int rm_load8(const unsigned char* flags, int64_t first, unsigned char f[8]) {
    const uint2 v = *reinterpret_cast<const uint2*>(flags + first);
    int s = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) { f[j] = (unsigned char)(((j < 4 ? v.x : v.y) >> (8 * (j & 3))) & 0xffu); s += f[j]; }
    return s;
}

// exclusive scan of one int per thread over a workgroup of RM_THREADS (4 waves); *total = the workgroup's sum
__device__ __forceinline__ int rm_block_exclusive(int v, int* total) {
    __shared__ int wave_sum_s[RM_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
    if (lane == 63) wave_sum_s[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < RM_THREADS / 64; ++w) { const int s = wave_sum_s[w]; if (w < wave) before += s; all += s; }
    __syncthreads();                          // (the kernels that call this twice reuse wave_sum_s)
    *total = all;
    return before + inc - v;
}

__global__ __launch_bounds__(RM_THREADS) void k_remove_block_counts(const unsigned char* __restrict__ flags, int* __restrict__ blk) {
    unsigned char f[8];
    const int s = rm_load8(flags, ((int64_t)blockIdx.x * RM_THREADS + threadIdx.x) * 8, f);
    int total;
    (void)rm_block_exclusive(s, &total);
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

// blk[0, n_blocks) -> its exclusive scan in place, blk[n_blocks] = head[1] = the sum.  ONE workgroup walks the array with a running
// carry (24 k counts for 50 M rows).  A store holds fewer than 2^31 rows, so every sum fits an int.
__global__ __launch_bounds__(RM_THREADS) void k_remove_scan_counts(int* __restrict__ blk, int64_t n_blocks, long long* __restrict__ head) {
    int carry = 0;
    for (int64_t b0 = 0; b0 < n_blocks; b0 += RM_THREADS) {
        const int64_t b = b0 + threadIdx.x;
        const int v = b < n_blocks ? blk[b] : 0;
        int total;
        const int ex = rm_block_exclusive(v, &total);
        if (b < n_blocks) blk[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) { blk[n_blocks] = carry; head[1] = carry; }
}

// excl[i] = rows dropped in front of row i; map[i] (when asked for) = the row's new global id, -1 for a dropped row
__global__ __launch_bounds__(RM_THREADS) void k_remove_offsets(const unsigned char* __restrict__ flags, const int* __restrict__ blk, int64_t ntotal,
                                                               int64_t id_base, int* __restrict__ excl, int64_t* __restrict__ map) {
    unsigned char f[8];
    const int64_t first = ((int64_t)blockIdx.x * RM_THREADS + threadIdx.x) * 8;
    const int s = rm_load8(flags, first, f);
    int total;
    int run = blk[blockIdx.x] + rm_block_exclusive(s, &total);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int64_t i = first + j;
        if (i < ntotal) {
            excl[i] = run;
            if (map) map[i] = f[j] ? -1 : id_base + i - run;
        }
        run += f[j];
    }
}

// what the planner needs of the prefix sum: the rows dropped in front of every slab's first row, then the dropped count of the store
__global__ __launch_bounds__(RM_THREADS) void k_remove_slab_counts(const int* __restrict__ excl, const int* __restrict__ blk, int64_t n_blocks,
                                                                   int64_t slab0, int64_t stage_rows, int64_t n_slabs, int64_t ntotal,
                                                                   int* __restrict__ slab_rb) {
    const int64_t j = (int64_t)blockIdx.x * RM_THREADS + threadIdx.x;
    if (j > n_slabs) return;
    const int64_t row = slab0 + j * stage_rows;
    slab_rb[j] = (j == n_slabs || row >= ntotal) ? blk[n_blocks] : excl[row];
}

// One row, `row_bytes` (a multiple of 8) from src to dst, both 8-byte aligned, by the 64 lanes of a wave.  Loads are 16 bytes wide and
// aligned: a source that starts 8 bytes past a 16-byte boundary (every second row of an fp16 store with dim % 8 == 4) gives its first
// 8 bytes on their own.  A 16-byte piece whose DESTINATION is only 8-byte aligned (source and destination row of different parity in
// such a store) is stored as two halves; the test is the same for every piece of the row, so the wave does not diverge.
__device__ __forceinline__ void rm_copy_row(char* __restrict__ dst, const char* __restrict__ src, int row_bytes, int lane) {
    const int head = (int)(reinterpret_cast<uintptr_t>(src) & 8);
    if (head && lane == 0) *reinterpret_cast<uint2*>(dst) = *reinterpret_cast<const uint2*>(src);
    const int n_vec = (row_bytes - head) >> 4;
    const bool dst_aligned = ((reinterpret_cast<uintptr_t>(dst) + head) & 8) == 0;
    for (int v = lane; v < n_vec; v += 64) {
        const uint4 x = *reinterpret_cast<const uint4*>(src + head + 16 * v);
        char* d = dst + head + 16 * v;
        if (dst_aligned) *reinterpret_cast<uint4*>(d) = x;
        else { *reinterpret_cast<uint2*>(d) = make_uint2(x.x, x.y); *reinterpret_cast<uint2*>(d + 8) = make_uint2(x.z, x.w); }
    }
    const int tail = head + 16 * n_vec;
    if (tail < row_bytes && lane == 63) *reinterpret_cast<uint2*>(dst + tail) = *reinterpret_cast<const uint2*>(src + tail);
}

struct RemoveMoveParams {
    char* rows = nullptr;                 // the store
    float* ynorm = nullptr;               // |y|^2 per row (L2 stores), or nullptr
    char* stage = nullptr;                // staging rows
    float* stage_norm = nullptr;
    const unsigned char* flags = nullptr;
    const int* excl = nullptr;
    int kind = KNN_REMOVE_DIRECT;
    int row_bytes = 0;
    int64_t row0 = 0, rows_n = 0, dst0 = 0;     // RemoveLaunch
    int64_t ntotal = 0, stage_rows = 0;         // bounds
};

// One launch of the plan, one wave per row (grid-stride).  GATHER: kept row i of [row0, row0 + rows_n) -> staging slot
// (i - excl[i]) - dst0.  SCATTER: staging slot s of [0, rows_n) -> store row dst0 + s.  DIRECT: kept row i -> store row i - excl[i],
// which the plan guarantees lies below row0.  A launch reads rows of the store or writes them, or writes only below what it reads.
__global__ __launch_bounds__(RM_THREADS) void k_remove_move(const RemoveMoveParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * (RM_THREADS / 64) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * (RM_THREADS / 64);
    for (int64_t w = wave0; w < p.rows_n; w += n_waves) {
        if (p.kind == KNN_REMOVE_SCATTER) {
            const int64_t d = p.dst0 + w;
            if (w >= p.stage_rows || d < 0 || d >= p.ntotal) continue;
            rm_copy_row(p.rows + (size_t)d * p.row_bytes, p.stage + (size_t)w * p.row_bytes, p.row_bytes, lane);
            if (p.ynorm && lane == 0) p.ynorm[d] = p.stage_norm[w];
            continue;
        }
        const int64_t i = p.row0 + w;
        if (i >= p.ntotal || p.flags[i]) continue;
        const int64_t d = i - p.excl[i];
        if (p.kind == KNN_REMOVE_GATHER) {
            const int64_t s = d - p.dst0;
            if (s < 0 || s >= p.stage_rows) continue;
            rm_copy_row(p.stage + (size_t)s * p.row_bytes, p.rows + (size_t)i * p.row_bytes, p.row_bytes, lane);
            if (p.ynorm && lane == 0) p.stage_norm[s] = p.ynorm[i];
        } else {
            if (d < 0 || d >= p.row0) continue;
            rm_copy_row(p.rows + (size_t)d * p.row_bytes, p.rows + (size_t)i * p.row_bytes, p.row_bytes, lane);
            if (p.ynorm && lane == 0) p.ynorm[d] = p.ynorm[i];
        }
    }
}

// what a removal leaves of the state the handle derived from its rows.  Rows in front of r0 (the first removed position) did not move:
// their part of the plane, of rscale / rbias (k_hi_rows writes them with the plane) and of the per-tile terms stays, and so do the
// centring vector, mu_norm, uniform_e and the plane's layout.  The watermarks fall to r0: the next search that wants them rewrites the
// plane from r0 on and recomputes the tiles from tile r0 / KW_M on, as after an append.  `stat` holds MAXIMA over the rows seen so
// far and is left alone: the maximum over a superset of the rows is at least the maximum over the rows, so eps only widens and the
// certificate stays sound.
static void knn_remove_derived(radad_knn_t h, int64_t r0, int64_t ntotal_after) {
    h->hi_rows = std::min(h->hi_rows, r0);
    h->stat_rows = std::min(h->stat_rows, r0);
    h->ab_rows = std::min(h->ab_rows, r0 / KW_M * KW_M);      // (whole tiles: the tile that holds r0 is taken again from its first row)
    h->tune.rows_removed(ntotal_after);
}

static int knn_remove_locked(radad_knn_t h, const int64_t* ids_dev, int64_t n_ids, int64_t* old_to_new_dev, int64_t* n_removed_out, hipStream_t st) {
    const int64_t n = h->ntotal;
    const size_t rb = h->row_bytes();
    const bool l2 = h->ynorm != nullptr;
    h->last_remove_launches = 0; h->last_remove_bytes = 0;
    // searches on other streams may still read the rows and the workspace
    RADAD_HIP_CHECK(hipDeviceSynchronize());
    if (n == 0 || n_ids == 0) {
        if (old_to_new_dev && n > 0) {
            // nothing goes: the identity map (a flag array of zeros through the same kernel)
            const RemoveLayout L0 = knn_remove_layout(n, rb, knn_remove_stage_rows(rb, h->opt_remove_stage_rows), l2);
            int rc = knn_workspace(h, L0.stage);      // (flags, counts and offsets only)
            if (rc) return rc;
            char* ws = static_cast<char*>(h->ws);
            RADAD_HIP_CHECK(hipMemsetAsync(ws + L0.flags, 0, L0.blk + (size_t)(L0.n_blocks + 1) * sizeof(int) - L0.flags, st));
            hipLaunchKernelGGL(k_remove_offsets, dim3((unsigned)L0.n_blocks), dim3(RM_THREADS), 0, st, (const unsigned char*)(ws + L0.flags),
                               (const int*)(ws + L0.blk), n, h->id_base, (int*)(ws + L0.excl), old_to_new_dev);
            RADAD_HIP_CHECK(hipGetLastError());
            RADAD_HIP_CHECK(hipStreamSynchronize(st));
        }
        return RADAD_OK;
    }
    const int64_t S = knn_remove_stage_rows(rb, h->opt_remove_stage_rows);
    const RemoveLayout L = knn_remove_layout(n, rb, S, l2);
    // (a failed allocation returns here: nothing of the store has been touched)
    int rc = knn_workspace(h, L.bytes);
    if (rc) return rc;
    char* ws = static_cast<char*>(h->ws);
    unsigned char* flags = reinterpret_cast<unsigned char*>(ws + L.flags);
    int* blk = reinterpret_cast<int*>(ws + L.blk);
    int* excl = reinterpret_cast<int*>(ws + L.excl);
    int* slab_rb = reinterpret_cast<int*>(ws + L.slab_rb);
    long long* head = reinterpret_cast<long long*>(ws + L.head);

    // mark + scan
    long long host_head[2] = {(long long)n, 0};
    RADAD_HIP_CHECK(hipMemsetAsync(flags, 0, (size_t)L.n_blocks * KNN_REMOVE_SCAN_ROWS, st));
    RADAD_HIP_CHECK(hipMemcpyAsync(head, host_head, sizeof(host_head), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_remove_mark, dim3((unsigned)ceil_div64(n_ids, RM_THREADS)), dim3(RM_THREADS), 0, st, ids_dev, n_ids, h->id_base, n, flags, head);
    hipLaunchKernelGGL(k_remove_block_counts, dim3((unsigned)L.n_blocks), dim3(RM_THREADS), 0, st, (const unsigned char*)flags, blk);
    hipLaunchKernelGGL(k_remove_scan_counts, dim3(1), dim3(RM_THREADS), 0, st, blk, L.n_blocks, head);
    hipLaunchKernelGGL(k_remove_offsets, dim3((unsigned)L.n_blocks), dim3(RM_THREADS), 0, st, (const unsigned char*)flags, (const int*)blk, n,
                       h->id_base, excl, old_to_new_dev);
    RADAD_HIP_CHECK(hipGetLastError());
    RADAD_HIP_CHECK(hipMemcpyAsync(host_head, head, sizeof(host_head), hipMemcpyDeviceToHost, st));
    RADAD_HIP_CHECK(hipStreamSynchronize(st));
    const int64_t r0 = host_head[0], removed = host_head[1];
    if (removed <= 0) return RADAD_OK;
    if (r0 < 0 || r0 >= n || removed > n) { radad_set_error("radad_knn_remove_ids: inconsistent scan (first %lld, removed %lld of %lld)", (long long)r0, (long long)removed, (long long)n); return RADAD_EHIP; }

    // the prefix sum at the slab starts -> the plan
    const int64_t n_slabs = knn_remove_n_slabs(n, r0, S);
    std::vector<int> rbv((size_t)n_slabs + 1);
    hipLaunchKernelGGL(k_remove_slab_counts, dim3((unsigned)ceil_div64(n_slabs + 1, RM_THREADS)), dim3(RM_THREADS), 0, st, (const int*)excl,
                       (const int*)blk, L.n_blocks, knn_remove_slab0(r0, S), S, n_slabs, n, slab_rb);
    RADAD_HIP_CHECK(hipGetLastError());
    RADAD_HIP_CHECK(hipMemcpyAsync(rbv.data(), slab_rb, rbv.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    RADAD_HIP_CHECK(hipStreamSynchronize(st));
    const RemovePlan plan = knn_remove_plan(n, rb, r0, h->opt_remove_stage_rows, l2, rbv.data());

    // From here on rows move: the store counts as changed whatever happens.
    h->ntotal = n - removed;
    knn_remove_derived(h, r0, h->ntotal);
    RemoveMoveParams mp;
    mp.rows = h->rows; mp.ynorm = h->ynorm; mp.stage = ws + L.stage; mp.stage_norm = l2 ? reinterpret_cast<float*>(ws + L.stage_norm) : nullptr;
    mp.flags = flags; mp.excl = excl; mp.row_bytes = (int)rb; mp.ntotal = n; mp.stage_rows = S;
    const int64_t max_grid = (int64_t)std::max(h->n_cus, 64) * 16;      // grid-stride beyond 16 workgroups of 4 waves per CU
    for (const RemoveLaunch& l : plan.launches) {
        mp.kind = l.kind; mp.row0 = l.row0; mp.rows_n = l.rows; mp.dst0 = l.dst0;
        const unsigned grid = (unsigned)std::min<int64_t>(max_grid, ceil_div64(l.rows, RM_THREADS / 64));
        hipLaunchKernelGGL(k_remove_move, dim3(grid), dim3(RM_THREADS), 0, st, mp);
    }
    RADAD_HIP_CHECK(hipGetLastError());
    // the staging buffer is the search workspace: a search on another stream must not find the moves still running
    RADAD_HIP_CHECK(hipStreamSynchronize(st));
    h->last_remove_launches = (int)plan.launches.size();
    h->last_remove_bytes = (int64_t)plan.bytes_moved;
    if (n_removed_out) *n_removed_out = removed;
    return RADAD_OK;
}

}  // namespace

extern "C" {

int radad_knn_remove_ids(radad_knn_t h, const int64_t* ids_dev, int64_t n_ids, int64_t* old_to_new_dev, int64_t* n_removed_out, void* stream) {
    RADAD_REQUIRE(h, "NULL handle");
    RADAD_REQUIRE(n_ids >= 0, "radad_knn_remove_ids: n_ids < 0");
    RADAD_REQUIRE(ids_dev || n_ids == 0, "radad_knn_remove_ids: ids is NULL");
    if (n_removed_out) *n_removed_out = 0;
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    // (the second half of a begun search reads rows / ntotal live while its candidate ids date from the first half)
    if (h->pending.valid || h->pending_excl.valid) {
        radad_set_error("radad_knn_remove_ids: a begun search (radad_knn_search_begin) must be finished or aborted before the store changes");
        return RADAD_ESTATE;
    }
    return knn_remove_locked(h, ids_dev, n_ids, old_to_new_dev, n_removed_out, (hipStream_t)stream);
}

int radad_knn_remove_ids_host(radad_knn_t h, const int64_t* ids_host, int64_t n_ids, int64_t* n_removed_out) {
    RADAD_REQUIRE(h, "NULL handle");
    RADAD_REQUIRE(n_ids >= 0, "radad_knn_remove_ids_host: n_ids < 0");
    RADAD_REQUIRE(ids_host || n_ids == 0, "radad_knn_remove_ids_host: ids is NULL");
    int64_t* tmp = nullptr;
    if (n_ids > 0) {
        DeviceGuard g(h->device);
        if (hipMalloc(&tmp, (size_t)n_ids * sizeof(int64_t)) != hipSuccess) { (void)hipGetLastError(); radad_set_error("hipMalloc of the id list failed"); return RADAD_ENOMEM; }
        const hipError_t e = hipMemcpy(tmp, ids_host, (size_t)n_ids * sizeof(int64_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(tmp); radad_set_error("H2D copy failed: %s", hipGetErrorString(e)); return RADAD_EHIP; }
    }
    const int rc = radad_knn_remove_ids(h, tmp, n_ids, nullptr, n_removed_out, nullptr);      // (returns with the moves complete)
    if (tmp) { DeviceGuard g(h->device); (void)hipFree(tmp); }
    return rc;
}

int radad_knn_last_remove(radad_knn_t h, int* n_launches, int64_t* bytes_moved) {
    RADAD_REQUIRE(h, "NULL handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (n_launches) *n_launches = h->last_remove_launches;
    if (bytes_moved) *bytes_moved = h->last_remove_bytes;
    return RADAD_OK;
}

}  // extern "C"
