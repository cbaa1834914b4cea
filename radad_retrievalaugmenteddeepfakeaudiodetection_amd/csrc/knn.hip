// knn.hip -- HBM-resident vector store + brute-force top-k for gfx950 (MI355X).
//
// Replaces the faiss IndexFlatL2 / IndexFlatIP object RADAD keeps in VectorDatabase.index
// (vector_database.py:56-97 create, :138 add, :181 search; pipeline.py:503 reconstruct).
//
// Kernels
//   k_rows_prepare   : append path -- copy (IP), copy + |y|^2 (L2) or normalise (cosine) incoming rows.
//   k_knn_f32        : the scan.  S = Y . Q^T on v_mfma_f32_32x32x2_f32 (exact f32) with a fused
//                      per-workgroup top-k: 128 store rows x 128 queries per tile, K stepped 32 at a
//                      time through double-buffered LDS; the store rows are the MFMA "A" side so that a
//                      lane owns ONE query column and its running k-th-best threshold lives in a register.
//   k_merge_refine   : picks k+6 fp32 candidates per query from the partial lists, re-scores them in float64 and
//                      ranks by (distance, id); k_merge_lists: P-way merge of final per-shard lists.
//   k_gather_rows    : batched reconstruct.
//
// Layout in HBM: rows [capacity, dim] fp32 row-major (insertion order), ynorm [capacity] fp32 (L2 only).
// Partial results: score [nq, n_splits, k] fp32 + local row index int32, same shape.
#include "common.h"
#include "knn_plan.h"

#include <algorithm>
#include <atomic>
#include <type_traits>
#include <mutex>
#include <new>
#include <stdlib.h>
#include <string.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <vector>

namespace {

// (KT_M x KT_N = 128 store rows x 128 queries per tile, KNN_THREADS = 256: knn_plan.h)
constexpr int KT_K = 32;        // K step
constexpr int KT_LD = KT_K + 4; // padded LDS row (floats): 36-dword stride is conflict-free for ds_read_b128
constexpr int KS_LD = KT_M + 4;  // score-tile row (floats): 132-dword stride keeps b128 writes and reads conflict-free
constexpr int IDX_SENTINEL = 0x7fffffff;

struct KnnParams {
    const void* db = nullptr;     // [n, dim] fp32, or fp16 when db_f16
    const float* ynorm = nullptr; // [n] (L2) or nullptr
    const void* q = nullptr;      // [nq, dim] (already normalised for cosine); fp16 for the fp16 tile kernel, fp32 otherwise
    int db_f16 = 0;
    int64_t n = 0;
    int nq = 0;
    int dim = 0;
    int k = 0;
    int l2 = 0;                   // 1: score = 2*dot - |y|^2 ; 0: score = dot
    int n_qtiles = 0;
    int n_splits = 0;             // multiple of 8
    int64_t chunk_rows = 0;       // rows per split, multiple of KT_M
    float* part_score = nullptr;  // [nq, n_splits, k]
    int* part_idx = nullptr;      // [nq, n_splits, k]
    int debug = 0;                // timing experiments only (RADAD_DEBUG_KNN): 1 = skip the top-k epilogue
};
static_assert(std::is_trivially_copyable_v<KnnParams>, "kernel argument");

__device__ __forceinline__ bool better(float s, int i, float ws, int wi) {
    return s > ws || (s == ws && i < wi);
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// One 128 x 128 tile of S = Y . Q^T over the full depth: acc[mt][nt] (wave sub-tile 64 x 64 as 2 x 2 MFMA 32x32 blocks).
// Global -> LDS staging uses buffer loads: the descriptors are wave-uniform (SGPRs), rows past the end of the
// chunk / of the query block fall outside num_records and read as zero, and a thread needs only four 32-bit
// offsets for all of its loads (the K step goes into the scalar offset).
struct TileCtx {
    int dim, nk, debug;
    unsigned voff[4];     // byte offset of (row ld_r + 32 i, col ld_c) inside a tile
    int ld_r, ld_c;
    int wm, wn, l31, lh;
};

template <bool A_F16>
__device__ __forceinline__ void knn_tile_gemm(const TileCtx& c, __amdgpu_buffer_rsrc_t ra_desc, __amdgpu_buffer_rsrc_t rq_desc,
                                              float* sA, float* sB, f32x16 (&acc)[2][2]) {
    f32x4 ra[4], rb[4];
    auto gload = [&](int kc) {
        // columns past `dim` (last K step when dim % 32 != 0) must read as zero: push the OFFSET out of range rather
        // than selecting on the loaded data -- a select would make the compiler wait for the loads right here
        const bool kin = kc * KT_K + c.ld_c < c.dim;
        const int soff = kc * KT_K * (int)sizeof(float);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned vo = kin ? c.voff[i] : 0x7FFF0000u;
            if (A_F16) {      // fp16 store: 4 halfs per lane, decoded to fp32 on the way to LDS (exact)
                typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
                const u32x2 hv = __builtin_amdgcn_raw_buffer_load_b64(ra_desc, kin ? (c.voff[i] >> 1) : 0x7FFF0000u, soff >> 1, 0);
                const f16x4 h4 = __builtin_bit_cast(f16x4, hv);
                ra[i] = f32x4{(float)h4[0], (float)h4[1], (float)h4[2], (float)h4[3]};
            } else {
                ra[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ra_desc, vo, soff, 0));
            }
            rb[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rq_desc, vo, soff, 0));
        }
    };
    auto swrite = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = c.ld_r + 32 * i;
            *reinterpret_cast<f32x4*>(sA + (buf * KT_M + r) * KT_LD + c.ld_c) = ra[i];
            *reinterpret_cast<f32x4*>(sB + (buf * KT_N + r) * KT_LD + c.ld_c) = rb[i];
        }
    };
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    gload(0);
    swrite(0);
    __syncthreads();
    for (int kc = 0; kc < c.nk; ++kc) {
        const int buf = kc & 1;
        if (kc + 1 < c.nk) gload(kc + 1);
        const float* a_base = sA + (buf * KT_M + c.wm * 64 + c.l31) * KT_LD + 4 * c.lh;
        const float* b_base = sB + (buf * KT_N + c.wn * 64 + c.l31) * KT_LD + 4 * c.lh;
#pragma unroll
        for (int kk = 0; kk < KT_K / 8; ++kk) {
            // lanes 0-31 hold k = 8kk+j, lanes 32-63 k = 8kk+4+j of their row: one ds_read_b128 feeds 4 MFMAs
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(a_base + kk * 8);
            const f32x4 a1 = *reinterpret_cast<const f32x4*>(a_base + 32 * KT_LD + kk * 8);
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(b_base + kk * 8);
            const f32x4 b1 = *reinterpret_cast<const f32x4*>(b_base + 32 * KT_LD + kk * 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], b0[j], acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], b1[j], acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], b0[j], acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], b1[j], acc[1][1], 0, 0, 0);
            }
        }
        if (kc + 1 < c.nk) swrite(buf ^ 1);
        __syncthreads();
    }
}

// Same tile product, software-pipelined ACROSS tiles: on entry chunk 0 of this tile already sits in LDS buffer
// (gbuf & 1); during the last K step the first chunk of the NEXT tile is fetched, so no tile starts by waiting
// for HBM.  On exit buffer (gbuf & 1) holds the next tile's chunk 0 (if has_next) and the other one is free.
__device__ __forceinline__ void knn_tile_gemm_pipelined(const TileCtx& c, __amdgpu_buffer_rsrc_t cur_desc,
                                                        __amdgpu_buffer_rsrc_t next_desc, bool has_next,
                                                        __amdgpu_buffer_rsrc_t rq_desc, float* sA, float* sB, int& gbuf,
                                                        f32x16 (&acc)[2][2]) {
    f32x4 ra[4], rb[4];
    auto gload = [&](__amdgpu_buffer_rsrc_t a_desc, int kc) {
        const bool kin = kc * KT_K + c.ld_c < c.dim;
        const int soff = kc * KT_K * (int)sizeof(float);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned vo = kin ? c.voff[i] : 0x7FFF0000u;
            ra[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(a_desc, vo, soff, 0));
            rb[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rq_desc, vo, soff, 0));
        }
    };
    auto swrite = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = c.ld_r + 32 * i;
            *reinterpret_cast<f32x4*>(sA + (buf * KT_M + r) * KT_LD + c.ld_c) = ra[i];
            *reinterpret_cast<f32x4*>(sB + (buf * KT_N + r) * KT_LD + c.ld_c) = rb[i];
        }
    };
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    for (int kc = 0; kc < c.nk; ++kc) {
        const int buf = gbuf & 1;
        const bool more = kc + 1 < c.nk;
        if (!RADAD_DBG(c.debug, 2)) {
            if (more) gload(cur_desc, kc + 1);
            else if (has_next) gload(next_desc, 0);
        }
        const float* a_base = sA + (buf * KT_M + c.wm * 64 + c.l31) * KT_LD + 4 * c.lh;
        const float* b_base = sB + (buf * KT_N + c.wn * 64 + c.l31) * KT_LD + 4 * c.lh;
#pragma unroll
        for (int kk = 0; kk < KT_K / 8; ++kk) {
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(a_base + kk * 8);
            const f32x4 a1 = *reinterpret_cast<const f32x4*>(a_base + 32 * KT_LD + kk * 8);
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(b_base + kk * 8);
            const f32x4 b1 = *reinterpret_cast<const f32x4*>(b_base + 32 * KT_LD + kk * 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], b0[j], acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], b1[j], acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], b0[j], acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], b1[j], acc[1][1], 0, 0, 0);
            }
        }
        if ((more || has_next) && !RADAD_DBG(c.debug, 4)) swrite(buf ^ 1);
        if (!RADAD_DBG(c.debug, 8)) __syncthreads();
        ++gbuf;
    }
}

// (re)load chunk 0 of a tile into buffer `buf`: block prologue, and after the rare overflow path clobbered the tiles
__device__ __forceinline__ void knn_tile_prime(const TileCtx& c, __amdgpu_buffer_rsrc_t a_desc, __amdgpu_buffer_rsrc_t rq_desc,
                                               float* sA, float* sB, int buf) {
    const bool kin = c.ld_c < c.dim;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned vo = kin ? c.voff[i] : 0x7FFF0000u;
        const int r = c.ld_r + 32 * i;
        *reinterpret_cast<f32x4*>(sA + (buf * KT_M + r) * KT_LD + c.ld_c) =
            __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(a_desc, vo, 0, 0));
        *reinterpret_cast<f32x4*>(sB + (buf * KT_N + r) * KT_LD + c.ld_c) =
            __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rq_desc, vo, 0, 0));
    }
    __syncthreads();
}

// ---- LDS-DMA variant of the tile product (register-list kernel) -------------------------------------------------
// The ablation of the register-staged loop showed the ds_write_b128 pass costing 8 % of the scan (7.84 -> 7.20 ms
// without it): staging now goes HBM/L2 -> LDS directly with `buffer_load_dwordx4 ... lds`, no VGPR round trip, no
// ds_write, 32 VGPRs freed.  LDS-DMA writes each wave-instruction's 64 x 16 B linearly, so the tiles are UNPADDED
// (128-byte rows) and bank conflicts are avoided by an XOR swizzle applied on the SOURCE side and on the reads:
// 16-byte chunk c of row r lives at chunk c ^ ((r >> 1) & 7).  A 16-lane ds_read_b128 group then covers all 64 banks.
constexpr int KD_ROW_BYTES = KT_K * 4;            // 128
constexpr int KD_TILE_BYTES = KT_M * KD_ROW_BYTES;   // 16 KB per operand per buffer
typedef __attribute__((address_space(3))) void* lds_ptr_t;

struct DmaCtx {
    int dim, nk, debug;
    unsigned voff[4];        // byte offset in the tile's global rows of this lane's 16 B, per DMA instruction
    unsigned dst[4];         // wave-uniform LDS byte offset (within one operand tile) of each DMA instruction
    unsigned rd_a, rd_b;     // LDS byte offset of this lane's A / B row (mt = 0 / nt = 0)
    unsigned rd_x;           // (lh ^ swizzle) << 4: XOR-ed with 32*kk gives the chunk offset inside the row
};

__device__ __forceinline__ DmaCtx make_dma_ctx(int dim, int tid, int debug, int esize) {
    DmaCtx c;
    c.dim = dim; c.nk = (dim * esize + KD_ROW_BYTES - 1) / KD_ROW_BYTES; c.debug = debug;   // 128 bytes of every row per K step
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int grp = wave * 4 + i;                 // 8-row group written by this instruction
        const int r = grp * 8 + (lane >> 3);
        const int pc = lane & 7;                      // physical chunk this lane fills
        const int lc = pc ^ ((r >> 1) & 7);           // logical chunk it must fetch
        c.voff[i] = (unsigned)(r * dim * esize + lc * 16);
        c.dst[i] = (unsigned)(grp * 1024);
    }
    const int l31 = lane & 31, lh = lane >> 5;
    const int wm = wave & 1, wn = wave >> 1;
    c.rd_a = (unsigned)((wm * 64 + l31) * KD_ROW_BYTES);
    c.rd_b = (unsigned)((wn * 64 + l31) * KD_ROW_BYTES);
    c.rd_x = (unsigned)((lh ^ ((l31 >> 1) & 7)) << 4);
    return c;
}

// issue the 8 DMA loads of one K chunk of (A tile, Q tile) into buffer `buf`
__device__ __forceinline__ void dma_issue(const DmaCtx& c, __amdgpu_buffer_rsrc_t a_desc, __amdgpu_buffer_rsrc_t q_desc, char* sA,
                                          char* sB, int buf, int kc) {
    const int soff = kc * KD_ROW_BYTES;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(a_desc, (lds_ptr_t)(sA + buf * KD_TILE_BYTES + c.dst[i]), 16, c.voff[i], soff, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(q_desc, (lds_ptr_t)(sB + buf * KD_TILE_BYTES + c.dst[i]), 16, c.voff[i], soff, 0, 0);
    }
}

template <bool F16, typename Hook>
__device__ __forceinline__ void knn_tile_gemm_dma(const DmaCtx& c, __amdgpu_buffer_rsrc_t cur_desc, __amdgpu_buffer_rsrc_t next_desc,
                                                  bool has_next, __amdgpu_buffer_rsrc_t q_desc, char* sA, char* sB, int& gbuf,
                                                  f32x16 (&acc)[2][2], Hook&& after_first_barrier) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    for (int kc = 0; kc < c.nk; ++kc) {
        const int buf = gbuf & 1;
        if (!RADAD_DBG(c.debug, 2)) {
            if (kc + 1 < c.nk) dma_issue(c, cur_desc, q_desc, sA, sB, buf ^ 1, kc + 1);
            else if (has_next) dma_issue(c, next_desc, q_desc, sA, sB, buf ^ 1, 0);
        }
        const char* a_row = sA + buf * KD_TILE_BYTES + c.rd_a;
        const char* b_row = sB + buf * KD_TILE_BYTES + c.rd_b;
#pragma unroll
        for (int kk = 0; kk < KT_K / 8; ++kk) {
            const unsigned off = c.rd_x ^ (unsigned)(32 * kk);      // chunk (2kk + lh) ^ swizzle, in bytes
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(a_row + off);
            const f32x4 a1 = *reinterpret_cast<const f32x4*>(a_row + 32 * KD_ROW_BYTES + off);
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(b_row + off);
            const f32x4 b1 = *reinterpret_cast<const f32x4*>(b_row + 32 * KD_ROW_BYTES + off);
            if constexpr (F16) {
                // the same 16 bytes are 8 halfs: k = 16kk + 8lh + j of the row -- exactly the A/B lane map of
                // v_mfma_f32_32x32x16_f16, so one MFMA (16x the fp32 rate) replaces the four below
                const f16x8 ha0 = __builtin_bit_cast(f16x8, a0), ha1 = __builtin_bit_cast(f16x8, a1);
                const f16x8 hb0 = __builtin_bit_cast(f16x8, b0), hb1 = __builtin_bit_cast(f16x8, b1);
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ha0, hb0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ha0, hb1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ha1, hb0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ha1, hb1, acc[1][1], 0, 0, 0);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], b0[j], acc[0][0], 0, 0, 0);
                    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], b1[j], acc[0][1], 0, 0, 0);
                    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], b0[j], acc[1][0], 0, 0, 0);
                    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], b1[j], acc[1][1], 0, 0, 0);
                }
            }
        }
        if (!RADAD_DBG(c.debug, 8)) __syncthreads();      // waits vmcnt(0): the DMA issued above has landed for everyone
        ++gbuf;
        if (kc == 0) after_first_barrier();       // work deferred from the previous tile's epilogue (no barriers inside)
    }
}

__device__ __forceinline__ TileCtx make_tile_ctx(int dim, int tid) {
    TileCtx c;
    c.debug = 0;
    c.dim = dim;
    c.nk = (dim + KT_K - 1) / KT_K;
    c.ld_r = tid >> 3;
    c.ld_c = (tid & 7) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) c.voff[i] = (unsigned)(((c.ld_r + 32 * i) * dim + c.ld_c) * (int)sizeof(float));
    const int lane = tid & 63, wave = tid >> 6;
    c.wm = wave & 1; c.wn = wave >> 1; c.l31 = lane & 31; c.lh = lane >> 5;
    return c;
}
// descriptor over `rows` rows of `dim` floats starting at `base` (wave-uniform inputs only)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rows_desc(const void* base, int rows, int dim, int esize = 4) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, rows * dim * esize, 0x00020000);
}

template <bool A_F16>
__global__ __launch_bounds__(KNN_THREADS, 2) void k_knn_f32(KnnParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sA = reinterpret_cast<float*>(smem);          // [2][KT_M][KT_LD]
    float* sB = sA + 2 * KT_M * KT_LD;                   // [2][KT_N][KT_LD]
    float* sS = sA;                                      // [KT_N][KS_LD] score tile, aliases both (epilogue only)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave & 1;    // which 64-row half of the store tile
    const int wn = wave >> 1;   // which 64-query half
    const int l31 = lane & 31;
    const int lh = lane >> 5;

    // XCD-aware mapping: blocks b and b+8 share an XCD (round-robin dispatch), so the n_qtiles blocks
    // that stream the SAME store chunk are placed on one XCD and run together -> the chunk is pulled
    // from HBM once and re-served from that XCD's L2.  Speed only; any placement is correct.
    const int bid = blockIdx.x;
    const int xcd = bid & 7;
    const int slot = bid >> 3;
    const int qt = slot % p.n_qtiles;
    const int split = (slot / p.n_qtiles) * 8 + xcd;

    const int q0 = qt * KT_N;
    const int64_t chunk_begin = (int64_t)split * p.chunk_rows;
    const int64_t chunk_end = min(chunk_begin + p.chunk_rows, p.n);
    const int k = p.k;

    // this block's output lists double as the running top-k lists (rarely touched; L2-resident)
    // thread t < 128 owns query q0+t for the whole scan: its threshold stays in a register.
    float my_thr = -INFINITY;
    float* my_ls = nullptr;
    int* my_li = nullptr;
    if (tid < KT_N && q0 + tid < p.nq) {
        my_ls = p.part_score + ((int64_t)(q0 + tid) * p.n_splits + split) * k;
        my_li = p.part_idx + ((int64_t)(q0 + tid) * p.n_splits + split) * k;
        for (int j = 0; j < k; ++j) { my_ls[j] = -INFINITY; my_li[j] = IDX_SENTINEL; }
    }
    if (chunk_begin >= chunk_end) return;

    const TileCtx tc = make_tile_ctx(p.dim, tid);
    const __amdgpu_buffer_rsrc_t q_desc =
        rows_desc(reinterpret_cast<const float*>(p.q) + (int64_t)q0 * p.dim, min(KT_N, p.nq - q0), p.dim);
    constexpr int AES = A_F16 ? 2 : 4;      // bytes per stored element

    for (int64_t row0 = chunk_begin; row0 < chunk_end; row0 += KT_M) {
        f32x16 acc[2][2];
        knn_tile_gemm<A_F16>(tc, rows_desc(reinterpret_cast<const char*>(p.db) + row0 * p.dim * AES,
                                           (int)min((int64_t)KT_M, chunk_end - row0), p.dim, AES), q_desc, sA, sB, acc);

        // ---- fused top-k epilogue -------------------------------------------------------------
        // acc[mt][nt][r] = dot(store row row0 + wm*64 + mt*32 + (r&3) + 8*(r>>2) + 4*lh,
        //                      query     q0   + wn*64 + nt*32 + l31)
        // The tile buffers are free now: park the 128x128 score tile in them, query-major
        // (S[q][row], row stride KS_LD), then ONE thread per query filters its 128 scores against the
        // k-th best it carries in a register and inserts the rare survivors into its list.
        const int rowlimit = (int)min((int64_t)KT_M, chunk_end - row0);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int rl = wm * 64 + mt * 32 + 8 * g + 4 * lh;   // rows rl..rl+3 = registers 4g..4g+3
                f32x4 v0, v1;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float s0 = acc[mt][0][4 * g + i], s1 = acc[mt][1][4 * g + i];
                    if (p.l2) {
                        const float yn = p.ynorm[min(row0 + rl + i, p.n - 1)];
                        s0 = 2.f * s0 - yn;
                        s1 = 2.f * s1 - yn;
                    }
                    v0[i] = s0;
                    v1[i] = s1;
                }
                *reinterpret_cast<f32x4*>(sS + (wn * 64 + l31) * KS_LD + rl) = v0;
                *reinterpret_cast<f32x4*>(sS + (wn * 64 + 32 + l31) * KS_LD + rl) = v1;
            }
        __syncthreads();
        if (tid < KT_N && q0 + tid < p.nq) {
            const float* srow = sS + tid * KS_LD;
            for (int c = 0; c < rowlimit; c += 4) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(srow + c);
                const float vm = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
                if (vm >= my_thr) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float sc = v[i];
                        const int id = (int)(row0 + c + i);
                        if (c + i < rowlimit && sc >= my_thr && better(sc, id, my_ls[k - 1], my_li[k - 1])) {
                            int pos = k - 1;
                            while (pos > 0 && better(sc, id, my_ls[pos - 1], my_li[pos - 1])) {
                                my_ls[pos] = my_ls[pos - 1];
                                my_li[pos] = my_li[pos - 1];
                                --pos;
                            }
                            my_ls[pos] = sc;
                            my_li[pos] = id;
                            my_thr = my_ls[k - 1];
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
}

// ---- scan kernel, register-list variant (k + margin <= KSEL) ---------------------------------------------------
// Same MFMA main loop as k_knn_f32; the fused top-k differs:
//   * thread t < 128 owns query q0+t and keeps its KSEL best (score, row) pairs in REGISTERS as 64-bit sortable
//     keys (ordered-float score in the high word, ~row in the low word: one u64 compare == (score, -row) order);
//     an insertion is a fully unrolled compare/select ladder -- no memory traffic, no pointer chasing.
//   * every lane filters its 64 accumulators against its two queries' thresholds (LDS, 1 float each) and pushes the
//     rare survivors into a per-query LDS slot buffer (CAND_CAP entries, ds_add_rtn for the slot);
//   * a query that overflows its buffer in one tile (always the first tile of a chunk, or adversarially ordered
//     data) takes the exact slow path: the whole 128x128 score tile is parked in LDS and its owner re-reads its row.
constexpr int CAND_CAP = 8;
typedef unsigned long long u64;

__device__ __forceinline__ u64 pack_key(float s, int id) {
    unsigned u = __float_as_uint(s);
    u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;
    return ((u64)u << 32) | (u64)(0xFFFFFFFFu - (unsigned)id);
}
__device__ __forceinline__ float key_score(u64 k) {
    unsigned u = (unsigned)(k >> 32);
    u ^= (u >> 31) ? 0x80000000u : 0xFFFFFFFFu;
    return __uint_as_float(u);
}
__device__ __forceinline__ int key_id(u64 k) { return (int)(0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull)); }

template <int KSEL>
__device__ __forceinline__ void list_insert(u64 (&l)[KSEL], u64 key) {
    if (key <= l[KSEL - 1]) return;
#pragma unroll
    for (int j = KSEL - 1; j >= 1; --j) {
        const bool up = key > l[j - 1];            // key ranks before entry j-1: that entry moves down to j
        const bool here = !up && key > l[j];       // key lands at j
        l[j] = up ? l[j - 1] : (here ? key : l[j]);
    }
    l[0] = key > l[0] ? key : l[0];
}

template <int KSEL, bool F16>
__global__ __launch_bounds__(KNN_THREADS, 2) void k_knn_f32_reg(KnnParams p) {
    constexpr int ES = F16 ? 2 : 4;          // bytes per element of BOTH operands (fp16 store is scanned with fp16 queries)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sA = smem;                                                  // [2][128 rows][128 B], swizzled
    char* sB = smem + 2 * KD_TILE_BYTES;                              // [2][128 rows][128 B], swizzled
    float2* s_cand = reinterpret_cast<float2*>(smem + 4 * KD_TILE_BYTES);   // [KT_N][CAND_CAP] (score, row bits), NOT aliased:
                                                                      // it outlives the tile (drained during the next K loop)
    float* s_thr = reinterpret_cast<float*>(s_cand + KT_N * CAND_CAP);   // [KT_N] current KSEL-th best score of each query
    int* s_cnt = reinterpret_cast<int*>(s_thr + KT_N);                // [KT_N] candidates pushed this tile
    int* s_flag = s_cnt + KT_N;                                       // [1] some query overflowed its slots this tile
    char* sS = smem;                                                  // [KT_N][512 B] swizzled score tile of the overflow path

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int l31 = lane & 31, lh = lane >> 5;

    const int bid = blockIdx.x;              // XCD-aware mapping: see k_knn_f32
    const int xcd = bid & 7;
    const int slot_b = bid >> 3;
    const int qt = slot_b % p.n_qtiles;
    const int split = (slot_b / p.n_qtiles) * 8 + xcd;

    const int q0 = qt * KT_N;
    const int64_t chunk_begin = (int64_t)split * p.chunk_rows;
    const int64_t chunk_end = min(chunk_begin + p.chunk_rows, p.n);
    const bool owner = tid < KT_N && q0 + tid < p.nq;

    const u64 SENT = pack_key(-INFINITY, IDX_SENTINEL);
    u64 lst[KSEL];
#pragma unroll
    for (int j = 0; j < KSEL; ++j) lst[j] = SENT;
    if (tid < KT_N) { s_thr[tid] = -INFINITY; s_cnt[tid] = 0; }
    if (tid == 0) *s_flag = 0;
    __syncthreads();

    const DmaCtx dc = make_dma_ctx(p.dim, tid, p.debug, ES);
    const __amdgpu_buffer_rsrc_t q_desc =
        rows_desc(reinterpret_cast<const char*>(p.q) + (int64_t)q0 * p.dim * ES, min(KT_N, p.nq - q0), p.dim, ES);
    const int ql[2] = {wn * 64 + l31, wn * 64 + 32 + l31};
    const bool qvalid[2] = {q0 + ql[0] < p.nq, q0 + ql[1] < p.nq};

    auto tile_desc = [&](int64_t r0) {
        return rows_desc(reinterpret_cast<const char*>(p.db) + r0 * p.dim * ES,
                         (int)max((int64_t)0, min((int64_t)KT_M, chunk_end - r0)), p.dim, ES);
    };
    int gbuf = 0;
    if (chunk_begin < chunk_end) {
        dma_issue(dc, tile_desc(chunk_begin), q_desc, sA, sB, 0, 0);
        __syncthreads();
    }
    // owners fold their slot buffer into the register list; no barrier inside, so it can run in the shadow of the
    // next tile's MFMA work (the pushes it reads were published by the epilogue's barrier)
    auto drain = [&]() {
        if (owner) {
            const int c = min(s_cnt[tid], CAND_CAP);
            if (c > 0) {
                for (int i = 0; i < c; ++i) {
                    const float2 cv = s_cand[tid * CAND_CAP + i];
                    list_insert<KSEL>(lst, pack_key(cv.x, __float_as_int(cv.y)));
                }
                s_thr[tid] = key_score(lst[KSEL - 1]);
            }
        }
        if (tid < KT_N) s_cnt[tid] = 0;
    };
    bool pending = false;
    for (int64_t row0 = chunk_begin; row0 < chunk_end; row0 += KT_M) {
        f32x16 acc[2][2];
        const bool has_next = row0 + KT_M < chunk_end;
        knn_tile_gemm_dma<F16>(dc, tile_desc(row0), tile_desc(row0 + KT_M), has_next, q_desc, sA, sB, gbuf, acc,
                          [&]() { if (pending) { drain(); pending = false; } });
        if (RADAD_DBG(p.debug, 1)) {      // timing experiment: keep the accumulators alive, skip the epilogue
            if (acc[0][0][0] + acc[0][1][5] + acc[1][0][9] + acc[1][1][15] == 12345.678f) s_thr[tid & 127] = 1.f;
            continue;
        }
        // ---- fused top-k epilogue -------------------------------------------------------------------------
        const int rowlimit = (int)min((int64_t)KT_M, chunk_end - row0);
        if (p.l2) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int rl = wm * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    const float yn = p.ynorm[min(row0 + rl, p.n - 1)];
                    acc[mt][0][r] = 2.f * acc[mt][0][r] - yn;
                    acc[mt][1][r] = 2.f * acc[mt][1][r] - yn;
                }
        }
        // phase 1: every lane filters its 2 x 32 scores and pushes survivors to its queries' slot buffers
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const float thr = s_thr[ql[nt]];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                float gm = acc[mt][nt][0];
#pragma unroll
                for (int r = 1; r < 16; ++r) gm = fmaxf(gm, acc[mt][nt][r]);
                if (qvalid[nt] && gm >= thr) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int rl = wm * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                        if (rl < rowlimit && acc[mt][nt][r] >= thr) {
                            const int sl = atomicAdd(&s_cnt[ql[nt]], 1);
                            if (sl < CAND_CAP)
                                s_cand[ql[nt] * CAND_CAP + sl] = make_float2(acc[mt][nt][r], __int_as_float((int)(row0 + rl)));
                            else
                                *s_flag = 1;
                        }
                    }
                }
            }
        }
        __syncthreads();                 // pushes, counters and the overflow flag are visible to everyone
        if (*s_flag == 0) {
            // common case: nothing overflowed.  The drain is deferred into the next tile's K loop (or done right here
            // for the last tile); no second barrier, the next K loop's own barriers order everything.
            if (has_next && dc.nk >= 2) pending = true;     // nk == 1: the only K-loop barrier precedes the drain hook
            else drain();
            continue;
        }
        // overflow path (exact, slower; always the first tile of a chunk): owners whose slots sufficed drain them, the
        // others re-read their whole row from the score tile, parked query-major over the tile buffers (512-byte rows,
        // 16-byte chunk c of query q at chunk c ^ (q & 15): conflict-free b128 writes and reads).
        const bool over = owner && s_cnt[tid] > CAND_CAP;
        if (!over) drain();
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int ch = (wm * 64 + mt * 32 + 8 * g + 4 * lh) >> 2;   // rows 4ch..4ch+3 = registers 4g..4g+3
                f32x4 v0, v1;
#pragma unroll
                for (int i = 0; i < 4; ++i) { v0[i] = acc[mt][0][4 * g + i]; v1[i] = acc[mt][1][4 * g + i]; }
                *reinterpret_cast<f32x4*>(sS + ql[0] * 512 + ((ch ^ (ql[0] & 15)) << 4)) = v0;
                *reinterpret_cast<f32x4*>(sS + ql[1] * 512 + ((ch ^ (ql[1] & 15)) << 4)) = v1;
            }
        __syncthreads();
        if (tid == 0) *s_flag = 0;
        if (over) {
            for (int c = 0; c < rowlimit; c += 4) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(sS + tid * 512 + (((c >> 2) ^ (tid & 15)) << 4));
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (c + i < rowlimit) list_insert<KSEL>(lst, pack_key(v[i], (int)(row0 + c + i)));
            }
            s_thr[tid] = key_score(lst[KSEL - 1]);
            s_cnt[tid] = 0;
        }
        __syncthreads();
        if (has_next) {                  // the score tile overwrote the prefetched chunk: fetch it again
            dma_issue(dc, tile_desc(row0 + KT_M), q_desc, sA, sB, gbuf & 1, 0);
            __syncthreads();
        }
    }
    // the lists leave the registers once, at the end of the chunk
    if (owner) {
        float* ls = p.part_score + ((int64_t)(q0 + tid) * p.n_splits + split) * p.k;
        int* li = p.part_idx + ((int64_t)(q0 + tid) * p.n_splits + split) * p.k;
#pragma unroll
        for (int j = 0; j < KSEL; ++j)
            if (j < p.k) { ls[j] = key_score(lst[j]); li[j] = key_id(lst[j]); }
    }
}

#include "knn_hi.inc"

// ---- small-batch scan (nq <= 16: the online `predict` case, pipeline.py:1038-1054) ------------------------------
// With a handful of queries the scan is HBM-bound (2 flop per stored byte per query), so the 128-query tile above
// would burn 8x-128x the needed MFMA time.  Here every WAVE streams its own slice of the store, 16 rows per step,
// whole 2 KB rows in one burst of 16-byte loads straight from HBM into registers (no LDS for the store: it is read exactly once), against the <=16 queries parked in LDS.
// v_mfma_f32_16x16x4_f32 with the store rows as A and the queries as B leaves a lane with ONE query column
// (lane & 15) and 4 rows per group, so the filter threshold is a register.  Each wave keeps private top-k lists
// (lanes 0-15 own one query each, lists in registers); survivors travel through a per-wave LDS slot buffer that can
// never overflow (16 slots per query = everything one step can produce).  No workgroup barrier inside the scan.
// (SQ_THREADS, SQ_NQ, SQ_SLOTS, SQ_LDS_BUDGET: knn_plan.h)
static_assert(sizeof(float2) == 8 && sizeof(u64) == 8 && sizeof(_Float16) == 2, "knn_plan.h sizes the streaming kernels' LDS (SQ_SLOT_BYTES, knn_sq_lds_hi) with these as literals");

struct SmallQParams {
    const float* db = nullptr; const float* ynorm = nullptr; const float* q = nullptr; // fp32 store only
    int64_t n = 0;
    int nq = 0, dim = 0, k = 0, l2 = 0;
    int rows_per_wave = 0;      // multiple of 16
    int n_parts = 0;            // workgroups = lists per query
    float* part_score = nullptr; int* part_idx = nullptr; // [nq, n_parts, k]
};
static_assert(std::is_trivially_copyable_v<SmallQParams>, "kernel argument");

template <int KSEL>
__global__ __launch_bounds__(SQ_THREADS, 2) void k_knn_f32_smallq(SmallQParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int qld = p.dim + 4;                                    // padded query row: conflict-free b128 reads
    float* sQ = reinterpret_cast<float*>(smem);                   // [nq][dim + 4]: only the queries there are (the reference's
                                                                  // predict() search is ONE query of dim 5376 / 3584)
    float2* sCand = reinterpret_cast<float2*>(sQ + p.nq * qld);   // [4 waves][16 q][SQ_SLOTS]
    int* sCnt = reinterpret_cast<int*>(sCand + 4 * SQ_NQ * 24);         // [4 waves][16]; the slot area is sized for the final
                                                                        // hand-over of 3 x 16 x 32 keys (12 KB) as well

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    for (int i = tid; i < p.nq * (p.dim >> 2); i += SQ_THREADS) {
        const int qq = i / (p.dim >> 2), c4 = i % (p.dim >> 2);
        *reinterpret_cast<f32x4*>(sQ + qq * qld + c4 * 4) = *reinterpret_cast<const f32x4*>(p.q + (int64_t)qq * p.dim + c4 * 4);
    }
    if (tid < 4 * SQ_NQ) sCnt[tid] = 0;
    __syncthreads();

    const int part = blockIdx.x * 4 + wave;      // this wave's slice of the store
    const int64_t w_begin = (int64_t)part * p.rows_per_wave;
    const int64_t w_end = min(w_begin + p.rows_per_wave, p.n);
    float2* myCand = sCand + wave * SQ_NQ * SQ_SLOTS;
    int* myCnt = sCnt + wave * SQ_NQ;

    const u64 SENT = pack_key(-INFINITY, IDX_SENTINEL);
    u64 lst[KSEL];                       // meaningful in lanes 0..15 (lane = query)
#pragma unroll
    for (int j = 0; j < KSEL; ++j) lst[j] = SENT;
    float thr = -INFINITY;               // threshold of query (lane & 15), refreshed from the owner lane
    // K mapping inside a 32-float block: load h (0/1), element j of lane group g is k = 16h + 4g + j, so one load
    // instruction reads 64 CONTIGUOUS bytes of each of its 16 rows and the pair covers the whole 128-byte line.
    const float* qrow = sQ + min(r16, p.nq - 1) * qld + 4 * g;     // columns >= nq repeat the last query (never admitted below)
    const int nkb = p.dim >> 5;

    for (int64_t row0 = w_begin; row0 < w_end; row0 += 16) {
        // 16 rows per step; a lane issues ALL its loads of a 512-float panel (32 x 16 B = the whole 2 KB row at
        // dim 512) before the first MFMA, so each row is fetched in one burst and 32 loads per lane are in flight.
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};       // even / odd K blocks: two MFMA chains
        const int64_t ra = min(row0 + r16, p.n - 1);                             // clamp: masked below
        const float* pa = p.db + ra * p.dim + 4 * g;
        constexpr int PKB = KSEL <= 16 ? 16 : 8;      // K blocks per panel (the 32-entry lists leave fewer registers)
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
        // acc0[e] + acc1[e]: row row0 + 4g + e, query r16
        bool any = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t row = row0 + 4 * g + e;
            float sc = acc0[e] + acc1[e];
            if (p.l2) sc = 2.f * sc - p.ynorm[min(row, p.n - 1)];
            if (row < w_end && r16 < p.nq && sc >= thr) {
                const int sl = atomicAdd(&myCnt[r16], 1);          // < SQ_SLOTS by construction (4 x 4 lanes)
                myCand[r16 * SQ_SLOTS + sl] = make_float2(sc, __int_as_float((int)row));
                any = true;
            }
        }
        if (__any(any)) {                                              // wave-uniform; LDS ops of one wave are ordered
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
    // one list per WORKGROUP leaves the kernel: waves 1-3 hand their lists to wave 0 through the slot buffer
    __syncthreads();
    u64* sKeys = reinterpret_cast<u64*>(sCand);                     // [3][16][KSEL] (<= the slot buffer's 16 KB)
    if (wave > 0 && lane < SQ_NQ) {
#pragma unroll
        for (int j = 0; j < KSEL; ++j) sKeys[((wave - 1) * SQ_NQ + lane) * KSEL + j] = lst[j];
    }
    __syncthreads();
    if (wave == 0 && lane < p.nq) {
        for (int w = 0; w < 3; ++w)
            for (int j = 0; j < KSEL; ++j) list_insert<KSEL>(lst, sKeys[(w * SQ_NQ + lane) * KSEL + j]);
        float* ls = p.part_score + ((int64_t)lane * p.n_parts + blockIdx.x) * p.k;
        int* li = p.part_idx + ((int64_t)lane * p.n_parts + blockIdx.x) * p.k;
#pragma unroll
        for (int j = 0; j < KSEL; ++j)
            if (j < p.k) { ls[j] = key_score(lst[j]); li[j] = key_id(lst[j]); }
    }
}

// ---- a SMALL store (<= RF_STAGE_MAX rows: the IVF index's centroids, vector_database.py:65-70; a database of a few thousand files):
// all scores, no lists.  The register-list kernels keep k + margin <= 32 candidates per (query, row slice) in sorted lists -- with
// 4096 rows over 16 workgroups nearly every row is an insertion (k_knn_f32_smallq<32>: 0.14 ms for ONE query against 4096 x 512,
// of which the 8 MB of rows are 1 us).  Here every (row, query) score is written out -- v_mfma_f32_16x16x4_f32 on the fp32
// operands themselves, a wave per 16 rows x 16 queries -- as the query's candidate buffer in the emit-mode layout of the
// certified tile scan (score [nq][plen], idx [nq][plen], cnt [nq] = n), and k_merge_refine<true> selects on its staged copy,
// re-scores in float64 and certifies against eps(q) of the fp32 products (k_hi_rows, exact_ops).
struct DenseParams {
    const float* db = nullptr; const float* ynorm = nullptr; const float* q = nullptr; // fp32 store only
    int64_t n = 0;
    int nq = 0, dim = 0, l2 = 0;
    int plen = 0;               // row stride of score / idx: a multiple of 4, >= n
    float* score = nullptr; int* idx = nullptr; int* cnt = nullptr;
};
static_assert(std::is_trivially_copyable_v<DenseParams>, "kernel argument");

// <RT, QT>: 16-row x 16-query tiles per wave.  <1, 1> for the batches of <= 16 queries (one wave per 16 rows: parallel over the rows);
// <2, 4> otherwise: 32 rows x 64 queries per wave -- every operand a wave loads feeds 4 resp. 2 MFMAs (<1, 1> on 1024 queries x 4096
// centroids pulled 1 GB through the L2s for 4 GFLOP: 0.122 ms, the L2 bandwidth).
template <int RT, int QT>
__global__ __launch_bounds__(256) void k_knn_dense(DenseParams p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * (64 * RT) + wave * (16 * RT);
    const int q0 = blockIdx.y * (16 * QT);
    if (row0 >= p.plen) return;
    const float* pa[RT];
    const float* pb[QT];
#pragma unroll
    for (int r = 0; r < RT; ++r) pa[r] = p.db + min(row0 + 16 * r + r16, p.n - 1) * p.dim + 4 * g;
#pragma unroll
    for (int t = 0; t < QT; ++t) pb[t] = p.q + (int64_t)min(q0 + 16 * t + r16, p.nq - 1) * p.dim + 4 * g;
    constexpr int NA = RT * QT == 1 ? 2 : 1;           // accumulators per tile (one tile alone: two chains hide the MFMA latency)
    constexpr int KB = RT * QT == 1 ? 4 : 2;           // 16-element K blocks per panel; two panels in registers: the next one's loads
                                                       // are in flight while the current one's MFMAs issue
    f32x4 acc[RT][QT][NA];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int t = 0; t < QT; ++t)
#pragma unroll
            for (int c = 0; c < NA; ++c) acc[r][t][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nkb = p.dim >> 4;
    f32x4 a0[RT][KB], b0[QT][KB], a1[RT][KB], b1[QT][KB];
    auto load = [&](f32x4 (&a)[RT][KB], f32x4 (&b)[QT][KB], int kp) {
#pragma unroll
        for (int u = 0; u < KB; ++u) {
            const int kb = min(kp + u, nkb - 1);       // (a panel past the end re-reads the last block; its products are not used)
#pragma unroll
            for (int r = 0; r < RT; ++r) a[r][u] = *reinterpret_cast<const f32x4*>(pa[r] + kb * 16);
#pragma unroll
            for (int t = 0; t < QT; ++t) b[t][u] = *reinterpret_cast<const f32x4*>(pb[t] + kb * 16);
        }
    };
    auto mma = [&](const f32x4 (&a)[RT][KB], const f32x4 (&b)[QT][KB], int kp) {
#pragma unroll
        for (int u = 0; u < KB; ++u)
            if (kp + u < nkb) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < RT; ++r)
#pragma unroll
                        for (int t = 0; t < QT; ++t)
                            acc[r][t][u % NA] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r][u][j], b[t][u][j], acc[r][t][u % NA], 0, 0, 0);
            }
    };
    load(a0, b0, 0);
    for (int kp = 0; kp < nkb; kp += 2 * KB) {
        load(a1, b1, kp + KB);
        mma(a0, b0, kp);
        load(a0, b0, kp + 2 * KB);
        mma(a1, b1, kp + KB);
    }
    // acc[r][t][.][e]: row row0 + 16 r + 4 g + e, query q0 + 16 t + r16
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        const int qq = q0 + 16 * t + r16;
        if (qq >= p.nq) continue;
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const int64_t rb = row0 + 16 * r + 4 * g;
            f32x4 sc;
            int id[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t row = rb + e;
                float d = acc[r][t][0][e];
                if (NA == 2) d += acc[r][t][NA - 1][e];
                const bool on = row < p.n;
                sc[e] = on ? (p.l2 ? 2.f * d - p.ynorm[row] : d) : -INFINITY;
                id[e] = on ? (int)row : IDX_SENTINEL;
            }
            if (rb < p.plen) {
                *reinterpret_cast<f32x4*>(p.score + (int64_t)qq * p.plen + rb) = sc;
                *reinterpret_cast<int4*>(p.idx + (int64_t)qq * p.plen + rb) = make_int4(id[0], id[1], id[2], id[3]);
            }
        }
        if (blockIdx.x == 0 && wave == 0 && g == 0) p.cnt[qq] = (int)p.n;
    }
}

// ---- the same small-batch scan over the f16 plane (certified mode) -----------------------------------------------------
// Half the bytes: the hi plane of an fp32 store (or an fp16 store itself) is streamed instead of the fp32 rows, one
// v_mfma_f32_16x16x32_f16 per 32 elements of 16 rows against the f16-rounded queries in LDS.  The scores carry the error bound
// eps(q) of the certified scan (k_hi_rows), and k_merge_refine certifies or rejects every query exactly as it does for the
// tile kernel (complete top-(k + margin) lists per workgroup, no admission floor): the online search reads 1 GB instead of 2.
struct SmallQHiParams {
    const _Float16* db = nullptr;      // [n][dim] f16 rows
    const float* rscale = nullptr;     // [n] per-row scale, or nullptr: uscale for every row
    float uscale = 1.f;
    const float* rbias = nullptr;      // [n] per-row bias magnitude (|y'|^2 for L2, mu.y for a centred IP / cosine plane), or nullptr
    float bias_sign = 1.f, mult = 1.f; // score = mult a + bias_sign rbias[row] + qconst[query]   (knn_hi.inc, RSC 2)
    const float* qconst = nullptr;     // [nq] or nullptr
    const _Float16* q = nullptr;       // [nq][dim] f16 queries (scaled per query; centred when the plane is)
    const float* qscale = nullptr;     // [nq]
    int64_t n = 0;
    int nq = 0, dim = 0, k = 0;
    int rows_per_wave = 0;             // multiple of 16
    int n_parts = 0;                   // workgroups = lists per query
    float* part_score = nullptr; int* part_idx = nullptr; // [nq, n_parts, k]
};
static_assert(std::is_trivially_copyable_v<SmallQHiParams>, "kernel argument");

// (launch bounds: 155 VGPRs = 3 waves per SIMD for KSEL 16; forcing 4 (128 VGPRs) spills the 16-load panel: 0.41 instead of 0.21 ms)
template <int KSEL>
__global__ __launch_bounds__(SQ_THREADS, 2) void k_knn_hi_smallq(SmallQHiParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int qld = p.dim + 8;                                    // padded query row (halfs): 16-byte chunks of the 16 rows fall in distinct banks
    _Float16* sQ = reinterpret_cast<_Float16*>(smem);             // [nq][dim + 8]
    float2* sCand = reinterpret_cast<float2*>(sQ + p.nq * qld);   // [4 waves][16 q][SQ_SLOTS]
    int* sCnt = reinterpret_cast<int*>(sCand + 4 * SQ_NQ * 24);   // [4 waves][16]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    for (int i = tid; i < p.nq * (p.dim >> 3); i += SQ_THREADS) {
        const int qq = i / (p.dim >> 3), c8 = i % (p.dim >> 3);
        *reinterpret_cast<f16x8*>(sQ + qq * qld + c8 * 8) = *reinterpret_cast<const f16x8*>(p.q + (int64_t)qq * p.dim + c8 * 8);
    }
    if (tid < 4 * SQ_NQ) sCnt[tid] = 0;
    __syncthreads();

    const int part = blockIdx.x * 4 + wave;      // this wave's slice of the store
    const int64_t w_begin = (int64_t)part * p.rows_per_wave;
    const int64_t w_end = min(w_begin + p.rows_per_wave, p.n);
    float2* myCand = sCand + wave * SQ_NQ * SQ_SLOTS;
    int* myCnt = sCnt + wave * SQ_NQ;

    const u64 SENT = pack_key(-INFINITY, IDX_SENTINEL);
    u64 lst[KSEL];                       // meaningful in lanes 0..15 (lane = query)
#pragma unroll
    for (int j = 0; j < KSEL; ++j) lst[j] = SENT;
    float thr = -INFINITY;               // threshold of query (lane & 15), refreshed from the owner lane
    const float qs = r16 < p.nq ? p.qscale[r16] * p.mult : 0.f;
    const float qc = (r16 < p.nq && p.qconst) ? p.qconst[r16] : 0.f;
    // lane (r16, g) holds elements 32 kb + 8 g .. + 7 of row r16 (A) and of query r16 (B): one load instruction reads 64
    // contiguous bytes of each of its 16 rows, two consecutive ones a whole 128-byte line
    const _Float16* qrow = sQ + min(r16, p.nq - 1) * qld + 8 * g;   // columns >= nq repeat the last query (never admitted below)
    const int nkb = p.dim >> 5;

    for (int64_t row0 = w_begin; row0 < w_end; row0 += 16) {
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};       // even / odd K blocks: two MFMA chains
        const int64_t ra = min(row0 + r16, p.n - 1);                             // clamp: masked below
        const _Float16* pa = p.db + ra * p.dim + 8 * g;
        float rs[4], yn[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t row = min(row0 + 4 * g + e, p.n - 1);
            rs[e] = p.rscale ? p.rscale[row] : p.uscale;
            yn[e] = p.rbias ? p.bias_sign * p.rbias[row] + qc : qc;
        }
        constexpr int PKB = KSEL <= 16 ? 16 : 8;      // K blocks per panel (the 32-entry lists leave fewer registers)
        for (int kp = 0; kp < nkb; kp += PKB) {
            const int nb = min(PKB, nkb - kp);
            f16x8 v[PKB];
#pragma unroll
            for (int kb = 0; kb < PKB; ++kb)
                if (kb < nb) v[kb] = *reinterpret_cast<const f16x8*>(pa + (kp + kb) * 32);
#pragma unroll
            for (int kb = 0; kb < PKB; ++kb)
                if (kb < nb) {
                    const f16x8 b = *reinterpret_cast<const f16x8*>(qrow + (kp + kb) * 32);
                    if (kb & 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(v[kb], b, acc1, 0, 0, 0);
                    else acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(v[kb], b, acc0, 0, 0, 0);
                }
        }
        // acc0[e] + acc1[e]: row row0 + 4g + e, query r16
        bool any = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t row = row0 + 4 * g + e;
            const float sc = fmaf((acc0[e] + acc1[e]) * rs[e], qs, yn[e]);
            if (row < w_end && r16 < p.nq && sc >= thr) {
                const int sl = atomicAdd(&myCnt[r16], 1);          // < SQ_SLOTS by construction (4 x 4 lanes)
                myCand[r16 * SQ_SLOTS + sl] = make_float2(sc, __int_as_float((int)row));
                any = true;
            }
        }
        if (__any(any)) {                                              // wave-uniform; LDS ops of one wave are ordered
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
    // one list per WORKGROUP leaves the kernel: waves 1-3 hand their lists to wave 0 through the slot buffer
    __syncthreads();
    u64* sKeys = reinterpret_cast<u64*>(sCand);                     // [3][16][KSEL] (<= the slot buffer's 16 KB)
    if (wave > 0 && lane < SQ_NQ) {
#pragma unroll
        for (int j = 0; j < KSEL; ++j) sKeys[((wave - 1) * SQ_NQ + lane) * KSEL + j] = lst[j];
    }
    __syncthreads();
    if (wave == 0 && lane < p.nq) {
        for (int w = 0; w < 3; ++w)
            for (int j = 0; j < KSEL; ++j) list_insert<KSEL>(lst, sKeys[(w * SQ_NQ + lane) * KSEL + j]);
        float* ls = p.part_score + ((int64_t)lane * p.n_parts + blockIdx.x) * p.k;
        int* li = p.part_idx + ((int64_t)lane * p.n_parts + blockIdx.x) * p.k;
#pragma unroll
        for (int j = 0; j < KSEL; ++j)
            if (j < p.k) { ls[j] = key_score(lst[j]); li[j] = key_id(lst[j]); }
    }
}

// ---- the same stream as a threshold filter: the range search of a small batch (RADAD_RANGE_STREAM) -----------------------------------
// k_knn_hi_smallq's stream body -- queries in LDS, one wave per slice of rows_per_wave rows, 16 rows per step, two MFMA chains, the
// same scale / bias / query terms -- with nothing to select: a range search's floor is fixed per query (thr[q] = T - eps(q),
// k_range_floor), so there are no register lists, no slot buffer and no hand-over between waves.  A (row, query) pair whose score
// reaches the floor takes the next slot of the query's candidate buffer idx[q][cap] with one returning atomic on cnt[q]; the counter
// counts past cap (cnt > cap: overflow, k_range_refine sends the query to the exact range kernel) while nothing is written past it.
// Scores are not stored: k_range_refine re-scores every emitted row in float64 and reads nothing else of the scan.  A NaN score (the
// per-call bias of an excluded row) passes no compare, also against a floor of -inf.  The order of a query's entries depends on the
// order its atomics arrive in; the set does not, and the re-rank sorts.  LDS: the query block alone.
struct RangeSmallQParams : SmallQHiParams {       // (k, n_parts, part_score, part_idx: not read)
    const float* thr = nullptr;        // [nq] admission floors
    int* cnt = nullptr;                // [nq] rows emitted, zeroed before the launch
    int* idx = nullptr;                // [nq][cap] emitted rows
    int cap = 0;
};
static_assert(std::is_trivially_copyable_v<RangeSmallQParams>, "kernel argument");

__global__ __launch_bounds__(SQ_THREADS, 2) void k_range_hi_smallq(RangeSmallQParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int qld = p.dim + 8;                                    // padded query row (halfs), as k_knn_hi_smallq's
    _Float16* sQ = reinterpret_cast<_Float16*>(smem);             // [nq][dim + 8]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    for (int i = tid; i < p.nq * (p.dim >> 3); i += SQ_THREADS) {
        const int qq = i / (p.dim >> 3), c8 = i % (p.dim >> 3);
        *reinterpret_cast<f16x8*>(sQ + qq * qld + c8 * 8) = *reinterpret_cast<const f16x8*>(p.q + (int64_t)qq * p.dim + c8 * 8);
    }
    __syncthreads();

    const int part = blockIdx.x * 4 + wave;      // this wave's slice of the store (beyond the store: w_end <= w_begin, no step runs)
    const int64_t w_begin = (int64_t)part * p.rows_per_wave;
    const int64_t w_end = min(w_begin + p.rows_per_wave, p.n);

    const bool live = r16 < p.nq;                // columns >= nq repeat the last query and never emit
    const float thr = live ? p.thr[r16] : INFINITY;
    const float qs = live ? p.qscale[r16] * p.mult : 0.f;
    const float qc = (live && p.qconst) ? p.qconst[r16] : 0.f;
    const _Float16* qrow = sQ + min(r16, p.nq - 1) * qld + 8 * g;
    const int nkb = p.dim >> 5;
    int* my_cnt = p.cnt + min(r16, p.nq - 1);
    int* my_idx = p.idx + (int64_t)min(r16, p.nq - 1) * p.cap;

    for (int64_t row0 = w_begin; row0 < w_end; row0 += 16) {
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};       // even / odd K blocks: two MFMA chains
        const int64_t ra = min(row0 + r16, p.n - 1);                             // clamp: masked below
        const _Float16* pa = p.db + ra * p.dim + 8 * g;
        float rs[4], yn[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t row = min(row0 + 4 * g + e, p.n - 1);
            rs[e] = p.rscale ? p.rscale[row] : p.uscale;
            yn[e] = p.rbias ? p.bias_sign * p.rbias[row] + qc : qc;
        }
        constexpr int PKB = 16;                       // K blocks per panel
        for (int kp = 0; kp < nkb; kp += PKB) {
            const int nb = min(PKB, nkb - kp);
            f16x8 v[PKB];
#pragma unroll
            for (int kb = 0; kb < PKB; ++kb)
                if (kb < nb) v[kb] = *reinterpret_cast<const f16x8*>(pa + (kp + kb) * 32);
#pragma unroll
            for (int kb = 0; kb < PKB; ++kb)
                if (kb < nb) {
                    const f16x8 b = *reinterpret_cast<const f16x8*>(qrow + (kp + kb) * 32);
                    if (kb & 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(v[kb], b, acc1, 0, 0, 0);
                    else acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(v[kb], b, acc0, 0, 0, 0);
                }
        }
        // acc0[e] + acc1[e]: row row0 + 4g + e, query r16
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t row = row0 + 4 * g + e;
            const float sc = fmaf((acc0[e] + acc1[e]) * rs[e], qs, yn[e]);
            if (row < w_end && live && sc >= thr) {
                const int slot = atomicAdd(my_cnt, 1);
                if (slot < p.cap) my_idx[slot] = (int)row;           // (the counter stays below 2^31: a store holds fewer rows)
            }
        }
    }
}

// ---- the same streaming scan, K SPLIT over the four waves of a workgroup (small stores of wide rows) ---------------------------
// The reference's own online search is ONE query of dim 5376 against 25 423 rows (pipeline.py:1038-1054, config.py:48-56): 1 589
// 16-row steps in all.  With a wave per row slice that is at most 1 589 waves (6 per CU) each streaming 10.5 KB rows: too few loads
// in flight to cover the HBM latency (measured 2.0 TB/s).  Here the four waves of a workgroup take a quarter of the row's elements
// each for the SAME 16 rows, so every 16-row step keeps 4 waves busy (6 356 wave-steps over the store); their partial products
// meet in LDS, are added in a fixed order (deterministic) by wave 0, which also keeps the workgroup's top-k lists.
template <int KSEL>
__global__ __launch_bounds__(SQ_THREADS, KSEL <= 16 ? 3 : 2) void k_knn_hi_smallq_ksplit(SmallQHiParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int qld = p.dim + 8;
    _Float16* sQ = reinterpret_cast<_Float16*>(smem);             // [nq][dim + 8]
    float2* sCand = reinterpret_cast<float2*>(sQ + p.nq * qld);   // [16 q][SQ_SLOTS] (wave 0's)
    int* sCnt = reinterpret_cast<int*>(sCand + 4 * SQ_NQ * 24);   // [16]
    f32x4* sPart = reinterpret_cast<f32x4*>(sCand + SQ_NQ * SQ_SLOTS);   // [2 parities][3 waves][64 lanes]: partial sums of waves 1-3 (inside the slot area)

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    for (int i = tid; i < p.nq * (p.dim >> 3); i += SQ_THREADS) {
        const int qq = i / (p.dim >> 3), c8 = i % (p.dim >> 3);
        *reinterpret_cast<f16x8*>(sQ + qq * qld + c8 * 8) = *reinterpret_cast<const f16x8*>(p.q + (int64_t)qq * p.dim + c8 * 8);
    }
    if (tid < SQ_NQ) sCnt[tid] = 0;
    __syncthreads();

    const int64_t w_begin = (int64_t)blockIdx.x * p.rows_per_wave;      // (here: rows per WORKGROUP)
    const int64_t w_end = min(w_begin + p.rows_per_wave, p.n);
    const u64 SENT = pack_key(-INFINITY, IDX_SENTINEL);
    u64 lst[KSEL];                       // wave 0, lanes 0..15 (lane = query)
#pragma unroll
    for (int j = 0; j < KSEL; ++j) lst[j] = SENT;
    float thr = -INFINITY;
    const float qs = r16 < p.nq ? p.qscale[r16] * p.mult : 0.f;
    const float qc = (r16 < p.nq && p.qconst) ? p.qconst[r16] : 0.f;
    const int nkb = p.dim >> 5;
    const int kb0 = (nkb * wave) >> 2, kb1 = (nkb * (wave + 1)) >> 2;       // this wave's K blocks
    const _Float16* qrow = sQ + min(r16, p.nq - 1) * qld + 8 * g;
    int par = 0;
    for (int64_t row0 = w_begin; row0 < w_end; row0 += 16, par ^= 1) {
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        const int64_t ra = min(row0 + r16, p.n - 1);
        const _Float16* pa = p.db + ra * p.dim + 8 * g;
        constexpr int PKB = 16;
        for (int kp = kb0; kp < kb1; kp += PKB) {
            const int nb = min(PKB, kb1 - kp);
            f16x8 v[PKB];
#pragma unroll
            for (int kb = 0; kb < PKB; ++kb)
                if (kb < nb) v[kb] = *reinterpret_cast<const f16x8*>(pa + (kp + kb) * 32);
#pragma unroll
            for (int kb = 0; kb < PKB; ++kb)
                if (kb < nb) {
                    const f16x8 b = *reinterpret_cast<const f16x8*>(qrow + (kp + kb) * 32);
                    if (kb & 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(v[kb], b, acc1, 0, 0, 0);
                    else acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(v[kb], b, acc0, 0, 0, 0);
                }
        }
        f32x4 sum = acc0 + acc1;
        if (wave > 0) sPart[(par * 3 + wave - 1) * 64 + lane] = sum;
        __syncthreads();                 // (one barrier per step: the partial buffers alternate, so step t + 1's writes cannot
                                         // overtake wave 0's reads of step t)
        if (wave == 0) {
            sum = ((sum + sPart[(par * 3 + 0) * 64 + lane]) + sPart[(par * 3 + 1) * 64 + lane]) + sPart[(par * 3 + 2) * 64 + lane];
            bool any = false;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t row = row0 + 4 * g + e;
                const int64_t rc = min(row, p.n - 1);
                const float rs = p.rscale ? p.rscale[rc] : p.uscale;
                const float yn = p.rbias ? p.bias_sign * p.rbias[rc] + qc : qc;
                const float sc = fmaf(sum[e] * rs, qs, yn);
                if (row < w_end && r16 < p.nq && sc >= thr) {
                    const int sl = atomicAdd(&sCnt[r16], 1);
                    sCand[r16 * SQ_SLOTS + sl] = make_float2(sc, __int_as_float((int)row));
                    any = true;
                }
            }
            if (__any(any)) {
                if (lane < SQ_NQ) {
                    const int c = sCnt[lane];
                    for (int i = 0; i < c; ++i) {
                        const float2 cv = sCand[lane * SQ_SLOTS + i];
                        list_insert<KSEL>(lst, pack_key(cv.x, __float_as_int(cv.y)));
                    }
                    sCnt[lane] = 0;
                }
                thr = __shfl(key_score(lst[KSEL - 1]), r16, 64);
            }
        }
    }
    if (wave == 0 && lane < p.nq) {
        float* ls = p.part_score + ((int64_t)lane * p.n_parts + blockIdx.x) * p.k;
        int* li = p.part_idx + ((int64_t)lane * p.n_parts + blockIdx.x) * p.k;
#pragma unroll
        for (int j = 0; j < KSEL; ++j)
            if (j < p.k) { ls[j] = key_score(lst[j]); li[j] = key_id(lst[j]); }
    }
}

constexpr size_t knn_reg_lds_bytes() { return 4 * KD_TILE_BYTES + sizeof(float2) * KT_N * CAND_CAP + sizeof(float) * KT_N + sizeof(int) * KT_N + 16; }

// ---- merge of sorted partial lists -----------------------------------------------------------------------
// element j of partial list `part` of query q sits at [(q*n_parts + part)*part_len + j]; lists are sorted best-first by
// (score, -row) and padded with sentinels.  One wave per query; each lane walks the heads of lists lane, lane+64, ...
//
// k_merge_refine (inside radad_knn_search): the scan is a FILTER, this kernel decides.  With a = the scan's score and
//   eps(q) a bound on |a - exact score| (k_hi_rows), a_k the k-th best a over all lists:
//     * every row of the exact top-k has a >= tau = a_k - 2 eps   (the k rows with the best a have exact scores >= a_k - eps,
//       so the exact k-th score is >= a_k - eps, and a row that reaches it has a >= a_k - 2 eps);
//     * so all listed rows with a >= tau are RE-SCORED in float64 straight from the stored rows (L2 as sum (q-y)^2, no
//       cancellation) and ranked by (float64 distance, id);
//     * the result is CERTIFIED to be the exact float64 brute force when no unlisted row can have a >= tau: no list was
//       used up by the selection while full (its tail could hide such rows), the scan's admission floor thr_init is
//       <= tau (rows below the floor were never listed), the scan dropped nothing for this query (qflag), and the
//       candidate buffer (cap) sufficed.  Uncertified queries are appended to flag_sel for the exact kernel below.
//   eps == nullptr (IVF list scans): legacy behaviour -- the `cap` best candidates are re-scored, no certificate.
// k_merge_lists<KeyT> (radad_topk_merge / _f64): plain P-way merge of final per-shard lists, no rescoring.
// (KNN_MARGIN, KNN_CERT_EXTRA, KNN_CERT_CAP, KNN_F16_MAX_K, KW_SAMPLE_SPLITS, RF_STAGE_MAX, RF_STAGE_MAX_SMALLQ: knn_plan.h)
// (IVF_MAX_K: ivf_plan.h)


struct RefineParams {
    const float* score = nullptr;      // [nq, n_parts, part_len] fp32 scan scores (larger is better), each list sorted
    const int* idx = nullptr;          // [nq, n_parts, part_len] local row or IDX_SENTINEL
    int n_parts = 0, k = 0, dim = 0, l2 = 0;
    int part_len = 0;                  // entries per partial list
    int cap = 0;                       // candidates that can be re-scored per query (>= k)
    const float* eps = nullptr;        // [nq] error bound of the scan scores, or nullptr = legacy mode (exactly `cap` candidates)
    const float* thr_init = nullptr;   // optional [nq]: admission floor of the scan (rows below it were never listed)
    const int* qflag = nullptr;        // optional [nq]: the scan dropped a candidate of this query
    const int* part_cnt = nullptr;     // optional [nq] (emit-mode scan, n_parts == 1): entries filled in the query's buffer; > part_len = overflow
    const float* global_lb = nullptr;  // optional [nq] (sharded search): the best lower bound any shard has of the exact k-th best score
    const float* ak_in = nullptr;      // optional [nq] (emit-mode scan, two-half search): a_k as k_kth_floor found it for the bounds
    int* flag_count = nullptr;         // certified mode: [1] number of uncertified queries (atomicAdd) ...
    int* flag_sel = nullptr;           // ... and their indices, in arrival order
    int* stats = nullptr;              // optional [5]: sum of candidates re-scored, queries rejected for: buffer full / list used up /
                                       // floor above tau / dropped by the scan
    int64_t nq = 0;
    const void* db = nullptr;          // stored rows (normalised for cosine); fp16 when db_f16
    int db_f16 = 0;
    const float* q = nullptr;          // the fp32 queries (normalised for cosine)
    const int64_t* id_map = nullptr;   // optional: reported id = id_map[row] (IVF: list-sorted position -> insertion id), ties by it
    int64_t id_base = 0;
    float* out_dist = nullptr;         // [nq, k]
    int64_t* out_idx = nullptr;        // [nq, k]
    double* out_key = nullptr;         // optional [nq, k] float64 distances
    int debug = 0;                     // timing experiments only (-DRADAD_DEBUG_HOOKS, RADAD_DEBUG_KNN): 128 no statistics atomics, 256 no re-score, 512 no ranking, 1024 no fp32 funnel
    int* qflag_out = nullptr;          // optional [nq] (certified mode): the certificate's verdict per query, 0 = certified (no caller left: IVF reads flag_sel)
    const int* only_flagged = nullptr; // optional [nq]: workgroups of queries whose entry is 0 leave at once (no caller left: see k_ivf_exact)
};
static_assert(std::is_trivially_copyable_v<RefineParams>, "kernel argument");

// One workgroup (256 threads) per query: thread t looks after lists t, t + 256, ... (<= RF_MAXL of them); the k rounds
// are block-wide arg-max reductions over cached list heads (only the winning list re-reads its head), the walk to tau and
// the append are parallel over the lists, the float64 re-score runs 16 candidates per pass (16 lanes each, all loads of a
// pass in flight), the ranking is one thread per candidate.
constexpr int RF_THREADS = 256;
constexpr int RF_MAXL = 4;               // lists per thread: n_parts <= 1024

// (refine_lds_bytes: knn_plan.h)

// STAGED (certified mode, n_parts * part_len <= RF_STAGE_MAX): all of the query's list entries are first copied to LDS in ONE
// round of independent loads, and the k selection rounds, the gathering of everything >= tau and the used-up test run on that
// copy.  The unstaged form walks the lists in global memory: every round's winner re-reads its list head and every list is
// walked entry by entry, i.e. 30-50 DEPENDENT trips to L2/HBM per query -- 0.17 ms for 1024 queries that re-score 150 rows
// each, where the re-scoring itself needs a tenth of that.
// The k-th largest of the NE scores staged in LDS (e_sc; -inf = "no entry", the smallest key), by a 4-pass radix select on the
// order-preserving image of the float bits.  Only the VALUE is found.  Called by all NT (>= 256 = the bins) threads of the
// block; hist [256] and xchg [2] are LDS scratch; e_sc needs no barrier of its own (the first pass's publishes it; so does the
// early exit).  Returns -inf when NE < k.
template <int NT = 256>
__device__ __forceinline__ float radix_select_kth(const float* e_sc, int NE, int k, int* hist, int* xchg) {
    static_assert(NT >= 256 && NT % 64 == 0, "one thread per bin at least");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    auto okey = [](float v) { const unsigned u = __float_as_uint(v); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); };
    unsigned prefix = 0, pmask = 0;
    int krem = k;
    const bool have_k = NE >= k;                                         // (block-uniform)
    for (int shift = 24; shift >= 0 && have_k; shift -= 8) {
        if (NT == 256 || tid < 256) hist[tid] = 0;                       // 256 bins
        __syncthreads();                                                 // (first pass: also publishes e_sc)
        for (int i = tid; i < NE; i += NT) {
            const unsigned key = okey(e_sc[i]);
            if ((key & pmask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
        }
        __syncthreads();
        if (wave == 0) {                                                 // the digit that holds the krem-th largest matching key
            int c[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) c[j] = hist[4 * lane + j];
            const int s4 = c[0] + c[1] + c[2] + c[3];
            int incl = s4;                                               // matching keys in this lane's bins and all higher ones
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_down(incl, o, 64);
                if (lane + o < 64) incl += t;
            }
            int above = incl - s4;
            if (above < krem && krem <= incl) {                          // exactly one lane
#pragma unroll
                for (int j = 3; j >= 0; --j) {
                    if (above + c[j] >= krem) { xchg[0] = 4 * lane + j; xchg[1] = krem - above; break; }
                    above += c[j];
                }
            }
        }
        __syncthreads();
        prefix |= (unsigned)xchg[0] << shift;
        pmask |= 255u << shift;
        krem = xchg[1];
    }
    if (!have_k) { __syncthreads(); return -INFINITY; }                  // publishes e_sc all the same
    const unsigned u = (prefix & 0x80000000u) ? (prefix & 0x7fffffffu) : ~prefix;
    return __uint_as_float(u);
}

// k_kth_floor: between the two phases of the certified tile scan (and, for a sharded search, after it).  One workgroup per query:
// a_k = the k-th best score among the candidates emitted so far (-inf when there are fewer than k, or the buffer overflowed).
//   floor_io  (optional) [nq]: raised to a_k - 2 eps -- a score k rows are KNOWN to reach, lowered by the scan's error on both
//             sides: every row of the exact top-k scores at least that, so the rest of the store is scanned with it;
//   lb_out    (optional) [nq][k]: the k best scan scores, each lowered by eps -- lower bounds of the exact scores of k DIFFERENT rows
//             of this store (unordered; -inf where there are fewer).  Shards exchange them: the k-th largest of all shards' values
//             is a lower bound of the exact k-th best score of the whole store.
struct KthParams {
    const float* score = nullptr; // [nq][cap]
    const int* cnt = nullptr;     // [nq]
    int cap = 0, k = 0;
    const float* eps = nullptr;   // [nq]
    float* floor_io = nullptr;
    float* lb_out = nullptr;
    float* ak_out = nullptr;      // optional [nq]: a_k itself (the re-rank of a two-half search takes it instead of selecting again)
};
static_assert(std::is_trivially_copyable_v<KthParams>, "kernel argument");
__global__ __launch_bounds__(RF_THREADS) void k_kth_floor(KthParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem_k[];
    float* e_sc = reinterpret_cast<float*>(smem_k);                      // [cap]
    int* hist = reinterpret_cast<int*>(e_sc + p.cap);                    // [256]
    int* xchg = hist + 256;
    const int64_t q = blockIdx.x;
    const int c = p.cnt[q];
    const int NE = c <= p.cap ? c : 0;                                   // an overflowed buffer proves nothing (its query is rejected)
    for (int i = threadIdx.x; i < NE; i += RF_THREADS) e_sc[i] = p.score[q * p.cap + i];
    const float a_k = radix_select_kth(e_sc, NE, p.k, hist, xchg);
    const float e = p.eps[q];
    if (threadIdx.x == 0 && p.ak_out) p.ak_out[q] = a_k;
    if (threadIdx.x == 0 && p.floor_io && a_k > -INFINITY) p.floor_io[q] = fmaxf(p.floor_io[q], a_k - 2.f * e);
    if (p.lb_out) {
        float* out = p.lb_out + q * p.k;
        if (!(a_k > -INFINITY)) {
            for (int j = threadIdx.x; j < p.k; j += RF_THREADS) out[j] = -INFINITY;
            return;                                                          // (block-uniform)
        }
        if (threadIdx.x == 0) xchg[0] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < NE; i += RF_THREADS)                   // fewer than k entries are above the k-th best
            if (e_sc[i] > a_k) { const int pos = atomicAdd(&xchg[0], 1); if (pos < p.k) out[pos] = e_sc[i] - e; }
        __syncthreads();
        for (int j = min(xchg[0], p.k) + threadIdx.x; j < p.k; j += RF_THREADS) out[j] = a_k - e;
    }
}

// the scan's first admission floor: the rank-th best of the sample pre-pass's entries (n_ent per query, unsorted; a sentinel
// index = no entry), lowered by 2 eps -- a_k over the WHOLE store is >= the rank-th best of any subset for rank >= k, so the
// floor is <= tau = a_k - 2 eps always.  -inf when the sample holds fewer entries.  One workgroup per query (k_thr_from_parts, its
// predecessor, walked the 512 list heads `rank` times with a wave: 19 us against 6).
__global__ __launch_bounds__(RF_THREADS) void k_floor_from_sample(const float* __restrict__ score, const int* __restrict__ idx, int n_ent, int rank,
                                                                 const float* __restrict__ eps, float* __restrict__ thr) {
    extern __shared__ __attribute__((aligned(16))) char smem_f[];
    float* e_sc = reinterpret_cast<float*>(smem_f);                      // [n_ent]
    int* hist = reinterpret_cast<int*>(e_sc + n_ent);                    // [256]
    int* xchg = hist + 256;
    const int64_t q = blockIdx.x;
    for (int i = threadIdx.x; i < n_ent; i += RF_THREADS)
        e_sc[i] = idx[q * n_ent + i] != IDX_SENTINEL ? score[q * n_ent + i] : -INFINITY;
    const float a = radix_select_kth(e_sc, n_ent, rank, hist, xchg);
    if (threadIdx.x == 0) thr[q] = a > -INFINITY ? a - 2.f * eps[q] : -INFINITY;
}

// (A one-wave-per-query form -- the <= 1024 sample entries in 16 registers per lane, the rank by a 32-step binary search on the keys with
// ballot counts, no LDS -- was built in round 5 and measured at 15.0 us against this kernel's 11.6 for 1024 queries: one wave walks
// its dependent chain of loads and 32 search steps alone, where this one puts four waves on a query.  Removed.)

// The float64 re-score of k_merge_refine and k_range_refine: the candidates c_id[0, nsel) of one query (LDS, rows of the store) -> c_key.
// 16 lanes per candidate, 32 candidates per pass (two per 16-lane group), all row loads of a pass issued before the first multiply
// (the stored rows are random 2 KB reads: latency-bound unless many are in flight).  L2 as sum (q - y)^2: no cancellation.  Called by all
// RF_THREADS threads; a candidate's key depends on its row and the query alone, not on its place in c_id.
// EXACT_ORDER (the stream route of a range search, k_range_refine<.., true>): the key is k_exact_scan_any's bit for bit, so that a
// batch of <= 16 queries gets the same float64 keys whether RADAD_KNN_OPT_RANGE_SMALLQ sends it to the stream or to the exact route.
// That kernel gives chunk c (4 elements) of a row to lane c % 64, adds a lane's products in ascending c (L2: subtracts the squares),
// folds lanes l and l ^ 32, then ^ 16, ^ 8 ... and negates an L2 sum at the end.  Here lane l16 of a candidate's 16 keeps four partial
// sums -- those of lanes l16, l16 + 16, l16 + 32, l16 + 48 there: chunk u * 16 + l16 of a sweep belongs to partial u % 4 -- and folds
// them (0 + 2) + (1 + 3) before the 16-lane fold both forms share.  The plain form is the code it was.
// (tests/test_gpu_knn_range_smallq.py compares the two routes' keys bit for bit at dim 64, 128 and 576, inner product and L2: a
// change of either kernel's sums shows there.)
template <bool EXACT_ORDER = false>
__device__ __forceinline__ void refine_rescore_f64(const void* db, int db_f16, const float* qrow, int dim, int l2, const int* c_id,
                                                   double* c_key, int nsel) {
    const int tid = threadIdx.x, sub = tid >> 4, l16 = tid & 15;
    for (int c0 = 0; c0 < nsel; c0 += 32) {
        int cc[2];
        bool on[2];
        int64_t rid[2];
        double acc[2] = {0.0, 0.0};
        double part[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};       // (EXACT_ORDER)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            cc[h] = c0 + 16 * h + sub;
            on[h] = cc[h] < nsel;
            rid[h] = on[h] ? (int64_t)c_id[cc[h]] : 0;
        }
        for (int i0 = 0; i0 < dim; i0 += 512) {                 // 16 lanes x 8 x 4 elements per sweep
            f32x4 b[2][8];
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int i = i0 + (u * 16 + l16) * 4;
                    b[h][u] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (on[h] && i < dim) {
                        if (db_f16) {
                            const f16x4 h4 = *reinterpret_cast<const f16x4*>(reinterpret_cast<const _Float16*>(db) + rid[h] * dim + i);
                            b[h][u] = f32x4{(float)h4[0], (float)h4[1], (float)h4[2], (float)h4[3]};
                        } else {
                            b[h][u] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(db) + rid[h] * dim + i);
                        }
                    }
                }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + (u * 16 + l16) * 4;
                if (i < dim) {
                    const f32x4 a = *reinterpret_cast<const f32x4*>(qrow + i);
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            if constexpr (EXACT_ORDER) {
                                // (the roundings of that kernel as compiled: the first element of a chunk joins the sum fused,
                                // the other three as a rounded product -- stated here, not left to the contraction of this loop)
#pragma clang fp contract(off)
                                const double x = (double)a[e], y = (double)b[h][u][e], d = x - y;
                                if (e == 0) part[h][u & 3] = l2 ? __builtin_fma(-d, d, part[h][u & 3]) : __builtin_fma(x, y, part[h][u & 3]);
                                else { const double t = l2 ? d * -d : x * y; part[h][u & 3] = part[h][u & 3] + t; }
                            } else {
                                if (l2) { const double d = (double)a[e] - (double)b[h][u][e]; acc[h] += d * d; }
                                else acc[h] += (double)a[e] * (double)b[h][u][e];
                            }
                        }
                }
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if constexpr (EXACT_ORDER) acc[h] = (part[h][0] + part[h][2]) + (part[h][1] + part[h][3]);
#pragma unroll
            for (int ofs = 8; ofs > 0; ofs >>= 1) acc[h] += __shfl_xor(acc[h], ofs, 64);
            if (on[h] && l16 == 0) c_key[cc[h]] = (EXACT_ORDER && l2) ? -acc[h] : acc[h];
        }
    }
}

template <bool STAGED>
__global__ __launch_bounds__(RF_THREADS) void k_merge_refine(RefineParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem_m[];
    double* c_key = reinterpret_cast<double*>(smem_m);                   // [cap] float64 distance of a candidate
    int64_t* c_gid = reinterpret_cast<int64_t*>(c_key + p.cap);          // [cap] its reported id (before id_base)
    int* c_id = reinterpret_cast<int*>(c_gid + p.cap);                   // [cap] its local row
    float* w_sc = reinterpret_cast<float*>(c_id + p.cap);                // [2][4] per-wave winners of a round (double-buffered)
    int* w_id = reinterpret_cast<int*>(w_sc + 8);                        // [2][4]
    int* w_pt = w_id + 8;                                                // [2][4]
    int* w_cnt = w_pt + 8;                                               // [4] per-wave counts of the append
    float* e_sc = reinterpret_cast<float*>(smem_m + refine_lds_bytes(p.cap));      // STAGED: [n_parts * part_len] scores ...
    int* e_id = reinterpret_cast<int*>(e_sc + (STAGED ? p.n_parts * p.part_len : 0));   // ... and rows; then the radix select's 256 bins
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q = blockIdx.x;
    if (p.only_flagged && !p.only_flagged[q]) return;                     // (workgroup-uniform)
    const bool cert = p.eps != nullptr;
    const float two_eps = cert ? 2.f * p.eps[q] : 0.f;
    const int64_t qbase = q * p.n_parts;
    float tau = -INFINITY;
    int nsel = 0;
    int why = 0;                             // bit 0: candidate buffer full, 1: a full list used up, 2: admission floor above tau, 3: dropped
    const float floor_q = (cert && p.thr_init) ? p.thr_init[q] : -INFINITY;     // (read here: off the dependent chain below)
    const int dropped_q = (cert && p.qflag) ? p.qflag[q] : 0;

  if constexpr (STAGED) {
    // (emit-mode scan: ONE unsorted buffer of part_len entries per query, of which part_cnt[q] are filled -- more means overflow)
    const int filled = p.part_cnt ? p.part_cnt[q] : 0;
    const int NE = p.part_cnt ? min(filled, p.part_len) : p.n_parts * p.part_len;
    const int64_t ebase = qbase * p.part_len;
    int* hist = e_id + p.n_parts * p.part_len;                           // [256] digit histogram of the radix select
    for (int i = tid; i < NE; i += RF_THREADS) {
        const int id = p.idx[ebase + i];
        const float sc = p.score[ebase + i];
        e_id[i] = id;
        e_sc[i] = id != IDX_SENTINEL ? sc : -INFINITY;
    }
    // a_k = the k-th largest scan score (radix_select_kth: only the VALUE is needed -- every entry >= tau = a_k - 2 eps is re-scored,
    // the k best among them; the first version found the k best one by one, k rounds of a block-wide arg-max with two barriers
    // each: 40 % of this kernel)
    {
        float a_k;
        if (p.ak_in) { a_k = p.ak_in[q]; __syncthreads(); }             // (the barrier publishes e_sc, as the select's would)
        else a_k = radix_select_kth(e_sc, NE, p.k, hist, w_pt);
        if (a_k > -INFINITY) tau = a_k - two_eps;                        // (fewer than k listed rows: tau stays -inf, all of them go on)
    }
    // (Round 5, measured and reverted: halving the band.  tau = a_k - 2 eps pays eps twice; scoring the <= 32 rows with a >= a_k in fp32
    // first gives L = the k-th largest of their s - e, a lower bound of the exact k-th best, and only rows with a + eps >= L can be
    // among the exact k best.  On the benchmark's store that cut the re-scored rows from 151 to 105 per query -- and the kernel went
    // from 73 to 79 us: one more dependent stage per workgroup costs more than the 30 % of row reads it saves; this kernel is bound
    // by its chain of dependent round trips, not by bytes.)
    // sharded search: no row whose score is below (the best lower bound any shard has of the exact k-th best) - eps can be in the
    // GLOBAL top-k, whatever this shard's own k-th best is -- the re-rank takes only what can still matter
    if (cert && p.global_lb) tau = fmaxf(tau, p.global_lb[q] - 0.5f * two_eps);
    // everything >= tau goes on to the re-score; the used-up test: a FULL list whose last (= smallest) entry is >= tau
    int cnt = 0, used_up = 0;
    for (int i = tid; i < NE; i += RF_THREADS) cnt += (e_id[i] != IDX_SENTINEL && e_sc[i] >= tau) ? 1 : 0;
    if (p.part_cnt) used_up = filled > p.part_len ? 1 : 0;             // the scan emitted more than the buffer holds
    else
        for (int l = tid; l < p.n_parts; l += RF_THREADS) {
            const int last = l * p.part_len + p.part_len - 1;
            if (e_id[last] != IDX_SENTINEL && e_sc[last] >= tau) used_up = 1;
        }
    int incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) w_cnt[wave] = incl;
    used_up = __syncthreads_or(used_up);
    int base_slot = incl - cnt, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { if (w < wave) base_slot += w_cnt[w]; total += w_cnt[w]; }
    if (cnt > 0)
        for (int i = tid; i < NE; i += RF_THREADS) {
            const int id = e_id[i];
            if (id != IDX_SENTINEL && e_sc[i] >= tau) {
                if (base_slot < p.cap) c_id[base_slot] = id;
                ++base_slot;
            }
        }
    nsel = total;
    if (nsel > p.cap) { nsel = p.cap; why |= 1; }
    if (used_up) why |= 2;
  } else {

    // cached heads of this thread's lists
    int pos[RF_MAXL];
    float hsc[RF_MAXL];
    int hid[RF_MAXL];
    auto fetch = [&](int part, int at, float& sc, int& id) {
        id = IDX_SENTINEL; sc = -INFINITY;
        if (part < p.n_parts && at < p.part_len) {
            const int64_t off = (qbase + part) * p.part_len + at;
            id = p.idx[off];
            if (id != IDX_SENTINEL) sc = p.score[off];
        }
    };
#pragma unroll
    for (int i = 0; i < RF_MAXL; ++i) { pos[i] = 0; fetch(tid + RF_THREADS * i, 0, hsc[i], hid[i]); }

    // 1) the k best by scan score (legacy mode: `cap` of them, and that is all): fixes a_k and tau = a_k - 2 eps
    const int rounds = cert ? min(p.k, p.cap) : p.cap;
    for (int o = 0; o < rounds; ++o) {
        float bs = -INFINITY;
        int bi = IDX_SENTINEL, bp = -1;
#pragma unroll
        for (int i = 0; i < RF_MAXL; ++i)
            if (hid[i] != IDX_SENTINEL && (bp < 0 || hsc[i] > bs || (hsc[i] == bs && hid[i] < bi))) { bs = hsc[i]; bi = hid[i]; bp = tid + RF_THREADS * i; }
#pragma unroll
        for (int ofs = 32; ofs > 0; ofs >>= 1) {
            const float os = __shfl_xor(bs, ofs, 64);
            const int oi = __shfl_xor(bi, ofs, 64);
            const int op = __shfl_xor(bp, ofs, 64);
            if (op >= 0 && (bp < 0 || os > bs || (os == bs && oi < bi))) { bs = os; bi = oi; bp = op; }
        }
        const int slot = (o & 1) * 4;
        if (lane == 0) { w_sc[slot + wave] = bs; w_id[slot + wave] = bi; w_pt[slot + wave] = bp; }
        __syncthreads();
        bs = w_sc[slot]; bi = w_id[slot]; bp = w_pt[slot];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const float os = w_sc[slot + w];
            const int oi = w_id[slot + w], op = w_pt[slot + w];
            if (op >= 0 && (bp < 0 || os > bs || (os == bs && oi < bi))) { bs = os; bi = oi; bp = op; }
        }
        if (bp < 0) break;                                   // every list exhausted (block-uniform)
        if ((bp & (RF_THREADS - 1)) == tid) {
#pragma unroll
            for (int i = 0; i < RF_MAXL; ++i)
                if (bp == tid + RF_THREADS * i) { pos[i] += 1; fetch(bp, pos[i], hsc[i], hid[i]); }
        }
        if (tid == 0) c_id[nsel] = bi;
        ++nsel;
        if (cert && nsel == p.k) tau = bs - two_eps;
    }
    if (cert && p.global_lb && nsel == p.k) tau = fmaxf(tau, p.global_lb[q] - 0.5f * two_eps);     // (sharded search: see the staged form)
    if (cert) {
        int cnt = 0, used_up = 0;
        int endp[RF_MAXL];
#pragma unroll
        for (int i = 0; i < RF_MAXL; ++i) {
            const int part = tid + RF_THREADS * i;
            int e = pos[i];
            if (nsel == p.k && part < p.n_parts) {           // walk on while the entries are >= tau (sorted lists)
                const int64_t lb = (qbase + part) * p.part_len;
                while (e < p.part_len) {
                    const int id = p.idx[lb + e];
                    if (id == IDX_SENTINEL || p.score[lb + e] < tau) break;
                    ++e;
                }
            }
            endp[i] = e;
            cnt += e - pos[i];
            // a full list whose entries are ALL >= tau may hide more such rows; everything else a list hides is below its
            // first entry < tau (or, for a list that never filled up, below the admission floor)
            if (part < p.n_parts && e >= p.part_len && p.idx[(qbase + part) * p.part_len + p.part_len - 1] != IDX_SENTINEL) used_up = 1;
        }
        // slots by a prefix sum over the block (lists in thread order)
        int incl = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        if (lane == 63) w_cnt[wave] = incl;
        used_up = __syncthreads_or(used_up);
        int base_slot = nsel + incl - cnt, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { if (w < wave) base_slot += w_cnt[w]; total += w_cnt[w]; }
#pragma unroll
        for (int i = 0; i < RF_MAXL; ++i) {
            const int part = tid + RF_THREADS * i;
            const int n_i = endp[i] - pos[i];
            if (n_i > 0) {
                const int64_t lb = (qbase + part) * p.part_len;
                for (int j = 0; j < n_i; ++j)
                    if (base_slot + j < p.cap) c_id[base_slot + j] = p.idx[lb + pos[i] + j];
                base_slot += n_i;
            }
        }
        nsel += total;
        if (nsel > p.cap) { nsel = p.cap; why |= 1; }
        if (used_up) why |= 2;
    }
  }
    if (cert) {
        // rows below the floor are unlisted: the floor must not exceed tau (tau = -inf when fewer than k rows are listed, unless a
        // global bound set it)
        if (floor_q > -INFINITY && !(floor_q <= tau)) why |= 4;
        if (dropped_q) why |= 8;
        if (tid == 0) {
            if (why) p.flag_sel[atomicAdd(p.flag_count, 1)] = (int)q;
            if (p.qflag_out) p.qflag_out[q] = why;
            if (p.stats && !RADAD_DBG(p.debug, 128)) {
                atomicAdd(&p.stats[0], nsel);
                for (int b2 = 0; b2 < 4; ++b2) if (why & (1 << b2)) atomicAdd(&p.stats[1 + b2], 1);
            }
        }
    }
    __syncthreads();                         // c_id complete
    // 1b) fp32 funnel (certified mode, more candidates than results): every candidate is scored ONCE in fp32 -- s = q.y, or
    //     (2q - y).y = |q|^2 - |q - y|^2 for L2 -- together with e = gamma sum |products|, a rigorous bound on that sum's
    //     rounding error (every term passes through at most dim/16 + 4 fused accumulations; gamma has slack for the
    //     accumulation of e itself and for forming s -+ e).  A candidate with at least k others CERTAINLY above it
    //     (s_j - e_j > s_c + e_c) cannot be among the exact k best and is dropped; only the survivors -- k plus the few within
    //     ~1e-6 of the k-th -- go through the float64 re-score and the ranking, whose cost is linear resp. quadratic in the
    //     count (with 150 candidates per query they were two thirds of this kernel).
    //     (a handful beyond k -- the fp32 scans' candidates, the IVF index's coarse step -- go straight to float64: the funnel's pass over
    //     their rows costs what it saves)
    if (cert && nsel > p.k + 16 && !RADAD_DBG(p.debug, 1024)) {
        float2* f_lh = reinterpret_cast<float2*>(c_key);                 // (s - e, s + e) per candidate; c_key is free until 2)
        int* tmp_id = reinterpret_cast<int*>(c_gid);                     // survivors' rows; c_gid is free until 3)
        const float gamma = (float)(p.dim / 16 + 8) * 5.9604645e-08f * 1.01f;
        const float* qrow = p.q + q * p.dim;
        const int sub = tid >> 4, l16 = tid & 15;
        for (int c0 = 0; c0 < nsel; c0 += 32) {
            int cc[2];
            bool on[2];
            int64_t rid[2];
            float sdot[2] = {0.f, 0.f}, sabs[2] = {0.f, 0.f};
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                cc[h] = c0 + 16 * h + sub;
                on[h] = cc[h] < nsel;
                rid[h] = on[h] ? (int64_t)c_id[cc[h]] : 0;
            }
            for (int i0 = 0; i0 < p.dim; i0 += 512) {
                f32x4 b[2][8];
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int i = i0 + (u * 16 + l16) * 4;
                        b[h][u] = f32x4{0.f, 0.f, 0.f, 0.f};
                        if (on[h] && i < p.dim) {
                            if (p.db_f16) {
                                const f16x4 h4 = *reinterpret_cast<const f16x4*>(reinterpret_cast<const _Float16*>(p.db) + rid[h] * p.dim + i);
                                b[h][u] = f32x4{(float)h4[0], (float)h4[1], (float)h4[2], (float)h4[3]};
                            } else {
                                b[h][u] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(p.db) + rid[h] * p.dim + i);
                            }
                        }
                    }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int i = i0 + (u * 16 + l16) * 4;
                    if (i < p.dim) {
                        const f32x4 a = *reinterpret_cast<const f32x4*>(qrow + i);
#pragma unroll
                        for (int h = 0; h < 2; ++h)
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const float y = b[h][u][e];
                                const float x = p.l2 ? 2.f * a[e] - y : a[e];      // (one more rounding per term for L2: inside gamma's slack)
                                sdot[h] = fmaf(x, y, sdot[h]);
                                sabs[h] = fmaf(fabsf(x), fabsf(y), sabs[h]);
                            }
                    }
                }
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int ofs = 8; ofs > 0; ofs >>= 1) {
                    sdot[h] += __shfl_xor(sdot[h], ofs, 64);
                    sabs[h] += __shfl_xor(sabs[h], ofs, 64);
                }
                if (on[h] && l16 == 0) {
                    const float e = gamma * sabs[h] + 4.8e-7f * fabsf(sdot[h]);      // + 4 ulp for forming s -+ e
                    f_lh[cc[h]] = make_float2(sdot[h] - e, sdot[h] + e);
                }
            }
        }
        __syncthreads();
        // survivors: fewer than k candidates certainly above (T threads per candidate share the count)
        const int T = nsel <= 64 ? 4 : (nsel <= 128 ? 2 : 1);
        const int part = tid & (T - 1);
        int n_keep = 0;                                                  // survivors so far (block-uniform)
        for (int c0 = 0; c0 < nsel; c0 += RF_THREADS / T) {
            const int c = c0 + tid / T;
            const bool onc = c < nsel;
            const float hi_c = onc ? f_lh[c].y : 0.f;
            int above = 0;
            for (int j = part; j < nsel; j += T) above += (int)(f_lh[j].x > hi_c);
            if (T >= 2) above += __shfl_xor(above, 1, 64);
            if (T == 4) above += __shfl_xor(above, 2, 64);
            const bool keep = onc && part == 0 && !(above >= p.k);       // (NaN scores compare false everywhere: kept)
            const unsigned long long m = __ballot(keep);
            if (lane == 0) w_cnt[wave] = __popcll(m);
            __syncthreads();
            int base = n_keep, total = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) { if (w < wave) base += w_cnt[w]; total += w_cnt[w]; }
            if (keep) tmp_id[base + __popcll(m & ((1ull << lane) - 1ull))] = c_id[c];
            n_keep += total;
            __syncthreads();
        }
        for (int c = tid; c < n_keep; c += RF_THREADS) c_id[c] = tmp_id[c];
        nsel = n_keep;
        __syncthreads();
    }
    // 2) float64 re-score (refine_rescore_f64)
    refine_rescore_f64(p.db, p.db_f16, p.q + q * p.dim, p.dim, p.l2, c_id, c_key, RADAD_DBG(p.debug, 256) ? 0 : nsel);
    __syncthreads();
    // 3) rank by (distance, id): L2 ascending, IP descending; ids are unique so ranks are a permutation.  Rank = number of
    //    candidates that come first, counted branch-free over "larger is better" keys by 1, 2 or 4 threads per candidate
    //    (the first version -- one thread per candidate, short-circuit compares, the id map looked up inside the loop --
    //    was a third of this kernel's time)
    const int nrank = RADAD_DBG(p.debug, 512) ? 0 : nsel;
    for (int c = tid; c < nrank; c += RF_THREADS) {
        c_gid[c] = p.id_map ? p.id_map[c_id[c]] : (int64_t)c_id[c];
        double kc = p.l2 ? -c_key[c] : c_key[c];
        // a NaN key (non-finite query or row) compares false with everything: several candidates would take the same rank and
        // leave output slots unwritten.  It ranks last instead, among its kind by id: the order stays total.
        if (kc != kc) kc = -(double)INFINITY;
        c_key[c] = kc;
    }
    __syncthreads();
    {
        const int T = nrank <= 64 ? 4 : (nrank <= 128 ? 2 : 1);
        const int part = tid & (T - 1);
        for (int c0 = 0; c0 < nrank; c0 += RF_THREADS / T) {
            const int c = c0 + tid / T;
            const bool onc = c < nrank;
            const double kc = onc ? c_key[c] : 0.0;
            const int64_t ic = onc ? c_gid[c] : 0;
            int rank = 0;
            for (int j = part; j < nrank; j += T) {
                const double kj = c_key[j];
                const int64_t ij = c_gid[j];
                rank += (int)((kj > kc) | ((kj == kc) & (ij < ic)));
            }
            if (T >= 2) rank += __shfl_xor(rank, 1, 64);
            if (T == 4) rank += __shfl_xor(rank, 2, 64);
            if (onc && part == 0 && rank < p.k) {
                const double kd = p.l2 ? -kc : kc;
                p.out_dist[q * p.k + rank] = (float)kd;
                p.out_idx[q * p.k + rank] = ic + p.id_base;
                if (p.out_key) p.out_key[q * p.k + rank] = kd;
            }
        }
    }
    for (int o = nsel + tid; o < p.k; o += RF_THREADS) {   // faiss fills what it cannot find with -1 / +-inf
        p.out_dist[q * p.k + o] = p.l2 ? INFINITY : -INFINITY;
        p.out_idx[q * p.k + o] = -1;
        if (p.out_key) p.out_key[q * p.k + o] = p.l2 ? (double)INFINITY : -(double)INFINITY;
    }
}

// ---- the re-rank of a range search (radad_knn_range_search, tile route) ------------------------------------------------------------
// The scan ran with the floor T - eps(q) (k_range_floor), so a query's candidate buffer holds EVERY row whose exact score reaches T
// unless it overflowed.  One workgroup per query:
//   * cnt > cap: the buffer proves nothing -- the query is appended to flag_sel for the exact range pass, its count zeroed for it;
//   * else ALL cnt emitted rows (holes skipped) are re-scored in float64 from the stored rows (refine_rescore_f64: the keys of
//     radad_knn_search_f64, bit for bit), the strict test decides membership (L2: key < radius, IP / cosine: key > radius; a NaN key
//     passes neither), out_count = the number that pass;
//   * the passing rows are ranked by (key, lower row) with a bitonic sort over the next power of two >= cnt entries in LDS (rows that
//     fail and the padding carry the worst key and the largest row: they sort last), and the best min(count, m) are written;
//     the other slots get -1 / NaN / NaN.
// LDS: 12 bytes per buffer entry (float64 key + row), 48 KB at the 4096 entries the range plan runs with.
constexpr int RG_MAX_CAP = 4096;         // entries the sort is sized for (a power of two)
struct RangeRefineParams {
    const int* idx = nullptr;           // [nq][cap] rows the scan emitted, IDX_SENTINEL = no entry
    const int* cnt = nullptr;           // [nq] entries emitted (> cap: overflow)
    int cap = 0, dim = 0, l2 = 0, db_f16 = 0, m = 0;
    const void* db = nullptr;           // stored rows (normalised for cosine)
    const float* q = nullptr;           // the fp32 queries (normalised for cosine)
    double radius = 0.0;
    int64_t id_base = 0, ntotal = 0;
    int* flag_count = nullptr;          // [1] queries left to the exact range pass ...
    int* flag_sel = nullptr;            // ... and their indices
    int* out_count = nullptr;           // [nq]
    float* out_dist = nullptr;          // [nq, m]
    int64_t* out_idx = nullptr;         // [nq, m]
    double* out_key = nullptr;          // optional [nq, m]
};
static_assert(std::is_trivially_copyable_v<RangeRefineParams>, "kernel argument");
constexpr size_t range_refine_lds_bytes() { return (size_t)RG_MAX_CAP * 12 + 64; }
// PER_QUERY (k_range_refine<true>, radad_knn_range_search_excl_pq): the scan emitted a query's excluded rows like any others; the
// query's live tags are staged in LDS (as k_excl_pq_scrub does) and both passes of the compaction below treat an emitted row whose tag
// is among them as one more hole -- such a row is never re-scored, never counted, never sorted.  Overflow is decided on the emitted
// count, excluded rows included.  The plain instantiation takes RangeRefineParams and is the code it was.
struct RangeRefinePqParams : RangeRefineParams {
    const int64_t* tags = nullptr;      // [ntotal] row tags
    const int64_t* q_tags = nullptr;    // [nq, n_tags]
    const int* q_cnt = nullptr;         // [nq] or NULL = n_tags for every query (clamped to [0, n_tags] here)
    int n_tags = 0;
};
static_assert(std::is_trivially_copyable_v<RangeRefinePqParams>, "kernel argument");
constexpr size_t range_refine_pq_lds_bytes() { return range_refine_lds_bytes() + (size_t)RADAD_EXCL_PQ_MAX_TAGS * sizeof(int64_t); }
static_assert(range_refine_lds_bytes() % 8 == 0, "the tags behind the plain form's LDS are 8-byte entries");

// EXACT_ORDER (k_range_refine<.., true>, the stream route): refine_rescore_f64<true>, the exact range kernel's keys bit for bit.
template <bool PER_QUERY = false, bool EXACT_ORDER = false>
__global__ __launch_bounds__(RF_THREADS) void k_range_refine(std::conditional_t<PER_QUERY, RangeRefinePqParams, RangeRefineParams> p) {
    extern __shared__ __attribute__((aligned(16))) char smem_g[];
    double* c_key = reinterpret_cast<double*>(smem_g);                   // [RG_MAX_CAP]
    int* c_id = reinterpret_cast<int*>(c_key + RG_MAX_CAP);              // [RG_MAX_CAP]
    int* w_cnt = c_id + RG_MAX_CAP;                                      // [4]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q = blockIdx.x;
    const int filled = p.cnt[q];
    if (filled > p.cap) {                                                // (workgroup-uniform)
        if (tid == 0) { p.flag_sel[atomicAdd(p.flag_count, 1)] = (int)q; p.out_count[q] = 0; }
        return;
    }
    // the emitted rows, holes and rows outside the store left out (slots by a prefix sum over the block, as k_merge_refine's)
    const int NE = max(filled, 0);
    const int* ebuf = p.idx + q * p.cap;
    int64_t* s_tag = reinterpret_cast<int64_t*>(smem_g + range_refine_lds_bytes());     // (PER_QUERY) [RADAD_EXCL_PQ_MAX_TAGS], behind the plain form's LDS
    int n_tag = 0;
    if constexpr (PER_QUERY) {
        n_tag = min(max(p.q_cnt ? p.q_cnt[q] : p.n_tags, 0), min(p.n_tags, RADAD_EXCL_PQ_MAX_TAGS));
        if (tid < n_tag) s_tag[tid] = p.q_tags[q * p.n_tags + tid];
        __syncthreads();
    }
    // an entry the re-score takes: a row of the store that (PER_QUERY) the query does not exclude
    auto taken = [&](int id) -> bool {
        if (id == IDX_SENTINEL || id < 0 || id >= p.ntotal) return false;
        if constexpr (PER_QUERY) {
            if (n_tag > 0) {
                const int64_t t = p.tags[id];
                bool excluded = false;
                for (int e = 0; e < n_tag; ++e) excluded |= s_tag[e] == t;
                return !excluded;
            }
        }
        return true;
    };
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
    refine_rescore_f64<EXACT_ORDER>(p.db, p.db_f16, p.q + q * p.dim, p.dim, p.l2, c_id, c_key, nsel);
    __syncthreads();
    // membership, and "larger is better" keys for the ranking
    int P = 1;
    while (P < nsel) P <<= 1;                                            // <= RG_MAX_CAP: nsel <= cap <= RG_MAX_CAP (the host checks)
    int n_pass = 0;
    for (int i0 = 0; i0 < P; i0 += RF_THREADS) {
        const int i = i0 + tid;
        bool pass = false;
        if (i < nsel) {
            const double key = c_key[i];
            pass = p.l2 ? key < p.radius : key > p.radius;
            c_key[i] = pass ? (p.l2 ? -key : key) : -(double)INFINITY;
            if (!pass) c_id[i] = IDX_SENTINEL;
        } else if (i < P) {
            c_key[i] = -(double)INFINITY;
            c_id[i] = IDX_SENTINEL;
        }
        n_pass += __syncthreads_count(pass);
    }
    // (a passing key is never the worst key: -inf passes no strict test, +inf squared distance neither -- the n_pass best entries are
    // exactly the passing rows)
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
        const double kd = have ? (p.l2 ? -c_key[o] : c_key[o]) : (double)nan_f;
        p.out_dist[q * p.m + o] = have ? (float)kd : nan_f;
        p.out_idx[q * p.m + o] = have ? (int64_t)c_id[o] + p.id_base : -1;
        if (p.out_key) p.out_key[q * p.m + o] = kd;
    }
}

// the admission floor of a range search: thr[q] = T - eps[q], lowered two more ulps (the subtraction rounds to nearest: one ulp makes
// it a lower bound of T - eps, the second covers the rounding of the scan's own compare (thr - qc) qs); T = -inf stays -inf.  A query
// whose eps is not a number >= 0 (non-finite operands) gets -inf: its buffer overflows and the exact pass answers it.
__global__ __launch_bounds__(256) void k_range_floor(const float* __restrict__ eps, float T, float* __restrict__ thr, int64_t nq) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    const float e = eps[i];
    float f = -INFINITY;
    if (e >= 0.f && e < INFINITY) f = nextafterf(nextafterf(T - e, -INFINITY), -INFINITY);
    thr[i] = f;
}

// ---- the re-rank of a SMALL batch (<= 16 queries: the online predict() search, pipeline.py:1038-1054) -------------------------
// k_merge_refine is one 256-thread workgroup per query: with one query that is ONE workgroup walking 500-800 partial lists (the
// streaming kernels write one per workgroup) and re-scoring its candidates 16 lanes at a time -- 0.123 ms of the reference's own
// search (25 423 x 5376, k 15), twice its scan; 45 us on the 1 M x 512 store.  Where the time went: the radix select's LDS-atomic
// histogram over all 16 K staged entries (~30 us), then 11 dependent sweeps of row loads per re-score pass, twice (fp32 funnel,
// float64).  This form:
//   * RS_SPLIT workgroups of 1024 threads per query, thread t <-> partial list t (<= RS_MAX_PARTS lists, sorted best-first);
//   * tau from the list HEADS only: h_k = the k-th largest head is a lower bound of a_k (k different lists reach it), so
//     tau = h_k - 2 eps admits every row the certificate needs (knn.hip: k_merge_refine's header) -- and, the store being split
//     over hundreds of lists, hardly any more (h_k = a_k unless two of the k best rows share a list);
//   * the lists are walked while their entries are >= tau (sorted: usually 0 or 1 step), slots by a block prefix sum -- every
//     workgroup of the query computes the same candidate list;
//   * float64 re-score of ALL candidates (no fp32 funnel: there are few), one WAVE per candidate with the row's loads of a sweep
//     (4096 elements) in flight together, the candidates dealt round-robin to the RS_SPLIT x 16 waves of the query;
//   * the keys meet in global memory; the workgroup that arrives last (device-scope counter, as k_exact_scan's slices) ranks
//     them, writes the result and the certificate's verdict.
constexpr int RS_THREADS = 1024;
constexpr int RS_WAVES = RS_THREADS / 64;
constexpr int RS_SPLIT = 8;
constexpr int RS_MAX_PARTS = RS_THREADS;
constexpr int RS_MAX_CAP = KNN_CERT_CAP + 128;     // candidates per query (rs_key's rows); larger caps take k_merge_refine
constexpr size_t refine_small_lds_bytes(int cap) { return (size_t)cap * 20 + (size_t)RS_MAX_PARTS * 4 + 256 * 4 + 256; }

__global__ __launch_bounds__(RS_THREADS) void k_refine_small(RefineParams p, double* __restrict__ wkey, int* __restrict__ wcount) {
    extern __shared__ __attribute__((aligned(16))) char smem_s[];
    double* c_key = reinterpret_cast<double*>(smem_s);                   // [cap]
    int64_t* c_gid = reinterpret_cast<int64_t*>(c_key + p.cap);          // [cap]
    int* c_id = reinterpret_cast<int*>(c_gid + p.cap);                   // [cap]
    float* heads = reinterpret_cast<float*>(c_id + p.cap);               // [RS_MAX_PARTS]
    int* hist = reinterpret_cast<int*>(heads + RS_MAX_PARTS);            // [256]
    int* xch = hist + 256;                                               // [2] select, [16] wave counts, [1] arrival
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = blockIdx.x;
    const int64_t q = blockIdx.y;
    const float two_eps = 2.f * p.eps[q];
    const float floor_q = p.thr_init ? p.thr_init[q] : -INFINITY;
    const int dropped_q = p.qflag ? p.qflag[q] : 0;
    const int64_t lb = (q * p.n_parts + tid) * p.part_len;               // this thread's list
    const bool have = tid < p.n_parts;

    int hid = IDX_SENTINEL;
    float hs = -INFINITY;
    if (have) { hid = p.idx[lb]; const float s0 = p.score[lb]; if (hid != IDX_SENTINEL) hs = s0; }
    heads[tid] = hs;
    const float h_k = radix_select_kth<RS_THREADS>(heads, p.n_parts, p.k, hist, xch);
    float tau = h_k > -INFINITY ? h_k - two_eps : -INFINITY;             // (fewer than k lists: everything listed goes on)
    if (p.global_lb) tau = fmaxf(tau, p.global_lb[q] - 0.5f * two_eps);  // (sharded search: see k_merge_refine)
    int cnt = 0, used_up = 0;
    if (have && hid != IDX_SENTINEL && hs >= tau) {
        cnt = 1;
        while (cnt < p.part_len) {
            const int id = p.idx[lb + cnt];
            if (id == IDX_SENTINEL || !(p.score[lb + cnt] >= tau)) break;
            ++cnt;
        }
        if (cnt == p.part_len) used_up = 1;                              // a FULL list of entries >= tau may hide more such rows
    }
    int incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) xch[2 + wave] = incl;
    used_up = __syncthreads_or(used_up);
    int base_slot = incl - cnt, total = 0;
#pragma unroll
    for (int w = 0; w < RS_WAVES; ++w) { const int c = xch[2 + w]; if (w < wave) base_slot += c; total += c; }
    for (int j = 0; j < cnt; ++j)
        if (base_slot + j < p.cap) c_id[base_slot + j] = j == 0 ? hid : p.idx[lb + j];
    int nsel = total, why = 0;
    if (nsel > p.cap) { nsel = p.cap; why |= 1; }
    if (used_up) why |= 2;
    if (floor_q > -INFINITY && !(floor_q <= tau)) why |= 4;
    if (dropped_q) why |= 8;
    __syncthreads();                                                     // c_id complete

    // float64 re-score: wave (r, wave) takes candidates r * 16 + wave, + RS_SPLIT * 16, ...
    {
        const float* qrow = p.q + q * p.dim;
        for (int c = r * RS_WAVES + wave; c < nsel; c += RS_SPLIT * RS_WAVES) {
            const int64_t rid = (int64_t)c_id[c];
            double acc = 0.0;
            for (int i0 = 0; i0 < p.dim; i0 += 4096) {                   // 64 lanes x 16 x 4 elements per sweep
                f32x4 b[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    const int i = i0 + (u * 64 + lane) * 4;
                    b[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (i < p.dim) {
                        if (p.db_f16) {
                            const f16x4 h4 = *reinterpret_cast<const f16x4*>(reinterpret_cast<const _Float16*>(p.db) + rid * p.dim + i);
                            b[u] = f32x4{(float)h4[0], (float)h4[1], (float)h4[2], (float)h4[3]};
                        } else {
                            b[u] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(p.db) + rid * p.dim + i);
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    const int i = i0 + (u * 64 + lane) * 4;
                    if (i < p.dim) {
                        const f32x4 a = *reinterpret_cast<const f32x4*>(qrow + i);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            if (p.l2) { const double d = (double)a[e] - (double)b[u][e]; acc += d * d; }
                            else acc += (double)a[e] * (double)b[u][e];
                        }
                    }
                }
            }
#pragma unroll
            for (int ofs = 32; ofs > 0; ofs >>= 1) acc += __shfl_xor(acc, ofs, 64);
            if (lane == 0) wkey[q * p.cap + c] = acc;
        }
    }
    __threadfence();                                     // release: this workgroup's keys are visible device-wide before the counter moves
    __syncthreads();
    if (tid == 0) {
        const int old = atomicAdd(&wcount[q], 1);
        xch[18] = old == RS_SPLIT - 1;
        if (old == RS_SPLIT - 1) wcount[q] = 0;          // ready for the next search
    }
    __syncthreads();
    if (!xch[18]) return;                                // (workgroup-uniform)
    __threadfence();                                     // acquire
    if (tid == 0) {
        if (why) p.flag_sel[atomicAdd(p.flag_count, 1)] = (int)q;
        if (p.stats) {
            atomicAdd(&p.stats[0], nsel);
            for (int b2 = 0; b2 < 4; ++b2) if (why & (1 << b2)) atomicAdd(&p.stats[1 + b2], 1);
        }
    }
    // rank by (distance, id), as k_merge_refine's step 3
    for (int c = tid; c < nsel; c += RS_THREADS) {
        c_gid[c] = p.id_map ? p.id_map[c_id[c]] : (int64_t)c_id[c];
        double kc = __builtin_nontemporal_load(&wkey[q * p.cap + c]);
        if (p.l2) kc = -kc;
        if (kc != kc) kc = -(double)INFINITY;            // a NaN key ranks last, among its kind by id
        c_key[c] = kc;
    }
    __syncthreads();
    {
        const int T = nsel <= 256 ? 4 : 2;               // (nsel <= cap <= 512)
        const int part = tid & (T - 1);
        for (int c0 = 0; c0 < nsel; c0 += RS_THREADS / T) {
            const int c = c0 + tid / T;
            const bool onc = c < nsel;
            const double kc = onc ? c_key[c] : 0.0;
            const int64_t ic = onc ? c_gid[c] : 0;
            int rank = 0;
            for (int j = part; j < nsel; j += T) {
                const double kj = c_key[j];
                const int64_t ij = c_gid[j];
                rank += (int)((kj > kc) | ((kj == kc) & (ij < ic)));
            }
            rank += __shfl_xor(rank, 1, 64);
            if (T == 4) rank += __shfl_xor(rank, 2, 64);
            if (onc && part == 0 && rank < p.k) {
                const double kd = p.l2 ? -kc : kc;
                p.out_dist[q * p.k + rank] = (float)kd;
                p.out_idx[q * p.k + rank] = ic + p.id_base;
                if (p.out_key) p.out_key[q * p.k + rank] = kd;
            }
        }
    }
    for (int o = nsel + tid; o < p.k; o += RS_THREADS) {   // faiss fills what it cannot find with -1 / +-inf
        p.out_dist[q * p.k + o] = p.l2 ? INFINITY : -INFINITY;
        p.out_idx[q * p.k + o] = -1;
        if (p.out_key) p.out_key[q * p.k + o] = p.l2 ? (double)INFINITY : -(double)INFINITY;
    }
}

// ---- exact float64 search of the queries the certificate rejected --------------------------------------------------
// Driven entirely from the device: the number of queries (*count) and their indices (sel) were written by
// k_merge_refine; the launch geometry is fixed, workgroups with nothing to do leave at once.  One launch takes the rejected
// queries sel[slot0 .. slot0 + nslots) (the partial lists of nslots queries are what the workspace holds; larger batches at large
// k take several launches, knn_exact_slots).  Slice s of the store
// (n_slices row ranges) is scanned by workgroups (s, y); workgroup (s, y) takes the query groups y, y + gridDim.y, ...
// of `group` (<= 8) queries each.  A wave reads one row per step (coalesced), every lane multiplies its elements with
// the group's queries from LDS in float64, a butterfly sum leaves the (row, query) scores in all lanes; each wave keeps
// its exact top-k per query as a sorted LDS list (wave-cooperative insertion), the workgroup merges its waves' lists
// and writes one list per (query slot, slice); the slice that arrives last for a query group merges the slices (exact_merge_slot)
// and overwrites the queries' results.
// Keys are "larger is better" doubles (inner product, or minus the squared distance); order (key desc, id asc).
// (KX_THREADS, KX_WAVES, KX_SLICES, KX_LDS_MAX, KX_PART_BUDGET and the grouping knn_exact_group / knn_exact_slots: knn_plan.h)
constexpr int KX_GROUPS_Y = 4;

struct ExactParams {
    const void* db = nullptr; int db_f16 = 0;
    const float* q = nullptr;  // [nq][dim] fp32 queries (normalised for cosine)
    const int* sel = nullptr;  // [*count] query indices
    const int* count = nullptr;
    int64_t n = 0; int dim = 0, k = 0, l2 = 0, group = 1;
    int64_t slice_rows = 0;
    int slot0 = 0, nslots = 0; // this launch's rejected queries: sel[slot0 ..], at most nslots of them
    double* pkey = nullptr;    // [nslots][KX_SLICES][k]
    int* pidx = nullptr;
    int64_t id_base = 0;
    float* out_dist = nullptr; int64_t* out_idx = nullptr; double* out_key = nullptr;
    int* host_stats = nullptr; // pinned host memory (device-visible): the kernel leaves the search's 6 counters and its batch size ([7]) there, then ...
    int stamp = 0;             // ... this value in host_stats[6] (the search's sequence number + 1): the host reads a report only when its stamp is there
    int nq_report = 0;         // the search's batch size (travels with the report: the host may be many searches ahead when it reads it)
    int* arrive = nullptr;     // [query groups] arrival counters of the slices (zero between launches: the last arrival resets its own)
    // the row-filtered instantiation only (k_exact_scan_excl, radad_knn_search_excl): bit (row & 63) of admit[row >> 6] set = the row
    // takes part; unfilled result slots are -1 / NaN there (the padding of radad_filter_topk) instead of -1 / +-inf
    const unsigned long long* admit = nullptr;
    // the per-query instantiation only (k_exact_scan_excl_pq, radad_knn_search_excl_pq): no bitmap; row r takes part for query j iff
    // row_tags[r] is not among the first clamp(q_cnt[j], 0, m) entries of q_tags[j, :] (q_cnt NULL = m for every query); 1 <= m <= 64
    const int64_t* row_tags = nullptr;
    const int64_t* q_tags = nullptr;
    const int* q_cnt = nullptr;
    int m = 0;
    // the range instantiations only (k_exact_scan_range, radad_knn_range_search; with `admit` or the tags above: k_exact_scan_range_excl
    // / _range_excl_pq, among the rows the query admits): a row enters a query's list only when its key passes the strict test
    // key > range_t (inner product: the radius; L2: minus the radius, the keys here being minus the squared distance), and every row
    // that passes is counted into out_count[query] (zeroed by the caller); padding -1 / NaN / NaN
    int* out_count = nullptr;
    double range_t = 0.0;
};
static_assert(std::is_trivially_copyable_v<ExactParams>, "kernel argument");

__device__ __forceinline__ bool kx_better(double ka, int ia, double kb, int ib) { return ka > kb || (ka == kb && ia < ib); }
// the LDS reads and writes of one wave on either side stay on their side (lanes read entries that other lanes then overwrite)
__device__ __forceinline__ void kx_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <bool FILTERED>
__device__ __forceinline__ void exact_merge_slot(const ExactParams& p, int slot, int lane);

// FILTERED is a compile-time parameter: the unfiltered instantiation (k_exact_scan) is the code it was before the filter existed;
// k_exact_scan_excl scans the rows a bitmap admits (radad_knn_search_excl): the float64 brute force among the rows not excluded.
// PER_QUERY (with FILTERED, k_exact_scan_excl_pq, radad_knn_search_excl_pq): every query of a group has an admissible set of its
// own, <= 64 excluded tags each.  Lane l holds tag l of each of the group's queries; per row one load of the row's tag and one
// ballot per query say which of the group's lists the row may enter.  A row nobody of the group admits is not loaded.
// RANGE (alone, k_exact_scan_range, radad_knn_range_search): every row is read; the strict threshold test stands in front of the list
// insertion, and each wave counts the rows that pass per query of its group -- one atomicAdd per wave, slice and query into
// out_count.  The lists, the slice merge and the last-arrival merge are the other forms', with k = max_per_query.
// RANGE with FILTERED (k_exact_scan_range_excl / _excl_pq, radad_knn_range_search_excl / _excl_pq): the strict test, the count and the
// insertion happen only for the queries that admit the row -- the bitmap bit (the row is skipped before it is loaded, as in the
// filtered form), or bit j of adm_q (a row nobody of the group admits is not loaded either).  An excluded row is never counted.
template <bool FILTERED, bool PER_QUERY = false, bool RANGE = false>
__global__ __launch_bounds__(KX_THREADS) void k_exact_scan_any(ExactParams p) {
    static_assert(FILTERED || !PER_QUERY, "the per-query form is a filtered form");
    const int count = min(*p.count - p.slot0, p.nslots);       // this launch's queries
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && p.host_stats) {
        *reinterpret_cast<volatile int*>(&p.host_stats[6]) = 0;          // the slot is being rewritten: no report until the new stamp is there
        __threadfence_system();
        for (int i = 0; i < 6; ++i) p.host_stats[i] = p.count[i];       // count + 5 statistics
        p.host_stats[7] = p.nq_report;
        __threadfence_system();
        *reinterpret_cast<volatile int*>(&p.host_stats[6]) = p.stamp;
    }
    if (count <= 0) return;
    __shared__ int s_last;
    extern __shared__ __attribute__((aligned(16))) char smem_x[];
    const int G = p.group;
    float* sQ = reinterpret_cast<float*>(smem_x);                                   // [G][dim]
    double* sKey = reinterpret_cast<double*>(smem_x + (size_t)G * p.dim * 4);       // [KX_WAVES][G][k]
    int* sId = reinterpret_cast<int*>(sKey + (size_t)KX_WAVES * G * p.k);           // [KX_WAVES][G][k]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r_begin = (int64_t)blockIdx.x * p.slice_rows;
    const int64_t r_end = min(r_begin + p.slice_rows, p.n);
    const int n_groups = (count + G - 1) / G;
    const int nv = p.dim >> 2;
    for (int g = blockIdx.y; g < n_groups; g += gridDim.y) {
        const int ng = min(G, count - g * G);
        __syncthreads();
        for (int i = tid; i < ng * nv; i += KX_THREADS) {
            const int qq = i / nv, c4 = i % nv;
            reinterpret_cast<f32x4*>(sQ + (size_t)qq * p.dim)[c4] =
                reinterpret_cast<const f32x4*>(p.q + (int64_t)p.sel[p.slot0 + g * G + qq] * p.dim)[c4];
        }
        double* wKey = sKey + (size_t)wave * G * p.k;
        int* wId = sId + (size_t)wave * G * p.k;
        for (int i = lane; i < G * p.k; i += 64) { wKey[i] = -INFINITY; wId[i] = IDX_SENTINEL; }
        int64_t qt[8];                                    // (PER_QUERY) tag `lane` of the group's query j ...
        bool qv[8];                                       // ... and whether the query's clamped count reaches it
        if constexpr (PER_QUERY) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                qt[j] = 0; qv[j] = false;
                if (j < ng) {
                    const int64_t qq = p.sel[p.slot0 + g * G + j];
                    const int cnt = min(max(p.q_cnt ? p.q_cnt[qq] : p.m, 0), p.m);
                    qv[j] = lane < cnt;
                    if (qv[j]) qt[j] = p.q_tags[qq * p.m + lane];
                }
            }
        }
        __syncthreads();
        int n_in[8];                                      // (RANGE) rows of this wave that passed the threshold, per query of the group
        if constexpr (RANGE) {
#pragma unroll
            for (int j = 0; j < 8; ++j) n_in[j] = 0;
        }
        int64_t adm_w = -1;                               // (FILTERED) the bitmap word in hand: one load per 64 rows of the slice
        unsigned long long adm = 0ull;
        for (int64_t row = r_begin + wave; row < r_end; row += KX_WAVES) {
            if (FILTERED && !PER_QUERY) {
                // wave-uniform, before any load of the row: an excluded row costs this bit and nothing else
                if ((row >> 6) != adm_w) { adm_w = row >> 6; adm = p.admit[adm_w]; }
                if (!__builtin_amdgcn_readfirstlane((int)((adm >> (row & 63)) & 1ull))) continue;
            }
            unsigned adm_q = 0u;                          // (PER_QUERY) bit j: query j of the group admits the row (wave-uniform)
            if constexpr (PER_QUERY) {
                const int64_t t = p.row_tags[row];        // one address for the wave
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (j < ng && __ballot(qv[j] && qt[j] == t) == 0ull) adm_q |= 1u << j;
                if (adm_q == 0u) continue;                // before any load of the row
            }
            double part[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) part[j] = 0.0;
            for (int i = lane; i < nv; i += 64) {
                f32x4 y;
                if (p.db_f16) {
                    const f16x4 h4 = reinterpret_cast<const f16x4*>(reinterpret_cast<const _Float16*>(p.db) + row * p.dim)[i];
                    y = f32x4{(float)h4[0], (float)h4[1], (float)h4[2], (float)h4[3]};
                } else {
                    y = reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(p.db) + row * p.dim)[i];
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    if (j < ng) {
                        const f32x4 x = reinterpret_cast<const f32x4*>(sQ + (size_t)j * p.dim)[i];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            if (p.l2) { const double d = (double)x[e] - (double)y[e]; part[j] -= d * d; }
                            else part[j] += (double)x[e] * (double)y[e];
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (j < ng && (!PER_QUERY || ((adm_q >> j) & 1u))) {
                    double v = part[j];
#pragma unroll
                    for (int ofs = 32; ofs > 0; ofs >>= 1) v += __shfl_xor(v, ofs, 64);
                    // wave-uniform from here: insert (v, row) into the sorted list of query j when it beats the k-th entry
                    double* lk = wKey + (size_t)j * p.k;
                    int* li = wId + (size_t)j * p.k;
                    bool within = true;                      // (RANGE) strict, before the insertion; a NaN key passes nothing
                    if constexpr (RANGE) { within = v > p.range_t; n_in[j] += within ? 1 : 0; }
                    if (within && kx_better(v, (int)row, lk[p.k - 1], li[p.k - 1])) {
                        // strips of 64 entries (lane l <-> entry 64 s + l), the LAST strip first: a strip reads its entries, counts
                        // the better ones and moves the others one place down -- onto the next strip's first entry, which that
                        // strip has already read.  The better entries are a prefix of the sorted list: a strip of nothing but
                        // better entries ends the walk (all strips before it are better too).
                        int pos = 0;
                        for (int s0 = (p.k - 1) & ~63; s0 >= 0; s0 -= 64) {
                            const int e = s0 + lane;
                            double ek = -INFINITY;
                            int ei = IDX_SENTINEL;
                            if (e < p.k) { ek = lk[e]; ei = li[e]; }
                            const bool b = e < p.k && kx_better(ek, ei, v, (int)row);
                            const int nb = __popcll(__ballot(b));
                            kx_wave_sync();                          // every lane has read its entry before any moves one down
                            if (e < p.k && !b && e + 1 < p.k) { lk[e + 1] = ek; li[e + 1] = ei; }
                            kx_wave_sync();
                            pos += nb;
                            if (nb == 64) { pos += s0; break; }      // (wave-uniform)
                        }
                        if (lane == (pos & 63)) { lk[pos] = v; li[pos] = (int)row; }
                    }
                }
            }
        }
        if constexpr (RANGE) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < ng && lane == 0 && n_in[j] > 0) atomicAdd(p.out_count + p.sel[p.slot0 + g * G + j], n_in[j]);
        }
        __syncthreads();
        // wave j merges the KX_WAVES lists of query j (lane 0, serial: k * 8 comparisons) into the slice's partial list
        if (wave < ng && lane == 0) {
            int pos[KX_WAVES];
#pragma unroll
            for (int w = 0; w < KX_WAVES; ++w) pos[w] = 0;
            const int64_t ob = ((int64_t)(g * G + wave) * KX_SLICES + blockIdx.x) * p.k;       // (slot local to the launch)
            for (int o = 0; o < p.k; ++o) {
                double bk = -INFINITY; int bi = IDX_SENTINEL, bw = -1;
#pragma unroll
                for (int w = 0; w < KX_WAVES; ++w) {
                    if (pos[w] < p.k) {
                        const double kk = sKey[((size_t)w * G + wave) * p.k + pos[w]];
                        const int ii = sId[((size_t)w * G + wave) * p.k + pos[w]];
                        if (ii != IDX_SENTINEL && (bw < 0 || kx_better(kk, ii, bk, bi))) { bk = kk; bi = ii; bw = w; }
                    }
                }
                p.pkey[ob + o] = bw < 0 ? -INFINITY : bk;
                p.pidx[ob + o] = bw < 0 ? IDX_SENTINEL : bi;
                if (bw >= 0) {
#pragma unroll
                    for (int w = 0; w < KX_WAVES; ++w) if (w == bw) ++pos[w];
                }
            }
        }
        // the slice that arrives LAST for this query group merges the group's KX_SLICES partial lists (it used to be a second launch --
        // and the usual search, with nothing rejected, paid two empty launches and the gap between them)
        __threadfence();                                 // release: this slice's lists are visible device-wide before the counter moves
        __syncthreads();
        if (tid == 0) {
            const int old = atomicAdd(&p.arrive[g], 1);
            s_last = old == KX_SLICES - 1;
            if (s_last) p.arrive[g] = 0;                 // ready for the next launch
        }
        __syncthreads();
        if (s_last) {                                    // (workgroup-uniform)
            __threadfence();                             // acquire
            if (wave < ng) exact_merge_slot<FILTERED || RANGE>(p, g * G + wave, lane);
        }
    }
}

constexpr auto k_exact_scan = k_exact_scan_any<false>;
constexpr auto k_exact_scan_excl = k_exact_scan_any<true>;
constexpr auto k_exact_scan_excl_pq = k_exact_scan_any<true, true>;
constexpr auto k_exact_scan_range = k_exact_scan_any<false, false, true>;
constexpr auto k_exact_scan_range_excl = k_exact_scan_any<true, false, true>;
constexpr auto k_exact_scan_range_excl_pq = k_exact_scan_any<true, true, true>;

// one wave: merge the KX_SLICES partial lists of this launch's rejected-query slot `slot`, overwrite the query's output rows
template <bool FILTERED>
__device__ __forceinline__ void exact_merge_slot(const ExactParams& p, int slot, int lane) {
    static_assert(KX_SLICES == 64, "one list per lane");
    {
    const int64_t q = p.sel[p.slot0 + slot];
    const double* lk = p.pkey + ((int64_t)slot * KX_SLICES + lane) * p.k;
    const int* li = p.pidx + ((int64_t)slot * KX_SLICES + lane) * p.k;
    int pos = 0;
    for (int o = 0; o < p.k; ++o) {
        double hk = -INFINITY; int hi = IDX_SENTINEL;
        if (pos < p.k) { hk = lk[pos]; hi = li[pos]; }
        double bk = hk; int bi = hi;
#pragma unroll
        for (int ofs = 32; ofs > 0; ofs >>= 1) {
            const double ok = __shfl_xor(bk, ofs, 64);
            const int oi = __shfl_xor(bi, ofs, 64);
            if (oi != IDX_SENTINEL && (bi == IDX_SENTINEL || kx_better(ok, oi, bk, bi))) { bk = ok; bi = oi; }
        }
        if (bi != IDX_SENTINEL && hi == bi) ++pos;          // ids are unique: exactly one lane advances
        if (lane == 0) {
            const bool none = bi == IDX_SENTINEL;
            const double pad = FILTERED ? (double)__int_as_float(0x7fc00000) : (p.l2 ? (double)INFINITY : -(double)INFINITY);
            const double d = none ? pad : (p.l2 ? -bk : bk);
            p.out_dist[q * p.k + o] = (float)d;
            p.out_idx[q * p.k + o] = none ? -1 : (int64_t)bi + p.id_base;
            if (p.out_key) p.out_key[q * p.k + o] = d;
        }
    }
    }
}

template <typename KeyT>
struct ListMergeParams {
    const KeyT* key = nullptr;    // [n_parts, nq, k] final distances of each shard
    const int64_t* idx = nullptr; // [n_parts, nq, k] global ids, -1 = unfilled
    int n_parts = 0, k = 0, l2 = 0;
    int64_t nq = 0;
    float* out_dist = nullptr;
    int64_t* out_idx = nullptr;
    double* out_key = nullptr;    // optional (KeyT == double)
};
static_assert(std::is_trivially_copyable_v<ListMergeParams<float>> && std::is_trivially_copyable_v<ListMergeParams<double>>, "kernel argument");

template <typename KeyT>
__global__ __launch_bounds__(256) void k_merge_lists(ListMergeParams<KeyT> p) {
    extern __shared__ int s_pos_all[];   // [4 waves][n_parts]
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * 4 + wave;
    if (q >= p.nq) return;
    int* s_pos = s_pos_all + wave * p.n_parts;
    for (int i = lane; i < p.n_parts; i += 64) s_pos[i] = 0;
    for (int o = 0; o < p.k; ++o) {
        KeyT bs = 0;             // "larger is better" key
        int64_t bi = INT64_MAX;
        int bp = -1;
        for (int part = lane; part < p.n_parts; part += 64) {
            const int pos = s_pos[part];
            if (pos >= p.k) continue;
            const int64_t off = ((int64_t)part * p.nq + q) * p.k + pos;
            const int64_t id = p.idx[off];
            if (id < 0) continue;
            const KeyT key = p.l2 ? -p.key[off] : p.key[off];
            if (bp < 0 || key > bs || (key == bs && id < bi)) { bs = key; bi = id; bp = part; }
        }
#pragma unroll
        for (int ofs = 32; ofs > 0; ofs >>= 1) {
            const KeyT os = __shfl_xor(bs, ofs, 64);
            const int64_t oi = __shfl_xor(bi, ofs, 64);
            const int op = __shfl_xor(bp, ofs, 64);
            if (op >= 0 && (bp < 0 || os > bs || (os == bs && oi < bi))) { bs = os; bi = oi; bp = op; }
        }
        if (bp >= 0 && (bp & 63) == lane) s_pos[bp] += 1;
        if (lane == 0) {
            const KeyT d = bp < 0 ? (p.l2 ? (KeyT)INFINITY : -(KeyT)INFINITY) : (p.l2 ? -bs : bs);
            p.out_dist[q * p.k + o] = (float)d;
            p.out_idx[q * p.k + o] = bp < 0 ? -1 : bi;
            if (p.out_key) p.out_key[q * p.k + o] = (double)d;
        }
    }
}

// ---- append path ----------------------------------------------------------------------------------
// one wave per row.  mode 0: copy; 1: copy + ynorm = sum x^2; 2: x / (sqrt(sum x^2) + 1e-12)
// OutT = float: as above.  OutT = _Float16 (fp16 store / fp16 scan queries): values are rounded to nearest-even on the
// way out and |y|^2 is taken of the ROUNDED row, so the L2 score 2 q.y - |y|^2 is consistent with what is stored.
template <typename OutT>
__global__ __launch_bounds__(256) void k_rows_prepare(const float* in, OutT* out, float* ynorm, int64_t n, int dim, int mode) {
    constexpr bool H = sizeof(OutT) == 2;
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const f32x4* src = reinterpret_cast<const f32x4*>(in + row * dim);
    const int nv = dim >> 2;
    auto put = [&](int i, f32x4 v) {
        if constexpr (H) {
            const f16x4 h4 = {(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
            reinterpret_cast<f16x4*>(out + row * dim)[i] = h4;
        } else {
            reinterpret_cast<f32x4*>(out + row * dim)[i] = v;
        }
    };
    float ss = 0.f;
    if (mode != 0) {
        for (int i = lane; i < nv; i += 64) {
            f32x4 v = src[i];
            if (H && mode == 1) { v[0] = (float)(_Float16)v[0]; v[1] = (float)(_Float16)v[1]; v[2] = (float)(_Float16)v[2]; v[3] = (float)(_Float16)v[3]; }
            ss += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
        }
        ss = wave_sum(ss);
    }
    if (mode == 2) {
        const float den = sqrtf(ss) + 1e-12f;
        for (int i = lane; i < nv; i += 64) {
            f32x4 v = src[i];
            v[0] = v[0] / den; v[1] = v[1] / den; v[2] = v[2] / den; v[3] = v[3] / den;
            put(i, v);
        }
    } else {
        if (H || reinterpret_cast<const void*>(in) != reinterpret_cast<const void*>(out))
            for (int i = lane; i < nv; i += 64) put(i, src[i]);
        if (mode == 1 && lane == 0) ynorm[row] = ss;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_gather_rows(const T* __restrict__ db, const int64_t* __restrict__ idx,
                                                     int64_t n_out, int64_t ntotal, int64_t id_base, int dim,
                                                     float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t o = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= n_out) return;
    const int64_t r = idx[o] - id_base;
    const bool ok = idx[o] >= 0 && r >= 0 && r < ntotal;
    f32x4* dst = reinterpret_cast<f32x4*>(out + o * dim);
    const T* src = db + (ok ? r : 0) * dim;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    for (int i = lane; i < (dim >> 2); i += 64) {
        f32x4 v = z;
        if (ok) {
            if constexpr (sizeof(T) == 2) {
                const f16x4 h4 = reinterpret_cast<const f16x4*>(src)[i];
                v = f32x4{(float)h4[0], (float)h4[1], (float)h4[2], (float)h4[3]};       // fp16 -> fp32 is exact
            } else {
                v = reinterpret_cast<const f32x4*>(src)[i];
            }
        }
        dst[i] = v;
    }
}

// |y|^2 of stored rows (fp32 or fp16): used when a snapshot is loaded into an L2 store
template <typename T>
__global__ __launch_bounds__(256) void k_row_sqnorm(const T* __restrict__ rows, int64_t n, int dim, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    float ss = 0.f;
    for (int i = lane; i < dim; i += 64) { const float v = (float)rows[r * dim + i]; ss += v * v; }
    ss = wave_sum(ss);
    if (lane == 0) out[r] = ss;
}

// exclusion + compaction of search hits (retrieve_similar_vectors, pipeline.py:491-515): one thread per query row
__global__ __launch_bounds__(256) void k_filter_topk(const float* __restrict__ in_dist, const int64_t* __restrict__ in_idx,
                                                     int64_t nq, int k_in, int k_keep, const int64_t* __restrict__ tags,
                                                     int64_t ntotal, int64_t id_base, const int64_t* __restrict__ excl,
                                                     int64_t n_excl, float* __restrict__ out_dist, int64_t* __restrict__ out_idx) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    int kept = 0;
    for (int j = 0; j < k_in && kept < k_keep; ++j) {
        const int64_t id = in_idx[q * k_in + j];
        const int64_t r = id - id_base;
        if (id < 0 || r < 0 || r >= ntotal) continue;
        bool drop = false;
        if (n_excl > 0) {
            const int64_t t = tags[r];
            int64_t lo = 0, hi = n_excl;                    // binary search in the sorted exclusion set
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (excl[mid] < t) lo = mid + 1; else hi = mid;
            }
            drop = lo < n_excl && excl[lo] == t;
        }
        if (drop) continue;
        out_idx[q * k_keep + kept] = id;
        out_dist[q * k_keep + kept] = in_dist[q * k_in + j];
        ++kept;
    }
    for (; kept < k_keep; ++kept) {
        out_idx[q * k_keep + kept] = -1;
        out_dist[q * k_keep + kept] = __int_as_float(0x7fc00000);   // NaN, as pipeline.py:515
    }
}

// ---- exclusion-aware search (radad_knn_search_excl): the exact top-k among the rows whose tag is not excluded ----------------------
// t in the ascending exclusion set?  (the binary search of k_filter_topk)
__device__ __forceinline__ bool excl_has(const int64_t* __restrict__ excl, int64_t n_excl, int64_t t) {
    int64_t lo = 0, hi = n_excl;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (excl[mid] < t) lo = mid + 1; else hi = mid;
    }
    return lo < n_excl && excl[lo] == t;
}

struct ExclCompactParams {
    const float* in_dist = nullptr;     // [nq, k_in] the fast pass's hits: the certified search at k_fetch, ordered by (float64 distance, id)
    const int64_t* in_idx = nullptr;    // [nq, k_in] global ids, -1 = unfilled slot
    const double* in_key = nullptr;     // [nq, k_in] float64 keys
    int64_t nq = 0;
    int k_in = 0, k_keep = 0;
    int whole = 0;                      // the caller asked for more hits than the store has rows and the list was cut to them
    const int64_t* tags = nullptr;      // [ntotal] row tags (read only when n_excl > 0)
    int64_t ntotal = 0, id_base = 0;
    const int64_t* excl = nullptr;      // [n_excl] ascending exclusion set
    int64_t n_excl = 0;
    float* out_dist = nullptr;          // [nq, k_keep]
    int64_t* out_idx = nullptr;         // [nq, k_keep]
    double* out_key = nullptr;          // [nq, k_keep]; optional unless FRONTIER
    int* count = nullptr;               // !FRONTIER: [1] listed-query counter (device scope) ...
    int* sel = nullptr;                 // ... and [nq] the listed queries
    double* fr_key = nullptr;           // FRONTIER: [nq] frontier keys ...
    int64_t* fr_idx = nullptr;          // ... ids, -1 = nothing of the shard is unseen ...
    int* own = nullptr;                 // ... and [nq] 1 = the shard's list is short although rows are unseen
    // PER_QUERY (radad_knn_search_excl_pq / _pq_begin) instead of excl / n_excl: query q excludes the first clamp(q_cnt[q], 0, m)
    // tags of q_tags[q, :] (q_cnt NULL = m for every query); 0 <= m <= 64
    const int64_t* q_tags = nullptr;
    const int* q_cnt = nullptr;
    int m = 0;
};
static_assert(std::is_trivially_copyable_v<ExclCompactParams>, "kernel argument");

// Certificate + compaction: one wave per query walks the query's k_in exact hits (unfilled slots id -1) in strips of 64 and keeps,
// in order, the first k_keep whose tag is not excluded; the rest of the row is padded with id -1 / NaN.
// !FRONTIER (radad_knn_search_excl, the whole store): the row is PROVED -- the exact top-k_keep among the admissible rows -- when
// it holds k_keep survivors (an admissible row outside the list ranks behind the whole list), or when the list is all the store
// has (an unfilled slot, or `whole`).  Any other query is appended to sel[] (count[0]) for the row-filtered exact pass, which
// overwrites its row.
// FRONTIER (radad_knn_search_excl_begin, one shard of a row-sharded store): a shard cannot prove a query alone, so nothing is listed
// here; instead the query gets a frontier (key, id): every admissible row of the shard that is not among the survivors written
// ranks strictly behind it.  It is the k_keep-th survivor when there are k_keep; else the last hit of the fast-pass list
// (admissible or not: the list is a prefix of the shard's ranking); else, when the list is all the shard has, id -1 / key NaN:
// nothing is unseen.  own[q] = 1 for the query the other form would have listed: the only kind whose list the exact pass can
// still change.
// PER_QUERY: the same with the admission test of radad_knn_search_excl_pq -- lane l holds tag l of the wave's query; a hit's tag is
// compared with the query's tags one lane at a time (<= 64 register reads per strip, no memory).  A compile-time parameter: the
// batch-wide instantiations are the code they were.
template <bool FRONTIER, bool PER_QUERY = false>
__global__ __launch_bounds__(256) void k_excl_compact(ExclCompactParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= p.nq) return;                                      // (wave-uniform)
    int64_t my_tag = 0;                                         // (PER_QUERY) tag `lane` of this query, lanes [0, cnt)
    int cnt = 0;
    if constexpr (PER_QUERY) {
        cnt = p.m > 0 ? min(max(p.q_cnt ? p.q_cnt[q] : p.m, 0), p.m) : 0;
        if (lane < cnt) my_tag = p.q_tags[q * p.m + lane];
    }
    const int k_in = p.k_in, k_keep = p.k_keep;
    const double nan64 = (double)__int_as_float(0x7fc00000);
    int kept = 0;
    bool unfilled = false;
    for (int s0 = 0; s0 < k_in && kept < k_keep; s0 += 64) {
        const int j = s0 + lane;
        int64_t id = -1;
        bool keep = false;
        if (j < k_in) {
            id = p.in_idx[q * k_in + j];
            const int64_t r = id - p.id_base;
            keep = id >= 0 && r >= 0 && r < p.ntotal;
            if constexpr (!PER_QUERY) {
                if (keep && p.n_excl > 0) keep = !excl_has(p.excl, p.n_excl, p.tags[r]);
            }
        }
        if constexpr (PER_QUERY) {
            if (cnt > 0) {                                      // (wave-uniform; every lane takes part in the shuffles)
                const int64_t t = keep ? p.tags[id - p.id_base] : 0;
                for (int e = 0; e < cnt; ++e) {
                    const int64_t o = __shfl(my_tag, e, 64);    // (outside the condition: all lanes shuffle)
                    keep = keep && o != t;
                }
            }
        }
        unfilled |= __ballot(j < k_in && id < 0) != 0ull;
        const unsigned long long m = __ballot(keep);
        const int pos = kept + __popcll(m & ((1ull << lane) - 1ull));
        if (keep && pos < k_keep) {
            p.out_idx[q * k_keep + pos] = id;
            p.out_dist[q * k_keep + pos] = p.in_dist[q * k_in + j];
            if (FRONTIER || p.out_key) p.out_key[q * k_keep + pos] = p.in_key[q * k_in + j];
            if constexpr (FRONTIER)
                if (pos == k_keep - 1) { p.fr_key[q] = p.in_key[q * k_in + j]; p.fr_idx[q] = id; }
        }
        kept += __popcll(m);
    }
    kept = min(kept, k_keep);
    for (int o = kept + lane; o < k_keep; o += 64) {
        p.out_idx[q * k_keep + o] = -1;
        p.out_dist[q * k_keep + o] = __int_as_float(0x7fc00000);   // NaN, as pipeline.py:515
        if (FRONTIER || p.out_key) p.out_key[q * k_keep + o] = nan64;
    }
    if (lane != 0) return;
    const bool unseen = kept < k_keep && !unfilled && !p.whole;    // (k_in >= 1: the store is not empty)
    if constexpr (FRONTIER) {
        if (kept < k_keep) {
            p.fr_key[q] = unseen ? p.in_key[q * k_in + k_in - 1] : nan64;
            p.fr_idx[q] = unseen ? p.in_idx[q * k_in + k_in - 1] : -1;
        }
        p.own[q] = unseen ? 1 : 0;
    } else if (unseen) {
        p.sel[atomicAdd(p.count, 1)] = (int)q;
    }
}

// The admission bitmap of the filtered passes: bit (i & 63) of admit[i >> 6] = the tag of row i is not in the ascending exclusion
// set.  One thread per row, one ballot and one 64-bit word per wave; the host says how many words to write (the grid covers them).
// !VIA_LIDS (the row-filtered exact pass, k_exact_scan_excl): i is the row itself.  VIA_LIDS (the IVF list scans): i is a list-major
// position and the row is lids[i]; the host asks for one spare word behind the last, all zero.
// count: workgroups leave at once when *count == 0, no query was listed (the flat search's usual call); NULL = always build.
template <bool VIA_LIDS>
__global__ __launch_bounds__(256) void k_admit_bitmap(const int64_t* __restrict__ tags, const int64_t* __restrict__ lids, int64_t n,
                                                      const int64_t* __restrict__ excl, int64_t n_excl, const int* __restrict__ count,
                                                      unsigned long long* __restrict__ admit, int64_t n_words) {
    if (count && *count == 0) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;          // (whole waves: every lane ballots)
    const bool ok = i < n && !excl_has(excl, n_excl, tags[VIA_LIDS ? lids[i] : i]);
    const unsigned long long m = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && (i >> 6) < n_words) admit[i >> 6] = m;
}

// ---- the same over ROW SHARDS (radad_knn_search_excl_begin / _finish, radad_excl_merge_certify) -------------------------------------
// Flags to list: the queries the shards could not prove together (unproved[q] != 0) and whose list on THIS shard the exact pass can
// change (own[q]) become the sel[] / count pair the row-filtered exact pass reads.  A flagged query whose shard list is full, or is
// all the shard has, already holds the shard's exact admissible top k.
__global__ __launch_bounds__(256) void k_excl_flags_to_list(const int* __restrict__ unproved, const int* __restrict__ own, int64_t nq,
                                                            int* __restrict__ count, int* __restrict__ sel) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q < nq && unproved[q] != 0 && own[q] != 0) sel[atomicAdd(count, 1)] = (int)q;
}

struct ExclMergeParams {
    const double* key = nullptr;      // [n_parts, nq, k] float64 keys of each shard's survivors
    const int64_t* idx = nullptr;     // [n_parts, nq, k] global ids, -1 = padding
    const double* fr_key = nullptr;   // [n_parts, nq] frontiers
    const int64_t* fr_idx = nullptr;  // [n_parts, nq], -1 = the shard has nothing unseen
    int n_parts = 0, k = 0, l2 = 0;
    int64_t nq = 0;
    float* out_dist = nullptr;
    int64_t* out_idx = nullptr;
    double* out_key = nullptr;        // optional
    int* unproved = nullptr;          // [nq]
};
static_assert(std::is_trivially_copyable_v<ExclMergeParams>, "kernel argument");

// k_merge_lists<double>'s merge (one wave per query, (key, id) order, id -1 last) with the exclusion family's padding (-1 / NaN / NaN)
// and the certificate ACROSS shards: the query is proved iff for every shard with a frontier (id >= 0) the merged list holds k
// entries and its last one is the frontier entry or ranks ahead of it -- an admissible row in no list ranks behind its shard's
// frontier, hence behind M[k-1].
__global__ __launch_bounds__(256) void k_excl_merge_certify(ExclMergeParams p) {
    extern __shared__ int s_pos_all[];   // [4 waves][n_parts]
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * 4 + wave;
    if (q >= p.nq) return;
    int* s_pos = s_pos_all + wave * p.n_parts;
    for (int i = lane; i < p.n_parts; i += 64) s_pos[i] = 0;
    double bs = 0;               // "larger is better" key of the entry merged last
    int64_t bi = INT64_MAX;
    int bp = -1;
    for (int o = 0; o < p.k; ++o) {
        bs = 0; bi = INT64_MAX; bp = -1;
        for (int part = lane; part < p.n_parts; part += 64) {
            const int pos = s_pos[part];
            if (pos >= p.k) continue;
            const int64_t off = ((int64_t)part * p.nq + q) * p.k + pos;
            const int64_t id = p.idx[off];
            if (id < 0) continue;
            const double key = p.l2 ? -p.key[off] : p.key[off];
            if (bp < 0 || key > bs || (key == bs && id < bi)) { bs = key; bi = id; bp = part; }
        }
#pragma unroll
        for (int ofs = 32; ofs > 0; ofs >>= 1) {
            const double os = __shfl_xor(bs, ofs, 64);
            const int64_t oi = __shfl_xor(bi, ofs, 64);
            const int op = __shfl_xor(bp, ofs, 64);
            if (op >= 0 && (bp < 0 || os > bs || (os == bs && oi < bi))) { bs = os; bi = oi; bp = op; }
        }
        if (bp >= 0 && (bp & 63) == lane) s_pos[bp] += 1;
        if (lane == 0) {
            const double d = bp < 0 ? (double)__int_as_float(0x7fc00000) : (p.l2 ? -bs : bs);
            p.out_dist[q * p.k + o] = (float)d;
            p.out_idx[q * p.k + o] = bp < 0 ? -1 : bi;
            if (p.out_key) p.out_key[q * p.k + o] = d;
        }
    }
    // (bs, bi, bp) is M[k-1] on every lane, bp < 0 when the merged list is short
    bool bad = false;
    for (int part = lane; part < p.n_parts; part += 64) {
        const int64_t fi = p.fr_idx[(int64_t)part * p.nq + q];
        if (fi < 0) continue;
        const double fk = p.l2 ? -p.fr_key[(int64_t)part * p.nq + q] : p.fr_key[(int64_t)part * p.nq + q];
        bad |= !(bp >= 0 && (bs > fk || (bs == fk && bi <= fi)));
    }
    const unsigned long long any_bad = __ballot(bad);
    if (lane == 0) p.unproved[q] = any_bad != 0ull ? 1 : 0;
}

// out[r] = the k-th largest of in[r][0..m) (NaN ranks lowest).  One wave per row, a lane holds up to KTH_PER_LANE values; k - 1 rounds
// of "wave-wide maximum, its first holder drops it".  The sharded search's bound: m = G k lower bounds per query.
constexpr int KTH_PER_LANE = 20;         // m <= 1280 (8 shards x k = 128, or 40 x 32)
// Value j = g per_group + i of row r sits at in[(g n + r) per_group + i]: [groups][n][per_group], the layout an all-gather of the
// shards' [n][k] bound blocks produces (groups = 1: plain [n][m]).
__global__ __launch_bounds__(256) void k_kth_largest(const float* __restrict__ in, int64_t n, int groups, int per_group, int k,
                                                     float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const int m = groups * per_group;
    float v[KTH_PER_LANE];
#pragma unroll
    for (int i = 0; i < KTH_PER_LANE; ++i) {
        const int c = lane + 64 * i;
        const float x = c < m ? in[((int64_t)(c / per_group) * n + r) * per_group + c % per_group] : -INFINITY;
        v[i] = x == x ? x : -INFINITY;
    }
    float best = -INFINITY;
    for (int round = 0; round < k; ++round) {
        float mine = v[0];
#pragma unroll
        for (int i = 1; i < KTH_PER_LANE; ++i) mine = fmaxf(mine, v[i]);
        best = wave_max(mine);
        if (round + 1 == k) break;
        // the lowest lane holding `best` drops one copy of it
        const unsigned long long holders = __ballot(mine == best);
        if (holders == 0ull) break;                                   // (only when everything left is -inf)
        if (lane == __ffsll((long long)holders) - 1) {
            bool done = false;
#pragma unroll
            for (int i = 0; i < KTH_PER_LANE; ++i)
                if (!done && v[i] == best) { v[i] = -INFINITY; done = true; }
        }
    }
    if (lane == 0) out[r] = best;
}

constexpr size_t knn_lds_bytes() { return sizeof(float) * (2 * KT_M * KT_LD + 2 * KT_N * KT_LD); }
static_assert(KT_N * KS_LD <= 2 * KT_M * KT_LD + 2 * KT_N * KT_LD, "score tile must fit in the tile buffers");

}  // namespace

template <typename KeyT>
static int merge_lists(int metric, const KeyT* in_key, const int64_t* in_idx, int n_parts, int64_t nq, int k, float* out_dist,
                       int64_t* out_idx, double* out_key, int device, void* stream) {
    RADAD_REQUIRE(metric >= 0 && metric <= 2, "radad_topk_merge: bad metric");
    RADAD_REQUIRE(n_parts >= 1 && n_parts <= 4096 && k >= 1 && k <= RADAD_KNN_MAX_K && nq >= 0, "radad_topk_merge: bad shape");
    if (nq == 0) return RADAD_OK;
    RADAD_REQUIRE(in_key && in_idx && out_dist && out_idx, "radad_topk_merge: NULL buffer");
    DeviceGuard g(device);
    ListMergeParams<KeyT> m;
    m.key = in_key; m.idx = in_idx; m.n_parts = n_parts; m.k = k; m.l2 = metric == RADAD_METRIC_L2; m.nq = nq;
    m.out_dist = out_dist; m.out_idx = out_idx; m.out_key = out_key;
    hipLaunchKernelGGL(k_merge_lists<KeyT>, dim3((unsigned)ceil_div64(nq, 4)), dim3(256), 4 * n_parts * sizeof(int),
                       (hipStream_t)stream, m);
    RADAD_HIP_CHECK(hipGetLastError());
    return RADAD_OK;
}

// what phase 2 of a search needs from phase 1 (knn_search_phase1 / _phase2 below)
struct SearchCtx {
    bool valid = false;
    int64_t nq = 0;
    int k = 0, l2 = 0, cslot = 0, n_parts = 0, plen = 0, cap = 0, xgroup = 1;
    bool emit = false, use_floor = false;
    bool small_lists = false;          // the streaming kernels' output: one SORTED list per workgroup and query (k_refine_small)
    bool canonical = false;            // the scan's scores estimate q.y / -|q - y|^2 themselves (comparable across shards); the fp32
                                       // kernels' L2 score 2 q.y - |y|^2 lacks the -|q|^2: a cross-shard bound does not apply to it
    const float* q_use = nullptr;       // fp32 queries as the re-rank reads them (caller's buffer, or the workspace's normalised copy)
    bool have_ak = false;              // k_kth_floor left a_k in the workspace (ws.ak)
    bool hi_tile = false;              // the certified f16 tile scan took this search
    SearchLayout ws;
};

// the admission rule of an exclusion-aware search: one ascending set for the batch (radad_knn_search_excl), or <= 64 tags per query
// (radad_knn_search_excl_pq).  n_excl is the size of the set, or m: 0 = nothing is excluded, in either mode.
struct ExclRule {
    const int64_t* tags = nullptr;      // [ntotal] row tags
    const int64_t* excl = nullptr;      // batch-wide: [n_excl] ascending
    int64_t n_excl = 0;
    bool per_query = false;
    const int64_t* q_tags = nullptr;    // per query: [nq, m]
    const int* q_cnt = nullptr;         // [nq] or NULL = m for every query
    int m() const { return (int)n_excl; }
};

// an exclusion-aware search begun on a row shard (radad_knn_search_excl_begin / _pq_begin) without its _finish yet
struct ExclCtx {
    bool valid = false;
    int64_t nq = 0;
    int k = 0, l2 = 0;
    const float* q_use = nullptr;
    ExclRule rule;                      // (which admission rule it was begun with: _finish runs the exact pass of that rule)
    ExclLayout L;
};

// ---- handle -------------------------------------------------------------------------------------------
struct radad_knn_s {
    int dim = 0, metric = 0, device = 0;
    int64_t id_base = 0;
    int64_t ntotal = 0, capacity = 0;
    int f16 = 0;              // 1: rows are stored as IEEE fp16 (config.use_float16, vector_database.py:80)
    char* rows = nullptr;     // [capacity, dim] fp32 or fp16
    float* ynorm = nullptr;
    // f16 "hi plane" of an fp32 store for the certified scan (knn_hi.inc): built lazily, rows [0, hi_rows) are current
    _Float16* hi = nullptr;      // [hi_cap][dim]
    float* rscale = nullptr;     // [hi_cap] 2^-e per row (nullptr for cosine stores: one scale, 2^-14)
    int64_t hi_rows = 0, hi_cap = 0;
    int hi_off = 0;              // 1: disabled (RADAD_KNN_OPT_HI_PLANE 0 / RADAD_KNN_HI=0, or its allocation failed)
    // kernel choices of this handle (radad_knn_set_option; the environment names are announced overrides of the defaults set at creation)
    int opt_centre = -1;         // -1: decided per store from |mean|^2 / mean |y|^2; 0 never, 1 always
    int opt_smallq_hi = 1;       // small batches stream the f16 plane (0: the fp32 rows)
    int opt_wide_min_q = 17;     // smallest batch that takes the 256-query tile scan
    int opt_dense = 1;           // stores of <= RF_STAGE_MAX rows: all scores + select (k_knn_dense) instead of the register-list kernels
    size_t last_o_cnt = 0, last_o_thr = 0; int64_t last_emit_nq = 0;   // the last tile-scan search's candidate counters / floors in the workspace
    int last_scan_phases = 0;    // (radad_knn_last_scan_phases)
    unsigned* stat = nullptr;    // device [3] float bits: max |y'|, max |y' - yh| (y' = y - mu when the plane is centred, else y) and
                                 // max |y| over rows [0, stat_rows)
    int64_t stat_rows = 0;
    // centred plane (decided when the plane is built, from the rows the store holds then): the plane holds f16((y - mu) 2^e)
    float* cmu = nullptr;        // [dim] the common component, or nullptr: plane of the rows themselves
    float mu_norm = 0.f, mu_sq = 0.f;   // |mu| (rounded up: it enters error bounds) and |mu|^2 as summed on the device
    float* rbias = nullptr;      // [hi_cap] per-row bias of a centred plane: |y - mu|^2 (L2) or mu.y (IP / cosine)
    float* kacc = nullptr;       // K-split tile scan (small stores of wide rows): partial accumulators of the two halves of a tile ...
    int* kflag = nullptr;        // ... and the arrival counters (zero between launches)
    int64_t kacc_tiles = 0;
    int* xarrive = nullptr;      // exact pass: arrival counters of the query groups (zero between launches)
    int64_t xarrive_cap = 0;
    // radad_knn_search_excl: a workspace of its own beside `ws` (which the fast pass inside the call may re-allocate): the fast pass's
    // k_fetch lists | listed-query counter | listed queries | admission bitmap | the filtered exact pass's partial lists
    // (radad_knn_range_search keeps the partial lists of its exact pass here as well: RangeLayout, knn_plan.h)
    void* excl_ws = nullptr;
    size_t excl_ws_bytes = 0, excl_o_count = 0;
    int64_t last_excl_nq = 0;    // batch size of the most recent exclusion-aware search (radad_knn_last_excl)
    int64_t last_xs_nq = 0;      // radad_knn_search_excl_scan: batch size and route of the most recent one (radad_knn_last_excl_scan; its
    int last_xs_route = RADAD_EXCL_SCAN_EXACT;      // count of exactly answered queries is copied to host_count[HC_XS_EXACT] behind it)
    int64_t last_rg_nq = 0;      // radad_knn_range_search: batch size and route of the most recent one (radad_knn_last_range; its count
    int last_rg_route = RADAD_RANGE_EXACT;          // of exactly answered queries is copied to host_count[HC_RG_EXACT] behind it)
    double* rs_key = nullptr;    // k_refine_small: [SQ_NQ][KNN_CERT_CAP] float64 keys of the candidates, where the query's workgroups meet
    int* rs_count = nullptr;     // ... and [SQ_NQ] arrival counters (zero between launches)
    int uniform_e = HI_E_PER_ROW; // one power-of-two scale 2^e for every row of the plane (rows of one magnitude), or HI_E_PER_ROW
    // early abandon of scan tiles (knn_hi.inc, ABANDON; knn_plan.h): the store's suffix norms per aligned KW_M-row tile, kept with the
    // rows the statistics kernel has seen -- built with the plane, extended by appends (only the tiles touched: an atomic max, which an
    // append can only raise), started over whenever the statistics start over (a new plane, a loaded snapshot)
    int opt_abandon = 1;         // RADAD_KNN_OPT_ABANDON
    int opt_range_smallq = 0;    // RADAD_KNN_OPT_RANGE_SMALLQ
    float* tile_ry = nullptr;    // [2][tile_ry_cap]: per tile the largest suffix norm, then the largest accumulator start (bias_sign x bias)
    int64_t tile_ry_cap = 0;     // tiles
    int64_t ab_rows = 0;         // rows [0, ab_rows) are in tile_ry ...
    int ab_from = 0;             // ... as norms from this element on
    void* ab_ws = nullptr;       // a search's per-query terms (AbandonLayout)
    size_t ab_ws_bytes = 0;
    bool ab_search_ready = false;// this search's per-query terms are written (knn_prepare_queries decides, once; the scan reads it)
    size_t last_o_ab = 0;        // the last search's abandon counters in the workspace, and the tile tasks of its abandoning launches
    int64_t last_ab_tasks = -1;  // (-1: no search yet)
    // the abandoning scan's tiles dealt by ticket (knn_abandon_deal, knn_plan.h): KNN_DEAL_SETS sets of counters, one per launch of a
    // search, all zeroed by the search's query preparation (allocated with the per-query terms: knn_abandon_terms_ready)
    int opt_abandon_deal = 0;    // RADAD_KNN_OPT_ABANDON_DEAL (off by default: profiles/abandon_deal_ab.txt)
    int n_cus = 0;               // compute units of the device (radad_knn_create)
    int* deal_cnt = nullptr;     // [KNN_DEAL_COUNTERS]
    int last_deal_launches = 0, last_deal_workgroups = 0, last_deal_granule = 0;      // radad_knn_last_abandon_deal
    // a vetoed tile's few live rows deferred to a dense tail (knn_abandon_defer, knn_plan.h): a deferring launch counts in its own set
    // of deal_cnt (it is never dealt too: knn_defer_counter); the lists are a buffer of the handle's own, sized for the whole store
    int opt_abandon_defer = 1;   // RADAD_KNN_OPT_ABANDON_DEFER (measured: profiles/abandon_defer_ab.txt)
    int* defer_list = nullptr;   // [KNN_DEFER_MAX_QTILES][defer_list_cap]
    int64_t defer_list_cap = 0;
    int last_defer_launches = 0; // tails launched by the last search (radad_knn_last_abandon_defer) ...
    unsigned last_defer_sets = 0;// ... and the counter sets they used, one bit each
    // the next tile's head fetched at the abandon checkpoint (knn_abandon_ahead, knn_plan.h): two counters per launch in its set of deal_cnt
    int opt_abandon_ahead = 1;   // RADAD_KNN_OPT_ABANDON_AHEAD (measured: profiles/abandon_ahead_ab.txt)
    unsigned last_ahead_sets = 0;// the counter sets the last search's prefetching launches used, one bit each (radad_knn_last_abandon_ahead)
    // removing rows in place (knn_remove.inc; the plan: knn_remove_plan, knn_plan.h)
    int opt_remove_stage_rows = 0;       // RADAD_KNN_OPT_REMOVE_STAGE_ROWS: slab size in rows, 0 = what KNN_REMOVE_STAGE_BYTES holds
    int last_remove_launches = 0;        // move launches of the last removal and the bytes they read + wrote (radad_knn_last_remove)
    int64_t last_remove_bytes = 0;
    // queries the certificate rejected in the most recent search: counted on the device, copied to pinned host memory
    // behind the search (no synchronisation inside search); feeds the adaptive tuning and radad_knn_last_recheck
    int* host_count = nullptr;   // pinned [2][8]: rejected queries, sum of candidates, rejections by reason x 4, [6] the report's stamp, [7] its batch size
    // ... and behind the two reports one slot each for a count that is copied behind its search and read after a wait:
    static constexpr int HC_LOOK = 16;        // the look before the exact pass: queries the certificate rejected (knn_search_phase2)
    static constexpr int HC_XS_EXACT = 17;    // queries the exact kernel answered in the last in-scan exclusion search (radad_knn_last_excl_scan)
    static constexpr int HC_RG_EXACT = 18;    // ... in the last range search (radad_knn_last_range)
    // what the handle does about batches the certificate mostly rejected -- reports, the look before the exact pass, re-deciding the
    // plane, wider buffers, the fp32 fallback: ONE policy, described and kept in KnnTuning (knn_plan.h); this file reads the pinned
    // slots, synchronises, rebuilds the plane and hands plain integers to it
    KnnTuning tune;
    bool owned_serial = false;   // the handle is private to another object that orders its calls itself (the IVF index's centroid store): no ev_done
    int* host_count_dev = nullptr;   // the same memory as the device sees it
    hipEvent_t ev_done = nullptr;
    hipEvent_t ev_begun = nullptr;      // end of radad_knn_search_begin's device work: _finish waits for it (it may run on another stream)
    bool have_last = false;
    hipStream_t last_stream = nullptr;   // where the last search was enqueued (the next one on ANOTHER stream orders itself behind it; the statistics calls synchronise on it)
    int64_t count_nq[2] = {0, 0};    // batch size of the search a slot belongs to
    size_t esize() const { return f16 ? 2 : 4; }
    size_t row_bytes() const { return (size_t)dim * esize(); }
    // search workspace (grown on demand, reused)
    void* ws = nullptr;
    size_t ws_bytes = 0;
    int last_qtiles = 0, last_splits = 0, last_threads = KNN_THREADS;
    int last_kind = RADAD_SCAN_F32_TILE;   // which scan kernel the last search ran (radad_knn_last_scan_kind)
    int last_scan_launches = 1;            // ... in how many launches
    EventRing prof;
    SearchCtx pending;           // radad_knn_search_begin without its _finish yet
    ExclCtx pending_excl;        // radad_knn_search_excl_begin without its _finish yet (at most one begun search, of either kind)
    std::mutex mu;
};

static void knn_drop_plane(radad_knn_t h);

static int knn_realloc(radad_knn_t h, int64_t cap) {
    char* nrows = nullptr;
    float* nnorm = nullptr;
    if (hipMalloc(&nrows, (size_t)cap * h->row_bytes()) != hipSuccess) {
        radad_set_error("hipMalloc of %lld x %d rows failed", (long long)cap, h->dim);
        return RADAD_ENOMEM;
    }
    if (h->metric == RADAD_METRIC_L2 && hipMalloc(&nnorm, (size_t)cap * sizeof(float)) != hipSuccess) {
        (void)hipFree(nrows);
        radad_set_error("hipMalloc of %lld norms failed", (long long)cap);
        return RADAD_ENOMEM;
    }
    (void)hipDeviceSynchronize();       // searches on other streams may still read the old buffers
    if (h->ntotal > 0) {
        RADAD_HIP_CHECK(hipMemcpy(nrows, h->rows, (size_t)h->ntotal * h->row_bytes(), hipMemcpyDeviceToDevice));
        if (nnorm) RADAD_HIP_CHECK(hipMemcpy(nnorm, h->ynorm, (size_t)h->ntotal * sizeof(float), hipMemcpyDeviceToDevice));
    }
    if (h->rows) (void)hipFree(h->rows);
    if (h->ynorm) (void)hipFree(h->ynorm);
    h->rows = nrows;
    h->ynorm = nnorm;
    h->capacity = cap;
    knn_drop_plane(h);                           // rebuilt lazily for the new capacity
    return RADAD_OK;
}

// geometric growth so repeated add() calls (vector_database.py:134-138 adds 10 000 rows at a time) stay O(n)
static int knn_grow(radad_knn_t h, int64_t need) {
    if (need <= h->capacity) return RADAD_OK;
    int64_t cap = std::max<int64_t>(need, h->capacity + h->capacity / 2);
    return knn_realloc(h, std::max<int64_t>(cap, 1024));
}

// grow the search workspace to `bytes` (every search lays its buffers out first and calls this with the layout's size)
static int knn_workspace(radad_knn_t h, size_t bytes) {
    if (bytes <= h->ws_bytes) return RADAD_OK;
    RADAD_HIP_CHECK(hipDeviceSynchronize());       // a search on another stream may still read the old one
    if (h->ws) (void)hipFree(h->ws);
    h->ws = nullptr;
    h->ws_bytes = 0;
    if (hipMalloc(&h->ws, bytes) != hipSuccess) {
        radad_set_error("hipMalloc of %zu workspace bytes failed", bytes);
        return RADAD_ENOMEM;
    }
    h->ws_bytes = bytes;
    return RADAD_OK;
}

// column means of the first `m` rows, deterministic: KM_SLICES partial sums per column in fixed order, then one block adds them
// up, and measures |mu|^2 against the rows' mean |y|^2 (out2[0], out2[1]) for the host's decision
constexpr int KM_SLICES = 64;
__global__ __launch_bounds__(256) void k_col_partial(const float* __restrict__ rows, int64_t m, int64_t row_stride, int dim, float* __restrict__ part /*[KM_SLICES][dim + 1]*/) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    const int64_t per = (m + KM_SLICES - 1) / KM_SLICES;
    const int64_t r0 = (int64_t)blockIdx.y * per, r1 = min(r0 + per, m);
    float s = 0.f, ss = 0.f;
    if (c < dim)
        for (int64_t r = r0; r < r1; ++r) { const float v = rows[r * row_stride * dim + c]; s += v; ss = fmaf(v, v, ss); }      // (sample row r = store row r x stride)
    if (c < dim) part[(int64_t)blockIdx.y * (dim + 1) + c] = s;
    // sum of squares of this block's columns and rows -> one value per (slice, column block), added up by k_col_final
    __shared__ float red[256];
    red[threadIdx.x] = ss;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) part[(int64_t)KM_SLICES * (dim + 1) + blockIdx.y * gridDim.x + blockIdx.x] = red[0];
}
__global__ __launch_bounds__(256) void k_col_final(const float* __restrict__ part, int64_t m, int dim, int n_cblocks, float* __restrict__ mu,
                                                   float* __restrict__ out2) {
    __shared__ float red[256];
    float mm = 0.f;
    for (int c = threadIdx.x; c < dim; c += 256) {
        float s = 0.f;
        for (int sl = 0; sl < KM_SLICES; ++sl) s += part[(int64_t)sl * (dim + 1) + c];
        const float v = s / (float)m;
        mu[c] = v;
        mm = fmaf(v, v, mm);
    }
    red[threadIdx.x] = mm;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    const float mu2 = red[0];
    __syncthreads();
    float ss = 0.f;
    for (int i = threadIdx.x; i < KM_SLICES * n_cblocks; i += 256) ss += part[(int64_t)KM_SLICES * (dim + 1) + i];
    red[threadIdx.x] = ss;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) { out2[0] = mu2; out2[1] = red[0] / (float)m; }
}

// max |x - mu| over the elements of the first m rows (non-negative floats order like their bit patterns)
__global__ __launch_bounds__(256) void k_absmax(const float* __restrict__ rows, const float* __restrict__ mu, int64_t m, int64_t row_stride, int dim,
                                                unsigned* __restrict__ out /*[2]: max, and min over rows of the row maximum*/) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= m) return;
    float mx = 0.f;
    for (int i = lane; i < dim; i += 64) mx = fmaxf(mx, fabsf(rows[row * row_stride * dim + i] - (mu ? mu[i] : 0.f)));
    mx = wave_max(mx);
    if (lane == 0) {        // (atomics only when the row moves an extreme it can see: same-address atomics serialise)
        const unsigned u = __float_as_uint(mx);
        if (u > *reinterpret_cast<volatile unsigned*>(&out[0])) atomicMax(&out[0], u);
        if (u < *reinterpret_cast<volatile unsigned*>(&out[1])) atomicMin(&out[1], u);
    }
}

static void knn_drop_plane(radad_knn_t h) {
    if (h->hi) (void)hipFree(h->hi);
    if (h->rscale) (void)hipFree(h->rscale);
    if (h->cmu) (void)hipFree(h->cmu);
    if (h->rbias) (void)hipFree(h->rbias);
    h->hi = nullptr; h->rscale = nullptr; h->cmu = nullptr; h->rbias = nullptr; h->mu_norm = 0.f; h->mu_sq = 0.f;
    h->hi_rows = 0; h->hi_cap = 0; h->uniform_e = HI_E_PER_ROW;
    h->ab_rows = 0;
}

// Decide whether the plane is CENTRED and compute mu (one-off, when the plane is built; synchronises).  Centred when the common
// component carries a noticeable part of the rows' energy (|mu|^2 >= 2 % of the mean |y|^2): pooled encoder embeddings do (all
// positive activations around a shared mean), random directions do not -- and an un-centred cosine plane keeps its one scale for
// the whole store, i.e. the scan variant without any per-score arithmetic.
constexpr int64_t KM_MAX_ROWS = 65536;
constexpr float KM_CENTRE_FRACTION = 0.02f;
static bool knn_choose_centre(radad_knn_t h, hipStream_t st) {
    const int64_t m = std::min<int64_t>(h->ntotal, KM_MAX_ROWS);
    if (m < 64 || h->f16) return false;
    const int centre_env = h->opt_centre;
    if (centre_env == 0) return false;
    const int ncb = (h->dim + 255) / 256;
    float *part = nullptr, *mu = nullptr, *out2 = nullptr;
    const size_t pbytes = ((size_t)KM_SLICES * (h->dim + 1) + (size_t)KM_SLICES * ncb) * sizeof(float);
    bool ok = hipMalloc(&part, pbytes) == hipSuccess && hipMalloc(&mu, (size_t)h->dim * sizeof(float)) == hipSuccess &&
              hipMalloc(&out2, 2 * sizeof(float)) == hipSuccess;
    float host2[2] = {0.f, 1.f};
    if (ok) {
        // (the sample is spread over the WHOLE store: its first rows alone say nothing about rows appended later)
        hipLaunchKernelGGL(k_col_partial, dim3(ncb, KM_SLICES), dim3(256), 0, st, (const float*)h->rows, m, std::max<int64_t>(1, h->ntotal / m), h->dim, part);
        hipLaunchKernelGGL(k_col_final, dim3(1), dim3(256), 0, st, (const float*)part, m, h->dim, ncb, mu, out2);
        ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(host2, out2, sizeof(host2), hipMemcpyDeviceToHost, st) == hipSuccess &&
             hipStreamSynchronize(st) == hipSuccess;
    }
    if (part) (void)hipFree(part);
    if (out2) (void)hipFree(out2);
    const bool centre = ok && (centre_env == 1 || host2[0] >= KM_CENTRE_FRACTION * host2[1]) && host2[0] > 0.f && host2[0] < INFINITY;
    if (!centre) { if (mu) (void)hipFree(mu); (void)hipGetLastError(); return false; }
    h->cmu = mu;
    h->mu_norm = sqrtf(host2[0]) * (1.0f + 0x1p-10f);
    h->mu_sq = host2[0];
    return true;
}

// The early abandon's per-tile terms (knn_plan.h), read off the values the scan multiplies -- the plane, or an fp16 store's own rows --
// once those are current: k_tile_terms recomputes every aligned KW_M-row tile from the first one an append touched, so the arrays are
// consistent wherever the plane is built, extended, rebuilt or reloaded.  Stores with per-row scales (RSC 1 / 2) keep none.
static void knn_ensure_tile_terms(radad_knn_t h, hipStream_t st, bool have_plane) {
    const int suf_from = knn_abandon_suffix_from(h->dim);
    const bool current = have_plane ? h->hi_rows == h->ntotal : (h->f16 != 0 && h->stat_rows == h->ntotal);
    if (!h->opt_abandon || suf_from <= 0 || h->rscale || !current || h->ntotal <= 0) return;
    const int64_t cap = knn_abandon_tiles(h->capacity);
    if (h->tile_ry_cap < cap) {
        float* grown = nullptr;
        if (hipMalloc(&grown, (size_t)cap * 2 * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); return; }
        if (h->tile_ry) { (void)hipStreamSynchronize(st); (void)hipFree(h->tile_ry); }
        h->tile_ry = grown; h->tile_ry_cap = cap; h->ab_rows = 0;
    }
    if (h->ab_from != suf_from) { h->ab_rows = 0; h->ab_from = suf_from; }
    if (h->ab_rows >= h->ntotal) return;
    TileTermsParams tp;
    tp.plane = h->f16 ? reinterpret_cast<const _Float16*>(h->rows) : h->hi;
    tp.dim = h->dim; tp.suf_from = suf_from; tp.n = h->ntotal;
    tp.tile0 = h->ab_rows / KW_M;
    const bool biased = h->metric == RADAD_METRIC_L2 || h->cmu;
    tp.rbias = biased ? (h->cmu ? h->rbias : h->ynorm) : nullptr;
    tp.bias_sign = h->metric == RADAD_METRIC_L2 ? -1.f : 1.f;
    tp.ry = h->tile_ry; tp.bmax = h->tile_ry + h->tile_ry_cap;
    hipLaunchKernelGGL(k_tile_terms, dim3((unsigned)(knn_abandon_tiles(h->ntotal) - tp.tile0)), dim3(256), 0, st, tp);
    if (hipGetLastError() == hipSuccess) h->ab_rows = h->ntotal;
}

// store statistics (max |y|, max |y - yh|) and, when wanted, the f16 hi plane, brought up to date with the rows
// (appends only touch the new rows).  Returns false when the plane was wanted but is not available.
static bool knn_ensure_hi(radad_knn_t h, hipStream_t st, bool want_plane) {
    if (!h->stat) {
        if (hipMalloc(&h->stat, 4 * sizeof(unsigned)) != hipSuccess) { (void)hipGetLastError(); return false; }
        (void)hipMemsetAsync(h->stat, 0, 4 * sizeof(unsigned), st);
        h->stat_rows = 0;
    }
    const bool plane = want_plane && !h->hi_off && !h->f16 && h->dim % 64 == 0;
    if (plane && h->tune.plane_rebuild_due(h->hi && h->hi_cap == h->capacity, h->ntotal)) {
        (void)hipDeviceSynchronize();
        knn_drop_plane(h);
        h->tune.plane_dropped_for_rebuild();
    }
    if (plane) h->tune.plane_wanted();
    const bool fresh = plane && (h->hi_cap != h->capacity || !h->hi);
    if (fresh) {
        (void)hipDeviceSynchronize();
        knn_drop_plane(h);
        h->tune.plane_is_new();                          // the next large search looks at its certificate before the exact pass
        const bool centred = knn_choose_centre(h, st);
        // One scale for the whole plane when the rows are of one magnitude (the largest row maximum within 2^6 of the smallest over
        // the rows the store holds now: clip embeddings are; rows scaled over 2^22, as a test does, are not): the scan then needs
        // no per-score arithmetic.  2^e puts the largest element in [2^12, 2^13): a later row up to 8x larger still fits f16, beyond
        // that it saturates and its (measured) residual rejects queries.  Un-centred cosine rows have |x| <= 1: e = 14 as before.
        if (h->metric != RADAD_METRIC_COSINE || centred) {
            unsigned* mm = nullptr;
            unsigned host[2] = {0u, 0x7f800000u};
            const int64_t m = std::min<int64_t>(h->ntotal, KM_MAX_ROWS);
            if (m > 0 && hipMalloc(&mm, 2 * sizeof(unsigned)) == hipSuccess) {
                (void)hipMemcpyAsync(mm, host, sizeof(host), hipMemcpyHostToDevice, st);
                hipLaunchKernelGGL(k_absmax, dim3((unsigned)ceil_div64(m, 4)), dim3(256), 0, st, (const float*)h->rows, (const float*)h->cmu, m,
                                   std::max<int64_t>(1, h->ntotal / m), h->dim, mm);
                if (hipMemcpyAsync(host, mm, sizeof(host), hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess) {
                    float mx, mn;
                    memcpy(&mx, &host[0], 4); memcpy(&mn, &host[1], 4);
                    if (mx > 0.f && mx < INFINITY && mn > 0.f && mx <= mn * 64.f) {
                        int fe;
                        (void)frexpf(mx, &fe);
                        h->uniform_e = std::max(-100, std::min(100, 13 - fe));
                    }
                }
                (void)hipFree(mm);
            }
            (void)hipGetLastError();
        }
        const bool per_row = (h->metric != RADAD_METRIC_COSINE || centred) && h->uniform_e == HI_E_PER_ROW;
        if (hipMalloc(&h->hi, (size_t)h->capacity * h->dim * 2) != hipSuccess ||
            (per_row && hipMalloc(&h->rscale, (size_t)h->capacity * sizeof(float)) != hipSuccess) ||
            (centred && hipMalloc(&h->rbias, (size_t)h->capacity * sizeof(float)) != hipSuccess)) {
            (void)hipGetLastError();
            knn_drop_plane(h);
            h->hi_off = 1;              // no room for the plane: stay on the fp32 kernels
        } else {
            h->hi_cap = h->capacity;
        }
        // the statistics describe the operands of the plane (y - mu when centred): start them over with it
        (void)hipMemsetAsync(h->stat, 0, 4 * sizeof(unsigned), st);
        h->stat_rows = 0;
    }
    const bool have_plane = plane && h->hi;
    const int64_t from = have_plane ? std::min(h->hi_rows, h->stat_rows) : h->stat_rows;
    if (from < h->ntotal) {
        HiRowsParams hp;
        hp.in = h->rows + (size_t)from * h->row_bytes(); hp.in_f16 = h->f16;
        hp.hi = have_plane ? h->hi + (size_t)from * h->dim : nullptr;
        hp.scale_out = (have_plane && h->rscale) ? h->rscale + from : nullptr;
        hp.stat_max = h->stat;
        hp.n = h->ntotal - from; hp.dim = h->dim;
        // un-centred cosine rows have |x| <= 1: one scale for the whole store (no per-score arithmetic in the scan);
        // an fp16 store is its own plane: statistics only, un-scaled
        hp.fixed_e = h->f16 ? 0 : ((h->metric == RADAD_METRIC_COSINE && !h->cmu) ? 14 : h->uniform_e);
        hp.l2 = h->metric == RADAD_METRIC_L2 ? 1 : 0; hp.exact_ops = h->f16 ? 1 : 0;
        // (a plane that exists keeps its centring for the statistics-only calls too: the statistics are those of ITS operands)
        hp.mu = h->cmu; hp.mu_norm = h->mu_norm; hp.mu_sq = h->mu_sq;
        hp.bias_out = (have_plane && h->rbias) ? h->rbias + from : nullptr;
        hipLaunchKernelGGL(k_hi_rows, dim3((unsigned)ceil_div64(hp.n, 4)), dim3(256), 0, st, hp);
        if (hipGetLastError() != hipSuccess) return false;
        h->stat_rows = h->ntotal;
        if (have_plane) h->hi_rows = h->ntotal;
        if (have_plane) {
            // what the plane's operands measure now (only searches that follow an append come through here: one small read-back)
            float host[2] = {0.f, 0.f};
            if (hipMemcpyAsync(host, h->stat, sizeof(host), hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess) {
                if (fresh) h->tune.plane_decided(host[0], host[1], h->ntotal);
                else if (h->tune.plane_outgrown(host[0], host[1])) return knn_ensure_hi(h, st, want_plane);      // decide again, now
            } else (void)hipGetLastError();
        }
    }
    knn_ensure_tile_terms(h, st, have_plane);
    return !want_plane || have_plane || h->f16;
}

extern "C" {

int radad_knn_create(int dim, int metric, int device, int64_t id_base, radad_knn_t* out) {
    return radad_knn_create_ex(dim, metric, RADAD_STORE_F32, device, id_base, out);
}

int radad_knn_create_ex(int dim, int metric, int store_dtype, int device, int64_t id_base, radad_knn_t* out) {
    RADAD_REQUIRE(out != nullptr, "radad_knn_create: out is NULL");
    RADAD_REQUIRE(store_dtype == RADAD_STORE_F32 || store_dtype == RADAD_STORE_F16, "radad_knn_create: unsupported store dtype %d", store_dtype);
    RADAD_REQUIRE(dim > 0 && (dim % 4) == 0, "radad_knn_create: dim must be a positive multiple of 4 (got %d)", dim);
    RADAD_REQUIRE(metric >= 0 && metric <= 2, "radad_knn_create: unsupported metric %d", metric);
    int ndev = 0;
    RADAD_HIP_CHECK(hipGetDeviceCount(&ndev));
    RADAD_REQUIRE(device >= 0 && device < ndev, "radad_knn_create: device %d not in [0,%d)", device, ndev);
    radad_knn_s* h = new (std::nothrow) radad_knn_s();
    if (!h) { radad_set_error("out of host memory"); return RADAD_ENOMEM; }
    h->dim = dim; h->metric = metric; h->device = device; h->id_base = id_base; h->f16 = store_dtype == RADAD_STORE_F16;
    // RADAD_KNN_HI=0 keeps every search on the fp32 kernels (bench.py --scan f32); read once, at creation
    // defaults of the handle's options (radad_knn_set_option changes them); an environment variable of the old name overrides the
    // default for handles created from now on, announced once on stderr -- for experiments only
    { const char* e = radad_env_override("RADAD_KNN_HI", "0 keeps every search of stores created from now on off the certified f16 scan (fp32 kernels: ~8x slower scans)"); h->hi_off = (e && atoi(e) == 0) ? 1 : 0; }
    { const char* e = radad_env_override("RADAD_KNN_CENTRE", "0 never centres the f16 plane, 1 always does (default: decided per store from |mean|^2 / mean |y|^2)"); h->opt_centre = e ? atoi(e) : -1; }
    { const char* e = radad_env_override("RADAD_KNN_SMALLQ_HI", "0 makes small batches stream the fp32 rows instead of the f16 plane (twice the bytes)"); h->opt_smallq_hi = e ? atoi(e) : 1; }
    { const char* e = radad_env_override("RADAD_WIDE_MIN_Q", "smallest batch that takes the 256-query tile scan (default 17)"); h->opt_wide_min_q = e ? atoi(e) : SQ_NQ + 1; }
    {
        DeviceGuard g(device);
        if (hipHostMalloc(reinterpret_cast<void**>(&h->host_count), 24 * sizeof(int), hipHostMallocDefault) != hipSuccess ||
            hipEventCreateWithFlags(&h->ev_done, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&h->ev_begun, hipEventDisableTiming) != hipSuccess) {
            radad_set_error("radad_knn_create: pinned counter / events could not be created");
            radad_knn_destroy(h);
            return RADAD_EHIP;
        }
        memset(h->host_count, 0, 24 * sizeof(int));
        { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) h->n_cus = cus; }
        if (hipHostGetDevicePointer(reinterpret_cast<void**>(&h->host_count_dev), h->host_count, 0) != hipSuccess) {
            radad_set_error("radad_knn_create: pinned counter is not device-visible");
            radad_knn_destroy(h);
            return RADAD_EHIP;
        }
    }
    *out = h;
    return RADAD_OK;
}

int radad_knn_destroy(radad_knn_t h) {
    if (!h) return RADAD_OK;
    {
        DeviceGuard g(h->device);
        if (h->rows) (void)hipFree(h->rows);
        if (h->ynorm) (void)hipFree(h->ynorm);
        if (h->ws) (void)hipFree(h->ws);
        if (h->hi) (void)hipFree(h->hi);
        if (h->rscale) (void)hipFree(h->rscale);
        if (h->cmu) (void)hipFree(h->cmu);
        if (h->rbias) (void)hipFree(h->rbias);
        if (h->stat) (void)hipFree(h->stat);
        if (h->kacc) (void)hipFree(h->kacc);
        if (h->kflag) (void)hipFree(h->kflag);
        if (h->xarrive) (void)hipFree(h->xarrive);
        if (h->excl_ws) (void)hipFree(h->excl_ws);
        if (h->rs_key) (void)hipFree(h->rs_key);
        if (h->rs_count) (void)hipFree(h->rs_count);
        if (h->tile_ry) (void)hipFree(h->tile_ry);
        if (h->ab_ws) (void)hipFree(h->ab_ws);
        if (h->deal_cnt) (void)hipFree(h->deal_cnt);
        if (h->defer_list) (void)hipFree(h->defer_list);
        if (h->host_count) (void)hipHostFree(h->host_count);
        if (h->ev_done) (void)hipEventDestroy(h->ev_done);
        if (h->ev_begun) (void)hipEventDestroy(h->ev_begun);
        h->prof.destroy();
    }
    delete h;
    return RADAD_OK;
}

int radad_knn_dim(radad_knn_t h, int* dim) { RADAD_REQUIRE(h && dim, "NULL argument"); *dim = h->dim; return RADAD_OK; }
int radad_knn_metric(radad_knn_t h, int* metric) { RADAD_REQUIRE(h && metric, "NULL argument"); *metric = h->metric; return RADAD_OK; }
int radad_knn_ntotal(radad_knn_t h, int64_t* n) { RADAD_REQUIRE(h && n, "NULL argument"); *n = h->ntotal; return RADAD_OK; }

int radad_knn_set_option(radad_knn_t h, int option, int value) {
    RADAD_REQUIRE(h, "NULL handle");
    std::lock_guard<std::mutex> lk(h->mu);
    switch (option) {
        case RADAD_KNN_OPT_HI_PLANE:
            RADAD_REQUIRE(value == 0 || value == 1, "radad_knn_set_option: HI_PLANE takes 0 or 1");
            RADAD_REQUIRE(h->hi == nullptr || value == 1, "radad_knn_set_option: the f16 plane of this store is already built; switch it off before the first large-batch search");
            h->hi_off = value ? 0 : 1;
            return RADAD_OK;
        case RADAD_KNN_OPT_CENTRE:
            RADAD_REQUIRE(value >= -1 && value <= 1, "radad_knn_set_option: CENTRE takes -1 (decide per store), 0 or 1");
            RADAD_REQUIRE(h->hi == nullptr, "radad_knn_set_option: the f16 plane of this store is already built; choose its centring before the first large-batch search");
            h->opt_centre = value;
            return RADAD_OK;
        case RADAD_KNN_OPT_SMALLQ_HI:
            RADAD_REQUIRE(value == 0 || value == 1, "radad_knn_set_option: SMALLQ_HI takes 0 or 1");
            h->opt_smallq_hi = value;
            return RADAD_OK;
        case RADAD_KNN_OPT_WIDE_MIN_Q:
            RADAD_REQUIRE(value >= 1, "radad_knn_set_option: WIDE_MIN_Q must be >= 1");
            h->opt_wide_min_q = value;
            return RADAD_OK;
        case RADAD_KNN_OPT_DENSE:
            RADAD_REQUIRE(value == 0 || value == 1, "radad_knn_set_option: DENSE takes 0 or 1");
            h->opt_dense = value;
            return RADAD_OK;
        case RADAD_KNN_OPT_ABANDON:
            RADAD_REQUIRE(value == 0 || value == 1, "radad_knn_set_option: ABANDON takes 0 or 1");
            h->opt_abandon = value;
            return RADAD_OK;
        case RADAD_KNN_OPT_ABANDON_DEAL:
            RADAD_REQUIRE(value == 0 || value == 1, "radad_knn_set_option: ABANDON_DEAL takes 0 or 1");
            h->opt_abandon_deal = value;
            return RADAD_OK;
        case RADAD_KNN_OPT_ABANDON_DEFER:
            RADAD_REQUIRE(value == 0 || value == 1, "radad_knn_set_option: ABANDON_DEFER takes 0 or 1");
            h->opt_abandon_defer = value;
            return RADAD_OK;
        case RADAD_KNN_OPT_ABANDON_AHEAD:
            RADAD_REQUIRE(value == 0 || value == 1, "radad_knn_set_option: ABANDON_AHEAD takes 0 or 1");
            h->opt_abandon_ahead = value;
            return RADAD_OK;
        case RADAD_KNN_OPT_RANGE_SMALLQ:
            RADAD_REQUIRE(value == 0 || value == 1, "radad_knn_set_option: RANGE_SMALLQ takes 0 or 1");
            h->opt_range_smallq = value;
            return RADAD_OK;
        case RADAD_KNN_OPT_REMOVE_STAGE_ROWS:
            RADAD_REQUIRE(value >= 0, "radad_knn_set_option: REMOVE_STAGE_ROWS takes a row count, or 0 for the default");
            h->opt_remove_stage_rows = value == 0 ? 0 : (int)std::max<int64_t>(value, KNN_REMOVE_MIN_STAGE_ROWS);
            return RADAD_OK;
        default:
            radad_set_error("radad_knn_set_option: unknown option %d", option);
            return RADAD_EINVAL;
    }
}

int radad_knn_reserve(radad_knn_t h, int64_t capacity) {
    RADAD_REQUIRE(h, "NULL handle");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    RADAD_REQUIRE(!h->pending.valid && !h->pending_excl.valid, "radad_knn_reserve: a begun search (radad_knn_search_begin) must be finished or aborted before the store changes");
    if (capacity <= h->capacity) return RADAD_OK;
    RADAD_HIP_CHECK(hipDeviceSynchronize());
    return knn_realloc(h, capacity);
}

int radad_knn_add(radad_knn_t h, const float* rows_dev, int64_t n, void* stream) {
    RADAD_REQUIRE(h, "NULL handle");
    RADAD_REQUIRE(n >= 0, "radad_knn_add: n < 0");
    if (n == 0) return RADAD_OK;
    RADAD_REQUIRE(rows_dev, "radad_knn_add: rows is NULL");
    RADAD_REQUIRE(h->ntotal + n < (int64_t)IDX_SENTINEL, "radad_knn_add: more than 2^31-2 rows per store (shard it)");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    // (the second half of a begun search reads rows / ntotal live while its candidate ids date from the first half)
    RADAD_REQUIRE(!h->pending.valid && !h->pending_excl.valid, "radad_knn_add: a begun search (radad_knn_search_begin) must be finished or aborted before the store changes");
    hipStream_t st = (hipStream_t)stream;
    if (h->ntotal + n > h->capacity) {
        RADAD_HIP_CHECK(hipStreamSynchronize(st));   // the old buffers may still be in use on `st`
        int rc = knn_grow(h, h->ntotal + n);
        if (rc) return rc;
    }
    const int mode = h->metric == RADAD_METRIC_COSINE ? 2 : (h->metric == RADAD_METRIC_L2 ? 1 : 0);
    char* dst = h->rows + (size_t)h->ntotal * h->row_bytes();
    float* yn = h->ynorm ? h->ynorm + h->ntotal : nullptr;
    const unsigned grid = (unsigned)ceil_div64(n, 4);
    if (h->f16) hipLaunchKernelGGL(k_rows_prepare<_Float16>, dim3(grid), dim3(256), 0, st, rows_dev, (_Float16*)dst, yn, n, h->dim, mode);
    else hipLaunchKernelGGL(k_rows_prepare<float>, dim3(grid), dim3(256), 0, st, rows_dev, (float*)dst, yn, n, h->dim, mode);
    RADAD_HIP_CHECK(hipGetLastError());
    h->ntotal += n;
    return RADAD_OK;
}

int radad_knn_add_host(radad_knn_t h, const float* rows_host, int64_t n) {
    RADAD_REQUIRE(h, "NULL handle");
    if (n == 0) return RADAD_OK;
    RADAD_REQUIRE(rows_host && n > 0, "radad_knn_add_host: bad rows/n");
    float* tmp = nullptr;
    {
        DeviceGuard g(h->device);
        const size_t bytes = (size_t)n * h->dim * sizeof(float);
        if (hipMalloc(&tmp, bytes) != hipSuccess) { radad_set_error("hipMalloc of staging buffer failed"); return RADAD_ENOMEM; }
        hipError_t e = hipMemcpy(tmp, rows_host, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(tmp); radad_set_error("H2D copy failed: %s", hipGetErrorString(e)); return RADAD_EHIP; }
    }
    int rc = radad_knn_add(h, tmp, n, nullptr);
    {
        DeviceGuard g(h->device);
        hipError_t e = hipStreamSynchronize(nullptr);
        (void)hipFree(tmp);
        if (rc == RADAD_OK && e != hipSuccess) { radad_set_error("add failed: %s", hipGetErrorString(e)); rc = RADAD_EHIP; }
    }
    return rc;
}

int radad_knn_search(radad_knn_t h, const float* q_dev, int64_t nq, int k, float* out_dist_dev, int64_t* out_idx_dev,
                     void* stream) {
    return radad_knn_search_f64(h, q_dev, nq, k, out_dist_dev, out_idx_dev, nullptr, stream);
}

static int knn_search_core(radad_knn_t h, const void* q_dev, int q_dtype, int64_t nq, int k, int margin, float* out_dist_dev,
                           int64_t* out_idx_dev, double* out_key_dev, void* stream);

int radad_knn_search_f64(radad_knn_t h, const float* q_dev, int64_t nq, int k, float* out_dist_dev, int64_t* out_idx_dev,
                         double* out_key_dev, void* stream) {
    return knn_search_core(h, q_dev, RADAD_Q_F32, nq, k, KNN_MARGIN, out_dist_dev, out_idx_dev, out_key_dev, stream);
}

int radad_knn_search_ex(radad_knn_t h, const void* q_dev, int q_dtype, int64_t nq, int k, float* out_dist_dev,
                        int64_t* out_idx_dev, double* out_key_dev, void* stream) {
    RADAD_REQUIRE(q_dtype == RADAD_Q_F32 || q_dtype == RADAD_Q_BF16, "radad_knn_search_ex: unsupported query dtype %d", q_dtype);
    return knn_search_core(h, q_dev, q_dtype, nq, k, KNN_MARGIN, out_dist_dev, out_idx_dev, out_key_dev, stream);
}

}  // extern "C"

__global__ __launch_bounds__(256) void k_fill_f32(float* __restrict__ out, int64_t n, float v) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = v;
}

// bf16 -> fp32 (exact): queries handed over as bfloat16 (BASELINE config 5) are decoded once, then take the fp32 path
__global__ __launch_bounds__(256) void k_bf16_to_f32(const unsigned short* __restrict__ in, float* __restrict__ out, int64_t n) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
    const u16x4 b = *reinterpret_cast<const u16x4*>(in + i);
    *reinterpret_cast<f32x4*>(out + i) = f32x4{__uint_as_float((unsigned)b[0] << 16), __uint_as_float((unsigned)b[1] << 16),
                                               __uint_as_float((unsigned)b[2] << 16), __uint_as_float((unsigned)b[3] << 16)};
}

template <typename T>
static inline T* ws_at(radad_knn_t h, size_t off) { return reinterpret_cast<T*>((char*)h->ws + off); }

// K split of the tile scan over two workgroups per tile: when a launch has one tile per workgroup, at most 128 workgroups (half the
// chip) and at least 16 K steps (dim >= 1024) -- the reference's own store, 25 423 x 5376: 100 tiles of 84 K steps.  Returns 1 or 2 and
// makes sure the scratch exists (allocated once per handle; the counters start, and are left, at zero).
static int knn_tile_ksplit(radad_knn_t h, int qtiles_grid, int n_splits, int64_t chunk_rows, int64_t rows, hipStream_t st) {
    const int64_t tiles = ceil_div64(rows, KW_M);
    if (chunk_rows != KW_M || (int64_t)qtiles_grid * n_splits > 128 || h->dim * 2 / 128 < 16) return 1;
    const int64_t need = tiles * qtiles_grid;
    if ((size_t)need * 2 * 32 * KW_THREADS * sizeof(f32x4) > ((size_t)256 << 20)) return 1;      // (a spread sample over a large store: not worth 0.5 MB per tile)
    if (need > h->kacc_tiles) {
        (void)hipStreamSynchronize(st);
        if (h->kacc) (void)hipFree(h->kacc);
        if (h->kflag) (void)hipFree(h->kflag);
        h->kacc = nullptr; h->kflag = nullptr; h->kacc_tiles = 0;
        if (hipMalloc(&h->kacc, (size_t)need * 2 * 32 * KW_THREADS * sizeof(f32x4)) != hipSuccess ||
            hipMalloc(&h->kflag, (size_t)need * sizeof(int)) != hipSuccess || hipMemset(h->kflag, 0, (size_t)need * sizeof(int)) != hipSuccess) {
            (void)hipGetLastError();
            if (h->kacc) (void)hipFree(h->kacc);
            if (h->kflag) (void)hipFree(h->kflag);
            h->kacc = nullptr; h->kflag = nullptr;
            return 1;                                   // no room: the un-split launch is always possible
        }
        h->kacc_tiles = need;
    }
    return 2;
}

// The search proper.  `margin` spare entries per (query, chunk) list on the fp32 tile kernels (KNN_MARGIN for user
// searches; the IVF coarse quantiser asks for fewer so that nprobe = 32 still fits the 32-entry register lists).
//
// Scan (a filter), one of:
//   certified f16 tile scan (knn_hi.inc)   batches > 16 queries (or small batches too wide for the streaming kernel's LDS) on
//                                     stores of >= 16384 rows, k <= 128: hi plane of an fp32 store or the fp16 store itself; emits
//                                     every row at or above the query's admission floor into the query's candidate buffer
//   k_knn_hi_smallq / k_knn_f32_smallq     <= 16 queries: HBM-bound streaming of the f16 plane / the fp32 rows
//   k_knn_f32_reg / k_knn_f32         the fp32 (or fp16-operand) tile kernels, lists of k + margin
// then k_merge_refine: float64 re-rank of every candidate within 2 eps of the k-th, per-query certificate; then the
// exact float64 kernel for the queries the certificate rejected (device-driven, usually zero work).  Nothing in here
// synchronises with the host unless the workspace has to grow.
//
// Two halves around an optional exchange (radad_knn_search_begin / _finish, for row-sharded stores): phase 1 prepares the queries
// and scans, and can report per query a lower bound of the exact k-th best score of THIS store; phase 2 re-ranks -- with the
// maximum of the shards' bounds, only what can still be among the global k best -- and runs the exact kernel.

// the most recent search's device work is complete (its statistics are in the pinned host copy)
static hipError_t knn_wait_last_search(radad_knn_t h) {
    if (!h->have_last) return hipSuccess;
    if (hipStreamSynchronize(h->last_stream) == hipSuccess) return hipSuccess;
    (void)hipGetLastError();                            // (the stream is gone: everything on the device, then)
    return hipDeviceSynchronize();
}

// how the certificates of earlier searches fared: any report that has arrived and was not looked at yet (KnnTuning decides what
// follows from it); this search takes over slot tune.slot().  The volatile reads, the fences and the re-check of the stamp are the
// synchronisation with the device's writes.
// (until round 4 an event behind every search was waited for here: an event record between dependent kernels costs the stream ~6 us,
// a tenth of an online search.  The exact kernel stamps its report; one that has not arrived yet is simply not looked at.)
static void knn_consume_reports(radad_knn_t h) {
    for (int sl = 0; sl < 2; ++sl) {
        volatile int* rep = reinterpret_cast<volatile int*>(h->host_count + 8 * sl);
        const int stamp = rep[6];
        if (!h->tune.report_is_new(sl, stamp)) continue;
        std::atomic_thread_fence(std::memory_order_acquire);
        const int rejected = rep[0], rep_nq = rep[7];
        std::atomic_thread_fence(std::memory_order_acquire);
        if (rep[6] != stamp) continue;                    // the device is rewriting the slot right now: next search
        h->tune.consume_report(sl, stamp, rejected, rep_nq, h->tune.appended_since_plane(h->hi != nullptr, h->ntotal));
    }
}

static StoreFacts knn_store_facts(radad_knn_t h) {
    StoreFacts s;
    s.ntotal = h->ntotal; s.dim = h->dim; s.metric = h->metric; s.f16 = h->f16; s.hi_off = h->hi_off;
    s.opt_centre = h->opt_centre; s.opt_smallq_hi = h->opt_smallq_hi; s.opt_wide_min_q = h->opt_wide_min_q; s.opt_dense = h->opt_dense;
    s.cap_boost = h->tune.cap_boost;
    s.opt_range_smallq = h->opt_range_smallq;
    return s;
}

// The choice of the scan: the plan itself is knn_plan.h's (pure); here are its side effects, in this order and under these conditions
// on purpose -- the tuning state counts a skipped turn, the plane is built (knn_ensure_hi) -- the next searches of the handle see them.
static int knn_plan_scan(radad_knn_t h, int64_t nq, int k, int margin, hipStream_t st, ScanPlan* out) {
    bool use_hi = false, skipped_hi = false, smallq_hi = false;
    const TileEligibility t = knn_tile_eligibility(knn_store_facts(h), nq, k, margin);
    if (t.eligible) {
        if (!h->tune.take_tile_turn()) skipped_hi = true;
        else use_hi = knn_ensure_hi(h, st, true);
    }
    if (!use_hi && !knn_ensure_hi(h, st, false)) { radad_set_error("store statistics could not be computed"); return RADAD_EHIP; }
    // (the facts again: a plane that could not be allocated has switched itself off)
    if (knn_smallq_hi_eligible(knn_store_facts(h), nq, k, margin, use_hi, skipped_hi) && h->tune.take_smallq_turn())
        smallq_hi = knn_ensure_hi(h, st, true);
    ScanPlan p = knn_finish_plan(knn_store_facts(h), nq, k, margin, t, use_hi, smallq_hi);
    p.mu = (p.hi_q && !h->f16) ? h->cmu : nullptr;
    p.biased = p.hi_q && (p.l2 || p.mu);
    h->last_qtiles = p.reported_qtiles;
    h->last_threads = p.block_threads;
    h->last_kind = p.kind;
    *out = p;
    return RADAD_OK;
}

// the store's per-tile suffix norms are current and the handle's buffer holds the per-query terms of nq queries (grown here: a
// synchronising allocation the first time a batch size is seen); false = this search's launches run the plain scan
static bool knn_abandon_terms_ready(radad_knn_t h, int64_t nq) {
    if (!h->opt_abandon || !h->tile_ry || h->ab_rows != h->ntotal || h->ab_from <= 0 || h->ab_from != knn_abandon_suffix_from(h->dim)) return false;
    const AbandonLayout A = knn_abandon_layout(nq);
    if (A.bytes > h->ab_ws_bytes) {
        if (hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); return false; }
        if (h->ab_ws) (void)hipFree(h->ab_ws);
        h->ab_ws = nullptr; h->ab_ws_bytes = 0;
        if (hipMalloc(&h->ab_ws, A.bytes) != hipSuccess) { (void)hipGetLastError(); return false; }
        h->ab_ws_bytes = A.bytes;
    }
    // (the ticket counters of dealt launches: without them the launches stay static)
    if ((h->opt_abandon_deal || h->opt_abandon_defer || h->opt_abandon_ahead) && !h->deal_cnt && hipMalloc(&h->deal_cnt, KNN_DEAL_COUNTERS * sizeof(int)) != hipSuccess) { (void)hipGetLastError(); h->deal_cnt = nullptr; }
    // the deferral's lists: one per query tile, each as long as a launch over the whole store could fill (without them nothing defers)
    if (h->opt_abandon_defer && h->deal_cnt && h->defer_list_cap < knn_defer_list_cap(h->ntotal)) {
        (void)hipDeviceSynchronize();
        if (h->defer_list) (void)hipFree(h->defer_list);
        h->defer_list = nullptr; h->defer_list_cap = 0;
        const int64_t cap = knn_defer_list_cap(h->capacity > h->ntotal ? h->capacity : h->ntotal);
        if (hipMalloc(&h->defer_list, (size_t)KNN_DEFER_MAX_QTILES * cap * sizeof(int)) == hipSuccess) h->defer_list_cap = cap;
        else { (void)hipGetLastError(); h->defer_list = nullptr; }
    }
    return true;
}

// ---- queries: decode, normalise, round (+ scale) to f16, error bound.  Returns the fp32 queries the scan and the re-rank read.
static const float* knn_prepare_queries(radad_knn_t h, const ScanPlan& p, const SearchLayout& L, const void* q_in, int q_dtype, hipStream_t st) {
    const int64_t nq = p.nq;
    const float* q_use = (const float*)q_in;
    if (q_dtype == RADAD_Q_BF16) {
        float* qf = ws_at<float>(h, L.qf);
        const int64_t ne = nq * h->dim;
        hipLaunchKernelGGL(k_bf16_to_f32, dim3((unsigned)ceil_div64(ne, 1024)), dim3(256), 0, st, (const unsigned short*)q_in, qf, ne);
        q_use = qf;
    }
    const bool cosine = h->metric == RADAD_METRIC_COSINE;
    // k_hi_rows prepares the queries of every search: normalisation (cosine), f16 copy, error bound eps, cleared flags and counters
    // (|q|^2 is not needed: ranking uses 2 q.y - |y|^2 and the reported distance is re-scored exactly)
    {
        const bool f16_tile = p.kind == RADAD_SCAN_F16_TILE;
        HiRowsParams hp;
        hp.in = q_use;
        hp.hi = p.f16_queries() ? ws_at<_Float16>(h, L.qh) : nullptr;
        hp.scale_out = p.hi_q ? ws_at<float>(h, L.qscale) : nullptr;
        hp.eps_out = ws_at<float>(h, L.eps); hp.ystat = h->stat;
        hp.n = nq; hp.dim = h->dim;
        hp.fixed_e = p.hi_q ? HI_E_PER_ROW : 0;          // the fp16 tile kernel multiplies un-scaled fp16 queries
        hp.l2 = p.l2; hp.exact_ops = p.f16_queries() ? 0 : 1;
        hp.norm_out = cosine ? ws_at<float>(h, L.qn) : nullptr;
        hp.zero_flags = ws_at<int>(h, L.cnt); hp.zero_counters = ws_at<int>(h, L.fcount);
        hp.mu = p.mu; hp.mu_norm = p.mu ? h->mu_norm : 0.f; hp.mu_sq = p.mu ? h->mu_sq : 0.f; hp.biased = (p.biased || (f16_tile && p.l2)) ? 1 : 0;
        hp.qconst_out = p.biased ? ws_at<float>(h, L.qconst) : nullptr;
        hp.zero_ab = ws_at<int>(h, L.fcount) + KNN_AB_COUNTER0;
        h->ab_search_ready = p.kind == RADAD_SCAN_HI_TILE && knn_abandon_terms_ready(h, nq);
        if (h->ab_search_ready) {       // the abandon's per-query terms
            const AbandonLayout A = knn_abandon_layout(nq);
            hp.suf_from = h->ab_from;
            hp.suf_out = reinterpret_cast<float*>(static_cast<char*>(h->ab_ws) + A.rq);
            hp.ab_slack_out = reinterpret_cast<float*>(static_cast<char*>(h->ab_ws) + A.slack);
            hp.zero_deal = (h->opt_abandon_deal || h->opt_abandon_defer || h->opt_abandon_ahead) ? h->deal_cnt : nullptr;         // every launch's ticket counters, once per search, in a kernel the search runs anyway
        }
        launch_hi_rows(hp, st);
    }
    return cosine ? ws_at<const float>(h, L.qn) : q_use;
}

// ---- the certified f16 tile scan (knn_hi.inc) -------------------------------------------------------------------------------------
// (its phases -- row boundaries, one launch each -- are knn_hi_phases, knn_plan.h)
// the tile scan's kernel for one RSC (knn_hi.inc), the sample pre-pass's or the scan's own
static auto knn_hi_kernel(int rsc, bool sample, bool abandon = false) -> void (*)(KnnHiParams) {
    if (abandon) return rsc == 0 ? k_knn_hi_abandon<0> : k_knn_hi_abandon<3>;       // (knn_abandon_launch: RSC 0 and 3, never the sample)
    switch (rsc) {
        case 0: return sample ? k_knn_hi_sample<0> : k_knn_hi<0>;
        case 1: return sample ? k_knn_hi_sample<1> : k_knn_hi<1>;
        case 2: return sample ? k_knn_hi_sample<2> : k_knn_hi<2>;
        default: return sample ? k_knn_hi_sample<3> : k_knn_hi<3>;
    }
}

// ---- per-query exclusion sets on the tile scan (radad_knn_search_excl_scan_pq): the scrub ---------------------------------------------
// The scan cannot test a per-(row, query) rule, and does not have to: every floor it runs with is computed BETWEEN its launches by
// k_floor_from_sample / k_kth_floor from (score, row) entries in buffers, and the result by k_merge_refine<true> from the same
// buffers.  This kernel clears a query's excluded entries out of such a buffer in front of each of those readers: row = IDX_SENTINEL
// AND score = -inf (k_kth_floor reads scores only).  One workgroup per query; the query's <= 64 live tags sit in LDS; every thread
// walks entries i, i + 256, ... of the first min(count, cap) (cnt NULL: all cap -- the sample's lists), loads the tag of each entry
// that is not a hole already and compares it with the tags.  Idempotent: a cleared entry is a hole the next launch skips.  The
// counters are not touched: overflow stays "the scan emitted more than the buffer holds", excluded rows included.  A query with no
// live tag leaves at once.  Plain C++ stores.
struct ExclScrubParams {
    float* score = nullptr;             // [nq][cap]
    int* idx = nullptr;                 // [nq][cap] rows of the store, IDX_SENTINEL = no entry
    const int* cnt = nullptr;           // [nq] entries emitted (may exceed cap), or NULL = every buffer holds cap entries
    int cap = 0;
    const int64_t* tags = nullptr;      // [ntotal] row tags
    int64_t ntotal = 0;
    const int64_t* q_tags = nullptr;    // [nq, m]
    const int* q_cnt = nullptr;         // [nq] or NULL = m
    int m = 0;
};
static_assert(std::is_trivially_copyable_v<ExclScrubParams>, "kernel argument");
__global__ __launch_bounds__(256) void k_excl_pq_scrub(ExclScrubParams p) {
    __shared__ int64_t s_tag[RADAD_EXCL_PQ_MAX_TAGS];
    const int64_t q = blockIdx.x;
    const int cnt = min(max(p.q_cnt ? p.q_cnt[q] : p.m, 0), min(p.m, RADAD_EXCL_PQ_MAX_TAGS));
    if (cnt == 0) return;                                       // (workgroup-uniform)
    if ((int)threadIdx.x < cnt) s_tag[threadIdx.x] = p.q_tags[q * p.m + threadIdx.x];
    __syncthreads();
    const int ne = p.cnt ? min(max(p.cnt[q], 0), p.cap) : p.cap;
    float* sc = p.score + q * p.cap;
    int* id = p.idx + q * p.cap;
    for (int i = threadIdx.x; i < ne; i += 256) {
        const int row = id[i];
        if (row == IDX_SENTINEL || row < 0 || row >= p.ntotal) continue;
        const int64_t t = p.tags[row];
        bool excluded = false;
        for (int e = 0; e < cnt; ++e) excluded |= s_tag[e] == t;
        if (excluded) { id[i] = IDX_SENTINEL; sc[i] = -INFINITY; }
    }
}

// what radad_knn_search_excl_scan_pq hands to the tile scan: the rule to scrub with, the grid its planner gave, and (out) the launches made
struct ScanScrub {
    const ExclRule* rule = nullptr;
    int64_t grid = 0;
    int launched = 0;
};
static void knn_launch_scrub(radad_knn_t h, ScanScrub* s, float* score, int* idx, const int* cnt, int cap, hipStream_t st) {
    ExclScrubParams x;
    x.score = score; x.idx = idx; x.cnt = cnt; x.cap = cap;
    x.tags = s->rule->tags; x.ntotal = h->ntotal; x.q_tags = s->rule->q_tags; x.q_cnt = s->rule->q_cnt; x.m = s->rule->m();
    hipLaunchKernelGGL(k_excl_pq_scrub, dim3((unsigned)s->grid), dim3(256), 0, st, x);
    ++s->launched;
}

// row_bias: the bias array of a biased plan (p.biased), or NULL = the handle's own (radad_knn_search_excl_scan hands in its per-call
// array: NaN for the rows it excludes)
// scrub: NULL (every search but radad_knn_search_excl_scan_pq: nothing below changes), or the per-query rule -- k_excl_pq_scrub then
// runs on the sample's entries before k_floor_from_sample, on the candidate buffers before every k_kth_floor, and once more behind
// the last launch, so that whoever reads the buffers next (the re-rank) finds them scrubbed
// floors: NULL (every search but radad_knn_range_search: nothing below changes), or [nq] admission floors the caller has computed
// (k_range_floor; the search's own floor array, L.thr, so that radad_knn_last_emitted reports them): no floor is derived from rows
// then -- no sample pre-pass, no k_floor_from_sample, no k_kth_floor -- and the store is ONE launch (nothing changes between
// launches, so there is nothing to phase).  The launch takes the ABANDON instantiation by the same rule (knn_abandon_launch): the
// abandon compares the scan's own partial sums with the floor the emit uses, whatever that floor was derived from.
static int knn_scan_hi_tile(radad_knn_t h, const ScanPlan& p, const SearchLayout& L, hipStream_t st, const float* row_bias = nullptr,
                            ScanScrub* scrub = nullptr, const float* floors = nullptr) {
    const int64_t nq = p.nq;
    float* ps = ws_at<float>(h, L.ps);
    int* pi = ws_at<int>(h, L.pi);
    float* eps = ws_at<float>(h, L.eps);
    float* thr_init = ws_at<float>(h, L.thr);
    KnnHiParams wp;
    wp.db = h->f16 ? (const void*)h->rows : (const void*)h->hi;
    wp.rscale = h->f16 ? nullptr : h->rscale;
    wp.uscale = h->f16 ? 1.0f : (h->uniform_e != HI_E_PER_ROW ? ldexpf(1.0f, -h->uniform_e) : (h->metric == RADAD_METRIC_COSINE ? 0x1p-14f : 1.0f));
    // bias of the scale + bias variant: a centred plane has its own (|y - mu|^2 or mu.y); un-centred L2 uses |y|^2 as stored
    wp.rbias = row_bias ? row_bias : (p.mu ? h->rbias : h->ynorm); wp.bias_sign = p.l2 ? -1.f : 1.f; wp.mult = p.l2 ? 2.f : 1.f;
    wp.qconst = p.biased ? ws_at<float>(h, L.qconst) : nullptr;
    wp.q = ws_at<_Float16>(h, L.qh); wp.qscale = ws_at<float>(h, L.qscale);
    wp.n = h->ntotal; wp.nq = (int)nq; wp.row_bytes = h->dim * 2; wp.l2 = p.l2;
    wp.n_qtiles = p.n_qtiles; wp.part_score = ps; wp.part_idx = pi;
    wp.cand_cap = p.emit_cap; wp.cand_cnt = ws_at<int>(h, L.cnt);
#ifdef RADAD_DEBUG_HOOKS        // timing experiments only (make exp); never in the shipped library
    { const char* dbg = getenv("RADAD_DEBUG_KNN"); wp.debug = dbg ? atoi(dbg) : 0; }
    {   // RADAD_KNN_STAMPS=<file>: in-kernel s_memtime stamps of the 8 waves of workgroup 0, dumped after the scan (synchronises)
        static unsigned long long* stamp_buf = nullptr;
        if (getenv("RADAD_KNN_STAMPS")) {
            if (!stamp_buf) (void)hipMalloc(&stamp_buf, 8 * 4096 * 8);
            (void)hipMemsetAsync(stamp_buf, 0, 8 * 4096 * 8, st);
            wp.stamps = stamp_buf;
        }
    }
#endif
    const int rsc = p.biased ? (wp.rscale ? 2 : 3) : (wp.rscale ? 1 : 0);
    const auto scan = knn_hi_kernel(rsc, false), sample = knn_hi_kernel(rsc, true);
    const size_t lds = knn_hi_lds_bytes();
    // early abandon: the launches that qualify (knn_abandon_launch) take the ABANDON instantiation, with the store's per-tile and the
    // search's per-query suffix norms (knn_prepare_queries wrote the latter and says so: ab_search_ready)
    AbandonFacts af;
    af.opt_abandon = h->opt_abandon; af.rsc = rsc; af.floors = true; af.per_call_bias = row_bias != nullptr; af.dim = h->dim;
    af.terms_current = h->ab_search_ready;
    const AbandonLayout AL = knn_abandon_layout(nq);
    h->last_ab_tasks = 0; h->last_o_ab = L.fcount + KNN_AB_COUNTER0 * sizeof(int);
    h->last_deal_launches = h->last_deal_workgroups = h->last_deal_granule = 0;
    h->last_defer_launches = 0; h->last_defer_sets = 0;
    h->last_ahead_sets = 0;
    RADAD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(scan), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    RADAD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(sample), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // sample pre-pass: the (k + margin)-th best score over the first rows of the store is a score at least k rows reach, so the
    // scan admits from it (minus 2 eps) instead of -inf (the score of a (row, query) pair does not depend on the tiling).
    // Its lists live behind the candidate buffers.
    if (floors) wp.thr_init = floors;
    else {
        KnnHiParams sp = wp;
        // The sample's tiles are SPREAD over the store (every (tiles / s_splits)-th one).  The first s_splits tiles, as until round 4,
        // are a sample of the store only while its rows are in random order: on a store whose rows arrive cluster by cluster
        // (add_vectors_batch appends 10 000 rows at a time, vector_database.py:134-138) a query of the LAST cluster got a floor
        // from rows of the first -- so loose that every row of its own cluster passed it, the candidate buffer overflowed and the
        // certificate rejected all 256 queries of a batch (tests/test_gpu_reference_shapes.py::test_a_store_that_drifts...).
        sp.n_splits = p.s_splits; sp.chunk_rows = KW_M;
        sp.part_score = ps + L.cand_elems; sp.part_idx = pi + L.cand_elems;
        sp.chunk_stride = knn_hi_sample_stride(h->ntotal, p.s_splits);
        const int sq_grid = knn_hi_qtile_grid(sp.n_qtiles);
        // (the K split's scratch is indexed by row0 / KW_M: the sample's tiles lie anywhere in the store)
        sp.ksplit = knn_tile_ksplit(h, sq_grid, sp.n_splits, KW_M, h->ntotal, st);
        sp.kacc = h->kacc; sp.kflag = h->kflag;
        hipLaunchKernelGGL(sample, dim3((unsigned)(sq_grid * sp.n_splits * sp.ksplit)), dim3(KW_THREADS), lds, st, sp);
        const int n_ent = sp.n_splits * KW_SAMPLE_LIST;
        if (scrub) knn_launch_scrub(h, scrub, sp.part_score, sp.part_idx, nullptr, n_ent, st);
        hipLaunchKernelGGL(k_floor_from_sample, dim3((unsigned)nq), dim3(RF_THREADS), (size_t)n_ent * 4 + 1040, st, (const float*)sp.part_score,
                           (const int*)sp.part_idx, n_ent, p.ksel, (const float*)eps, thr_init);
        wp.thr_init = thr_init;
    }
    const std::vector<int64_t> r = knn_hi_phases(h->ntotal, nq, (int64_t)8 * p.s_splits * KW_M, floors ? true : knn_hi_one_go(p, h->ntotal));
    h->last_scan_launches = h->last_scan_phases = (int)r.size() - 1;
    for (size_t i = 0; i + 1 < r.size(); ++i) {       // rows [r0, r1) of the store, one full round (or two) of workgroups
        const int64_t r0 = r[i], r1 = r[i + 1];
        if (r0 > 0) {
            if (scrub) knn_launch_scrub(h, scrub, ps, pi, wp.cand_cnt, p.emit_cap, st);
            KthParams kp;
            kp.score = ps; kp.cnt = wp.cand_cnt; kp.cap = p.emit_cap; kp.k = p.k; kp.eps = eps; kp.floor_io = thr_init;
            hipLaunchKernelGGL(k_kth_floor, dim3((unsigned)nq), dim3(RF_THREADS), (size_t)p.emit_cap * 4 + 1040, st, kp);
        }
        KnnHiParams rp = wp;
        rp.db = (const char*)wp.db + (size_t)r0 * wp.row_bytes;
        rp.rscale = wp.rscale ? wp.rscale + r0 : nullptr;
        rp.rbias = wp.rbias ? wp.rbias + r0 : nullptr;
        rp.n = r1 - r0; rp.id_off = r0;
        rp.loose_floor = (r0 == 0 && r1 == h->ntotal && p.s_splits < KW_SAMPLE_SPLITS) ? 1 : 0;      // one launch behind a small sample
        // (the counting form for the FIRST phase of a large store -- its floor is the sample's, ~64 candidates per tile -- was measured
        // too: 0.883-0.887 against 0.874-0.877 ms per search, three alternations on one box, profiles/r5_ab_counting_emit_phase0.txt: no)
        int gq, gs; int64_t gc;
        knn_geometry_wide(rp.n, nq, &gq, &gs, &gc);
        rp.n_splits = gs; rp.chunk_rows = gc; rp.chunk_stride = gc;
        h->last_splits = gs;
        const int gq_grid = knn_hi_qtile_grid(gq);
        rp.ksplit = knn_tile_ksplit(h, gq_grid, gs, gc, rp.n, st);
        rp.kacc = h->kacc; rp.kflag = h->kflag;
        af.ksplit = rp.ksplit;
        const int ab_ck = knn_abandon_launch(af);
        auto launch_fn = scan;
        size_t launch_lds = lds;
        if (ab_ck > 0) {
            rp.ab_ck = ab_ck;
            rp.ab_rq = reinterpret_cast<const float*>(static_cast<const char*>(h->ab_ws) + AL.rq);
            rp.ab_slack = reinterpret_cast<const float*>(static_cast<const char*>(h->ab_ws) + AL.slack);
            rp.ab_ry = h->tile_ry + r0 / KW_M;          // (phases begin on tile boundaries: knn_hi_phases)
            rp.ab_b = h->tile_ry + h->tile_ry_cap + r0 / KW_M;
            rp.ab_count = ws_at<int>(h, L.fcount) + KNN_AB_COUNTER0;
            launch_fn = knn_hi_kernel(rsc, false, true);
            launch_lds = knn_hi_lds_bytes(true);
            RADAD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(launch_fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)launch_lds));
            h->last_ab_tasks += (int64_t)gq * ceil_div64(rp.n, KW_M);
            // dealt by ticket where that can help (knn_abandon_deal); each launch of the search has its own counter set
            DealFacts df;
            df.opt_deal = h->deal_cnt ? h->opt_abandon_deal : 0; df.ab_ck = ab_ck; df.launch = (int)i; df.row_tiles = ceil_div64(rp.n, KW_M);
            df.n_qtiles = gq; df.n_splits = gs; df.cus = h->n_cus;
            const DealPlan dp = knn_abandon_deal(df);
            if (dp.dealt) {
                rp.deal_g = dp.granule; rp.deal_tiles = (int)df.row_tiles;
                rp.deal_cnt = h->deal_cnt + knn_deal_counter((int)i, 0, 0);
                launch_fn = rsc == 0 ? k_knn_hi_abandon_deal<0> : k_knn_hi_abandon_deal<3>;
                RADAD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(launch_fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)launch_lds));
                ++h->last_deal_launches; h->last_deal_workgroups = dp.workgroups; h->last_deal_granule = dp.granule;
            }
        }
        // a deferring launch (knn_abandon_defer) lists the few live rows of its vetoed tiles and is followed by its tail, which scores
        // them in full with this launch's floors before anything reads the candidate buffers
        DeferPlan fp;
        if (ab_ck > 0) {
            DeferFacts ff;
            ff.opt_defer = (h->deal_cnt && h->defer_list) ? h->opt_abandon_defer : 0; ff.ab_ck = ab_ck; ff.dealt = rp.deal_cnt != nullptr;
            ff.launch = (int)i; ff.rows = rp.n; ff.row_bytes = rp.row_bytes; ff.n_qtiles = std::max(gq, rp.n_qtiles); ff.cus = h->n_cus;
            fp = knn_abandon_defer(ff);
            if (fp.defer && fp.list_cap > h->defer_list_cap) fp.defer = false;
        }
        // the checkpoint stage fetches the next tile's head where the tile is expected to leave (knn_abandon_ahead): the static-chunk
        // kernels, deferring or not
        if (h->deal_cnt && knn_abandon_ahead(h->opt_abandon_ahead, ab_ck, rp.deal_cnt != nullptr, (int)i)) {
            rp.ab_ahead = 1;
            rp.ah_count = h->deal_cnt + knn_ahead_counter((int)i);
            h->last_ahead_sets |= 1u << i;
        }
        KnnHiParams tp, rtp;
        RowTailPlan rt;
        auto tail_fn = launch_fn;
        if (fp.defer) {
            rp.df_cnt = h->deal_cnt + knn_defer_counter((int)i, 0);
            rp.df_list = h->defer_list; rp.df_cap = (int)fp.list_cap;
            rp.df_tasks = h->deal_cnt + knn_defer_tasks_counter((int)i);
            launch_fn = rsc == 0 ? k_knn_hi_abandon_defer<0> : k_knn_hi_abandon_defer<3>;
            launch_lds = knn_hi_lds_bytes(true, true);
            RADAD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(launch_fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)launch_lds));
            tp = rp;
            tp.ab_ck = 0; tp.n_splits = fp.tail_splits; tp.chunk_rows = tp.chunk_stride = KW_M; tp.ksplit = 1;
            tp.df_bytes = (unsigned)(rp.n * rp.row_bytes);
            // (the counting form of the emit: every row of a tail tile is a candidate of some query, and reserving slot by slot a wave
            // sat through ~30 atomic round trips one after the other -- 85 us per tail on the benchmark, measured; the set emitted is
            // the same, and nothing reads the buffers' order)
            tp.loose_floor = 1;
            tail_fn = rsc == 0 ? k_knn_hi_tail<0> : k_knn_hi_tail<3>;
            RADAD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(tail_fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            // short lists -- the usual case -- go to the row tail: 16-row groups over every CU (knn_defer_rowtail); each of the two
            // kernels reads the count and leaves a list that is the other's (knn_rowtail_takes)
            rt = knn_defer_rowtail(fp.list_cap, gq_grid, h->n_cus);
            rtp = tp;
            rtp.n_splits = rt.n_splits;
        }
        h->prof.begin(st);      // the event pair brackets a scan launch (the kernel the roofline is quoted on; the phases of one
                                // search are two entries) and, behind a deferring one, its tail
        hipLaunchKernelGGL(launch_fn, dim3((unsigned)(gq_grid * gs * rp.ksplit)), dim3(KW_THREADS), launch_lds, st, rp);
        if (fp.defer) {
            if (rsc == 0) hipLaunchKernelGGL(k_knn_hi_rowtail<0>, dim3((unsigned)(gq_grid * rt.n_splits)), dim3(KNN_ROWTAIL_THREADS), 0, st, rtp);
            else hipLaunchKernelGGL(k_knn_hi_rowtail<3>, dim3((unsigned)(gq_grid * rt.n_splits)), dim3(KNN_ROWTAIL_THREADS), 0, st, rtp);
            // (a list can only be the tile tail's where its capacity reaches past the row tail's share)
            if (!knn_rowtail_takes((int)std::min<int64_t>(fp.list_cap, INT_MAX)))
                hipLaunchKernelGGL(tail_fn, dim3((unsigned)(gq_grid * fp.tail_splits)), dim3(KW_THREADS), lds, st, tp);
            ++h->last_defer_launches; h->last_defer_sets |= 1u << i;
        }
        h->prof.end(st);
    }
    if (scrub) knn_launch_scrub(h, scrub, ps, pi, wp.cand_cnt, p.emit_cap, st);     // (for the re-rank)
#ifdef RADAD_DEBUG_HOOKS
    if (wp.stamps) {
        std::vector<unsigned long long> hs(8 * 4096);
        (void)hipStreamSynchronize(st);
        (void)hipMemcpy(hs.data(), wp.stamps, hs.size() * 8, hipMemcpyDeviceToHost);
        if (FILE* f = fopen(getenv("RADAD_KNN_STAMPS"), "wb")) { fwrite(hs.data(), 8, hs.size(), f); fclose(f); }
    }
#endif
    return RADAD_OK;
}

// ---- the other scans: one launch each ---------------------------------------------------------------------------------------------
static void knn_scan_dense(radad_knn_t h, const ScanPlan& p, const SearchLayout& L, const float* q_use, hipStream_t st) {
    DenseParams dp;
    dp.db = (const float*)h->rows; dp.ynorm = h->ynorm; dp.q = q_use; dp.n = h->ntotal; dp.nq = (int)p.nq; dp.dim = h->dim; dp.l2 = p.l2;
    dp.plen = p.dense_plen; dp.score = ws_at<float>(h, L.ps); dp.idx = ws_at<int>(h, L.pi); dp.cnt = ws_at<int>(h, L.cnt);
    h->prof.begin(st);
    if (p.nq <= SQ_NQ) hipLaunchKernelGGL((k_knn_dense<1, 1>), dim3((unsigned)ceil_div64(p.dense_plen, 64), (unsigned)ceil_div64(p.nq, 16)), dim3(256), 0, st, dp);
    else hipLaunchKernelGGL((k_knn_dense<2, 4>), dim3((unsigned)ceil_div64(p.dense_plen, 128), (unsigned)ceil_div64(p.nq, 64)), dim3(256), 0, st, dp);
    h->prof.end(st);
}

// a kernel of 16- or 32-entry lists with its dynamic LDS, set and launched on n_splits workgroups of SQ_THREADS
template <typename Params>
static int knn_launch_smallq(radad_knn_t h, void (*fn)(Params), const Params& sp, int n_splits, size_t lds, hipStream_t st) {
    RADAD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    h->prof.begin(st);
    hipLaunchKernelGGL(fn, dim3((unsigned)n_splits), dim3(SQ_THREADS), lds, st, sp);
    h->prof.end(st);
    return RADAD_OK;
}

// what every stream of the f16 plane is launched with
static void knn_fill_smallq_hi(radad_knn_t h, const ScanPlan& p, const SearchLayout& L, SmallQHiParams& sp) {
    sp.db = h->f16 ? (const _Float16*)h->rows : h->hi;
    sp.rscale = h->f16 ? nullptr : h->rscale;
    sp.uscale = h->f16 ? 1.0f : (h->uniform_e != HI_E_PER_ROW ? ldexpf(1.0f, -h->uniform_e) : (h->metric == RADAD_METRIC_COSINE ? 0x1p-14f : 1.0f));
    sp.rbias = p.biased ? (p.mu ? h->rbias : h->ynorm) : nullptr; sp.bias_sign = p.l2 ? -1.f : 1.f; sp.mult = p.l2 ? 2.f : 1.f;
    sp.qconst = p.biased ? ws_at<float>(h, L.qconst) : nullptr;
    sp.q = ws_at<_Float16>(h, L.qh); sp.qscale = ws_at<float>(h, L.qscale); sp.n = h->ntotal; sp.nq = (int)p.nq; sp.dim = h->dim; sp.k = p.ksel_sq;
    sp.rows_per_wave = p.sq_rows_per_wave; sp.n_parts = p.n_splits; sp.part_score = ws_at<float>(h, L.ps); sp.part_idx = ws_at<int>(h, L.pi);
}

static int knn_scan_hi_smallq(radad_knn_t h, const ScanPlan& p, const SearchLayout& L, hipStream_t st) {
    SmallQHiParams sp;
    knn_fill_smallq_hi(h, p, L, sp);
    const bool l16 = p.ksel_sq <= 16;
    const auto fn = p.sq_ksplit ? (l16 ? k_knn_hi_smallq_ksplit<16> : k_knn_hi_smallq_ksplit<32>) : (l16 ? k_knn_hi_smallq<16> : k_knn_hi_smallq<32>);
    return knn_launch_smallq(h, fn, sp, p.n_splits, p.sq_lds, st);
}

// the range search of a small batch (RADAD_RANGE_STREAM): one launch of k_range_hi_smallq from the floors in L.thr into the candidate
// buffers (L.pi, L.cnt: zeroed by knn_prepare_queries).  row_bias: the per-call bias array (one set for the batch), or NULL
static_assert(KNN_RANGE_STREAM_CAP == RG_MAX_CAP, "the stream's candidate buffers are what k_range_refine's sort is sized for");
static int knn_scan_range_smallq(radad_knn_t h, const ScanPlan& p, const SearchLayout& L, hipStream_t st, const float* row_bias) {
    RangeSmallQParams sp;
    knn_fill_smallq_hi(h, p, L, sp);
    if (row_bias) sp.rbias = row_bias;
    sp.thr = ws_at<const float>(h, L.thr); sp.cnt = ws_at<int>(h, L.cnt); sp.idx = ws_at<int>(h, L.pi); sp.cap = p.emit_cap;
    return knn_launch_smallq(h, k_range_hi_smallq, sp, p.n_splits, p.sq_lds, st);
}

static int knn_scan_f32_smallq(radad_knn_t h, const ScanPlan& p, const SearchLayout& L, const float* q_use, hipStream_t st) {
    SmallQParams sp;
    sp.db = (const float*)h->rows; sp.ynorm = h->ynorm; sp.q = q_use; sp.n = h->ntotal; sp.nq = (int)p.nq; sp.dim = h->dim; sp.k = p.ksel;
    sp.l2 = p.l2; sp.rows_per_wave = p.sq_rows_per_wave; sp.n_parts = p.n_splits; sp.part_score = ws_at<float>(h, L.ps); sp.part_idx = ws_at<int>(h, L.pi);
    return knn_launch_smallq(h, p.ksel <= 16 ? k_knn_f32_smallq<16> : k_knn_f32_smallq<32>, sp, p.n_splits, p.sq_lds, st);
}

// the fp32 (or fp16-operand) tile kernels, lists of k + margin per (query, split)
static int knn_scan_tile(radad_knn_t h, const ScanPlan& p, const SearchLayout& L, const float* q_use, hipStream_t st) {
    const bool f16_tile = p.kind == RADAD_SCAN_F16_TILE;
    KnnParams kp;
    kp.db = h->rows; kp.db_f16 = h->f16; kp.ynorm = h->ynorm; kp.q = f16_tile ? (const void*)ws_at<_Float16>(h, L.qh) : (const void*)q_use;
    kp.n = h->ntotal; kp.nq = (int)p.nq; kp.dim = h->dim; kp.k = p.ksel; kp.l2 = p.l2;
    kp.n_qtiles = p.n_qtiles; kp.n_splits = p.n_splits; kp.chunk_rows = p.chunk_rows; kp.part_score = ws_at<float>(h, L.ps); kp.part_idx = ws_at<int>(h, L.pi);
    void (*fn)(KnnParams);
    size_t lds;
    if (f16_tile || (!h->f16 && p.ksel <= 32 && h->dim % KT_K == 0)) {
        // tile kernel with LDS-DMA staging and register-resident lists: <list entries, fp16 operands>
        const bool l16 = p.ksel <= 16;
        fn = f16_tile ? (l16 ? k_knn_f32_reg<16, true> : k_knn_f32_reg<32, true>) : (l16 ? k_knn_f32_reg<16, false> : k_knn_f32_reg<32, false>);
        lds = knn_reg_lds_bytes();
    } else {
        // generic kernel (any k, any dim % 4 == 0): register staging, lists in the partial arrays; an fp16 store is
        // decoded to fp32 while staging and multiplied with the fp32 queries
        fn = h->f16 ? k_knn_f32<true> : k_knn_f32<false>;
        lds = knn_lds_bytes();
    }
    RADAD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    h->prof.begin(st);
    hipLaunchKernelGGL(fn, dim3((unsigned)(p.n_qtiles * p.n_splits)), dim3(KNN_THREADS), lds, st, kp);
    h->prof.end(st);
    return RADAD_OK;
}

// ---- sharded search: lower bounds of the exact scores of this store's k best rows, per query -------------------------------------
// (scan score - eps of the k rows with the best scan scores).  The scan score of the f16 tile kernel estimates q.y (inner product,
// cosine) or -|q - y|^2 (L2) whatever the plane's centring, so the bounds of different shards compare; the other kernels report none
// (-inf).
static void knn_report_lower_bounds(radad_knn_t h, const ScanPlan& p, const SearchLayout& L, float* lb_out, hipStream_t st) {
    if (p.kind == RADAD_SCAN_HI_TILE) {
        KthParams kp;
        kp.score = ws_at<float>(h, L.ps); kp.cnt = ws_at<int>(h, L.cnt); kp.cap = p.emit_cap; kp.k = p.k; kp.eps = ws_at<float>(h, L.eps);
        kp.lb_out = lb_out; kp.ak_out = ws_at<float>(h, L.ak);
        hipLaunchKernelGGL(k_kth_floor, dim3((unsigned)p.nq), dim3(RF_THREADS), (size_t)p.emit_cap * 4 + 1040, st, kp);
    } else {
        hipLaunchKernelGGL(k_fill_f32, dim3((unsigned)ceil_div64(p.nq * p.k, 256)), dim3(256), 0, st, lb_out, p.nq * p.k, -INFINITY);
    }
}

// a search on another stream than the last one waits for it; from here on `st` is where the handle's workspace is in use
static int knn_order_behind_last(radad_knn_t h, hipStream_t st) {
    if (h->have_last && !h->owned_serial && st != h->last_stream) {
        if (hipEventRecord(h->ev_done, h->last_stream) == hipSuccess) RADAD_HIP_CHECK(hipStreamWaitEvent(st, h->ev_done, 0));
        else { (void)hipGetLastError(); RADAD_HIP_CHECK(hipDeviceSynchronize()); }      // (that stream no longer exists)
    }
    // from here on this search's kernels go to `st` and use the handle's workspace: whatever comes next -- also after an error return
    // or radad_knn_search_abort between the halves -- orders itself behind `st` (until round 4 this was only recorded at the END
    // of phase 2: a search on another stream after an aborted one shared the workspace with kernels still running)
    h->last_stream = st;
    h->have_last = true;
    return RADAD_OK;
}

static int knn_search_phase1(radad_knn_t h, const void* q_in, int q_dtype, int64_t nq, int k, int margin, float* lb_out, hipStream_t st,
                             SearchCtx* ctx) {
    // one workspace per handle: a search on another stream waits for the previous one (threads are serialised by h->mu,
    // the device work by this event)
    // (searches share the handle's workspace.  On ONE stream they are ordered anyway; a search on another stream than the last one
    // first records an event behind whatever that stream holds and waits for it -- recording one behind EVERY search, as until round 4,
    // held the kernel after each search back ~6 us, 5 % of an online search)
    int rc = knn_order_behind_last(h, st);
    if (rc) return rc;

    h->prof.next_search();
    knn_consume_reports(h);
    const int cslot = h->tune.slot();
#ifdef RADAD_DEBUG_HOOKS
    if (getenv("RADAD_DEBUG_KNN")) h->tune.clear_skip();    // timing ablations (wrong results, every query rejected): stay on the kernel under test
#endif
    ScanPlan p;
    rc = knn_plan_scan(h, nq, k, margin, st, &p);
    if (rc) return rc;
    const SearchLayout L = knn_search_layout(knn_store_facts(h), p, q_dtype);
    rc = knn_workspace(h, L.bytes);
    if (rc) return rc;
    const float* q_use = knn_prepare_queries(h, p, L, q_in, q_dtype, st);
    RADAD_HIP_CHECK(hipGetLastError());

    switch (p.kind) {
        case RADAD_SCAN_HI_TILE: rc = knn_scan_hi_tile(h, p, L, st); break;
        case RADAD_SCAN_F32_DENSE: knn_scan_dense(h, p, L, q_use, st); break;
        case RADAD_SCAN_HI_SMALLQ: rc = knn_scan_hi_smallq(h, p, L, st); break;
        case RADAD_SCAN_F32_SMALLQ: rc = knn_scan_f32_smallq(h, p, L, q_use, st); break;
        default: rc = knn_scan_tile(h, p, L, q_use, st); break;
    }
    if (rc) return rc;
    const bool hi_tile = p.kind == RADAD_SCAN_HI_TILE;
    if (!hi_tile) { h->last_splits = p.n_splits; h->last_scan_launches = 1; h->last_ab_tasks = 0; }
    RADAD_HIP_CHECK(hipGetLastError());
    if (lb_out) {
        knn_report_lower_bounds(h, p, L, lb_out, st);
        RADAD_HIP_CHECK(hipGetLastError());
    }

    ctx->valid = true;
    ctx->nq = nq; ctx->k = k; ctx->l2 = p.l2; ctx->cslot = cslot; ctx->n_parts = p.n_parts; ctx->plen = p.plen; ctx->cap = p.cap; ctx->xgroup = p.xgroup;
    ctx->emit = hi_tile || p.kind == RADAD_SCAN_F32_DENSE; ctx->use_floor = hi_tile; ctx->hi_tile = hi_tile; ctx->q_use = q_use;
    ctx->small_lists = p.kind == RADAD_SCAN_HI_SMALLQ || p.kind == RADAD_SCAN_F32_SMALLQ;
    ctx->canonical = hi_tile || p.kind == RADAD_SCAN_HI_SMALLQ || !p.l2;
    ctx->have_ak = lb_out != nullptr && hi_tile;
    ctx->ws = L;
    h->last_o_cnt = L.cnt; h->last_o_thr = L.thr; h->last_emit_nq = hi_tile ? nq : 0;
    return RADAD_OK;
}

// ---- float64 re-rank + certificate of what phase 1 listed: results of every query, the rejected ones in flag_sel[0, *flag_count) ----
static int knn_rerank(radad_knn_t h, const SearchCtx& c, const float* global_lb, float* out_dist_dev, int64_t* out_idx_dev,
                      double* out_key_dev, hipStream_t st) {
    int* flag_count = ws_at<int>(h, c.ws.fcount);
    int* flag_sel = ws_at<int>(h, c.ws.fsel);
    const int64_t nq = c.nq;
    const int k = c.k;
    RefineParams m;
    m.score = ws_at<const float>(h, c.ws.ps); m.idx = ws_at<const int>(h, c.ws.pi); m.n_parts = c.n_parts; m.k = k; m.dim = h->dim; m.l2 = c.l2; m.nq = nq;
    m.part_len = c.plen; m.cap = c.cap;
    m.eps = ws_at<const float>(h, c.ws.eps); m.thr_init = c.use_floor ? ws_at<const float>(h, c.ws.thr) : nullptr;
    m.part_cnt = c.emit ? ws_at<const int>(h, c.ws.cnt) : nullptr; m.global_lb = c.canonical ? global_lb : nullptr;
    m.ak_in = c.have_ak ? ws_at<const float>(h, c.ws.ak) : nullptr;
    m.flag_count = flag_count; m.flag_sel = flag_sel;
    m.db = h->rows; m.db_f16 = h->f16; m.q = c.q_use; m.id_base = h->id_base; m.out_dist = out_dist_dev; m.out_idx = out_idx_dev;
    m.out_key = out_key_dev;
#ifdef RADAD_DEBUG_HOOKS
    { const char* dbg = getenv("RADAD_DEBUG_KNN"); m.debug = dbg ? atoi(dbg) : 0; }
#endif
    m.stats = flag_count + 1;
    RADAD_REQUIRE(c.n_parts <= RF_THREADS * RF_MAXL, "radad_knn_search: %d partial lists per query exceed the re-rank kernel's %d", c.n_parts,
                  RF_THREADS * RF_MAXL);
    if (c.small_lists && nq <= SQ_NQ && m.n_parts <= RS_MAX_PARTS && m.cap <= RS_MAX_CAP) {
        // a small batch: RS_SPLIT workgroups per query (k_refine_small)
        if (!h->rs_key) {                                // (once per handle: allocation and clearing synchronise)
            const size_t kb = (size_t)SQ_NQ * RS_MAX_CAP * sizeof(double);
            if (hipMalloc((void**)&h->rs_key, kb) != hipSuccess || hipMalloc((void**)&h->rs_count, SQ_NQ * sizeof(int)) != hipSuccess ||
                hipMemset(h->rs_count, 0, SQ_NQ * sizeof(int)) != hipSuccess) {
                (void)hipGetLastError();
                if (h->rs_key) (void)hipFree(h->rs_key);
                if (h->rs_count) (void)hipFree(h->rs_count);
                h->rs_key = nullptr; h->rs_count = nullptr;
                radad_set_error("hipMalloc of the small-batch re-rank's buffers failed");
                return RADAD_ENOMEM;
            }
        }
        const size_t rlds = refine_small_lds_bytes(c.cap);
        hipLaunchKernelGGL(k_refine_small, dim3(RS_SPLIT, (unsigned)nq), dim3(RS_THREADS), rlds, st, m, h->rs_key, h->rs_count);
    } else {   // certified mode with lists that fit the LDS: selection on a staged copy (one round of loads instead of a pointer chase)
        const size_t entries = (size_t)m.n_parts * m.part_len;
        RADAD_REQUIRE(!c.emit || (m.eps && entries <= (size_t)(nq <= SQ_NQ ? RF_STAGE_MAX_SMALLQ : RF_STAGE_MAX)),
                      "radad_knn_search: candidate buffer larger than the re-rank stages");
        if (m.eps && entries <= (size_t)(nq <= SQ_NQ ? RF_STAGE_MAX_SMALLQ : RF_STAGE_MAX)) {
            const size_t rlds = refine_lds_bytes(c.cap) + entries * 8 + 1024;
            if (rlds > 48 * 1024)
                RADAD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_merge_refine<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)rlds));
            hipLaunchKernelGGL(k_merge_refine<true>, dim3((unsigned)nq), dim3(RF_THREADS), rlds, st, m);
        }
        else
            hipLaunchKernelGGL(k_merge_refine<false>, dim3((unsigned)nq), dim3(RF_THREADS), refine_lds_bytes(c.cap), st, m);
    }
    RADAD_HIP_CHECK(hipGetLastError());
    return RADAD_OK;
}

// arrival counters of the exact kernels' query groups (zero between launches), room for nq of them
static int knn_ensure_xarrive(radad_knn_t h, int64_t nq, hipStream_t st) {
    if (nq <= h->xarrive_cap) return RADAD_OK;
    RADAD_HIP_CHECK(hipStreamSynchronize(st));
    if (h->xarrive) (void)hipFree(h->xarrive);
    h->xarrive = nullptr; h->xarrive_cap = 0;
    const int64_t cap = nq + nq / 2 + 64;
    if (hipMalloc((void**)&h->xarrive, (size_t)cap * sizeof(int)) != hipSuccess || hipMemset(h->xarrive, 0, (size_t)cap * sizeof(int)) != hipSuccess) {
        (void)hipGetLastError();
        if (h->xarrive) (void)hipFree(h->xarrive);
        h->xarrive = nullptr;
        radad_set_error("hipMalloc of the exact pass's arrival counters failed");
        return RADAD_ENOMEM;
    }
    h->xarrive_cap = cap;
    return RADAD_OK;
}

// The one place an exact pass is launched, whatever the instantiation of k_exact_scan_any: the queries x.sel[0, *x.count) of a batch
// of nq at k results (a range search: at most k listed), sized and driven by the device-side count.  The caller's `x` holds what
// its family owns -- queries, the listed ones, partial lists with their grouping (group, nslots), outputs, the admission rule, the
// range fields, stamp / nq_report; the store, k, the slices, the arrival counters (the caller made room for nq of them:
// knn_ensure_xarrive) and the launches are filled in here.
// first_host_stats: where the launch of the first slots leaves the search's report (knn_search_phase2); NULL for every family that
// posts none -- the handle's certificate report and its tuning belong to the plain search.
static int knn_launch_exact(radad_knn_t h, void (*kern)(ExactParams), ExactParams x, int64_t nq, int k, hipStream_t st,
                            int* first_host_stats = nullptr) {
    x.db = h->rows; x.db_f16 = h->f16; x.n = h->ntotal; x.dim = h->dim; x.k = k; x.id_base = h->id_base;
    x.slice_rows = ceil_div64(std::max<int64_t>(h->ntotal, 1), KX_SLICES);
    x.arrive = h->xarrive;
    // (with the kernel's static arrival flag <= KX_LDS_MAX: every entry point checked knn_exact_fits.  Until the width tests
    // searched 16380 x 1024 the launch asked for 16 bytes more than the kernel indexes, and the widest rows the limit admits
    // were refused by hipFuncSetAttribute: 160 KB of dynamic LDS plus the static flag)
    const size_t xlds = knn_exact_dyn_lds_bytes(h->dim, k);
    RADAD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)xlds));
    // (k beyond KNN_F16_MAX_K: groups of one or two queries, each a long insert and merge -- more of them in flight; the
    // geometry of k <= 128 is the measured one)
    const unsigned gy = k <= KNN_F16_MAX_K ? KX_GROUPS_Y : 8 * KX_GROUPS_Y;
    for (int64_t s0 = 0; s0 < nq; s0 += x.nslots) {      // (launches past the device-side count leave at once)
        x.slot0 = (int)s0;
        x.host_stats = s0 == 0 ? first_host_stats : nullptr;
        hipLaunchKernelGGL(kern, dim3(KX_SLICES, gy), dim3(KX_THREADS), xlds, st, x);
    }
    RADAD_HIP_CHECK(hipGetLastError());
    return RADAD_OK;
}

constexpr int RADAD_RETRY_INTERNAL = 1;     // knn_search_phase2 -> knn_search_core: retuned after a mass rejection, run the search again
static int knn_search_phase2(radad_knn_t h, const SearchCtx& c, const float* global_lb, bool may_retry, float* out_dist_dev, int64_t* out_idx_dev,
                             double* out_key_dev, hipStream_t st) {
    int* flag_count = ws_at<int>(h, c.ws.fcount);
    int* flag_sel = ws_at<int>(h, c.ws.fsel);
    const int64_t nq = c.nq;
    const int k = c.k;
    int rc = knn_rerank(h, c, global_lb, out_dist_dev, out_idx_dev, out_key_dev, st);
    if (rc) return rc;

    // ---- look before the exact pass (see KnnTuning) ------------------------------------------------------------------------------
    if (h->tune.looks_before_exact(c.hi_tile, nq, h->ntotal, h->dim)) {
        int* rej = h->host_count + h->HC_LOOK;
        RADAD_HIP_CHECK(hipMemcpyAsync(rej, flag_count, sizeof(int), hipMemcpyDeviceToHost, st));
        RADAD_HIP_CHECK(hipStreamSynchronize(st));
        if (h->tune.look_outcome(*rej, nq, may_retry, h->tune.appended_since_plane(h->hi != nullptr, h->ntotal))) return RADAD_RETRY_INTERNAL;
    }

    // ---- the queries the certificate rejected: exact float64 search, sized and driven by the device-side count ------
    {
        ExactParams x;
        x.q = c.q_use; x.sel = flag_sel; x.count = flag_count; x.l2 = c.l2;
        x.pkey = ws_at<double>(h, c.ws.xk); x.pidx = ws_at<int>(h, c.ws.xi);
        x.group = c.xgroup; x.nslots = (int)knn_exact_slots(nq, k, c.xgroup);
        x.out_dist = out_dist_dev; x.out_idx = out_idx_dev; x.out_key = out_key_dev;
        x.stamp = h->tune.stamp();
        // (a search beyond KNN_F16_MAX_K took no f16 scan: its rejections say nothing about the f16 scans' tuning, which reads
        // batch sizes of >= 64 only -- knn_consume_reports)
        x.nq_report = k <= KNN_F16_MAX_K ? (int)std::min<int64_t>(nq, 0x7fffffff) : 0;
        rc = knn_ensure_xarrive(h, nq, st);
        if (rc) return rc;
        rc = knn_launch_exact(h, k_exact_scan, x, nq, k, st, h->host_count_dev + 8 * c.cslot);
        if (rc) return rc;
        h->count_nq[c.cslot] = nq;                                    // (k_exact_scan writes the counters and its stamp to the pinned host copy)
        h->tune.search_issued();
    }
    h->last_stream = st;
    h->have_last = true;
    return RADAD_OK;
}

// one search on a handle whose mutex the caller holds; *ctx_out (optional): what the search that ran prepared (its queries)
static int knn_search_locked(radad_knn_t h, const void* q_in, int q_dtype, int64_t nq, int k, int margin, float* out_dist_dev,
                             int64_t* out_idx_dev, double* out_key_dev, hipStream_t st, SearchCtx* ctx_out) {
    for (int attempt = 0;; ++attempt) {       // (at most: plane re-decided, buffers widened, fp32 kernels)
        SearchCtx c;
        int rc = knn_search_phase1(h, q_in, q_dtype, nq, k, margin, nullptr, st, &c);
        if (rc) return rc;
        rc = knn_search_phase2(h, c, nullptr, attempt < 3, out_dist_dev, out_idx_dev, out_key_dev, st);
        if (rc != RADAD_RETRY_INTERNAL) {
            if (ctx_out) *ctx_out = c;
            return rc;
        }
    }
}

static int knn_search_core(radad_knn_t h, const void* q_in, int q_dtype, int64_t nq, int k, int margin, float* out_dist_dev,
                           int64_t* out_idx_dev, double* out_key_dev, void* stream) {
    RADAD_REQUIRE(h, "NULL handle");
    RADAD_REQUIRE(k >= 1 && k <= RADAD_KNN_MAX_K, "radad_knn_search: k=%d outside [1,%d]", k, RADAD_KNN_MAX_K);
    RADAD_REQUIRE(nq >= 0 && nq < (1ll << 31) - KT_N, "radad_knn_search: bad nq");
    // (before anything is enqueued: the outputs stay untouched and the handle usable -- knn_exact_fits, knn_plan.h)
    RADAD_REQUIRE(knn_exact_fits(h->dim, k), "radad_knn_search: dim %d x k %d too large for the exact kernel (dim * 4 + 96 k + 16 <= %zu)", h->dim, k, KX_LDS_MAX);
    if (nq == 0) return RADAD_OK;
    RADAD_REQUIRE(q_in && out_dist_dev && out_idx_dev, "radad_knn_search: NULL buffer");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    RADAD_REQUIRE(!h->pending.valid && !h->pending_excl.valid, "radad_knn_search: a radad_knn_search_begin on this handle has not been finished");
    return knn_search_locked(h, q_in, q_dtype, nq, k, margin, out_dist_dev, out_idx_dev, out_key_dev, (hipStream_t)stream, nullptr);
}

// ---- exclusion-aware search ---------------------------------------------------------------------------------------------------------
// fast pass = the certified search at k_fetch (every scan path, float64 keys) -> k_excl_compact<false>: certificate per query, results of the
// proved ones -> k_exact_scan_excl for the listed ones, sized and driven by the device-side count like the exact pass of any search.
static int knn_excl_reserve(radad_knn_t h, size_t bytes) {
    if (bytes <= h->excl_ws_bytes) return RADAD_OK;
    RADAD_HIP_CHECK(hipDeviceSynchronize());              // an earlier search of this kind may still read the old one
    if (h->excl_ws) (void)hipFree(h->excl_ws);
    h->excl_ws = nullptr; h->excl_ws_bytes = 0;
    if (hipMalloc(&h->excl_ws, bytes) != hipSuccess) {
        (void)hipGetLastError();
        radad_set_error("hipMalloc of %zu bytes for the exclusion-aware search failed", bytes);
        return RADAD_ENOMEM;
    }
    h->excl_ws_bytes = bytes;
    return RADAD_OK;
}

// the admission bitmap of a batch rule, one bit per row in admit[0, n_words): all ones when nothing is excluded (the tags may be
// NULL then).  count: NULL, or a device-side count of listed queries -- the bitmap is built only when *count > 0
static int knn_admit_bitmap(radad_knn_t h, const ExclRule& r, const int* count, unsigned long long* admit, int64_t n_words, hipStream_t st) {
    if (r.n_excl > 0)
        hipLaunchKernelGGL(k_admit_bitmap<false>, dim3((unsigned)ceil_div64(n_words * 64, 256)), dim3(256), 0, st, r.tags,
                           (const int64_t*)nullptr, h->ntotal, r.excl, r.n_excl, count, admit, n_words);
    else
        RADAD_HIP_CHECK(hipMemsetAsync(admit, 0xff, (size_t)n_words * sizeof(unsigned long long), st));
    RADAD_HIP_CHECK(hipGetLastError());
    return RADAD_OK;
}

// the row-filtered exact pass for the queries in sel[0, *count): bitmap (built only when *count > 0), then k_exact_scan_excl sized and
// driven by the device-side count like the exact pass of any search; it overwrites those queries' rows of out_*
// (per-query rule: no bitmap; k_exact_scan_excl_pq compares the row's tag with the group's query tags)
static int knn_excl_exact_pass(radad_knn_t h, const ExclLayout& L, int64_t nq, int k, int l2, const float* q_use, const ExclRule& r,
                               float* out_dist_dev, int64_t* out_idx_dev, double* out_key_dev, hipStream_t st) {
    auto at = [&](size_t o) { return (char*)h->excl_ws + o; };
    ExactParams x;
    x.q = q_use; x.sel = (int*)at(L.sel); x.count = (int*)at(L.count); x.l2 = l2;
    x.pkey = (double*)at(L.xk); x.pidx = (int*)at(L.xi); x.group = L.xgroup; x.nslots = (int)L.xslots;
    x.out_dist = out_dist_dev; x.out_idx = out_idx_dev; x.out_key = out_key_dev;
    if (r.per_query) { x.row_tags = r.tags; x.q_tags = r.q_tags; x.q_cnt = r.q_cnt; x.m = r.m(); }
    else {
        const int rc = knn_admit_bitmap(h, r, x.count, (unsigned long long*)at(L.admit), L.n_words, st);
        if (rc) return rc;
        x.admit = (const unsigned long long*)at(L.admit);
    }
    // (the fast pass made room for nq groups; zero between launches)
    RADAD_REQUIRE(h->xarrive && nq <= h->xarrive_cap, "radad_knn_search_excl: the fast pass left no arrival counters for %lld queries", (long long)nq);
    return knn_launch_exact(h, r.per_query ? k_exact_scan_excl_pq : k_exact_scan_excl, x, nq, k, st);
}

// the part the whole-store call and the shard's first half share: layout -> workspace -> the fast pass at kf into fd / fi / fk ->
// compaction into out_* (begun: into the workspace's bd / bi / bk, with frontier and own flags instead of the listing)
static int knn_excl_fast_pass(radad_knn_t h, const void* q_in, int q_dtype, int64_t nq, int k, int k_fetch, const ExclRule& r,
                              float* out_dist_dev, int64_t* out_idx_dev, double* out_key_dev,
                              double* fr_key_dev, int64_t* fr_idx_dev, hipStream_t st, bool begun, SearchCtx* c, ExclLayout* Lout) {
    const ExclLayout L = knn_excl_layout(knn_store_facts(h), nq, k, k_fetch, r.n_excl, begun, r.per_query);
    int rc = knn_excl_reserve(h, L.bytes);
    if (rc) return rc;
    auto at = [&](size_t o) { return (char*)h->excl_ws + o; };
    rc = knn_search_locked(h, q_in, q_dtype, nq, L.kf, KNN_MARGIN, (float*)at(L.fd), (int64_t*)at(L.fi), (double*)at(L.fk), st, c);
    if (rc) return rc;
    RADAD_HIP_CHECK(hipMemsetAsync(at(L.count), 0, 256, st));
    ExclCompactParams p;
    p.in_dist = (const float*)at(L.fd); p.in_idx = (const int64_t*)at(L.fi); p.in_key = (const double*)at(L.fk);
    p.nq = nq; p.k_in = L.kf; p.k_keep = k; p.whole = L.whole;
    p.tags = r.tags; p.ntotal = h->ntotal; p.id_base = h->id_base;
    if (r.per_query) { p.q_tags = r.q_tags; p.q_cnt = r.q_cnt; p.m = r.m(); }
    else { p.excl = r.excl; p.n_excl = r.n_excl; }
    p.out_dist = begun ? (float*)at(L.bd) : out_dist_dev;
    p.out_idx = begun ? (int64_t*)at(L.bi) : out_idx_dev;
    p.out_key = begun ? (double*)at(L.bk) : out_key_dev;
    p.count = (int*)at(L.count); p.sel = (int*)at(L.sel);
    p.fr_key = fr_key_dev; p.fr_idx = fr_idx_dev; p.own = begun ? (int*)at(L.own) : nullptr;
    const dim3 grid((unsigned)ceil_div64(nq, 4));
    if (r.per_query) {
        if (begun) hipLaunchKernelGGL((k_excl_compact<true, true>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((k_excl_compact<false, true>), grid, dim3(256), 0, st, p);
    } else if (begun) hipLaunchKernelGGL(k_excl_compact<true>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(k_excl_compact<false>, grid, dim3(256), 0, st, p);
    RADAD_HIP_CHECK(hipGetLastError());
    h->excl_o_count = L.count;
    h->last_excl_nq = nq;
    *Lout = L;
    return RADAD_OK;
}

static int knn_search_excl_locked(radad_knn_t h, const void* q_in, int q_dtype, int64_t nq, int k, int k_fetch, const ExclRule& r,
                                  float* out_dist_dev, int64_t* out_idx_dev, double* out_key_dev, hipStream_t st) {
    SearchCtx c;
    ExclLayout L;
    int rc = knn_excl_fast_pass(h, q_in, q_dtype, nq, k, k_fetch, r, out_dist_dev, out_idx_dev, out_key_dev, nullptr,
                                nullptr, st, false, &c, &L);
    if (rc) return rc;
    if (r.n_excl == 0) return RADAD_OK;                        // nothing excluded: every query is proved by its own list
    return knn_excl_exact_pass(h, L, nq, k, c.l2, c.q_use, r, out_dist_dev, out_idx_dev, out_key_dev, st);
}

// first half over a row shard: the fast pass with frontier into the workspace; the caller gets copies
static int knn_search_excl_begin_locked(radad_knn_t h, const void* q_in, int q_dtype, int64_t nq, int k, int k_fetch, const ExclRule& r,
                                        double* out_key_dev, int64_t* out_idx_dev,
                                        double* fr_key_dev, int64_t* fr_idx_dev, hipStream_t st) {
    SearchCtx c;
    ExclLayout L;
    int rc = knn_excl_fast_pass(h, q_in, q_dtype, nq, k, k_fetch, r, nullptr, nullptr, nullptr, fr_key_dev, fr_idx_dev,
                                st, true, &c, &L);
    if (rc) return rc;
    auto at = [&](size_t o) { return (char*)h->excl_ws + o; };
    RADAD_HIP_CHECK(hipMemcpyAsync(out_key_dev, at(L.bk), (size_t)nq * k * sizeof(double), hipMemcpyDeviceToDevice, st));
    RADAD_HIP_CHECK(hipMemcpyAsync(out_idx_dev, at(L.bi), (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    RADAD_HIP_CHECK(hipEventRecord(h->ev_begun, st));
    ExclCtx& e = h->pending_excl;
    e.valid = true; e.nq = nq; e.k = k; e.l2 = c.l2; e.q_use = c.q_use; e.rule = r; e.L = L;
    return RADAD_OK;
}

// the argument checks radad_knn_search_excl and radad_knn_search_excl_begin share (nq_min: the latter refuses an empty batch)
static int knn_excl_check_args(const char* fn, radad_knn_t h, int q_dtype, int64_t nq, int64_t nq_min, int k, int k_fetch,
                               const int64_t* row_tags_dev, const int64_t* excl_sorted_dev, int64_t n_excl) {
    RADAD_REQUIRE(h, "NULL handle");
    RADAD_REQUIRE(q_dtype == RADAD_Q_F32 || q_dtype == RADAD_Q_BF16, "%s: unsupported query dtype %d", fn, q_dtype);
    RADAD_REQUIRE(k >= 1 && k <= RADAD_KNN_MAX_K, "%s: k=%d outside [1,%d]", fn, k, RADAD_KNN_MAX_K);
    RADAD_REQUIRE(k_fetch >= k && k_fetch <= RADAD_KNN_MAX_K, "%s: k_fetch=%d outside [k=%d,%d]", fn, k_fetch, k, RADAD_KNN_MAX_K);
    // (the fast pass searches at k_fetch >= k, the row-filtered exact pass at k: refused here, before either is enqueued)
    RADAD_REQUIRE(knn_exact_fits(h->dim, k_fetch), "%s: dim %d x k_fetch %d too large for the exact kernel (dim * 4 + 96 k + 16 <= %zu)", fn, h->dim, k_fetch, KX_LDS_MAX);
    RADAD_REQUIRE(nq >= nq_min && nq < (1ll << 31) - KT_N, "%s: bad nq", fn);
    RADAD_REQUIRE(n_excl >= 0 && (n_excl == 0 || (excl_sorted_dev && row_tags_dev)),
                  "%s: %lld excluded tags need the exclusion set and the row tags", fn, (long long)n_excl);
    return RADAD_OK;
}

static ExclRule knn_excl_rule_batch(const int64_t* row_tags_dev, const int64_t* excl_sorted_dev, int64_t n_excl) {
    ExclRule r;
    r.tags = row_tags_dev; r.excl = excl_sorted_dev; r.n_excl = n_excl;
    return r;
}

// the argument checks of the per-query forms beyond knn_excl_check_args (called with n_excl = 0), and their rule
static int knn_excl_pq_rule(const char* fn, const int64_t* row_tags_dev, const int64_t* q_tags_dev, int m, const int32_t* q_tag_counts_dev,
                            ExclRule* r) {
    RADAD_REQUIRE(m >= 0 && m <= RADAD_EXCL_PQ_MAX_TAGS, "%s: m=%d tags per query outside [0,%d] (one wave compares them: RADAD_EXCL_PQ_MAX_TAGS)",
                  fn, m, RADAD_EXCL_PQ_MAX_TAGS);
    RADAD_REQUIRE(m == 0 || (q_tags_dev && row_tags_dev), "%s: %d tags per query need the query tags and the row tags", fn, m);
    r->tags = row_tags_dev; r->n_excl = m; r->per_query = true; r->q_tags = q_tags_dev; r->q_cnt = m > 0 ? q_tag_counts_dev : nullptr;
    return RADAD_OK;
}

// ---- exclusion inside the certified tile scan (radad_knn_search_excl_scan) ----------------------------------------------------------
// The per-call bias array of the tile route: the plane's bias (NULL = none: an un-centred IP / cosine plane, an fp16 store) where the
// bitmap admits the row, NaN where it does not.  The scan starts a row's accumulators at its bias: a NaN start makes every score of
// the row NaN, and no compare of the scan passes a NaN (DESIGN, "exclusion inside the tile scan", names each of them).
__global__ __launch_bounds__(256) void k_excl_scan_bias(const unsigned long long* __restrict__ admit, const float* __restrict__ bias,
                                                        int64_t n, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool ok = (admit[i >> 6] >> (i & 63)) & 1ull;
    out[i] = ok ? (bias ? bias[i] : 0.f) : __int_as_float(0x7fc00000);
}
// the exact route: every query of the batch is listed for the row-filtered exact kernel
__global__ __launch_bounds__(256) void k_excl_scan_list_all(int* __restrict__ sel, int* __restrict__ count, int64_t nq) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nq) sel[i] = (int)i;
    if (i == 0) *count = (int)nq;
}
// this family's padding where the re-rank left id -1 with +-inf (fewer admissible rows than k, all of them listed): NaN / NaN
__global__ __launch_bounds__(256) void k_excl_scan_pad(float* __restrict__ dist, const int64_t* __restrict__ idx, double* __restrict__ key, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && idx[i] < 0) {
        dist[i] = __int_as_float(0x7fc00000);
        if (key) key[i] = (double)__int_as_float(0x7fc00000);
    }
}

// the steps the in-scan families share (the two forms of knn_search_excl_scan_locked, knn_range_search_locked):
// the per-call bias array of a batch rule, at `off` of the exclusion workspace, in front of a scan that runs the biased instantiation
static float* knn_launch_excl_scan_bias(radad_knn_t h, const ScanPlan& p, const unsigned long long* admit, size_t off, hipStream_t st) {
    float* bias = reinterpret_cast<float*>((char*)h->excl_ws + off);
    hipLaunchKernelGGL(k_excl_scan_bias, dim3((unsigned)ceil_div64(h->ntotal, 256)), dim3(256), 0, st, admit,
                       (const float*)(p.mu ? h->rbias : (p.l2 ? h->ynorm : nullptr)), h->ntotal, bias);
    return bias;
}
// the exact route answers the whole batch: every query is listed
static void knn_launch_list_all(int* flag_sel, int* flag_count, int64_t nq, hipStream_t st) {
    hipLaunchKernelGGL(k_excl_scan_list_all, dim3((unsigned)ceil_div64(nq, 256)), dim3(256), 0, st, flag_sel, flag_count, nq);
}
// the end of a call: how many queries the exact kernel answered, into the family's pinned slot for its read-back (radad_knn_last_excl_scan
// / radad_knn_last_range; pinned memory: no synchronisation here)
static int knn_post_exact_count(radad_knn_t h, int slot, const int* flag_count, hipStream_t st) {
    RADAD_HIP_CHECK(hipMemcpyAsync(h->host_count + slot, flag_count, sizeof(int), hipMemcpyDeviceToHost, st));
    return RADAD_OK;
}

// One call, two routes (knn_excl_scan_route), two forms of the rule.  Neither consumes a certificate report, takes a turn off the
// tuning state, looks before its exact pass or posts a report: KnnTuning is read (hi_skip) and otherwise left as it was found.
//   one set for the batch   (radad_knn_search_excl_scan) the plan of the plain search over the handle's own facts; the bitmap and, on
//                           the tile route, the NaN bias in front of the scan, which runs the biased instantiation; the listed queries
//                           go to k_exact_scan_excl with the same bitmap;
//   a set per query         (radad_knn_search_excl_scan_pq) routes, facts, plan and scrub launches are knn_excl_scan_pq_plan's
//                           (knn_plan.h).  Tile route: the PLAIN search's preparation, scan launches (early abandon included) and
//                           re-rank over widened candidate buffers, with k_excl_pq_scrub in front of every reader of the sample's
//                           entries and of the candidate buffers (knn_scan_hi_tile); the queries the certificate rejects -- overflow
//                           of a buffer by a large crowd among them -- go to k_exact_scan_excl_pq with the query tags.
static int knn_search_excl_scan_locked(const char* fn, radad_knn_t h, const void* q_in, int q_dtype, int64_t nq, int k, const ExclRule& r,
                                       float* out_dist_dev, int64_t* out_idx_dev, double* out_key_dev, hipStream_t st) {
    int rc = knn_order_behind_last(h, st);
    if (rc) return rc;
    const bool pq = r.per_query;
    // (one set for the batch: the sample geometry of the eligibility taken HERE stays the plan's when a plane that could not be
    // allocated has the plan made again)
    const TileEligibility t = knn_tile_eligibility(knn_store_facts(h), nq, k, KNN_MARGIN);
    ExclScanPqPlan X;
    auto make_plan = [&] {
        if (pq) { X = knn_excl_scan_pq_plan(knn_store_facts(h), nq, k, r.m(), h->tune.hi_skip); return; }
        X = ExclScanPqPlan();                                      // (no scrub launches, no phase count to hold the scan to)
        X.facts = knn_store_facts(h);
        X.route = knn_excl_scan_route(X.facts, nq, k, h->tune.hi_skip);
        X.plan = knn_finish_plan(X.facts, nq, k, KNN_MARGIN, t, X.route == RADAD_EXCL_SCAN_TILE, false);
    };
    make_plan();
    bool tile = X.route == RADAD_EXCL_SCAN_TILE;
    if (tile && !knn_ensure_hi(h, st, true)) {                     // (a plane that cannot be allocated switches itself off: exact route)
        tile = false;
        make_plan();
        RADAD_REQUIRE(X.route == RADAD_EXCL_SCAN_EXACT, "%s: a store without a plane planned the tile route", fn);
    }
    if (!tile && !knn_ensure_hi(h, st, false)) { radad_set_error("store statistics could not be computed"); return RADAD_EHIP; }
    ScanPlan p = X.plan;
    p.mu = (p.hi_q && !h->f16) ? h->cmu : nullptr;                 // the plain search's instantiation (knn_plan_scan) ...
    // ... (one set for the batch: the biased one whatever the plane -- RSC 0 / 1 run as RSC 3 / 2 with a zero bias for the admitted rows
    // and a zero query constant: k_hi_rows writes mu.q' + |mu|^2 = 0 without a centre)
    p.biased = p.hi_q && (!pq || p.l2 || p.mu);
    const SearchLayout L = knn_search_layout(X.facts, p, q_dtype);
    rc = knn_workspace(h, L.bytes);
    if (rc) return rc;
    // the admission bitmap, with the bias array behind it on the tile route: one set for the batch -- and m == 0, where nothing is
    // excluded and the tags may be NULL: the per-query exact kernel reads a tag per row, so the rejected queries of such a call take
    // the bitmap form with every bit set
    const bool bitmap = !pq || r.m() == 0;
    const ExclScanLayout B = knn_excl_scan_layout(X.facts, pq ? RADAD_EXCL_SCAN_EXACT : X.route);
    if (bitmap) {
        rc = knn_excl_reserve(h, B.bytes);
        if (rc) return rc;
    }
    rc = knn_ensure_xarrive(h, nq, st);
    if (rc) return rc;
    h->last_emit_nq = 0;                                           // (the workspace no longer holds the last plain tile scan's counters)
    h->last_xs_nq = 0;
    unsigned long long* admit = bitmap ? reinterpret_cast<unsigned long long*>((char*)h->excl_ws + B.admit) : nullptr;
    if (bitmap) {
        rc = knn_admit_bitmap(h, r, nullptr, admit, B.n_words, st);
        if (rc) return rc;
    }
    const float* q_use = knn_prepare_queries(h, p, L, q_in, q_dtype, st);      // (clears the listed-query counter and the candidate counters)
    RADAD_HIP_CHECK(hipGetLastError());
    int* flag_count = ws_at<int>(h, L.fcount);
    int* flag_sel = ws_at<int>(h, L.fsel);

    if (tile) {
        // the plain search's scan, re-rank and certificate: over the admitted rows (one set for the batch: the bias array), or with the
        // scrub launches between the scan's (a set per query)
        float* bias = nullptr;
        if (!pq) {
            bias = knn_launch_excl_scan_bias(h, p, admit, B.bias, st);
            RADAD_HIP_CHECK(hipGetLastError());
        }
        ScanScrub scrub;
        scrub.rule = &r; scrub.grid = X.scrub_grid;
        h->prof.next_search();
        rc = knn_scan_hi_tile(h, p, L, st, bias, X.scrub_launches > 0 ? &scrub : nullptr);
        if (rc) return rc;
        RADAD_HIP_CHECK(hipGetLastError());
        RADAD_REQUIRE(!pq || (scrub.launched == X.scrub_launches && h->last_scan_phases == X.phases),
                      "%s: %d scrub launches over %d phases, planned %d over %d", fn, scrub.launched, h->last_scan_phases, X.scrub_launches,
                      X.phases);
        SearchCtx c;
        c.valid = true;
        c.nq = nq; c.k = k; c.l2 = p.l2; c.n_parts = p.n_parts; c.plen = p.plen; c.cap = p.cap; c.xgroup = p.xgroup;
        c.emit = true; c.use_floor = true; c.hi_tile = true; c.canonical = true; c.q_use = q_use; c.ws = L;
        h->last_o_cnt = L.cnt; h->last_o_thr = L.thr; h->last_emit_nq = nq;
        rc = knn_rerank(h, c, nullptr, out_dist_dev, out_idx_dev, out_key_dev, st);
        if (rc) return rc;
        hipLaunchKernelGGL(k_excl_scan_pad, dim3((unsigned)ceil_div64(nq * k, 256)), dim3(256), 0, st, out_dist_dev, (const int64_t*)out_idx_dev,
                           out_key_dev, nq * k);
    } else {
        knn_launch_list_all(flag_sel, flag_count, nq, st);
    }
    RADAD_HIP_CHECK(hipGetLastError());

    // ---- the listed queries (tile route: the ones the certificate rejected): the ROW-FILTERED float64 exact kernel, by the bitmap or
    // with each query's own tags.  No report.
    ExactParams x;
    x.q = q_use; x.sel = flag_sel; x.count = flag_count; x.l2 = p.l2;
    x.pkey = ws_at<double>(h, L.xk); x.pidx = ws_at<int>(h, L.xi);
    x.group = p.xgroup; x.nslots = (int)knn_exact_slots(nq, k, p.xgroup);
    x.out_dist = out_dist_dev; x.out_idx = out_idx_dev; x.out_key = out_key_dev;
    if (bitmap) x.admit = admit;
    else { x.row_tags = r.tags; x.q_tags = r.q_tags; x.q_cnt = r.q_cnt; x.m = r.m(); }
    rc = knn_launch_exact(h, bitmap ? k_exact_scan_excl : k_exact_scan_excl_pq, x, nq, k, st);
    if (rc) return rc;
    rc = knn_post_exact_count(h, h->HC_XS_EXACT, flag_count, st);
    if (rc) return rc;
    h->last_xs_nq = nq; h->last_xs_route = tile ? RADAD_EXCL_SCAN_TILE : RADAD_EXCL_SCAN_EXACT;
    return RADAD_OK;
}

// ---- certified range search (radad_knn_range_search) ------------------------------------------------------------------------------
// Route, facts, plan and the one scan launch are knn_range_plan's (knn_plan.h).  Tile route: the PLAIN search's preparation, RSC and
// bias (as the per-query form of knn_search_excl_scan_locked), k_range_floor into the search's floor array, one scan launch from
// those floors (early abandon included), k_range_refine; the queries whose buffer overflowed go, driven from the device, to the exact
// range kernel.
// Stream route (RADAD_KNN_OPT_RANGE_SMALLQ, <= 16 queries): the small-batch search's preparation and eps, the same floors, ONE launch of
// k_range_hi_smallq into the same buffers, and everything behind the scan as on the tile route -- but for the re-rank's re-score,
// which takes its sums in the exact kernel's order (k_range_refine<.., true>): the keys are the exact route's bit for bit.
// Exact route: that kernel for every query.  Like the siblings above: KnnTuning is read (hi_skip) and never written, no report is
// posted, no turn is taken.
// rule: NULL (radad_knn_range_search), or what the queries exclude (radad_knn_range_search_excl / _excl_pq; knn_range_excl_plan):
//   one set for the batch   the bitmap and the NaN bias of radad_knn_search_excl_scan in front of the scan, which then runs the biased
//                           instantiation with this eps and never emits an excluded row; the plain k_range_refine; overflow and the
//                           exact route go to k_exact_scan_range_excl with the same bitmap;
//   a set per query (m > 0; m == 0 arrives here as NULL)   the plain range search's scan, k_range_refine<true>, which drops a query's
//                           excluded rows while it compacts; overflow and the exact route go to k_exact_scan_range_excl_pq.
static int knn_range_search_locked(const char* fn, radad_knn_t h, const void* q_in, int q_dtype, int64_t nq, float radius, int m,
                                   const ExclRule* rule, int32_t* out_count_dev, float* out_dist_dev, int64_t* out_idx_dev,
                                   double* out_key_dev, hipStream_t st) {
    int rc = knn_order_behind_last(h, st);
    if (rc) return rc;
    const bool batch = rule && !rule->per_query, pq = rule && rule->per_query;
    struct { int route; StoreFacts facts; ScanPlan plan; int launches; } X;
    auto make_plan = [&] {
        if (rule) {
            const RangeExclPlan e = knn_range_excl_plan(knn_store_facts(h), nq, m, pq ? KNN_RANGE_EXCL_PER_QUERY : KNN_RANGE_EXCL_BATCH,
                                                        rule->m(), h->tune.hi_skip);
            X.route = e.route; X.facts = e.facts; X.plan = e.plan; X.launches = e.launches;
        } else {
            const RangePlan e = knn_range_plan(knn_store_facts(h), nq, m, h->tune.hi_skip);
            X.route = e.route; X.facts = e.facts; X.plan = e.plan; X.launches = e.launches;
        }
    };
    make_plan();
    bool tile = X.route == RADAD_RANGE_TILE, stream = X.route == RADAD_RANGE_STREAM;
    if ((tile || stream) && !knn_ensure_hi(h, st, true)) {         // (a plane that cannot be allocated switches itself off: exact route)
        tile = stream = false;
        make_plan();
        RADAD_REQUIRE(X.route == RADAD_RANGE_EXACT, "%s: a store without a plane planned the tile or the stream route", fn);
    }
    if (!tile && !stream && !knn_ensure_hi(h, st, false)) { radad_set_error("store statistics could not be computed"); return RADAD_EHIP; }
    ScanPlan p = X.plan;
    p.mu = (p.hi_q && !h->f16) ? h->cmu : nullptr;                 // the plain search's instantiation (knn_plan_scan) ...
    if (!batch) p.biased = p.hi_q && (p.l2 || p.mu);               // ... (one set for the batch: the biased one whatever the plane, the plan's)
    RADAD_REQUIRE(!(tile || stream) || p.emit_cap <= RG_MAX_CAP, "%s: %d-entry candidate buffers exceed the re-rank's %d", fn, p.emit_cap, RG_MAX_CAP);
    const SearchLayout L = knn_search_layout(X.facts, p, q_dtype);
    rc = knn_workspace(h, L.bytes);
    if (rc) return rc;
    // the exact pass's partial lists, k = m; one set for the batch: the bitmap and the bias array behind them
    const RangeExclLayout E = knn_range_excl_layout(X.facts, nq, m, X.route);
    const RangeLayout B = E.lists;
    rc = knn_excl_reserve(h, batch ? E.bytes : B.bytes);
    if (rc) return rc;
    rc = knn_ensure_xarrive(h, nq, st);
    if (rc) return rc;
    h->last_emit_nq = 0;                                           // (the workspace no longer holds the last plain tile scan's counters)
    h->last_xs_nq = 0;
    h->last_rg_nq = 0;
    unsigned long long* admit = batch ? reinterpret_cast<unsigned long long*>((char*)h->excl_ws + E.admit) : nullptr;
    if (batch) {
        rc = knn_admit_bitmap(h, *rule, nullptr, admit, E.n_words, st);
        if (rc) return rc;
    }
    const float* q_use = knn_prepare_queries(h, p, L, q_in, q_dtype, st);      // (clears the listed-query counter and the candidate counters)
    RADAD_HIP_CHECK(hipGetLastError());
    int* flag_count = ws_at<int>(h, L.fcount);
    int* flag_sel = ws_at<int>(h, L.fsel);

    if (tile || stream) {
        // one set for the batch: the per-call bias, NaN for the rows the bitmap does not admit (no compare of the scan passes a NaN)
        float* bias = batch ? knn_launch_excl_scan_bias(h, p, admit, E.bias, st) : nullptr;
        // scan scores estimate q.y (IP / cosine) or -|q - y|^2 (L2): the threshold in their units
        float* floors = ws_at<float>(h, L.thr);
        hipLaunchKernelGGL(k_range_floor, dim3((unsigned)ceil_div64(nq, 256)), dim3(256), 0, st, ws_at<const float>(h, L.eps),
                           p.l2 ? -radius : radius, floors, nq);
        RADAD_HIP_CHECK(hipGetLastError());
        h->prof.next_search();
        if (tile) rc = knn_scan_hi_tile(h, p, L, st, bias, nullptr, floors);
        else {                                                     // <= 16 queries: the plane streamed once, one launch
            rc = knn_scan_range_smallq(h, p, L, st, bias);
            h->last_splits = p.n_splits; h->last_scan_launches = h->last_scan_phases = 1; h->last_ab_tasks = 0;
        }
        if (rc) return rc;
        RADAD_HIP_CHECK(hipGetLastError());
        RADAD_REQUIRE(h->last_scan_launches == X.launches, "%s: %d scan launches, planned %d", fn, h->last_scan_launches, X.launches);
        h->last_o_cnt = L.cnt; h->last_o_thr = L.thr; h->last_emit_nq = nq;
        RangeRefinePqParams g;
        g.idx = ws_at<const int>(h, L.pi); g.cnt = ws_at<const int>(h, L.cnt); g.cap = p.emit_cap; g.dim = h->dim; g.l2 = p.l2;
        g.db_f16 = h->f16; g.m = m; g.db = h->rows; g.q = q_use; g.radius = (double)radius; g.id_base = h->id_base; g.ntotal = h->ntotal;
        g.flag_count = flag_count; g.flag_sel = flag_sel;
        g.out_count = out_count_dev; g.out_dist = out_dist_dev; g.out_idx = out_idx_dev; g.out_key = out_key_dev;
        if (pq) { g.tags = rule->tags; g.q_tags = rule->q_tags; g.q_cnt = rule->q_cnt; g.n_tags = rule->m(); }
        const size_t glds = pq ? range_refine_pq_lds_bytes() : range_refine_lds_bytes();
        // (the stream route: the instantiations whose float64 keys are the exact route's bit for bit -- a batch of <= 16 queries gets the
        // same keys with the option on and off)
        void (*const refine_pq)(RangeRefinePqParams) = stream ? k_range_refine<true, true> : k_range_refine<true, false>;
        void (*const refine_plain)(RangeRefineParams) = stream ? k_range_refine<false, true> : k_range_refine<false, false>;
        const void* refine = pq ? reinterpret_cast<const void*>(refine_pq) : reinterpret_cast<const void*>(refine_plain);
        RADAD_HIP_CHECK(hipFuncSetAttribute(refine, hipFuncAttributeMaxDynamicSharedMemorySize, (int)glds));
        h->prof.begin(st);                                         // (the call's second profile entry: its re-rank)
        if (pq) hipLaunchKernelGGL(refine_pq, dim3((unsigned)nq), dim3(RF_THREADS), glds, st, g);
        else hipLaunchKernelGGL(refine_plain, dim3((unsigned)nq), dim3(RF_THREADS), glds, st, static_cast<const RangeRefineParams&>(g));
        h->prof.end(st);
    } else {
        RADAD_HIP_CHECK(hipMemsetAsync(out_count_dev, 0, (size_t)nq * sizeof(int32_t), st));
        knn_launch_list_all(flag_sel, flag_count, nq, st);
    }
    RADAD_HIP_CHECK(hipGetLastError());

    // ---- the listed queries (tile and stream routes: k_range_refine zeroed their counts): the float64 exact range kernel at k = m,
    // its partial lists in the exclusion workspace; no report
    ExactParams x;
    x.q = q_use; x.sel = flag_sel; x.count = flag_count; x.l2 = p.l2;
    x.pkey = reinterpret_cast<double*>((char*)h->excl_ws + B.xk); x.pidx = reinterpret_cast<int*>((char*)h->excl_ws + B.xi);
    x.group = B.xgroup; x.nslots = (int)B.xslots;
    x.out_dist = out_dist_dev; x.out_idx = out_idx_dev; x.out_key = out_key_dev;
    x.out_count = out_count_dev;
    x.range_t = p.l2 ? -(double)radius : (double)radius;
    if (batch) x.admit = admit;
    if (pq) { x.row_tags = rule->tags; x.q_tags = rule->q_tags; x.q_cnt = rule->q_cnt; x.m = rule->m(); }
    rc = knn_launch_exact(h, batch ? k_exact_scan_range_excl : pq ? k_exact_scan_range_excl_pq : k_exact_scan_range, x, nq, m, st);
    if (rc) return rc;
    rc = knn_post_exact_count(h, h->HC_RG_EXACT, flag_count, st);
    if (rc) return rc;
    h->last_rg_nq = nq; h->last_rg_route = tile ? RADAD_RANGE_TILE : stream ? RADAD_RANGE_STREAM : RADAD_RANGE_EXACT;
    return RADAD_OK;
}

// the four top-k exclusion calls behind their own argument checks (as knn_range_search_entry for the range calls): in_scan = the
// admission test inside the tile scan (k_fetch is not used), else the two-pass search at k_fetch
static int knn_excl_search_entry(const char* fn, radad_knn_t h, const void* q_dev, int q_dtype, int64_t nq, int k, int k_fetch, bool in_scan,
                                 const ExclRule& r, float* out_dist_dev, int64_t* out_idx_dev, double* out_key_dev, void* stream) {
    if (nq == 0) return RADAD_OK;
    RADAD_REQUIRE(q_dev && out_dist_dev && out_idx_dev, "%s: NULL buffer", fn);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    RADAD_REQUIRE(!h->pending.valid && !h->pending_excl.valid, "%s: a radad_knn_search_begin on this handle has not been finished", fn);
    if (h->ntotal == 0) { radad_set_error("%s: the store is empty", fn); return RADAD_ESTATE; }
    if (in_scan) return knn_search_excl_scan_locked(fn, h, q_dev, q_dtype, nq, k, r, out_dist_dev, out_idx_dev, out_key_dev, (hipStream_t)stream);
    return knn_search_excl_locked(h, q_dev, q_dtype, nq, k, k_fetch, r, out_dist_dev, out_idx_dev, out_key_dev, (hipStream_t)stream);
}

extern "C" {

int radad_knn_search_begin(radad_knn_t h, const void* q_dev, int q_dtype, int64_t nq, int k, float* kth_lower_bound_dev, void* stream) {
    RADAD_REQUIRE(h, "NULL handle");
    RADAD_REQUIRE(q_dtype == RADAD_Q_F32 || q_dtype == RADAD_Q_BF16, "radad_knn_search_begin: unsupported query dtype %d", q_dtype);
    RADAD_REQUIRE(k >= 1 && k <= RADAD_KNN_MAX_K, "radad_knn_search_begin: k=%d outside [1,%d]", k, RADAD_KNN_MAX_K);
    RADAD_REQUIRE(nq > 0 && nq < (1ll << 31) - KT_N, "radad_knn_search_begin: bad nq");
    RADAD_REQUIRE(knn_exact_fits(h->dim, k), "radad_knn_search_begin: dim %d x k %d too large for the exact kernel (dim * 4 + 96 k + 16 <= %zu)", h->dim, k, KX_LDS_MAX);
    RADAD_REQUIRE(q_dev && kth_lower_bound_dev, "radad_knn_search_begin: NULL buffer");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    RADAD_REQUIRE(!h->pending.valid && !h->pending_excl.valid, "radad_knn_search_begin: the previous begin on this handle has not been finished");
    SearchCtx c;
    int rc = knn_search_phase1(h, q_dev, q_dtype, nq, k, KNN_MARGIN, kth_lower_bound_dev, (hipStream_t)stream, &c);
    if (rc) return rc;
    RADAD_HIP_CHECK(hipEventRecord(h->ev_begun, (hipStream_t)stream));
    h->pending = c;
    return RADAD_OK;
}

int radad_knn_search_abort(radad_knn_t h) {
    RADAD_REQUIRE(h, "NULL handle");
    std::lock_guard<std::mutex> lk(h->mu);
    h->pending.valid = false;                 // (the workspace of the abandoned first half is simply reused by the next search)
    h->pending_excl.valid = false;
    return RADAD_OK;
}

int radad_knn_search_finish(radad_knn_t h, const float* global_lower_bound_dev, float* out_dist_dev, int64_t* out_idx_dev,
                            double* out_key_dev, void* stream) {
    RADAD_REQUIRE(h, "NULL handle");
    RADAD_REQUIRE(out_dist_dev && out_idx_dev, "radad_knn_search_finish: NULL buffer");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    RADAD_REQUIRE(h->pending.valid, "radad_knn_search_finish: no search was begun on this handle");
    const SearchCtx c = h->pending;
    h->pending.valid = false;
    RADAD_HIP_CHECK(hipStreamWaitEvent((hipStream_t)stream, h->ev_begun, 0));       // the scan of _begin (no-op on the same stream)
    return knn_search_phase2(h, c, global_lower_bound_dev, false, out_dist_dev, out_idx_dev, out_key_dev, (hipStream_t)stream);
}

int radad_knn_search_excl(radad_knn_t h, const void* q_dev, int q_dtype, int64_t nq, int k, int k_fetch, const int64_t* row_tags_dev,
                          const int64_t* excl_sorted_dev, int64_t n_excl, float* out_dist_dev, int64_t* out_idx_dev, double* out_key_dev,
                          void* stream) {
    const char* fn = "radad_knn_search_excl";
    const int bad = knn_excl_check_args(fn, h, q_dtype, nq, 0, k, k_fetch, row_tags_dev, excl_sorted_dev, n_excl);
    if (bad) return bad;
    return knn_excl_search_entry(fn, h, q_dev, q_dtype, nq, k, k_fetch, false, knn_excl_rule_batch(row_tags_dev, excl_sorted_dev, n_excl),
                                 out_dist_dev, out_idx_dev, out_key_dev, stream);
}

int radad_knn_search_excl_pq(radad_knn_t h, const void* q_dev, int q_dtype, int64_t nq, int k, int k_fetch, const int64_t* row_tags_dev,
                             const int64_t* q_tags_dev, int m, const int32_t* q_tag_counts_dev, float* out_dist_dev, int64_t* out_idx_dev,
                             double* out_key_dev, void* stream) {
    const char* fn = "radad_knn_search_excl_pq";
    int bad = knn_excl_check_args(fn, h, q_dtype, nq, 0, k, k_fetch, nullptr, nullptr, 0);
    if (bad) return bad;
    ExclRule r;
    bad = knn_excl_pq_rule(fn, row_tags_dev, q_tags_dev, m, q_tag_counts_dev, &r);
    if (bad) return bad;
    return knn_excl_search_entry(fn, h, q_dev, q_dtype, nq, k, k_fetch, false, r, out_dist_dev, out_idx_dev, out_key_dev, stream);
}

int radad_knn_search_excl_scan(radad_knn_t h, const void* q_dev, int q_dtype, int64_t nq, int k, const int64_t* row_tags_dev,
                               const int64_t* excl_sorted_dev, int64_t n_excl, float* out_dist_dev, int64_t* out_idx_dev, double* out_key_dev,
                               void* stream) {
    const char* fn = "radad_knn_search_excl_scan";
    const int bad = knn_excl_check_args(fn, h, q_dtype, nq, 0, k, k, row_tags_dev, excl_sorted_dev, n_excl);
    if (bad) return bad;
    return knn_excl_search_entry(fn, h, q_dev, q_dtype, nq, k, k, true, knn_excl_rule_batch(row_tags_dev, excl_sorted_dev, n_excl),
                                 out_dist_dev, out_idx_dev, out_key_dev, stream);
}

int radad_knn_search_excl_scan_pq(radad_knn_t h, const void* q_dev, int q_dtype, int64_t nq, int k, const int64_t* row_tags_dev,
                                  const int64_t* q_tags_dev, int m, const int32_t* q_tag_counts_dev, float* out_dist_dev, int64_t* out_idx_dev,
                                  double* out_key_dev, void* stream) {
    const char* fn = "radad_knn_search_excl_scan_pq";
    int bad = knn_excl_check_args(fn, h, q_dtype, nq, 0, k, k, nullptr, nullptr, 0);
    if (bad) return bad;
    ExclRule r;
    bad = knn_excl_pq_rule(fn, row_tags_dev, q_tags_dev, m, q_tag_counts_dev, &r);
    if (bad) return bad;
    return knn_excl_search_entry(fn, h, q_dev, q_dtype, nq, k, k, true, r, out_dist_dev, out_idx_dev, out_key_dev, stream);
}

// the three range calls behind their own argument checks: rule NULL = nothing is excluded
static int knn_range_search_entry(const char* fn, radad_knn_t h, const void* q_dev, int q_dtype, int64_t nq, float radius, int max_per_query,
                                  const ExclRule* rule, int32_t* out_count_dev, float* out_dist_dev, int64_t* out_idx_dev,
                                  double* out_key_dev, void* stream) {
    if (nq == 0) return RADAD_OK;
    RADAD_REQUIRE(q_dev && out_count_dev && out_dist_dev && out_idx_dev, "%s: NULL buffer", fn);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    RADAD_REQUIRE(!h->pending.valid && !h->pending_excl.valid, "%s: a radad_knn_search_begin on this handle has not been finished", fn);
    if (h->ntotal == 0) { radad_set_error("%s: the store is empty", fn); return RADAD_ESTATE; }
    return knn_range_search_locked(fn, h, q_dev, q_dtype, nq, radius, max_per_query, rule, out_count_dev, out_dist_dev, out_idx_dev,
                                   out_key_dev, (hipStream_t)stream);
}
// what every range call refuses, before anything else
static int knn_range_check_args(const char* fn, radad_knn_t h, int q_dtype, int64_t nq, float radius, int max_per_query) {
    RADAD_REQUIRE(h, "NULL handle");
    RADAD_REQUIRE(q_dtype == RADAD_Q_F32 || q_dtype == RADAD_Q_BF16, "%s: unsupported query dtype %d", fn, q_dtype);
    RADAD_REQUIRE(max_per_query >= 1 && max_per_query <= RADAD_KNN_MAX_K, "%s: max_per_query=%d outside [1,%d]", fn, max_per_query,
                  RADAD_KNN_MAX_K);
    RADAD_REQUIRE(knn_exact_fits(h->dim, max_per_query), "%s: dim %d x max_per_query %d too large for the exact kernel (dim * 4 + 96 k + 16 <= %zu)",
                  fn, h->dim, max_per_query, KX_LDS_MAX);
    RADAD_REQUIRE(radius == radius, "%s: the radius is not a number", fn);
    RADAD_REQUIRE(nq >= 0 && nq < (1ll << 31) - KT_N, "%s: bad nq", fn);
    return RADAD_OK;
}

int radad_knn_range_search(radad_knn_t h, const void* q_dev, int q_dtype, int64_t nq, float radius, int max_per_query,
                           int32_t* out_count_dev, float* out_dist_dev, int64_t* out_idx_dev, double* out_key_dev, void* stream) {
    const int bad = knn_range_check_args("radad_knn_range_search", h, q_dtype, nq, radius, max_per_query);
    if (bad) return bad;
    return knn_range_search_entry("radad_knn_range_search", h, q_dev, q_dtype, nq, radius, max_per_query, nullptr, out_count_dev, out_dist_dev,
                                  out_idx_dev, out_key_dev, stream);
}

int radad_knn_range_search_excl(radad_knn_t h, const void* q_dev, int q_dtype, int64_t nq, float radius, int max_per_query,
                                const int64_t* row_tags_dev, const int64_t* excl_sorted_dev, int64_t n_excl, int32_t* out_count_dev,
                                float* out_dist_dev, int64_t* out_idx_dev, double* out_key_dev, void* stream) {
    const char* fn = "radad_knn_range_search_excl";
    const int bad = knn_range_check_args(fn, h, q_dtype, nq, radius, max_per_query);
    if (bad) return bad;
    RADAD_REQUIRE(n_excl >= 0 && (n_excl == 0 || (excl_sorted_dev && row_tags_dev)), "%s: %lld excluded tags need the exclusion set and the row tags",
                  fn, (long long)n_excl);
    const ExclRule r = knn_excl_rule_batch(row_tags_dev, excl_sorted_dev, n_excl);
    return knn_range_search_entry(fn, h, q_dev, q_dtype, nq, radius, max_per_query, &r, out_count_dev, out_dist_dev, out_idx_dev, out_key_dev, stream);
}

int radad_knn_range_search_excl_pq(radad_knn_t h, const void* q_dev, int q_dtype, int64_t nq, float radius, int max_per_query,
                                   const int64_t* row_tags_dev, const int64_t* q_tags_dev, int m, const int32_t* q_tag_counts_dev,
                                   int32_t* out_count_dev, float* out_dist_dev, int64_t* out_idx_dev, double* out_key_dev, void* stream) {
    const char* fn = "radad_knn_range_search_excl_pq";
    int bad = knn_range_check_args(fn, h, q_dtype, nq, radius, max_per_query);
    if (bad) return bad;
    ExclRule r;
    bad = knn_excl_pq_rule(fn, row_tags_dev, q_tags_dev, m, q_tag_counts_dev, &r);
    if (bad) return bad;
    // m == 0: nothing is excluded -- the plain range search outright
    return knn_range_search_entry(fn, h, q_dev, q_dtype, nq, radius, max_per_query, m > 0 ? &r : nullptr, out_count_dev, out_dist_dev, out_idx_dev,
                                  out_key_dev, stream);
}

int radad_knn_last_range(radad_knn_t h, int64_t* n_queries, int* route, int* n_exact) {
    RADAD_REQUIRE(h && route && n_exact, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    RADAD_HIP_CHECK(knn_wait_last_search(h));
    *n_exact = h->last_rg_nq > 0 ? *reinterpret_cast<volatile int*>(h->host_count + h->HC_RG_EXACT) : 0;
    *route = h->last_rg_route;
    if (n_queries) *n_queries = h->last_rg_nq;
    return RADAD_OK;
}

int radad_knn_last_excl_scan(radad_knn_t h, int64_t* n_queries, int* route, int* n_exact) {
    RADAD_REQUIRE(h && route && n_exact, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    RADAD_HIP_CHECK(knn_wait_last_search(h));
    *n_exact = h->last_xs_nq > 0 ? *reinterpret_cast<volatile int*>(h->host_count + h->HC_XS_EXACT) : 0;
    *route = h->last_xs_route;
    if (n_queries) *n_queries = h->last_xs_nq;
    return RADAD_OK;
}

int radad_knn_last_excl(radad_knn_t h, int64_t* n_queries, int* n_exact) {
    RADAD_REQUIRE(h && n_exact, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    RADAD_HIP_CHECK(knn_wait_last_search(h));
    *n_exact = 0;
    if (h->last_excl_nq > 0 && h->excl_ws)
        RADAD_HIP_CHECK(hipMemcpy(n_exact, (const char*)h->excl_ws + h->excl_o_count, sizeof(int), hipMemcpyDeviceToHost));
    if (n_queries) *n_queries = h->last_excl_nq;
    return RADAD_OK;
}

int radad_knn_search_excl_begin(radad_knn_t h, const void* q_dev, int q_dtype, int64_t nq, int k, int k_fetch, const int64_t* row_tags_dev,
                                const int64_t* excl_sorted_dev, int64_t n_excl, double* out_key_dev, int64_t* out_idx_dev,
                                double* frontier_key_dev, int64_t* frontier_idx_dev, void* stream) {
    const int bad = knn_excl_check_args("radad_knn_search_excl_begin", h, q_dtype, nq, 1, k, k_fetch, row_tags_dev, excl_sorted_dev, n_excl);
    if (bad) return bad;
    RADAD_REQUIRE(q_dev && out_key_dev && out_idx_dev && frontier_key_dev && frontier_idx_dev, "radad_knn_search_excl_begin: NULL buffer");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    RADAD_REQUIRE(!h->pending.valid && !h->pending_excl.valid, "radad_knn_search_excl_begin: the previous begin on this handle has not been finished");
    if (h->ntotal == 0) { radad_set_error("radad_knn_search_excl_begin: the store is empty"); return RADAD_ESTATE; }
    return knn_search_excl_begin_locked(h, q_dev, q_dtype, nq, k, k_fetch, knn_excl_rule_batch(row_tags_dev, excl_sorted_dev, n_excl),
                                        out_key_dev, out_idx_dev, frontier_key_dev, frontier_idx_dev, (hipStream_t)stream);
}

int radad_knn_search_excl_pq_begin(radad_knn_t h, const void* q_dev, int q_dtype, int64_t nq, int k, int k_fetch, const int64_t* row_tags_dev,
                                   const int64_t* q_tags_dev, int m, const int32_t* q_tag_counts_dev, double* out_key_dev,
                                   int64_t* out_idx_dev, double* frontier_key_dev, int64_t* frontier_idx_dev, void* stream) {
    int bad = knn_excl_check_args("radad_knn_search_excl_pq_begin", h, q_dtype, nq, 1, k, k_fetch, nullptr, nullptr, 0);
    if (bad) return bad;
    ExclRule r;
    bad = knn_excl_pq_rule("radad_knn_search_excl_pq_begin", row_tags_dev, q_tags_dev, m, q_tag_counts_dev, &r);
    if (bad) return bad;
    RADAD_REQUIRE(q_dev && out_key_dev && out_idx_dev && frontier_key_dev && frontier_idx_dev, "radad_knn_search_excl_pq_begin: NULL buffer");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    RADAD_REQUIRE(!h->pending.valid && !h->pending_excl.valid, "radad_knn_search_excl_pq_begin: the previous begin on this handle has not been finished");
    if (h->ntotal == 0) { radad_set_error("radad_knn_search_excl_pq_begin: the store is empty"); return RADAD_ESTATE; }
    return knn_search_excl_begin_locked(h, q_dev, q_dtype, nq, k, k_fetch, r, out_key_dev, out_idx_dev, frontier_key_dev, frontier_idx_dev,
                                        (hipStream_t)stream);
}

int radad_knn_search_excl_finish(radad_knn_t h, const int* unproved_dev, float* out_dist_dev, int64_t* out_idx_dev, double* out_key_dev,
                                 void* stream) {
    RADAD_REQUIRE(h, "NULL handle");
    RADAD_REQUIRE(out_dist_dev && out_idx_dev, "radad_knn_search_excl_finish: NULL buffer");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    RADAD_REQUIRE(h->pending_excl.valid, "radad_knn_search_excl_finish: no exclusion-aware search was begun on this handle");
    const ExclCtx e = h->pending_excl;
    h->pending_excl.valid = false;
    hipStream_t st = (hipStream_t)stream;
    RADAD_HIP_CHECK(hipStreamWaitEvent(st, h->ev_begun, 0));       // the device work of _begin (no-op on the same stream)
    h->last_stream = st;                                            // whatever comes next on the handle orders itself behind this
    h->have_last = true;
    auto at = [&](size_t o) { return (char*)h->excl_ws + o; };
    const size_t n = (size_t)e.nq * e.k;
    RADAD_HIP_CHECK(hipMemcpyAsync(out_dist_dev, at(e.L.bd), n * sizeof(float), hipMemcpyDeviceToDevice, st));
    RADAD_HIP_CHECK(hipMemcpyAsync(out_idx_dev, at(e.L.bi), n * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    if (out_key_dev) RADAD_HIP_CHECK(hipMemcpyAsync(out_key_dev, at(e.L.bk), n * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (!unproved_dev || e.rule.n_excl == 0) return RADAD_OK;           // nothing excluded: every shard list is the shard's exact top k
    hipLaunchKernelGGL(k_excl_flags_to_list, dim3((unsigned)ceil_div64(e.nq, 256)), dim3(256), 0, st, unproved_dev, (const int*)at(e.L.own),
                       e.nq, (int*)at(e.L.count), (int*)at(e.L.sel));
    RADAD_HIP_CHECK(hipGetLastError());
    return knn_excl_exact_pass(h, e.L, e.nq, e.k, e.l2, e.q_use, e.rule, out_dist_dev, out_idx_dev, out_key_dev, st);
}

int radad_excl_merge_certify(int metric, const double* in_key_dev, const int64_t* in_idx_dev, const double* frontier_key_dev,
                             const int64_t* frontier_idx_dev, int n_parts, int64_t nq, int k, float* out_dist_dev, int64_t* out_idx_dev,
                             double* out_key_dev, int* unproved_out_dev, int device, void* stream) {
    RADAD_REQUIRE(metric >= 0 && metric <= 2, "radad_excl_merge_certify: bad metric");
    RADAD_REQUIRE(n_parts >= 1 && n_parts <= 4096 && k >= 1 && k <= RADAD_KNN_MAX_K && nq >= 0, "radad_excl_merge_certify: bad shape");
    if (nq == 0) return RADAD_OK;
    RADAD_REQUIRE(in_key_dev && in_idx_dev && frontier_key_dev && frontier_idx_dev && out_dist_dev && out_idx_dev && unproved_out_dev,
                  "radad_excl_merge_certify: NULL buffer");
    DeviceGuard g(device);
    ExclMergeParams m;
    m.key = in_key_dev; m.idx = in_idx_dev; m.fr_key = frontier_key_dev; m.fr_idx = frontier_idx_dev;
    m.n_parts = n_parts; m.k = k; m.l2 = metric == RADAD_METRIC_L2; m.nq = nq;
    m.out_dist = out_dist_dev; m.out_idx = out_idx_dev; m.out_key = out_key_dev; m.unproved = unproved_out_dev;
    hipLaunchKernelGGL(k_excl_merge_certify, dim3((unsigned)ceil_div64(nq, 4)), dim3(256), 4 * n_parts * sizeof(int), (hipStream_t)stream, m);
    RADAD_HIP_CHECK(hipGetLastError());
    return RADAD_OK;
}

}  // extern "C"

extern "C" {

int radad_knn_search_host(radad_knn_t h, const float* q_host, int64_t nq, int k, float* out_dist_host,
                          int64_t* out_idx_host) {
    RADAD_REQUIRE(h, "NULL handle");
    if (nq == 0) return RADAD_OK;
    RADAD_REQUIRE(q_host && out_dist_host && out_idx_host && nq > 0 && k >= 1, "radad_knn_search_host: bad argument");
    DeviceGuard g(h->device);
    float *dq = nullptr, *dd = nullptr;
    int64_t* di = nullptr;
    const size_t qb = (size_t)nq * h->dim * sizeof(float);
    int rc = RADAD_OK;
    if (hipMalloc(&dq, qb) != hipSuccess || hipMalloc(&dd, (size_t)nq * k * sizeof(float)) != hipSuccess ||
        hipMalloc(&di, (size_t)nq * k * sizeof(int64_t)) != hipSuccess) {
        radad_set_error("hipMalloc of search staging buffers failed");
        rc = RADAD_ENOMEM;
    }
    if (rc == RADAD_OK && hipMemcpy(dq, q_host, qb, hipMemcpyHostToDevice) != hipSuccess) { radad_set_error("H2D copy failed"); rc = RADAD_EHIP; }
    if (rc == RADAD_OK) rc = radad_knn_search(h, dq, nq, k, dd, di, nullptr);
    if (rc == RADAD_OK && (hipMemcpy(out_dist_host, dd, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
                           hipMemcpy(out_idx_host, di, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost) != hipSuccess)) {
        radad_set_error("D2H copy failed: %s", hipGetErrorString(hipGetLastError()));
        rc = RADAD_EHIP;
    }
    if (dq) (void)hipFree(dq);
    if (dd) (void)hipFree(dd);
    if (di) (void)hipFree(di);
    return rc;
}

int radad_knn_reconstruct(radad_knn_t h, const int64_t* idx_dev, int64_t n, float* out_dev, void* stream) {
    RADAD_REQUIRE(h, "NULL handle");
    if (n == 0) return RADAD_OK;
    RADAD_REQUIRE(idx_dev && out_dev && n > 0, "radad_knn_reconstruct: bad argument");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    if (h->f16)
        hipLaunchKernelGGL(k_gather_rows<_Float16>, dim3((unsigned)ceil_div64(n, 4)), dim3(256), 0, (hipStream_t)stream,
                           (const _Float16*)h->rows, idx_dev, n, h->ntotal, h->id_base, h->dim, out_dev);
    else
        hipLaunchKernelGGL(k_gather_rows<float>, dim3((unsigned)ceil_div64(n, 4)), dim3(256), 0, (hipStream_t)stream,
                           (const float*)h->rows, idx_dev, n, h->ntotal, h->id_base, h->dim, out_dev);
    RADAD_HIP_CHECK(hipGetLastError());
    return RADAD_OK;
}

int radad_knn_reconstruct_host(radad_knn_t h, const int64_t* idx_host, int64_t n, float* out_host) {
    RADAD_REQUIRE(h, "NULL handle");
    if (n == 0) return RADAD_OK;
    RADAD_REQUIRE(idx_host && out_host && n > 0, "radad_knn_reconstruct_host: bad argument");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    // small n (pipeline.py:503 fetches K rows per query): copy row by row straight from the store
    for (int64_t i = 0; i < n; ++i) {
        const int64_t r = idx_host[i] - h->id_base;
        float* dst = out_host + i * h->dim;
        if (idx_host[i] < 0 || r < 0 || r >= h->ntotal) { memset(dst, 0, sizeof(float) * h->dim); continue; }
        if (h->f16) {
            std::vector<_Float16> tmp((size_t)h->dim);
            RADAD_HIP_CHECK(hipMemcpy(tmp.data(), h->rows + (size_t)r * h->row_bytes(), h->row_bytes(), hipMemcpyDeviceToHost));
            for (int c = 0; c < h->dim; ++c) dst[c] = (float)tmp[c];
        } else {
            RADAD_HIP_CHECK(hipMemcpy(dst, h->rows + (size_t)r * h->row_bytes(), h->row_bytes(), hipMemcpyDeviceToHost));
        }
    }
    return RADAD_OK;
}

int radad_knn_profile(radad_knn_t h, int enable) {
    RADAD_REQUIRE(h, "NULL handle");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    int rc = h->prof.enable(enable != 0, enable);
    if (rc) radad_set_error("hipEventCreate failed");
    return rc;
}

int radad_knn_profile_read(radad_knn_t h, float* ms_out, int cap, int* n_out) {
    RADAD_REQUIRE(h && ms_out && cap >= 0, "radad_knn_profile_read: bad argument");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    int rc = h->prof.read(ms_out, cap, n_out);
    if (rc) radad_set_error("reading profile events failed");
    return rc;
}

int radad_knn_last_recheck(radad_knn_t h, int* n_queries) {
    RADAD_REQUIRE(h && n_queries, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    const int ls = h->tune.last_slot();
    RADAD_HIP_CHECK(knn_wait_last_search(h));
    *n_queries = (h->host_count && h->tune.search_seq) ? h->host_count[8 * ls] : 0;
    return RADAD_OK;
}

int radad_knn_last_certificate(radad_knn_t h, int64_t* n_queries, int* stats6) {
    RADAD_REQUIRE(h && stats6, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    const int ls = h->tune.last_slot();
    RADAD_HIP_CHECK(knn_wait_last_search(h));
    for (int i = 0; i < 6; ++i) stats6[i] = (h->host_count && h->tune.search_seq) ? h->host_count[8 * ls + i] : 0;
    if (n_queries) *n_queries = h->tune.search_seq ? h->count_nq[ls] : 0;
    return RADAD_OK;
}

int radad_knn_last_launch(radad_knn_t h, int* n_query_tiles, int* n_db_splits, int* block_threads) {
    RADAD_REQUIRE(h, "NULL handle");
    if (n_query_tiles) *n_query_tiles = h->last_qtiles;
    if (n_db_splits) *n_db_splits = h->last_splits;
    if (block_threads) *block_threads = h->last_threads;
    return RADAD_OK;
}

int radad_knn_plane_info(radad_knn_t h, int* built, int* centred, int* one_scale) {
    RADAD_REQUIRE(h, "NULL handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (built) *built = (h->hi != nullptr && h->hi_rows > 0) ? 1 : 0;
    if (centred) *centred = h->cmu != nullptr ? 1 : 0;
    if (one_scale) *one_scale = (h->hi != nullptr && h->rscale == nullptr) ? 1 : 0;
    return RADAD_OK;
}

int radad_knn_plane_rebuilds(radad_knn_t h, int* n_out) {
    RADAD_REQUIRE(h && n_out, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    *n_out = h->tune.plane_rebuilds;
    return RADAD_OK;
}

int radad_knn_last_emitted(radad_knn_t h, int* counts_host, float* floors_host, int64_t nq) {
    RADAD_REQUIRE(h && counts_host, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    RADAD_REQUIRE(h->last_emit_nq > 0 && nq == h->last_emit_nq && h->ws, "radad_knn_last_emitted: the last search of this handle was not a tile scan of %lld queries", (long long)nq);
    RADAD_HIP_CHECK(knn_wait_last_search(h));
    RADAD_HIP_CHECK(hipMemcpy(counts_host, (const char*)h->ws + h->last_o_cnt, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost));
    if (floors_host) RADAD_HIP_CHECK(hipMemcpy(floors_host, (const char*)h->ws + h->last_o_thr, (size_t)nq * sizeof(float), hipMemcpyDeviceToHost));
    return RADAD_OK;
}

int radad_knn_last_abandon(radad_knn_t h, int64_t* checked, int64_t* skipped, int64_t* tasks) {
    RADAD_REQUIRE(h && checked && skipped && tasks, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    *checked = *skipped = *tasks = 0;
    if (h->last_ab_tasks <= 0 || !h->ws) return RADAD_OK;       // the last search launched no abandoning scan
    RADAD_HIP_CHECK(knn_wait_last_search(h));
    int c2[2] = {0, 0};
    RADAD_HIP_CHECK(hipMemcpy(c2, (const char*)h->ws + h->last_o_ab, sizeof(c2), hipMemcpyDeviceToHost));
    *checked = c2[0]; *skipped = c2[1]; *tasks = h->last_ab_tasks;
    return RADAD_OK;
}

int radad_knn_last_abandon_deal(radad_knn_t h, int* launches, int* workgroups, int* granule) {
    RADAD_REQUIRE(h && launches && workgroups && granule, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    *launches = *workgroups = *granule = 0;
    if (h->last_ab_tasks <= 0) return RADAD_OK;                 // the last search launched no abandoning scan
    *launches = h->last_deal_launches; *workgroups = h->last_deal_workgroups; *granule = h->last_deal_granule;
    return RADAD_OK;
}

int radad_knn_last_abandon_defer(radad_knn_t h, int64_t* tile_tasks_deferred, int64_t* rows_listed, int* tail_launches) {
    RADAD_REQUIRE(h && tile_tasks_deferred && rows_listed && tail_launches, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    *tile_tasks_deferred = *rows_listed = 0; *tail_launches = 0;
    if (h->last_ab_tasks <= 0 || h->last_defer_launches <= 0 || !h->deal_cnt) return RADAD_OK;       // the last search deferred nothing
    RADAD_HIP_CHECK(knn_wait_last_search(h));
    int c[KNN_DEAL_COUNTERS];
    RADAD_HIP_CHECK(hipMemcpy(c, h->deal_cnt, sizeof(c), hipMemcpyDeviceToHost));
    for (int s = 0; s < KNN_DEFER_SETS; ++s) {
        if (!(h->last_defer_sets >> s & 1u)) continue;
        for (int qt = 0; qt < KNN_DEFER_MAX_QTILES; ++qt) *rows_listed += c[knn_defer_counter(s, qt)];
        *tile_tasks_deferred += c[knn_defer_tasks_counter(s)];
    }
    *tail_launches = h->last_defer_launches;
    return RADAD_OK;
}

int radad_knn_last_abandon_ahead(radad_knn_t h, int64_t* heads_used, int64_t* heads_wasted) {
    RADAD_REQUIRE(h && heads_used && heads_wasted, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    *heads_used = *heads_wasted = 0;
    if (h->last_ab_tasks <= 0 || h->last_ahead_sets == 0 || !h->deal_cnt) return RADAD_OK;          // the last search prefetched no head
    RADAD_HIP_CHECK(knn_wait_last_search(h));
    int c[KNN_DEAL_COUNTERS];
    RADAD_HIP_CHECK(hipMemcpy(c, h->deal_cnt, sizeof(c), hipMemcpyDeviceToHost));
    for (int s = 0; s < KNN_DEAL_SETS; ++s) {
        if (!(h->last_ahead_sets >> s & 1u)) continue;
        *heads_used += c[knn_ahead_counter(s)];
        *heads_wasted += c[knn_ahead_counter(s) + 1];
    }
    return RADAD_OK;
}

int radad_knn_scan_geometry(int64_t n_rows, int64_t n_queries, int* query_tiles, int* chunks, int64_t* rows_per_chunk) {
    RADAD_REQUIRE(n_rows >= 1 && n_queries >= 1 && query_tiles && chunks && rows_per_chunk, "radad_knn_scan_geometry: bad argument");
    knn_geometry_wide(n_rows, n_queries, query_tiles, chunks, rows_per_chunk);
    return RADAD_OK;
}

int radad_knn_last_scan_phases(radad_knn_t h, int* n_phases) {
    RADAD_REQUIRE(h && n_phases, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    *n_phases = h->last_scan_phases;
    return RADAD_OK;
}

int radad_knn_tuning_info(radad_knn_t h, int* cap_boost, int* fp32_searches_left, int64_t* reports_consumed) {
    RADAD_REQUIRE(h && cap_boost && fp32_searches_left && reports_consumed, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    *cap_boost = h->tune.cap_boost;
    *fp32_searches_left = h->tune.hi_skip;
    *reports_consumed = h->tune.reports_consumed;
    return RADAD_OK;
}

int radad_knn_last_scan_launches(radad_knn_t h, int* n_launches) {
    RADAD_REQUIRE(h && n_launches, "NULL argument");
    *n_launches = h->last_scan_launches;
    return RADAD_OK;
}

int radad_knn_last_scan_kind(radad_knn_t h, int* kind) {
    RADAD_REQUIRE(h && kind, "NULL argument");
    *kind = h->last_kind;
    return RADAD_OK;
}

// ---- snapshot: "RADADKNN" | u32 version (2) | i32 dim | i32 metric | i32 store dtype | i64 ntotal | rows as stored
// (already normalised for cosine; fp32 or fp16).  Version 1 files (no dtype field, fp32 rows) are still read.
}  // extern "C"

namespace {

constexpr uint32_t SNAP_VERSION = 2;
constexpr size_t SNAP_STAGE_BYTES = 32ull << 20;   // two pinned staging buffers of this size per transfer

struct SnapHeader {
    uint32_t ver = 0;
    int32_t dim = 0, metric = 0, dtype = RADAD_STORE_F32;
    int64_t ntotal = 0;
    size_t payload_off = 0;   // byte offset of row 0
};

// "RADADKNN" | u32 ver | i32 dim | i32 metric | [v2: i32 dtype] | i64 ntotal | rows
bool snap_parse(const unsigned char* p, size_t len, SnapHeader* out) {
    if (len < 28 || memcmp(p, "RADADKNN", 8) != 0) return false;
    size_t o = 8;
    memcpy(&out->ver, p + o, 4); o += 4;
    if (out->ver != 1 && out->ver != 2) return false;
    memcpy(&out->dim, p + o, 4); o += 4;
    memcpy(&out->metric, p + o, 4); o += 4;
    out->dtype = RADAD_STORE_F32;
    if (out->ver >= 2) { memcpy(&out->dtype, p + o, 4); o += 4; }
    if (len < o + 8) return false;
    memcpy(&out->ntotal, p + o, 8); o += 8;
    out->payload_off = o;
    return out->dim > 0 && out->ntotal >= 0 && (out->dtype == RADAD_STORE_F32 || out->dtype == RADAD_STORE_F16);
}

// read-only mapping of a snapshot file; pages come in on demand, so a shard only touches its own byte range
struct SnapMap {
    int fd = -1;
    const unsigned char* base = nullptr;
    size_t len = 0;
    ~SnapMap() {
        if (base) munmap(const_cast<unsigned char*>(base), len);
        if (fd >= 0) close(fd);
    }
    int open_ro(const char* path) {
        fd = ::open(path, O_RDONLY);
        if (fd < 0) { radad_set_error("cannot open %s", path); return RADAD_EIO; }
        struct stat st;
        if (fstat(fd, &st) != 0 || st.st_size <= 0) { radad_set_error("%s: cannot stat / empty file", path); return RADAD_EIO; }
        len = (size_t)st.st_size;
        void* m = mmap(nullptr, len, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m == MAP_FAILED) { radad_set_error("%s: mmap failed", path); return RADAD_EIO; }
        base = static_cast<const unsigned char*>(m);
        return RADAD_OK;
    }
};

// two pinned buffers + a private stream: the CPU fills (or drains) one buffer while the DMA engine moves the other
struct PinnedPipe {
    char* buf[2] = {nullptr, nullptr};
    hipEvent_t done[2] = {nullptr, nullptr};
    hipStream_t st = nullptr;
    ~PinnedPipe() {
        for (int i = 0; i < 2; ++i) {
            if (done[i]) (void)hipEventDestroy(done[i]);
            if (buf[i]) (void)hipHostFree(buf[i]);
        }
        if (st) (void)hipStreamDestroy(st);
    }
    int init() {
        RADAD_HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        for (int i = 0; i < 2; ++i) {
            RADAD_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&buf[i]), SNAP_STAGE_BYTES, hipHostMallocDefault));
            RADAD_HIP_CHECK(hipEventCreateWithFlags(&done[i], hipEventDisableTiming));
        }
        return RADAD_OK;
    }
};

int snap_load_range(radad_knn_t h, const char* path, int64_t row0, int64_t n_rows) {
    SnapMap map;
    int rc = map.open_ro(path);
    if (rc) return rc;
    SnapHeader hd;
    const int32_t want = h->f16 ? RADAD_STORE_F16 : RADAD_STORE_F32;
    if (!snap_parse(map.base, map.len, &hd) || hd.dim != h->dim || hd.metric != h->metric || hd.dtype != want) {
        radad_set_error("%s: bad header or mismatch (file dim %d metric %d dtype %d, handle dim %d metric %d dtype %d)", path, hd.dim,
                        hd.metric, hd.dtype, h->dim, h->metric, want);
        return RADAD_EIO;
    }
    const size_t rb = h->row_bytes();
    if (map.len < hd.payload_off + (size_t)hd.ntotal * rb) { radad_set_error("%s: truncated", path); return RADAD_EIO; }
    if (n_rows < 0) n_rows = hd.ntotal - row0;
    RADAD_REQUIRE(row0 >= 0 && n_rows >= 0 && row0 + n_rows <= hd.ntotal, "radad_knn_load_range: rows outside the snapshot");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    RADAD_REQUIRE(!h->pending.valid && !h->pending_excl.valid, "radad_knn_load: a begun search (radad_knn_search_begin) must be finished or aborted before the store changes");
    RADAD_HIP_CHECK(hipDeviceSynchronize());
    h->ntotal = 0;
    h->hi_rows = 0; h->stat_rows = 0; h->ab_rows = 0;      // the hi plane, the statistics and the per-tile terms describe the old contents
    if (h->stat) RADAD_HIP_CHECK(hipMemset(h->stat, 0, 4 * sizeof(unsigned)));
    if ((rc = knn_grow(h, n_rows))) return rc;
    const unsigned char* src = map.base + hd.payload_off + (size_t)row0 * rb;
    const size_t total = (size_t)n_rows * rb;
    if (total) {
        (void)madvise(const_cast<unsigned char*>(map.base), map.len, MADV_SEQUENTIAL);
        PinnedPipe pipe;
        if ((rc = pipe.init())) return rc;
        int slot = 0;
        for (size_t off = 0; off < total; off += SNAP_STAGE_BYTES, slot ^= 1) {
            const size_t m = std::min(SNAP_STAGE_BYTES, total - off);
            RADAD_HIP_CHECK(hipEventSynchronize(pipe.done[slot]));      // the copy that last used this buffer has landed
            memcpy(pipe.buf[slot], src + off, m);                       // page-in + stage; overlaps the other buffer's DMA
            RADAD_HIP_CHECK(hipMemcpyAsync(h->rows + off, pipe.buf[slot], m, hipMemcpyHostToDevice, pipe.st));
            RADAD_HIP_CHECK(hipEventRecord(pipe.done[slot], pipe.st));
        }
        RADAD_HIP_CHECK(hipStreamSynchronize(pipe.st));
    }
    if (h->metric == RADAD_METRIC_L2 && n_rows > 0) {      // |y|^2 is not part of the snapshot
        const unsigned grid = (unsigned)ceil_div64(n_rows, 4);
        if (h->f16) hipLaunchKernelGGL(k_row_sqnorm<_Float16>, dim3(grid), dim3(256), 0, nullptr, (const _Float16*)h->rows, n_rows, h->dim, h->ynorm);
        else hipLaunchKernelGGL(k_row_sqnorm<float>, dim3(grid), dim3(256), 0, nullptr, (const float*)h->rows, n_rows, h->dim, h->ynorm);
        RADAD_HIP_CHECK(hipGetLastError());
        RADAD_HIP_CHECK(hipDeviceSynchronize());
    }
    h->ntotal = n_rows;
    return RADAD_OK;
}

}  // namespace

extern "C" {

int radad_knn_save(radad_knn_t h, const char* path) {
    RADAD_REQUIRE(h && path, "radad_knn_save: NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    RADAD_HIP_CHECK(hipDeviceSynchronize());
    FILE* f = fopen(path, "wb");
    if (!f) { radad_set_error("cannot open %s for writing", path); return RADAD_EIO; }
    const char magic[8] = {'R', 'A', 'D', 'A', 'D', 'K', 'N', 'N'};
    const uint32_t ver = SNAP_VERSION;
    const int32_t dim = h->dim, metric = h->metric, dtype = h->f16 ? RADAD_STORE_F16 : RADAD_STORE_F32;
    const int64_t nt = h->ntotal;
    bool ok = fwrite(magic, 1, 8, f) == 8 && fwrite(&ver, 4, 1, f) == 1 && fwrite(&dim, 4, 1, f) == 1 &&
              fwrite(&metric, 4, 1, f) == 1 && fwrite(&dtype, 4, 1, f) == 1 && fwrite(&nt, 8, 1, f) == 1;
    const size_t total = (size_t)nt * h->row_bytes();
    int rc = RADAD_OK;
    if (ok && total) {
        PinnedPipe pipe;
        if ((rc = pipe.init())) { fclose(f); return rc; }
        // D2H of chunk i+1 runs while chunk i is written to the file
        auto fetch = [&](size_t off, int slot) {
            const size_t m = std::min(SNAP_STAGE_BYTES, total - off);
            if (hipMemcpyAsync(pipe.buf[slot], h->rows + off, m, hipMemcpyDeviceToHost, pipe.st) != hipSuccess) return false;
            return hipEventRecord(pipe.done[slot], pipe.st) == hipSuccess;
        };
        int slot = 0;
        ok = fetch(0, 0);
        for (size_t off = 0; ok && off < total; off += SNAP_STAGE_BYTES, slot ^= 1) {
            const size_t m = std::min(SNAP_STAGE_BYTES, total - off);
            if (off + SNAP_STAGE_BYTES < total) ok = fetch(off + SNAP_STAGE_BYTES, slot ^ 1);
            ok = ok && hipEventSynchronize(pipe.done[slot]) == hipSuccess;
            ok = ok && fwrite(pipe.buf[slot], 1, m, f) == m;
        }
        (void)hipStreamSynchronize(pipe.st);
    }
    ok = (fclose(f) == 0) && ok;
    if (!ok) { radad_set_error("write to %s failed", path); return RADAD_EIO; }
    return RADAD_OK;
}

int radad_knn_load(radad_knn_t h, const char* path) {
    RADAD_REQUIRE(h && path, "radad_knn_load: NULL argument");
    return snap_load_range(h, path, 0, -1);
}

int radad_knn_load_range(radad_knn_t h, const char* path, int64_t row0, int64_t n_rows) {
    RADAD_REQUIRE(h && path, "radad_knn_load_range: NULL argument");
    return snap_load_range(h, path, row0, n_rows);
}

int radad_knn_snapshot_info(const char* path, int* dim_out, int* metric_out, int* store_dtype_out, int64_t* ntotal_out) {
    RADAD_REQUIRE(path, "radad_knn_snapshot_info: NULL path");
    FILE* f = fopen(path, "rb");
    if (!f) { radad_set_error("cannot open %s", path); return RADAD_EIO; }
    unsigned char head[32];
    const size_t got = fread(head, 1, sizeof(head), f);
    fclose(f);
    SnapHeader hd;
    if (!snap_parse(head, got, &hd)) { radad_set_error("%s: not a RADADKNN snapshot", path); return RADAD_EIO; }
    if (dim_out) *dim_out = hd.dim;
    if (metric_out) *metric_out = hd.metric;
    if (store_dtype_out) *store_dtype_out = hd.dtype;
    if (ntotal_out) *ntotal_out = hd.ntotal;
    return RADAD_OK;
}

int radad_topk_merge(int metric, const float* in_dist_dev, const int64_t* in_idx_dev, int n_parts, int64_t nq, int k,
                     float* out_dist_dev, int64_t* out_idx_dev, int device, void* stream) {
    return merge_lists<float>(metric, in_dist_dev, in_idx_dev, n_parts, nq, k, out_dist_dev, out_idx_dev, nullptr, device, stream);
}

int radad_topk_merge_f64(int metric, const double* in_key_dev, const int64_t* in_idx_dev, int n_parts, int64_t nq, int k,
                         float* out_dist_dev, int64_t* out_idx_dev, double* out_key_dev, int device, void* stream) {
    return merge_lists<double>(metric, in_key_dev, in_idx_dev, n_parts, nq, k, out_dist_dev, out_idx_dev, out_key_dev, device,
                               stream);
}

int radad_filter_topk(const float* in_dist_dev, const int64_t* in_idx_dev, int64_t nq, int k_in, int k_keep,
                      const int64_t* row_tags_dev, int64_t ntotal, int64_t id_base, const int64_t* excl_sorted_dev, int64_t n_excl,
                      float* out_dist_dev, int64_t* out_idx_dev, int device, void* stream) {
    RADAD_REQUIRE(nq >= 0 && k_in >= 0 && k_keep >= 1 && n_excl >= 0 && ntotal >= 0, "radad_filter_topk: bad shape");
    if (nq == 0) return RADAD_OK;
    RADAD_REQUIRE(out_dist_dev && out_idx_dev && (k_in == 0 || (in_dist_dev && in_idx_dev)), "radad_filter_topk: NULL buffer");
    RADAD_REQUIRE(n_excl == 0 || (excl_sorted_dev && row_tags_dev), "radad_filter_topk: exclusion set without tags");
    DeviceGuard g(device);
    hipLaunchKernelGGL(k_filter_topk, dim3((unsigned)ceil_div64(nq, 256)), dim3(256), 0, (hipStream_t)stream, in_dist_dev, in_idx_dev,
                       nq, k_in, k_keep, row_tags_dev, ntotal, id_base, excl_sorted_dev, n_excl, out_dist_dev, out_idx_dev);
    RADAD_HIP_CHECK(hipGetLastError());
    return RADAD_OK;
}

int radad_kth_largest(const float* in_dev, int64_t n, int groups, int per_group, int k, float* out_dev, int device, void* stream) {
    RADAD_REQUIRE(n >= 0 && groups >= 1 && per_group >= 1 && (int64_t)groups * per_group <= 64 * KTH_PER_LANE && k >= 1 && k <= groups * per_group,
                  "radad_kth_largest: bad shape (groups x per_group <= %d, 1 <= k <= groups x per_group)", 64 * KTH_PER_LANE);
    if (n == 0) return RADAD_OK;
    RADAD_REQUIRE(in_dev && out_dev, "radad_kth_largest: NULL buffer");
    DeviceGuard g(device);
    hipLaunchKernelGGL(k_kth_largest, dim3((unsigned)ceil_div64(n, 4)), dim3(256), 0, (hipStream_t)stream, in_dev, n, groups, per_group, k, out_dev);
    RADAD_HIP_CHECK(hipGetLastError());
    return RADAD_OK;
}

int radad_rownorm(const float* in_dev, float* out_dev, int64_t n, int dim, int device, void* stream) {
    RADAD_REQUIRE(dim > 0 && dim % 4 == 0 && n >= 0, "radad_rownorm: bad shape");
    if (n == 0) return RADAD_OK;
    RADAD_REQUIRE(in_dev && out_dev, "radad_rownorm: NULL buffer");
    DeviceGuard g(device);
    hipLaunchKernelGGL(k_rows_prepare<float>, dim3((unsigned)ceil_div64(n, 4)), dim3(256), 0, (hipStream_t)stream, in_dev, out_dev,
                       (float*)nullptr, n, dim, 2);
    RADAD_HIP_CHECK(hipGetLastError());
    return RADAD_OK;
}

}  // extern "C"

#include "knn_remove.inc"
#include "ivf.inc"
