// proj_train.inc -- ProjectionLayer training forward and backward (projection.py:68-106 under autograd) on gfx950.
// Included at the end of proj.hip: it reuses gemm_nt_splitk, k_splitk_finish, block_sum, raise_lds and the tile constants.
//
// Forward (no W5 W4 fold: the weights move every step).  M = B*K rows of x.
//   p = W1 x + b1    t = tanh(p)   s = W2 t + b2   a = softmax_K(s)
//   q = W3 x + b3    h = relu(q)   hbar = sum_k a_k h_k   [B,H]        (sum_K before W4: the softmax weights sum to one)
//   u = W4 hbar + b4 [B,D]         v = W5 u + b5  [B,H]
//   xh = (v - mean) rstd   n = xh g + beta   nd = n * mask * inv_keep   out = W6 nd + b6
// Saved for the backward beside x: t, h, a, hbar, u, xh, rstd (and the caller's mask).
//
// Backward, G = d out:
//   dnd = G W6   dW6 = G^T nd   db6 = sum_b G   dn = dnd * mask * inv_keep   dg = sum_b dn xh   dbeta = sum_b dn   dxh = dn g
//   dv = rstd (dxh - mean_H dxh - xh mean_H(dxh xh))   dW5 = dv^T u   db5 = sum_b dv   du = dv W5
//   dW4 = du^T hbar   db4 = sum_b du   dhbar = du W4
//   da_k = h_k . dhbar   dq = a_k dhbar [h > 0]   ds = a (da - sum_k a_k da_k)   dW2 = sum ds t   db2 = sum ds
//   dp = ds W2 (1 - t^2)   [dW1; dW3] = [dp | dq]^T x   db1 = sum dp   db3 = sum dq   dx = [dp | dq] [W1; W3]
// No [B,K,D] tensor other than x (and dx, when asked for) exists.  Every reduction has a fixed order (split partial products
// summed in split order, column sums in row order): no float atomics, the gradients are bitwise reproducible.

namespace {

constexpr int TRAIN_SPLIT_TARGET = 256;   // one block per CU before the reduction is split
constexpr int CS_ROWS = 256;              // rows per column-sum block
constexpr int CS_GROUPS = 16;             // ... in this many interleaved row groups of 64 columns
constexpr int PAIRWISE_MAX_K = 64;        // softmax backward in its cancellation-free pairwise form up to this many neighbours
constexpr int64_t TRAIN_MAX_DIM = (1 << 22) - 64;   // grid.y = ceil(dim / 64) stays under 65 536

struct GemmKmParams {
    const float* a; int64_t lda;      // A_KM ? [Kr, M] (dW = A^T B) : [M, Kr] (plain product)
    const float* b;                   // [Kr, N] row-major: rows [0, kr_lo) ...
    const float* b_hi; int kr_lo;     // ... and rows [kr_lo, Kr) of a second matrix stacked under the first (or unused)
    int64_t ldb;
    float* part;                      // [S, M, N] partial products of the reduction splits
    int M, N, Kr, chunks_per_split;
};

// part[z] = op(A)[:, Kz] B[Kz, :] over the reduction rows Kz of split z, on v_mfma_f32_32x32x2_f32 with the tile geometry of
// k_gemm_nt_splitk.  B (and A when A_KM) is stored reduction-major, so its tile goes to LDS as [GK][GT] and a lane reads its
// operand with one ds_read_b32 (32 consecutive floats per half wave: no bank conflict).  VEC: f32x4 loads, legal when the
// host has checked widths, strides and base alignment; otherwise dword loads bounded one by one.
template <bool A_KM, bool VEC>
__global__ __launch_bounds__(G_THREADS, 2) void k_gemm_km(GemmKmParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int A_BUF = A_KM ? GK * GT : GT * GLD;
    float* sA = reinterpret_cast<float*>(smem);   // [2][GK][GT] or [2][GT][GLD]
    float* sB = sA + 2 * A_BUF;                   // [2][GK][GT]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1, l31 = lane & 31, lh = lane >> 5;
    const int m0 = blockIdx.x * GT, n0 = blockIdx.y * GT;
    const int nk = (p.Kr + GK - 1) / GK;
    const int kb = blockIdx.z * p.chunks_per_split;
    const int ke = min(nk, kb + p.chunks_per_split);
    const int kc_r = tid >> 3, kc_c = (tid & 7) * 4;      // reduction-contiguous tile: row, first of four reduction columns
    const int km_k = tid >> 5, km_c = (tid & 31) * 4;     // reduction-major tile: reduction row, first of four columns
    f32x4 ra[4], rb[4];
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    auto load_km = [&](f32x4* dst, const float* base, const float* base_hi, int lo, int64_t ld, int c0, int ncols, int kc) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        const int col = c0 + km_c;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = kc * GK + km_k + 8 * i;
            dst[i] = z;
            if (k >= p.Kr) continue;
            const float* row = k < lo ? base + (int64_t)k * ld : base_hi + (int64_t)(k - lo) * ld;
            if constexpr (VEC) {
                if (col < ncols) dst[i] = *reinterpret_cast<const f32x4*>(row + col);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (col + j < ncols) dst[i][j] = row[col + j];
            }
        }
    };
    auto gload = [&](int kc) {
        if constexpr (A_KM) {
            load_km(ra, p.a, p.a, p.Kr, p.lda, m0, p.M, kc);
        } else {
            const int kcol = kc * GK + kc_c;
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int m = m0 + kc_r + 32 * i;
                ra[i] = z;
                if (m >= p.M) continue;
                const float* row = p.a + (int64_t)m * p.lda;
                if constexpr (VEC) {
                    if (kcol < p.Kr) ra[i] = *reinterpret_cast<const f32x4*>(row + kcol);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (kcol + j < p.Kr) ra[i][j] = row[kcol + j];
                }
            }
        }
        load_km(rb, p.b, p.b_hi, p.kr_lo, p.ldb, n0, p.N, kc);
    };
    auto swrite = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if constexpr (A_KM) *reinterpret_cast<f32x4*>(sA + buf * A_BUF + (km_k + 8 * i) * GT + km_c) = ra[i];
            else *reinterpret_cast<f32x4*>(sA + buf * A_BUF + (kc_r + 32 * i) * GLD + kc_c) = ra[i];
            *reinterpret_cast<f32x4*>(sB + buf * GK * GT + (km_k + 8 * i) * GT + km_c) = rb[i];
        }
    };
    gload(kb);
    swrite(0);
    __syncthreads();
    for (int kc = kb; kc < ke; ++kc) {
        const int buf = (kc - kb) & 1;
        if (kc + 1 < ke) gload(kc + 1);
        const float* a_base = sA + buf * A_BUF;
        const float* b_base = sB + buf * GK * GT + wn * 64 + l31;
#pragma unroll
        for (int kk = 0; kk < GK / 8; ++kk) {
            f32x4 a0, a1;
            if constexpr (!A_KM) {
                a0 = *reinterpret_cast<const f32x4*>(a_base + (wm * 64 + l31) * GLD + 4 * lh + kk * 8);
                a1 = *reinterpret_cast<const f32x4*>(a_base + (wm * 64 + 32 + l31) * GLD + 4 * lh + kk * 8);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = kk * 8 + 4 * lh + j;      // the same reduction index for both operands of MFMA j
                if constexpr (A_KM) {
                    a0[j] = a_base[k * GT + wm * 64 + l31];
                    a1[j] = a_base[k * GT + wm * 64 + 32 + l31];
                }
                const float b0 = b_base[k * GT], b1 = b_base[k * GT + 32];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], b1, acc[1][1], 0, 0, 0);
            }
        }
        if (kc + 1 < ke) swrite(buf ^ 1);
        __syncthreads();
    }
    // acc[mt][nt][r]: row m0 + wm*64 + mt*32 + (r&3) + 8(r>>2) + 4lh, column n0 + wn*64 + nt*32 + l31
    float* out = p.part + (int64_t)blockIdx.z * p.M * p.N;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int n = n0 + wn * 64 + nt * 32 + l31;
        if (n >= p.N) continue;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (m < p.M) out[(int64_t)m * p.N + n] = acc[mt][nt][r];
            }
    }
}

// out[m, n] = sum_z part[z, m, n] in split order; rows [m_lo, M) go to out_hi (two gradients stacked in one product)
__global__ __launch_bounds__(256) void k_km_finish(const float* __restrict__ part, int S, int64_t M, int N, float* __restrict__ out,
                                                   float* __restrict__ out_hi, int64_t m_lo) {
    const int64_t total = M * N;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        float v = 0.f;
        for (int z = 0; z < S; ++z) v += part[(int64_t)z * total + i];
        if (i < m_lo * N) out[i] = v; else out_hi[i - m_lo * N] = v;
    }
}

// dst[chunk, c] = sum over the chunk's rows of w[r] * A[r, c]: CS_GROUPS interleaved row groups, each in row order (eight loads
// in flight, added in that order), then the group sums in order.  One chunk writes the result itself; more chunks are summed
// in chunk order by k_colsum_finish.
__global__ __launch_bounds__(64 * CS_GROUPS) void k_colsum(const float* __restrict__ A, int64_t lda, int64_t R, int C,
                                                           const float* __restrict__ wrow, float* __restrict__ dst) {
    __shared__ float s[CS_GROUPS][64];
    const int cl = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + cl;
    const int64_t r0 = (int64_t)blockIdx.x * CS_ROWS, r1 = min(R, r0 + (int64_t)CS_ROWS);
    float v = 0.f;
    if (c < C) {
        for (int64_t r = r0 + g; r < r1; r += 8 * CS_GROUPS) {
            float x[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int64_t rr = r + i * CS_GROUPS;
                x[i] = rr < r1 ? (wrow ? wrow[rr] * A[rr * lda + c] : A[rr * lda + c]) : 0.f;
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) v += x[i];
        }
    }
    s[g][cl] = v;
    __syncthreads();
    if (g == 0 && c < C) {
        float t = s[0][cl];
#pragma unroll
        for (int i = 1; i < CS_GROUPS; ++i) t += s[i][cl];
        dst[(int64_t)blockIdx.x * C + c] = t;
    }
}

__global__ __launch_bounds__(256) void k_colsum_finish(const float* __restrict__ part, int n, int C, float* __restrict__ out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float v = 0.f;
    for (int i = 0; i < n; ++i) v += part[(int64_t)i * C + c];
    out[c] = v;
}

struct TrainTailParams {
    const float* part; int S;        // [S, B*K, 2H]: columns [0,H) = W1 x, [H,2H) = W3 x
    const float *b1, *w2, *b2, *b3;
    float *t, *h, *a, *hbar;         // [M,H], [M,H], [M], [B,H]
    int64_t B; int K, H;
};

// one block per batch row: K-split reduce -> tanh / relu -> scores -> softmax_K -> hbar (k_proj_tail up to hbar, keeping t, h, a)
__global__ __launch_bounds__(TAIL_THREADS) void k_train_tail(TrainTailParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int K = p.K, H = p.H;
    float* s_hc = reinterpret_cast<float*>(smem);   // [K][H] relu branch
    float* s_sw = s_hc + K * H;                     // [K][H] tanh(.) * w2
    float* s_score = s_sw + K * H;                  // [K]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = blockIdx.x;
    const int64_t MN = p.B * K * 2 * H;
    for (int idx = tid; idx < K * H; idx += TAIL_THREADS) {
        const int k = idx / H, h = idx - k * H;
        const float* src = p.part + ((b * K + k) * 2) * H + h;
        float sa = 0.f, sc = 0.f;
        for (int z = 0; z < p.S; ++z) {
            sa += src[(int64_t)z * MN];
            sc += src[(int64_t)z * MN + H];
        }
        const float tv = tanhf(sa + p.b1[h]), hv = fmaxf(sc + p.b3[h], 0.f);
        p.t[(b * K + k) * H + h] = tv;
        p.h[(b * K + k) * H + h] = hv;
        s_sw[idx] = tv * p.w2[h];
        s_hc[idx] = hv;
    }
    __syncthreads();
    for (int k = wave; k < K; k += TAIL_THREADS / 64) {
        float s = 0.f;
        for (int h = lane; h < H; h += 64) s += s_sw[k * H + h];
        s = wave_sum(s);
        if (lane == 0) s_score[k] = s + p.b2[0];
    }
    __syncthreads();
    float mx = -INFINITY, den = 0.f;
    for (int k = 0; k < K; ++k) mx = fmaxf(mx, s_score[k]);
    for (int k = 0; k < K; ++k) den += expf(s_score[k] - mx);
    const float rden = 1.0f / den;
    for (int k = tid; k < K; k += TAIL_THREADS) p.a[b * K + k] = expf(s_score[k] - mx) * rden;
    for (int h = tid; h < H; h += TAIL_THREADS) {
        float v = 0.f;
        for (int k = 0; k < K; ++k) v += expf(s_score[k] - mx) * rden * s_hc[k * H + h];
        p.hbar[b * H + h] = v;
    }
}

// one block per batch row: LayerNorm (biased variance, eps 1e-6) -> dropout by the caller's mask; W6 follows as a product of its
// own (one block per row would leave it to four waves per CU, waiting on loads)
__global__ __launch_bounds__(TAIL_THREADS) void k_train_head(const float* __restrict__ v, const float* __restrict__ ln_g,
                                                             const float* __restrict__ ln_b, const float* __restrict__ mask,
                                                             float inv_keep, float* __restrict__ xh, float* __restrict__ rstd_out,
                                                             float* __restrict__ nd, int H) {
    __shared__ float s_red[4];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const float* vr = v + b * H;
    float lsum = 0.f;
    for (int j = tid; j < H; j += TAIL_THREADS) lsum += vr[j];
    const float mu = block_sum(lsum, s_red) / (float)H;
    float lvar = 0.f;
    for (int j = tid; j < H; j += TAIL_THREADS) { const float d = vr[j] - mu; lvar += d * d; }
    const float rstd = 1.0f / sqrtf(block_sum(lvar, s_red) / (float)H + 1e-6f);
    if (tid == 0) rstd_out[b] = rstd;
    for (int j = tid; j < H; j += TAIL_THREADS) {
        const float x = (vr[j] - mu) * rstd;
        xh[b * H + j] = x;
        float n = x * ln_g[j] + ln_b[j];
        if (mask) n = n * mask[b * H + j] * inv_keep;
        nd[b * H + j] = n;
    }
}

// one block per batch row: G -> dnd -> dn -> LayerNorm backward -> dv.  Writes nd [B,H] (for dW6) and hb3 [B,3H] = [dn | dn xh | dv]
// (its column sums are dbeta, dg and db5).
__global__ __launch_bounds__(TAIL_THREADS) void k_head_bwd(const float* __restrict__ G, const float* __restrict__ w6,
                                                           const float* __restrict__ ln_g, const float* __restrict__ ln_b,
                                                           const float* __restrict__ mask, float inv_keep,
                                                           const float* __restrict__ xh, const float* __restrict__ rstd,
                                                           float* __restrict__ nd, float* __restrict__ hb3, int H, int O) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* s_g = reinterpret_cast<float*>(smem);    // [O]
    float* s_dxh = s_g + O;                         // [H]
    float* s_red = s_dxh + H;                       // [4]
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    for (int o = tid; o < O; o += TAIL_THREADS) s_g[o] = G[b * O + o];
    __syncthreads();
    float l1 = 0.f, l2 = 0.f;
    for (int j = tid; j < H; j += TAIL_THREADS) {
        float dnd = 0.f;
        for (int o = 0; o < O; ++o) dnd += s_g[o] * w6[(int64_t)o * H + j];
        const float x = xh[b * H + j];
        const float mk = mask ? mask[b * H + j] * inv_keep : 1.0f;
        const float dn = dnd * mk;
        nd[b * H + j] = (x * ln_g[j] + ln_b[j]) * mk;
        hb3[b * 3 * H + j] = dn;
        hb3[b * 3 * H + H + j] = dn * x;
        const float dxh = dn * ln_g[j];
        s_dxh[j] = dxh;
        l1 += dxh;
        l2 += dxh * x;
    }
    const float m1 = block_sum(l1, s_red) / (float)H;
    const float m2 = block_sum(l2, s_red) / (float)H;
    const float rs = rstd[b];
    for (int j = tid; j < H; j += TAIL_THREADS) hb3[b * 3 * H + 2 * H + j] = rs * (s_dxh[j] - m1 - xh[b * H + j] * m2);
}

// one block per batch row: dhbar, a, h, t -> ds [M] and [dp | dq] [M, 2H].  The gradient of relu at q = 0 is 0 (h > 0), as torch.
__global__ __launch_bounds__(TAIL_THREADS) void k_attn_bwd(const float* __restrict__ dhbar, const float* __restrict__ a,
                                                           const float* __restrict__ h, const float* __restrict__ t,
                                                           const float* __restrict__ w2, float* __restrict__ ds,
                                                           float* __restrict__ dpq, int K, int H) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* s_da = reinterpret_cast<float*>(smem);   // [K]
    float* s_ds = s_da + K;                         // [K]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = blockIdx.x;
    const float* dhb = dhbar + b * H;
    for (int k = wave; k < K; k += TAIL_THREADS / 64) {
        const float* hr = h + (b * K + k) * H;
        float v = 0.f;
        for (int j = lane; j < H; j += 64) v += hr[j] * dhb[j];
        v = wave_sum(v);
        if (lane == 0) s_da[k] = v;
    }
    __syncthreads();
    const float* ar = a + b * K;
    if (K <= PAIRWISE_MAX_K) {   // ds_k = a_k sum_j a_j (da_k - da_j): equal da give exactly zero, nothing is cancelled after the fact
        for (int k = tid; k < K; k += TAIL_THREADS) {
            float v = 0.f;
            for (int j = 0; j < K; ++j) v += ar[j] * (s_da[k] - s_da[j]);
            s_ds[k] = ar[k] * v;
        }
    } else {
        float dot = 0.f;
        for (int j = 0; j < K; ++j) dot += ar[j] * s_da[j];
        for (int k = tid; k < K; k += TAIL_THREADS) s_ds[k] = ar[k] * (s_da[k] - dot);
    }
    __syncthreads();
    for (int k = tid; k < K; k += TAIL_THREADS) ds[b * K + k] = s_ds[k];
    for (int idx = tid; idx < K * H; idx += TAIL_THREADS) {
        const int k = idx / H, j = idx - k * H;
        const int64_t m = b * K + k;
        const float tv = t[m * H + j], hv = h[m * H + j];
        dpq[m * 2 * H + j] = s_ds[k] * w2[j] * (1.0f - tv * tv);
        dpq[m * 2 * H + H + j] = hv > 0.f ? ar[k] * dhb[j] : 0.f;
    }
}

inline void red_plan(int64_t M, int N, int64_t Kr, int* splits, int* chunks_per_split) {
    const int nk = (int)std::max<int64_t>(1, ceil_div64(Kr, GK));   // (an empty batch only sizes a workspace)
    const int64_t tiles = std::max<int64_t>(1, ceil_div64(M, GT) * ceil_div64(N, GT));
    int64_t want = ceil_div64(TRAIN_SPLIT_TARGET, tiles);
    if (want < 1) want = 1;
    if (want > nk) want = nk;
    const int cps = (int)std::min<int64_t>(nk, std::max<int64_t>(4, ceil_div64(nk, want)));
    *chunks_per_split = cps;
    *splits = (int)ceil_div64(nk, cps);
}

// bytes of split partials a product needs (none when one split writes the result itself)
inline size_t km_part_bytes(int64_t M, int N, int64_t Kr, bool stacked_out) {
    int S, cps;
    red_plan(M, N, Kr, &S, &cps);
    return (S > 1 || stacked_out) ? al256((size_t)S * (size_t)M * (size_t)N * sizeof(float)) : 0;
}

// part (or the result itself, with one split) = op(A) B over S reduction splits of cps chunks, B = [b; b_hi] stacked at row kr_lo
template <bool A_KM>
int gemm_km_launch(const float* a, int64_t lda, const float* b, const float* b_hi, int kr_lo, int64_t ldb, int64_t M, int N, int64_t Kr,
                   float* dst, int S, int cps, hipStream_t st) {
    GemmKmParams p{a, lda, b, b_hi ? b_hi : b, b_hi ? kr_lo : (int)Kr, ldb, dst, (int)M, N, (int)Kr, cps};
    auto a16 = [](const float* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    const bool vec = N % 4 == 0 && ldb % 4 == 0 && a16(p.b) && a16(p.b_hi) && lda % 4 == 0 && a16(a) && (A_KM ? M % 4 == 0 : Kr % 4 == 0);
    const auto kern = vec ? k_gemm_km<A_KM, true> : k_gemm_km<A_KM, false>;
    constexpr size_t lds = sizeof(float) * 2 * ((A_KM ? GK * GT : GT * GLD) + GK * GT);   // 65 536 / 69 632 B: raise the limit
    const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                (int)lds);
    RADAD_HIP_CHECK(attr);
    hipLaunchKernelGGL(kern, dim3((unsigned)ceil_div64(M, GT), (unsigned)ceil_div64(N, GT), (unsigned)S), dim3(G_THREADS), lds, st,
                       p);
    RADAD_HIP_CHECK(hipGetLastError());
    return RADAD_OK;
}

// out [M,N] = op(A) B with B = [b; b_hi] stacked at reduction row kr_lo; rows [m_lo, M) of the result go to out_hi when given
template <bool A_KM>
int gemm_km(const float* a, int64_t lda, const float* b, const float* b_hi, int kr_lo, int64_t ldb, int64_t M, int N, int64_t Kr,
            float* part, float* out, float* out_hi, int64_t m_lo, hipStream_t st) {
    int S, cps, rc;
    red_plan(M, N, Kr, &S, &cps);
    const bool direct = S == 1 && !out_hi;
    if ((rc = gemm_km_launch<A_KM>(a, lda, b, b_hi, kr_lo, ldb, M, N, Kr, direct ? out : part, S, cps, st))) return rc;
    if (!direct) {
        const int64_t total = M * N;
        hipLaunchKernelGGL(k_km_finish, dim3((unsigned)std::min<int64_t>(ceil_div64(total, 256), 4096)), dim3(256), 0, st, part, S,
                           M, N, out, out_hi ? out_hi : out, out_hi ? m_lo : M);
        RADAD_HIP_CHECK(hipGetLastError());
    }
    return RADAD_OK;
}

// out[c] = sum_r w[r] A[r, c] (w NULL: plain column sums); scratch holds ceil(R / CS_ROWS) * C floats
int colsum(const float* A, int64_t lda, int64_t R, int C, const float* wrow, float* out, float* scratch, hipStream_t st) {
    const int64_t chunks = ceil_div64(R, CS_ROWS);
    hipLaunchKernelGGL(k_colsum, dim3((unsigned)chunks, (unsigned)ceil_div64(C, 64)), dim3(64 * CS_GROUPS), 0, st, A, lda, R, C, wrow,
                       chunks == 1 ? out : scratch);
    RADAD_HIP_CHECK(hipGetLastError());
    if (chunks > 1) {
        hipLaunchKernelGGL(k_colsum_finish, dim3((unsigned)ceil_div64(C, 256)), dim3(256), 0, st, scratch, (int)chunks, C, out);
        RADAD_HIP_CHECK(hipGetLastError());
    }
    return RADAD_OK;
}

inline bool train_shape_ok(int64_t batch, int k, int dim, int hidden, int out_dim) {
    return batch >= 0 && k >= 1 && dim > 0 && hidden > 0 && out_dim > 0 && hidden <= 4096 && out_dim <= 4096 && dim <= TRAIN_MAX_DIM &&
           batch < (1ll << 31) && batch * (int64_t)k < (1ll << 31) - GT;
}

inline size_t tail_lds_bytes(int k, int hidden) { return sizeof(float) * ((size_t)2 * k * hidden + 2 * hidden + k + 8); }

// workspace layout shared by the forward (part, v, nd) and the backward (everything)
struct TrainWs {
    size_t part, v, nd, hb3, du, dhbar, dpq, ds, cs, total;
    TrainWs(int64_t B, int K, int D, int H, int O) {
        const int64_t M = B * K;
        size_t pb = std::max(part_bytes(M, 2 * H, D), std::max(part_bytes(B, D, H), part_bytes(B, H, D)));
        pb = std::max(pb, part_bytes(B, O, H));                    // out = W6 nd
        pb = std::max(pb, km_part_bytes(O, H, B, false));          // dW6
        pb = std::max(pb, km_part_bytes(H, D, B, false));          // dW5
        pb = std::max(pb, km_part_bytes(B, D, H, false));          // du
        pb = std::max(pb, km_part_bytes(D, H, B, false));          // dW4
        pb = std::max(pb, km_part_bytes(B, H, D, false));          // dhbar
        pb = std::max(pb, km_part_bytes(2 * H, D, M, true));       // [dW1; dW3]
        pb = std::max(pb, km_part_bytes(M, D, 2 * H, false));      // dx
        size_t off = 0;
        auto take = [&](size_t floats) { const size_t o = off; off += al256(floats * sizeof(float)); return o; };
        part = 0; off = pb;
        v = take((size_t)B * H);
        nd = take((size_t)B * H);
        hb3 = take((size_t)B * 3 * H);
        du = take((size_t)B * D);
        dhbar = take((size_t)B * H);
        dpq = take((size_t)M * 2 * H);
        ds = take((size_t)M);
        cs = take((size_t)ceil_div64(M, CS_ROWS) * (size_t)std::max(std::max(2 * H, O), D));
        total = off;
    }
};

}  // namespace

extern "C" {

int64_t radad_projection_train_workspace_bytes(int64_t batch, int k, int dim, int hidden, int out_dim) {
    if (!train_shape_ok(batch, k, dim, hidden, out_dim)) return -1;
    return (int64_t)TrainWs(batch, k, dim, hidden, out_dim).total;
}

int radad_projection_train_forward(const radad_proj_weights* w, const float* x_dev, const float* mask_dev, float inv_keep,
                                   int64_t batch, int k, int dim, int hidden, int out_dim, const radad_proj_saved* saved,
                                   float* out_dev, float* workspace_dev, int64_t workspace_bytes, int device, void* stream) {
    RADAD_REQUIRE(w && saved && train_shape_ok(batch, k, dim, hidden, out_dim), "radad_projection_train_forward: bad shape");
    RADAD_REQUIRE(tail_lds_bytes(k, hidden) <= 160 * 1024, "projection tail: K*hidden does not fit the 160 KB LDS");
    if (batch == 0) return RADAD_OK;
    RADAD_REQUIRE(x_dev && out_dev && workspace_dev, "radad_projection_train_forward: NULL buffer");
    RADAD_REQUIRE(w->w1 && w->b1 && w->w2 && w->b2 && w->w3 && w->b3 && w->w4 && w->b4 && w->w5 && w->b5 && w->ln_g && w->ln_b &&
                      w->w6 && w->b6, "radad_projection_train_forward: NULL weight");
    RADAD_REQUIRE(saved->t && saved->h && saved->a && saved->hbar && saved->u && saved->xh && saved->rstd,
                  "radad_projection_train_forward: NULL saved-activation buffer");
    RADAD_REQUIRE(workspace_bytes >= radad_projection_train_workspace_bytes(batch, k, dim, hidden, out_dim),
                  "radad_projection_train_forward: workspace too small");
    DeviceGuard g(device);
    hipStream_t st = (hipStream_t)stream;
    const int64_t M = batch * k;
    const TrainWs L(batch, k, dim, hidden, out_dim);
    char* ws = reinterpret_cast<char*>(workspace_dev);
    float* part = (float*)(ws + L.part);
    float* v = (float*)(ws + L.v);
    int S = 1, rc;
    if ((rc = gemm_nt_splitk(x_dev, dim, w->w1, w->w3, hidden, dim, part, M, 2 * hidden, dim, &S, st))) return rc;
    TrainTailParams tp{part, S, w->b1, w->w2, w->b2, w->b3, saved->t, saved->h, saved->a, saved->hbar, batch, k, hidden};
    const size_t lds = tail_lds_bytes(k, hidden);
    if ((rc = raise_lds(k_train_tail, lds))) return rc;
    hipLaunchKernelGGL(k_train_tail, dim3((unsigned)batch), dim3(TAIL_THREADS), lds, st, tp);
    RADAD_HIP_CHECK(hipGetLastError());
    const auto fin_grid = [](int64_t total) { return dim3((unsigned)std::min<int64_t>(ceil_div64(total, 256), 4096)); };
    // u = W4 hbar + b4
    if ((rc = gemm_nt_splitk(saved->hbar, hidden, w->w4, w->w4, dim, hidden, part, batch, dim, hidden, &S, st))) return rc;
    hipLaunchKernelGGL(k_splitk_finish, fin_grid(batch * dim), dim3(256), 0, st, part, S, batch, dim, w->b4, (int)ACT_NONE, saved->u,
                       (int64_t)dim);
    RADAD_HIP_CHECK(hipGetLastError());
    // v = W5 u + b5
    if ((rc = gemm_nt_splitk(saved->u, dim, w->w5, w->w5, hidden, dim, part, batch, hidden, dim, &S, st))) return rc;
    hipLaunchKernelGGL(k_splitk_finish, fin_grid(batch * hidden), dim3(256), 0, st, part, S, batch, hidden, w->b5, (int)ACT_NONE, v,
                       (int64_t)hidden);
    RADAD_HIP_CHECK(hipGetLastError());
    float* nd = (float*)(ws + L.nd);
    hipLaunchKernelGGL(k_train_head, dim3((unsigned)batch), dim3(TAIL_THREADS), 0, st, v, w->ln_g, w->ln_b, mask_dev, inv_keep,
                       saved->xh, saved->rstd, nd, hidden);
    RADAD_HIP_CHECK(hipGetLastError());
    // out = W6 nd + b6
    if ((rc = gemm_nt_splitk(nd, hidden, w->w6, w->w6, out_dim, hidden, part, batch, out_dim, hidden, &S, st))) return rc;
    hipLaunchKernelGGL(k_splitk_finish, fin_grid(batch * out_dim), dim3(256), 0, st, part, S, batch, out_dim, w->b6, (int)ACT_NONE,
                       out_dev, (int64_t)out_dim);
    RADAD_HIP_CHECK(hipGetLastError());
    return RADAD_OK;
}

int radad_projection_backward(const radad_proj_weights* w, const float* x_dev, const float* mask_dev, float inv_keep,
                              const radad_proj_saved* saved, const float* grad_out_dev, int64_t batch, int k, int dim, int hidden,
                              int out_dim, const radad_proj_grads* grads, float* dx_dev, float* workspace_dev,
                              int64_t workspace_bytes, int device, void* stream) {
    RADAD_REQUIRE(w && saved && grads && train_shape_ok(batch, k, dim, hidden, out_dim), "radad_projection_backward: bad shape");
    RADAD_REQUIRE(tail_lds_bytes(k, hidden) <= 160 * 1024, "projection tail: K*hidden does not fit the 160 KB LDS");
    if (batch == 0) return RADAD_OK;
    RADAD_REQUIRE(x_dev && grad_out_dev && workspace_dev, "radad_projection_backward: NULL buffer");
    RADAD_REQUIRE(w->w1 && w->w2 && w->w3 && w->w4 && w->w5 && w->ln_g && w->ln_b && w->w6, "radad_projection_backward: NULL weight");
    RADAD_REQUIRE(saved->t && saved->h && saved->a && saved->hbar && saved->u && saved->xh && saved->rstd,
                  "radad_projection_backward: NULL saved-activation buffer");
    RADAD_REQUIRE(workspace_bytes >= radad_projection_train_workspace_bytes(batch, k, dim, hidden, out_dim),
                  "radad_projection_backward: workspace too small");
    RADAD_REQUIRE((grads->dw1 == nullptr) == (grads->dw3 == nullptr),
                  "radad_projection_backward: dw1 and dw3 come from one product, give both or neither");
    DeviceGuard g(device);
    hipStream_t st = (hipStream_t)stream;
    const int64_t M = batch * k;
    const int H = hidden, D = dim, O = out_dim;
    const TrainWs L(batch, k, dim, hidden, out_dim);
    char* ws = reinterpret_cast<char*>(workspace_dev);
    float* part = (float*)(ws + L.part);
    float* nd = (float*)(ws + L.nd);
    float* hb3 = (float*)(ws + L.hb3);
    float* du = (float*)(ws + L.du);
    float* dhbar = (float*)(ws + L.dhbar);
    float* dpq = (float*)(ws + L.dpq);
    float* ds = (float*)(ws + L.ds);
    float* cs = (float*)(ws + L.cs);
    const float* dv = hb3 + 2 * H;
    int rc;
    hipLaunchKernelGGL(k_head_bwd, dim3((unsigned)batch), dim3(TAIL_THREADS), sizeof(float) * ((size_t)O + H + 8), st, grad_out_dev,
                       w->w6, w->ln_g, w->ln_b, mask_dev, inv_keep, saved->xh, saved->rstd, nd, hb3, H, O);
    RADAD_HIP_CHECK(hipGetLastError());
    if (grads->dw6 && (rc = gemm_km<true>(grad_out_dev, O, nd, nullptr, 0, H, O, H, batch, part, grads->dw6, nullptr, 0, st))) return rc;
    if (grads->db6 && (rc = colsum(grad_out_dev, O, batch, O, nullptr, grads->db6, cs, st))) return rc;
    if (grads->dln_b && (rc = colsum(hb3, 3 * H, batch, H, nullptr, grads->dln_b, cs, st))) return rc;
    if (grads->dln_g && (rc = colsum(hb3 + H, 3 * H, batch, H, nullptr, grads->dln_g, cs, st))) return rc;
    if (grads->db5 && (rc = colsum(dv, 3 * H, batch, H, nullptr, grads->db5, cs, st))) return rc;
    if (grads->dw5 && (rc = gemm_km<true>(dv, 3 * H, saved->u, nullptr, 0, D, H, D, batch, part, grads->dw5, nullptr, 0, st))) return rc;
    const bool need_attn = grads->dw1 || grads->db1 || grads->dw2 || grads->db2 || grads->dw3 || grads->db3 || dx_dev;
    if (!(need_attn || grads->dw4 || grads->db4)) return RADAD_OK;
    if ((rc = gemm_km<false>(dv, 3 * H, w->w5, nullptr, 0, D, batch, D, H, part, du, nullptr, 0, st))) return rc;
    if (grads->dw4 && (rc = gemm_km<true>(du, D, saved->hbar, nullptr, 0, H, D, H, batch, part, grads->dw4, nullptr, 0, st))) return rc;
    if (grads->db4 && (rc = colsum(du, D, batch, D, nullptr, grads->db4, cs, st))) return rc;
    if (!need_attn) return RADAD_OK;
    if ((rc = gemm_km<false>(du, D, w->w4, nullptr, 0, H, batch, H, D, part, dhbar, nullptr, 0, st))) return rc;
    const size_t attn_lds = sizeof(float) * ((size_t)2 * k + 8);     // above the 64 KB default from k = 8 188 (legal with a tiny hidden)
    if ((rc = raise_lds(k_attn_bwd, attn_lds))) return rc;
    hipLaunchKernelGGL(k_attn_bwd, dim3((unsigned)batch), dim3(TAIL_THREADS), attn_lds, st, dhbar, saved->a, saved->h, saved->t,
                       w->w2, ds, dpq, k, H);
    RADAD_HIP_CHECK(hipGetLastError());
    if (grads->dw2 && (rc = colsum(saved->t, H, M, H, ds, grads->dw2, cs, st))) return rc;
    if (grads->db2 && (rc = colsum(ds, 1, M, 1, nullptr, grads->db2, cs, st))) return rc;
    if (grads->db1 && (rc = colsum(dpq, 2 * H, M, H, nullptr, grads->db1, cs, st))) return rc;
    if (grads->db3 && (rc = colsum(dpq + H, 2 * H, M, H, nullptr, grads->db3, cs, st))) return rc;
    if (grads->dw1 && (rc = gemm_km<true>(dpq, 2 * H, x_dev, nullptr, 0, D, 2 * H, D, M, part, grads->dw1, grads->dw3, H, st))) return rc;
    if (dx_dev && (rc = gemm_km<false>(dpq, 2 * H, w->w1, w->w3, H, D, M, D, 2 * H, part, dx_dev, nullptr, 0, st))) return rc;
    return RADAD_OK;
}

}  // extern "C"
