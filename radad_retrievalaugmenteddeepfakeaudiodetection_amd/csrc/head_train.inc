// head_train.inc -- training forward and backward of RADADModel's tail: the fuse Linear and the detection MLP
// (radad_model.py:38-41, detection_model.py:41-72,123-126 under autograd) on gfx950.
// Included at the end of proj.hip after proj_train.inc: it reuses gemm_nt_splitk, k_splitk_finish, gemm_km, k_km_finish and the
// tile constants.
//
// Forward, training mode.  a_0 = fused; hidden layer i reads a_{i-1} [B, dims[i]] and writes a_i [B, dims[i+1]]:
//   fused = Wf[:, :D] tpp + Wf[:, D:] proj + bf                       (two products into one stack of partials; no concatenation)
//   z = W_i a_{i-1} + b_i     mean, var (biased, mean of squared deviations from the mean) per column over the batch
//   xh = (z - mean) rstd      y = xh g + beta      a_i = max(y, 0) * mask * inv_keep
//   running_mean <- (1 - f) running_mean + f mean      running_var <- (1 - f) running_var + f var B / (B - 1)
//   logits = W_L a + b_L
// Saved for the backward: fused, and per hidden layer xh (z itself without BatchNorm), rstd, a_i.
//
// Backward, G = d logits:
//   dW_L = G^T a   db_L = sum_b G   da = G W_L
//   dy = da * mask * inv_keep [a_i > 0]   dg = sum_b dy xh   dbeta = sum_b dy   dxh = dy g
//   dz = rstd (dxh - mean_b dxh - xh mean_b(dxh xh))   (dz = dy without BatchNorm)   dW_i = dz^T a_{i-1}   db_i = sum_b dz
//   da_{i-1} = dz W_i
//   df = da_0   dWf = df^T [tpp | proj] (two products, written at column 0 and column D of the one [P, D+P] gradient)
//   dbf = sum_b df   dproj = df Wf[:, D:]   dtpp = df Wf[:, :D] (only when asked for)
// BatchNorm's statistics are per column: one workgroup owns a slab of SLAB_COLS columns and walks all B rows, so nothing
// is synchronised across the grid.  Every sum has a fixed order (split partials in split order, rows in SLAB_GROUPS interleaved
// groups each in row order, the groups in order): no float atomics, two runs give the same bits.  Matrices and products are fp32;
// what a column has one of -- its sums over the batch, mean, variance, rstd -- is accumulated in fp64 and rounded once.

namespace {

constexpr int SLAB_COLS = 64;      // columns a slab workgroup owns
constexpr int SLAB_GROUPS = 16;    // ... walked by this many interleaved row groups
constexpr int HEAD_TRAIN_MAX_WIDTH = 8192;
constexpr int HEAD_OUT_DIRECT_MAX = 8;   // output layers up to this width are row dot products, wider ones a split-K product

// every thread gets sum_g v_g over the row groups of its column, added in group order
__device__ __forceinline__ double slab_sum(double v, double (*s)[SLAB_COLS], int g, int cl) {
    __syncthreads();               // the previous sum has been read
    s[g][cl] = v;
    __syncthreads();
    double t = s[0][cl];
#pragma unroll
    for (int i = 1; i < SLAB_GROUPS; ++i) t += s[i][cl];
    return t;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct SlabFwdParams {
    const float* part; int S;          // [S, B, d] split partials of W a
    const float* bias;                 // [d]
    const float *gamma, *beta;         // [d], or both nullptr: no BatchNorm
    float *rmean, *rvar;               // [d] running statistics, or both nullptr
    float eps, factor;
    const float* mask; float inv_keep; // [B, d] of 0 / 1, or nullptr
    float *xh, *rstd, *act;            // [B, d], [d], [B, d]
    int64_t B; int d;
};

// one block per SLAB_COLS columns of a hidden layer: z = sum of the split partials + bias, rounded once (kept in xh between the
// passes: a thread re-reads only what it wrote itself); the column's mean, then its variance as the mean of squared deviations
// from that mean in a second pass; then xh, act and the running statistics.  Everything a column has one of (sums over the batch,
// mean, var, rstd) is held in fp64 and rounded once where it is stored: the matrices are fp32, their batch statistics cost nothing
// in fp64, and a column of 1000 +- 1 keeps its digits.
__global__ __launch_bounds__(SLAB_COLS * SLAB_GROUPS) void k_head_slab_fwd(SlabFwdParams p) {
    __shared__ double s[SLAB_GROUPS][SLAB_COLS];
    const int cl = threadIdx.x & (SLAB_COLS - 1), g = threadIdx.x / SLAB_COLS;
    const int c = blockIdx.x * SLAB_COLS + cl;
    const bool live = c < p.d;
    const int64_t BN = p.B * p.d;
    const double bias = live ? (double)p.bias[c] : 0.0;
    auto z_of = [&](int64_t r) {
        const float* src = p.part + r * p.d + c;
        double v = 0.0;
        for (int z = 0; z < p.S; ++z) v += (double)src[(int64_t)z * BN];
        return (float)(v + bias);
    };
    auto drop = [&](float a, int64_t i) { return p.mask ? a * p.mask[i] * p.inv_keep : a; };
    if (!p.gamma) {                    // no BatchNorm: xh is the pre-activation
        if (live)
            for (int64_t r = g; r < p.B; r += SLAB_GROUPS) {
                const float z = z_of(r);
                p.xh[r * p.d + c] = z;
                p.act[r * p.d + c] = drop(fmaxf(z, 0.f), r * p.d + c);
            }
        return;
    }
    double acc = 0.0;
    if (live)
        for (int64_t r = g; r < p.B; r += SLAB_GROUPS) {
            const float z = z_of(r);
            p.xh[r * p.d + c] = z;
            acc += (double)z;
        }
    const double mean = slab_sum(acc, s, g, cl) / (double)p.B;
    acc = 0.0;
    if (live)
        for (int64_t r = g; r < p.B; r += SLAB_GROUPS) {
            const double dv = (double)p.xh[r * p.d + c] - mean;
            acc += dv * dv;
        }
    const double var = slab_sum(acc, s, g, cl) / (double)p.B;
    const double rstd = 1.0 / sqrt(var + (double)p.eps);
    if (!live) return;
    const double gm = (double)p.gamma[c], bt = (double)p.beta[c];
    for (int64_t r = g; r < p.B; r += SLAB_GROUPS) {
        const int64_t i = r * p.d + c;
        const double x = ((double)p.xh[i] - mean) * rstd;
        p.xh[i] = (float)x;
        p.act[i] = drop(fmaxf((float)(x * gm + bt), 0.f), i);
    }
    if (g == 0) {
        p.rstd[c] = (float)rstd;
        if (p.rmean) {
            const double f = (double)p.factor;
            p.rmean[c] = (float)((1.0 - f) * (double)p.rmean[c] + f * mean);
            p.rvar[c] = (float)((1.0 - f) * (double)p.rvar[c] + f * (var * ((double)p.B / (double)(p.B - 1))));
        }
    }
}

struct SlabBwdParams {
    float* dz;                         // [B, d] in: da_i, out: dz
    const float* mask; float inv_keep;
    const float *act, *xh;             // [B, d] saved by the forward
    const float *gamma, *rstd;         // [d], or gamma nullptr: no BatchNorm
    float *dgamma, *dbeta, *db;        // [d] each, any of them nullptr: not wanted
    int64_t B; int d;
};

// one block per SLAB_COLS columns: dy in place of da, its two column sums (dbeta, dgamma), then dz in place of dy and db.
// The column sums and what is derived from them are fp64, as in the forward.
__global__ __launch_bounds__(SLAB_COLS * SLAB_GROUPS) void k_head_slab_bwd(SlabBwdParams p) {
    __shared__ double s[SLAB_GROUPS][SLAB_COLS];
    const int cl = threadIdx.x & (SLAB_COLS - 1), g = threadIdx.x / SLAB_COLS;
    const int c = blockIdx.x * SLAB_COLS + cl;
    const bool live = c < p.d;
    const bool bn = p.gamma != nullptr;
    double s1 = 0.0, s2 = 0.0;
    if (live)
        for (int64_t r = g; r < p.B; r += SLAB_GROUPS) {
            const int64_t i = r * p.d + c;
            float dy = p.dz[i];
            if (p.mask) dy = dy * p.mask[i] * p.inv_keep;
            if (!(p.act[i] > 0.f)) dy = 0.f;      // relu's gradient at 0 is 0, as torch; a masked element has act == 0
            p.dz[i] = dy;
            s1 += (double)dy;
            if (bn) s2 += (double)dy * (double)p.xh[i];
        }
    s1 = slab_sum(s1, s, g, cl);
    if (!bn) {
        if (live && g == 0 && p.db) p.db[c] = (float)s1;
        return;
    }
    s2 = slab_sum(s2, s, g, cl);
    double s3 = 0.0;
    if (live) {
        const double gm = (double)p.gamma[c], rs = (double)p.rstd[c];
        const double m1 = gm * s1 / (double)p.B, m2 = gm * s2 / (double)p.B;
        for (int64_t r = g; r < p.B; r += SLAB_GROUPS) {
            const int64_t i = r * p.d + c;
            const float dz = (float)(rs * ((double)p.dz[i] * gm - m1 - (double)p.xh[i] * m2));
            p.dz[i] = dz;
            s3 += (double)dz;
        }
    }
    s3 = slab_sum(s3, s, g, cl);
    if (live && g == 0) {
        if (p.dbeta) p.dbeta[c] = (float)s1;
        if (p.dgamma) p.dgamma[c] = (float)s2;
        if (p.db) p.db[c] = (float)s3;
    }
}

// out[c] = sum_r w[r] A[r, c] (w nullptr: plain column sums) over all R rows, one block per SLAB_COLS columns, the slab kernels'
// row order and fp64 accumulators: the bias gradients, and dW of an output layer of width one
__global__ __launch_bounds__(SLAB_COLS * SLAB_GROUPS) void k_head_colsum(const float* __restrict__ A, int64_t lda, int64_t R, int C,
                                                                       const float* __restrict__ wrow, float* __restrict__ out) {
    __shared__ double s[SLAB_GROUPS][SLAB_COLS];
    const int cl = threadIdx.x & (SLAB_COLS - 1), g = threadIdx.x / SLAB_COLS;
    const int c = blockIdx.x * SLAB_COLS + cl;
    double v = 0.0;
    if (c < C)
        for (int64_t r = g; r < R; r += SLAB_GROUPS) v += wrow ? (double)wrow[r] * (double)A[r * lda + c] : (double)A[r * lda + c];
    v = slab_sum(v, s, g, cl);
    if (c < C && g == 0) out[c] = (float)v;
}

// logits[b, o] = W[o, :] . a[b, :] + bias[o] for a narrow output layer: one wave per row, fp64 accumulators, lanes then the
// butterfly in a fixed order
__global__ __launch_bounds__(256) void k_head_out(const float* __restrict__ a, const float* __restrict__ w, const float* __restrict__ bias,
                                                  float* __restrict__ out, int64_t B, int din, int dout) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const float* ar = a + b * din;
    for (int o = 0; o < dout; ++o) {
        const float* wr = w + (int64_t)o * din;
        double v = 0.0;
        for (int j = lane; j < din; j += 64) v += (double)ar[j] * (double)wr[j];
        v = wave_sum_f64(v);
        if (lane == 0) out[b * dout + o] = (float)(v + (double)bias[o]);
    }
}

int head_colsum(const float* A, int64_t lda, int64_t R, int C, const float* wrow, float* out, hipStream_t st) {
    hipLaunchKernelGGL(k_head_colsum, dim3((unsigned)ceil_div64(C, SLAB_COLS)), dim3(SLAB_COLS * SLAB_GROUPS), 0, st, A, lda, R, C, wrow,
                       out);
    RADAD_HIP_CHECK(hipGetLastError());
    return RADAD_OK;
}

// out[m * ldo + n] = sum_z part[z, m, n] in split order: a product that lands inside a wider matrix
__global__ __launch_bounds__(256) void k_km_finish_ld(const float* __restrict__ part, int S, int64_t M, int N, float* __restrict__ out,
                                                      int64_t ldo) {
    const int64_t total = M * N;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = i / N;
        float v = 0.f;
        for (int z = 0; z < S; ++z) v += part[(int64_t)z * total + i];
        out[m * ldo + (i - m * N)] = v;
    }
}

// out[:, 0:N] (row stride ldo) = A^T B, A [Kr, M], B [Kr, N]
int gemm_km_strided_out(const float* a, int64_t lda, const float* b, int64_t ldb, int64_t M, int N, int64_t Kr, float* part, float* out,
                        int64_t ldo, hipStream_t st) {
    int S, cps, rc;
    red_plan(M, N, Kr, &S, &cps);
    if ((rc = gemm_km_launch<true>(a, lda, b, nullptr, 0, ldb, M, N, Kr, part, S, cps, st))) return rc;
    hipLaunchKernelGGL(k_km_finish_ld, dim3((unsigned)std::min<int64_t>(ceil_div64(M * N, 256), 4096)), dim3(256), 0, st, part, S, M, N,
                       out, ldo);
    RADAD_HIP_CHECK(hipGetLastError());
    return RADAD_OK;
}

inline bool head_train_dims_ok(int64_t batch, int dim, int proj_dim, int n_layers, const int32_t* dims) {
    if (!(batch >= 0 && batch < (1ll << 31) - GT && dim > 0 && dim <= TRAIN_MAX_DIM && proj_dim > 0 && proj_dim <= HEAD_TRAIN_MAX_WIDTH))
        return false;
    if (!(n_layers >= 1 && n_layers <= HEAD_MAX_LAYERS && dims && dims[0] == proj_dim)) return false;
    for (int l = 0; l <= n_layers; ++l)
        if (dims[l] <= 0 || dims[l] > HEAD_TRAIN_MAX_WIDTH) return false;
    return true;
}

// workspace layout shared by the forward (part) and the backward (everything)
struct HeadTrainWs {
    size_t part, part_hi, buf0, buf1, total;   // part_hi: where the proj half's partials follow the tpp half's
    HeadTrainWs(int64_t B, int D, int P, int n, const int32_t* dims) {
        part_hi = 0;
        {
            int S, cps;
            split_plan(B, P, D, &S, &cps);
            part_hi = (size_t)S * (size_t)B * (size_t)P * sizeof(float);
        }
        size_t pb = al256(part_hi + part_bytes(B, P, P));
        int maxw = P;
        for (int l = 0; l < n; ++l) {
            const int din = dims[l], dout = dims[l + 1];
            maxw = std::max(maxw, std::max(din, dout));
            pb = std::max(pb, part_bytes(B, dout, din));                 // z / logits
            pb = std::max(pb, km_part_bytes(dout, din, B, false));       // dW_i
            pb = std::max(pb, km_part_bytes(B, din, dout, false));       // da_{i-1}
        }
        pb = std::max(pb, km_part_bytes(P, D, B, true));                 // dWf, tpp half
        pb = std::max(pb, km_part_bytes(P, P, B, true));                 // dWf, proj half
        pb = std::max(pb, km_part_bytes(B, P, P, false));                // dproj
        pb = std::max(pb, km_part_bytes(B, D, P, false));                // dtpp
        size_t off = pb;
        auto take = [&](size_t floats) { const size_t o = off; off += al256(floats * sizeof(float)); return o; };
        part = 0;
        buf0 = take((size_t)B * maxw);
        buf1 = take((size_t)B * maxw);
        total = off;
    }
};

// the checks both calls share, each RADAD_EINVAL before any HIP call
int head_train_check(const char* who, const radad_head_train_weights* w, const radad_head_saved* saved, int64_t batch, int dim,
                     int proj_dim, bool forward) {
    RADAD_REQUIRE(w && saved, "%s: NULL struct", who);
    RADAD_REQUIRE(w->n_layers >= 1 && w->n_layers <= HEAD_MAX_LAYERS, "%s: bad shape: n_layers %d outside 1..%d", who, w->n_layers,
                  HEAD_MAX_LAYERS);
    RADAD_REQUIRE(w->dims[0] == proj_dim, "%s: bad shape: head input width %d != proj_dim %d", who, w->dims[0], proj_dim);
    RADAD_REQUIRE(head_train_dims_ok(batch, dim, proj_dim, w->n_layers, w->dims),
                  "%s: bad shape (batch < 2^31 - 128, every width in 1..%d)", who, HEAD_TRAIN_MAX_WIDTH);
    for (int l = 0; l + 1 < w->n_layers; ++l) {
        RADAD_REQUIRE((w->bn_gamma[l] == nullptr) == (w->bn_beta[l] == nullptr), "%s: layer %d: bn_gamma / bn_beta half NULL", who, l);
        RADAD_REQUIRE((w->bn_running_mean[l] == nullptr) == (w->bn_running_var[l] == nullptr),
                      "%s: layer %d: bn_running_mean / bn_running_var half NULL", who, l);
        RADAD_REQUIRE(!(w->bn_gamma[l] && batch == 1),
                      "%s: layer %d: BatchNorm in training mode needs more than 1 value per channel (batch == 1)", who, l);
    }
    if (batch == 0) return RADAD_OK;
    RADAD_REQUIRE(w->wf && (w->bf || !forward), "%s: NULL weight", who);
    for (int l = 0; l < w->n_layers; ++l) RADAD_REQUIRE(w->lw[l] && (w->lb[l] || !forward), "%s: NULL weight (layer %d)", who, l);
    RADAD_REQUIRE(saved->fused, "%s: NULL saved-activation buffer", who);
    for (int l = 0; l + 1 < w->n_layers; ++l)
        RADAD_REQUIRE(saved->xh[l] && saved->act[l] && (saved->rstd[l] || !w->bn_gamma[l]), "%s: NULL saved-activation buffer (layer %d)",
                      who, l);
    return RADAD_OK;
}

}  // namespace

extern "C" {

int64_t radad_fuse_head_train_workspace_bytes(int64_t batch, int dim, int proj_dim, int n_layers, const int32_t* dims) {
    if (!head_train_dims_ok(batch, dim, proj_dim, n_layers, dims)) return -1;
    return (int64_t)HeadTrainWs(batch, dim, proj_dim, n_layers, dims).total;
}

int radad_fuse_head_train_forward(const radad_head_train_weights* w, const float* tpp_dev, const float* proj_dev,
                                  const float* const* masks_dev, float inv_keep, int64_t batch, int dim, int proj_dim,
                                  const radad_head_saved* saved, float* logits_out_dev, float* workspace_dev, int64_t workspace_bytes,
                                  int device, void* stream) {
    const char* who = "radad_fuse_head_train_forward";
    int rc;
    if ((rc = head_train_check(who, w, saved, batch, dim, proj_dim, true))) return rc;
    if (batch == 0) return RADAD_OK;
    RADAD_REQUIRE(tpp_dev && proj_dev && logits_out_dev && workspace_dev, "%s: NULL buffer", who);
    RADAD_REQUIRE(workspace_bytes >= radad_fuse_head_train_workspace_bytes(batch, dim, proj_dim, w->n_layers, w->dims),
                  "%s: workspace too small", who);
    DeviceGuard g(device);
    hipStream_t st = (hipStream_t)stream;
    const int n = w->n_layers, P = proj_dim;
    const HeadTrainWs L(batch, dim, proj_dim, n, w->dims);
    char* ws = reinterpret_cast<char*>(workspace_dev);
    float* part = (float*)(ws + L.part);
    const auto fin_grid = [](int64_t total) { return dim3((unsigned)std::min<int64_t>(ceil_div64(total, 256), 4096)); };
    const int64_t ldwf = (int64_t)dim + P;
    int S = 1, S2 = 1;
    // fused: the tpp half's split partials, the proj half's behind them, summed in that order
    if ((rc = gemm_nt_splitk(tpp_dev, dim, w->wf, w->wf, P, ldwf, part, batch, P, dim, &S, st))) return rc;
    if ((rc = gemm_nt_splitk(proj_dev, P, w->wf + dim, w->wf + dim, P, ldwf, (float*)(ws + L.part_hi), batch, P, P, &S2, st))) return rc;
    hipLaunchKernelGGL(k_splitk_finish, fin_grid(batch * P), dim3(256), 0, st, part, S + S2, batch, P, w->bf, (int)ACT_NONE, saved->fused,
                       (int64_t)P);
    RADAD_HIP_CHECK(hipGetLastError());
    const float* a = saved->fused;
    for (int l = 0; l < n; ++l) {
        const int din = w->dims[l], dout = w->dims[l + 1];
        if (l + 1 == n && dout <= HEAD_OUT_DIRECT_MAX) {
            hipLaunchKernelGGL(k_head_out, dim3((unsigned)ceil_div64(batch, 4)), dim3(256), 0, st, a, w->lw[l], w->lb[l], logits_out_dev,
                               batch, din, dout);
            RADAD_HIP_CHECK(hipGetLastError());
            break;
        }
        if ((rc = gemm_nt_splitk(a, din, w->lw[l], w->lw[l], dout, din, part, batch, dout, din, &S, st))) return rc;
        if (l + 1 == n) {
            hipLaunchKernelGGL(k_splitk_finish, fin_grid(batch * dout), dim3(256), 0, st, part, S, batch, dout, w->lb[l], (int)ACT_NONE,
                               logits_out_dev, (int64_t)dout);
            RADAD_HIP_CHECK(hipGetLastError());
            break;
        }
        SlabFwdParams sp{part, S, w->lb[l], w->bn_gamma[l], w->bn_beta[l], w->bn_running_mean[l], w->bn_running_var[l], w->bn_eps[l],
                         w->bn_factor[l], masks_dev ? masks_dev[l] : nullptr, inv_keep, saved->xh[l], saved->rstd[l], saved->act[l],
                         batch, dout};
        hipLaunchKernelGGL(k_head_slab_fwd, dim3((unsigned)ceil_div64(dout, SLAB_COLS)), dim3(SLAB_COLS * SLAB_GROUPS), 0, st, sp);
        RADAD_HIP_CHECK(hipGetLastError());
        a = saved->act[l];
    }
    return RADAD_OK;
}

int radad_fuse_head_backward(const radad_head_train_weights* w, const float* tpp_dev, const float* proj_dev,
                             const float* const* masks_dev, float inv_keep, const radad_head_saved* saved,
                             const float* grad_logits_dev, int64_t batch, int dim, int proj_dim, const radad_head_grads* grads,
                             float* dtpp_dev, float* dproj_dev, float* workspace_dev, int64_t workspace_bytes, int device,
                             void* stream) {
    const char* who = "radad_fuse_head_backward";
    int rc;
    if ((rc = head_train_check(who, w, saved, batch, dim, proj_dim, false))) return rc;
    RADAD_REQUIRE(grads, "%s: NULL struct", who);
    if (batch == 0) return RADAD_OK;
    RADAD_REQUIRE(tpp_dev && proj_dev && grad_logits_dev && workspace_dev, "%s: NULL buffer", who);
    RADAD_REQUIRE(workspace_bytes >= radad_fuse_head_train_workspace_bytes(batch, dim, proj_dim, w->n_layers, w->dims),
                  "%s: workspace too small", who);
    DeviceGuard g(device);
    hipStream_t st = (hipStream_t)stream;
    const int n = w->n_layers, P = proj_dim, D = dim;
    const HeadTrainWs L(batch, dim, proj_dim, n, w->dims);
    char* ws = reinterpret_cast<char*>(workspace_dev);
    float* part = (float*)(ws + L.part);
    float* cur = (float*)(ws + L.buf0);      // d a_l, then dz_l in place
    float* nxt = (float*)(ws + L.buf1);
    const bool need_df = grads->dwf || grads->dbf || dproj_dev || dtpp_dev;
    const float* dz = grad_logits_dev;       // the output layer has no norm or activation: dz_L = G
    for (int l = n - 1; l >= 0; --l) {
        const int din = w->dims[l], dout = w->dims[l + 1];
        const float* a_in = l == 0 ? saved->fused : saved->act[l - 1];
        if (l + 1 < n) {
            SlabBwdParams sp{cur, masks_dev ? masks_dev[l] : nullptr, inv_keep, saved->act[l], saved->xh[l], w->bn_gamma[l],
                             saved->rstd[l], grads->dgamma[l], grads->dbeta[l], grads->dlb[l], batch, dout};
            hipLaunchKernelGGL(k_head_slab_bwd, dim3((unsigned)ceil_div64(dout, SLAB_COLS)), dim3(SLAB_COLS * SLAB_GROUPS), 0, st, sp);
            RADAD_HIP_CHECK(hipGetLastError());
            dz = cur;
        } else if (grads->dlb[l] && (rc = head_colsum(dz, dout, batch, dout, nullptr, grads->dlb[l], st))) {
            return rc;
        }
        if (grads->dlw[l]) {
            if (dout == 1) rc = head_colsum(a_in, din, batch, din, dz, grads->dlw[l], st);      // one output: a weighted column sum
            else rc = gemm_km<true>(dz, dout, a_in, nullptr, 0, din, dout, din, batch, part, grads->dlw[l], nullptr, 0, st);
            if (rc) return rc;
        }
        if (l == 0 && !need_df) return RADAD_OK;
        if ((rc = gemm_km<false>(dz, dout, w->lw[l], nullptr, 0, din, batch, din, dout, part, nxt, nullptr, 0, st))) return rc;
        float* t = cur; cur = nxt; nxt = t;
    }
    const float* df = cur;
    const int64_t ldwf = (int64_t)D + P;
    if (grads->dwf) {
        if ((rc = gemm_km_strided_out(df, P, tpp_dev, D, P, D, batch, part, grads->dwf, ldwf, st))) return rc;
        if ((rc = gemm_km_strided_out(df, P, proj_dev, P, P, P, batch, part, grads->dwf + D, ldwf, st))) return rc;
    }
    if (grads->dbf && (rc = head_colsum(df, P, batch, P, nullptr, grads->dbf, st))) return rc;
    if (dproj_dev && (rc = gemm_km<false>(df, P, w->wf + D, nullptr, 0, ldwf, batch, P, P, part, dproj_dev, nullptr, 0, st))) return rc;
    if (dtpp_dev && (rc = gemm_km<false>(df, P, w->wf, nullptr, 0, ldwf, batch, D, P, part, dtpp_dev, nullptr, 0, st))) return rc;
    return RADAD_OK;
}

}  // extern "C"
