// optim_step.inc -- what RADAD's training step does after the backward (pipeline.py:815-836), on gfx950:
// BCEWithLogitsLoss(pos_weight) with its gradient and the accuracy count, GradScaler.unscale_, clip_grad_norm_ per optimizer,
// torch.optim.Adam (weight_decay added to the gradient, not decoupled) per optimizer, GradScaler.step's skip and
// GradScaler.update.  Included at the end of proj.hip after head_train.inc.
//
// Four launches, no host round trip:
//   k_bce_logits    one workgroup: mean loss, d logits (times scale / n), correct count
//   k_optim_sumsq   one workgroup per chunk of OPTIM_CHUNK gradient elements: fp64 sum of (g inv_scale)^2 and a non-finite flag
//   k_optim_finish  one wave per group: the group's partials in chunk order -> norm, found_inf, clip coefficient, step count and
//                   Adam's two bias corrections; then one thread does GradScaler.update
//   k_adam_clip     one workgroup per chunk: g <- g inv_scale coef in place, then Adam on p, m, v in the same pass
// A chunk is OPTIM_CHUNK elements of one tensor whatever the grid or the device; a thread owns fixed elements of it; per-thread
// sums, the wave butterfly, the four waves in order, the chunks of a group lane-strided then the butterfly: every sum has one
// order, no float atomics, two runs give the same bits.  Data and per-element arithmetic are fp32 (torch's own op order); every
// sum and everything a group has one of (norm, coefficient, 1 - beta^t, lr / (1 - beta1^t)) is formed in fp64 and rounded once.
//
// The loss scale is read by k_bce_logits, k_optim_sumsq and k_optim_finish, which run in that order in front of its update
// inside k_optim_finish; k_adam_clip, which runs behind it, reads the copy of 1 / scale that k_optim_finish left in the
// workspace head (OptimScalars::inv_scale), never the scale itself.

namespace {

constexpr int OPTIM_CHUNK = 4096;        // elements of one tensor per chunk, and per workgroup: a constant, not a function of the grid
constexpr int OPTIM_THREADS = 256;
constexpr int OPTIM_VECS = OPTIM_CHUNK / (4 * OPTIM_THREADS);   // f32x4 per thread and array: element 4 (tid + 256 j) + i
constexpr int OPTIM_FINISH_THREADS = 64 * RADAD_OPTIM_MAX_GROUPS;
constexpr int BCE_THREADS = 256;
static_assert(OPTIM_VECS * 4 * OPTIM_THREADS == OPTIM_CHUNK, "a chunk is a whole number of f32x4 per thread");

// the step's tensors, by value in the kernel arguments (gradient pointers change every step): live tensors only, sorted by
// group, so a group's chunks are one range
struct OptimTable {
    float* p[RADAD_OPTIM_MAX_TENSORS];
    float* g[RADAD_OPTIM_MAX_TENSORS];
    float* m[RADAD_OPTIM_MAX_TENSORS];
    float* v[RADAD_OPTIM_MAX_TENSORS];
    int64_t numel[RADAD_OPTIM_MAX_TENSORS];
    int32_t chunk0[RADAD_OPTIM_MAX_TENSORS + 1];   // prefix sums of ceil(numel / OPTIM_CHUNK), strictly increasing
    int32_t group[RADAD_OPTIM_MAX_TENSORS];
    int32_t n;
};

struct OptimGroups {
    float lr[RADAD_OPTIM_MAX_GROUPS], beta1[RADAD_OPTIM_MAX_GROUPS], beta2[RADAD_OPTIM_MAX_GROUPS], eps[RADAD_OPTIM_MAX_GROUPS],
        wd[RADAD_OPTIM_MAX_GROUPS], max_norm[RADAD_OPTIM_MAX_GROUPS];
    int32_t chunk_lo[RADAD_OPTIM_MAX_GROUPS], chunk_hi[RADAD_OPTIM_MAX_GROUPS];
    int32_t n;
};

// head of the workspace: what k_optim_finish hands to k_adam_clip
struct OptimScalars {
    float inv_scale;                              // 1 / scale as it was before this step's update (1 without a scale)
    int32_t pad;
    float coef[RADAD_OPTIM_MAX_GROUPS];           // clip_grad_norm_'s clip_coef_clamped
    float step_size[RADAD_OPTIM_MAX_GROUPS];      // lr / (1 - beta1^t)
    float bc2_sqrt[RADAD_OPTIM_MAX_GROUPS];       // sqrt(1 - beta2^t)
    int32_t skip[RADAD_OPTIM_MAX_GROUPS];         // found_inf under a loss scale, or nothing to step
};

constexpr size_t OPTIM_WS_HEAD = 256;
static_assert(sizeof(OptimScalars) <= OPTIM_WS_HEAD, "the workspace head holds OptimScalars");
static_assert(sizeof(OptimTable) + sizeof(OptimGroups) + 64 <= 4096, "the tables travel as kernel arguments");

struct OptimWs {
    size_t partial, flag, total;
    explicit OptimWs(int64_t chunks) {
        partial = OPTIM_WS_HEAD;
        flag = partial + al256((size_t)chunks * sizeof(double));
        total = flag + al256((size_t)chunks * sizeof(int32_t));
    }
};

// the tensor that chunk c belongs to: the largest t with chunk0[t] <= c
__device__ __forceinline__ int optim_find(const int32_t* chunk0, int n, int c) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunk0[mid] <= c) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// mean BCE-with-logits loss (unscaled), its gradient times scale / n, and the count of (x > 0) == (y == 1).
// One workgroup, so the order of the sum is the same on any device: thread i adds elements i, i + 256, ... in fp64, then the
// butterfly, then the four waves in order.  Per element everything is fp64 and rounded once (n is a batch size).
// sigmoid(-x) is formed as 1 - sigmoid(x): on the saturated right side (x = -100 with y = 0, x = +100 with y = 1) the gradient
// is then exactly 0, as torch's float32 sigmoid makes it, and on the saturated wrong side it is scale w / n.
__global__ __launch_bounds__(BCE_THREADS) void k_bce_logits(const float* __restrict__ x, const float* __restrict__ y, int64_t n,
                                                            float pos_weight, const float* __restrict__ scale,
                                                            float* __restrict__ loss_out, float* __restrict__ dx,
                                                            int32_t* __restrict__ correct_out) {
    __shared__ double s_sum[BCE_THREADS / 64];
    __shared__ int s_cnt[BCE_THREADS / 64];
    const double s_over_n = (scale ? (double)*scale : 1.0) / (double)n;
    const double pw1 = (double)pos_weight - 1.0;
    double acc = 0.0;
    int cnt = 0;
    for (int64_t i = threadIdx.x; i < n; i += BCE_THREADS) {
        const double xi = (double)x[i], yi = (double)y[i];
        const double w = 1.0 + pw1 * yi;
        const double e = exp(-fabs(xi));
        acc += (1.0 - yi) * xi + w * (log1p(e) + fmax(-xi, 0.0));
        const double sig = xi >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
        dx[i] = (float)(s_over_n * ((1.0 - yi) - w * (1.0 - sig)));
        cnt += (x[i] > 0.f) == (y[i] == 1.f);
    }
    acc = wave_sum_f64(acc);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((threadIdx.x & 63) == 0) {
        s_sum[threadIdx.x >> 6] = acc;
        s_cnt[threadIdx.x >> 6] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = s_sum[0];
        int c = s_cnt[0];
        for (int w = 1; w < BCE_THREADS / 64; ++w) { t += s_sum[w]; c += s_cnt[w]; }
        *loss_out = (float)(t / (double)n);
        *correct_out = c;
    }
}

// one workgroup per chunk: partial[c] = sum over the chunk of (g inv_scale)^2 in fp64 (the product rounded to fp32 first: what
// unscale_ leaves is what clip_grad_norm_ measures), flag[c] = any element not finite.  16-byte loads where the tensor starts on
// a 16-byte boundary and the four elements lie inside the chunk; the chunk's last few elements, and every element of a tensor
// that starts elsewhere (a view), are single loads.  A thread owns the same elements either way, so the sum does not depend on
// the path.
__global__ __launch_bounds__(OPTIM_THREADS) void k_optim_sumsq(OptimTable T, const float* __restrict__ scale,
                                                               double* __restrict__ partial, int32_t* __restrict__ flag) {
    __shared__ double s_sum[OPTIM_THREADS / 64];
    const int c = blockIdx.x;
    const int t = optim_find(T.chunk0, T.n, c);
    const int64_t base = (int64_t)(c - T.chunk0[t]) * OPTIM_CHUNK;
    const int64_t left = T.numel[t] - base;
    const int cnt = left < OPTIM_CHUNK ? (int)left : OPTIM_CHUNK;
    const float* g = T.g[t] + base;
    const bool vec = al16(g);
    const float inv = scale ? (float)(1.0 / (double)*scale) : 1.f;
    double acc = 0.0;
    int bad = 0;
#pragma unroll
    for (int j = 0; j < OPTIM_VECS; ++j) {
        const int e = 4 * ((int)threadIdx.x + OPTIM_THREADS * j);
        f32x4 q = {0.f, 0.f, 0.f, 0.f};
        if (vec && e + 4 <= cnt) {
            q = *reinterpret_cast<const f32x4*>(g + e);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (e + i < cnt) q[i] = g[e + i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            bad |= !__builtin_isfinite(q[i]);
            const float u = q[i] * inv;
            acc += (double)u * (double)u;
        }
    }
    acc = wave_sum_f64(acc);
    bad = __syncthreads_or(bad);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = s_sum[0];
        for (int w = 1; w < OPTIM_THREADS / 64; ++w) s += s_sum[w];
        partial[c] = s;
        flag[c] = bad != 0;
    }
}

struct OptimFinishParams {
    OptimGroups G;
    float* scale; int32_t* tracker;        // both nullptr: no loss scale, nothing is skipped
    int32_t* steps; float* grad_norm; int32_t* found_inf;
    float growth, backoff; int interval;
    const double* partial; const int32_t* flag;
    OptimScalars* out;
};

// one workgroup; wave g owns group g: lane l adds the group's chunks l, l + 64, ... in order, then the butterfly.  Lane 0 writes
// norm, found_inf, the clip coefficient (clip_grad_norm_: max_norm / (norm + 1e-6) clamped at 1, a NaN stays a NaN) and, when
// the group steps, its new step count with Adam's bias corrections.  A group steps unless a loss scale is in use and it found a
// non-finite gradient, or it has no gradient at all this step.  Then thread 0 does GradScaler.update (_amp_update_scale_).
__global__ __launch_bounds__(OPTIM_FINISH_THREADS) void k_optim_finish(OptimFinishParams p) {
    __shared__ int s_found[RADAD_OPTIM_MAX_GROUPS];
    const int g = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (g < p.G.n) {
        const int lo = p.G.chunk_lo[g], hi = p.G.chunk_hi[g];
        double acc = 0.0;
        int bad = 0;
        for (int c = lo + lane; c < hi; c += 64) {
            acc += p.partial[c];
            bad |= p.flag[c];
        }
        acc = wave_sum_f64(acc);
        const int found = __ballot(bad) != 0;
        if (lane == 0) {
            const double norm = sqrt(acc);
            const double mx = (double)p.G.max_norm[g];
            double coef = 1.0;
            if (mx > 0.0) {
                coef = mx / (norm + 1e-6);
                if (coef > 1.0) coef = 1.0;
            }
            const bool skip = hi == lo || (p.scale != nullptr && found);
            if (!skip) {
                const int t = p.steps[g] + 1;
                p.steps[g] = t;
                const double bc1 = 1.0 - pow((double)p.G.beta1[g], (double)t);
                const double bc2 = 1.0 - pow((double)p.G.beta2[g], (double)t);
                p.out->step_size[g] = (float)((double)p.G.lr[g] / bc1);
                p.out->bc2_sqrt[g] = (float)sqrt(bc2);
            }
            p.out->coef[g] = (float)coef;
            p.out->skip[g] = skip;
            p.grad_norm[g] = (float)norm;
            p.found_inf[g] = found;
            s_found[g] = found;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float inv = 1.f;
        if (p.scale) {
            const float s = *p.scale;
            inv = (float)(1.0 / (double)s);
            int any = 0;
            for (int i = 0; i < p.G.n; ++i) any |= s_found[i];
            if (any) {
                *p.scale = s * p.backoff;
                *p.tracker = 0;
            } else {
                const int ok = *p.tracker + 1;
                if (ok == p.interval) {
                    const float grown = s * p.growth;
                    if (__builtin_isfinite(grown)) *p.scale = grown;
                    *p.tracker = 0;
                } else {
                    *p.tracker = ok;
                }
            }
        }
        p.out->inv_scale = inv;
    }
}

struct AdamConsts {
    float inv, coef, wd, b1, omb1, b2, omb2, step, bc2, eps;
};

// torch/optim/adam.py _single_tensor_adam on what unscale_ and clip_grad_norm_ left, in torch's op order
__device__ __forceinline__ void adam_elem(float& p, float& g, float& m, float& v, const AdamConsts& k) {
    g = g * k.inv * k.coef;                    // stays in .grad
    const float gd = g + k.wd * p;
    m = k.b1 * m + k.omb1 * gd;
    v = k.b2 * v + k.omb2 * gd * gd;
    p -= k.step * (m / (sqrtf(v) / k.bc2 + k.eps));
}

// one workgroup per chunk of a group that steps: one read and one write of p, g, m, v.  A whole chunk of four 16-byte aligned
// arrays is 16 wide loads in flight per thread; anything else (a tensor's last chunk, a view that starts mid-vector) goes
// element by element under the chunk's bound.
__global__ __launch_bounds__(OPTIM_THREADS) void k_adam_clip(OptimTable T, OptimGroups G, const OptimScalars* __restrict__ S) {
    const int c = blockIdx.x;
    const int t = optim_find(T.chunk0, T.n, c);
    const int gi = T.group[t];
    if (S->skip[gi]) return;
    const int64_t base = (int64_t)(c - T.chunk0[t]) * OPTIM_CHUNK;
    const int64_t left = T.numel[t] - base;
    const int cnt = left < OPTIM_CHUNK ? (int)left : OPTIM_CHUNK;
    float* p = T.p[t] + base;
    float* g = T.g[t] + base;
    float* m = T.m[t] + base;
    float* v = T.v[t] + base;
    AdamConsts k;
    k.inv = S->inv_scale; k.coef = S->coef[gi]; k.step = S->step_size[gi]; k.bc2 = S->bc2_sqrt[gi];
    k.wd = G.wd[gi]; k.eps = G.eps[gi];
    k.b1 = G.beta1[gi]; k.omb1 = (float)(1.0 - (double)k.b1);
    k.b2 = G.beta2[gi]; k.omb2 = (float)(1.0 - (double)k.b2);
    if (cnt == OPTIM_CHUNK && al16(p) && al16(g) && al16(m) && al16(v)) {
        f32x4 qp[OPTIM_VECS], qg[OPTIM_VECS], qm[OPTIM_VECS], qv[OPTIM_VECS];
#pragma unroll
        for (int j = 0; j < OPTIM_VECS; ++j) {
            const int e = 4 * ((int)threadIdx.x + OPTIM_THREADS * j);
            qp[j] = *reinterpret_cast<const f32x4*>(p + e);
            qg[j] = *reinterpret_cast<const f32x4*>(g + e);
            qm[j] = *reinterpret_cast<const f32x4*>(m + e);
            qv[j] = *reinterpret_cast<const f32x4*>(v + e);
        }
#pragma unroll
        for (int j = 0; j < OPTIM_VECS; ++j) {
            const int e = 4 * ((int)threadIdx.x + OPTIM_THREADS * j);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float a = qp[j][i], b = qg[j][i], mm = qm[j][i], vv = qv[j][i];
                adam_elem(a, b, mm, vv, k);
                qp[j][i] = a; qg[j][i] = b; qm[j][i] = mm; qv[j][i] = vv;
            }
            *reinterpret_cast<f32x4*>(p + e) = qp[j];
            *reinterpret_cast<f32x4*>(g + e) = qg[j];
            *reinterpret_cast<f32x4*>(m + e) = qm[j];
            *reinterpret_cast<f32x4*>(v + e) = qv[j];
        }
        return;
    }
    for (int e = threadIdx.x; e < cnt; e += OPTIM_THREADS) {
        float a = p[e], b = g[e], mm = m[e], vv = v[e];
        adam_elem(a, b, mm, vv, k);
        p[e] = a; g[e] = b; m[e] = mm; v[e] = vv;
    }
}

inline bool unit_open(float b) { return b >= 0.f && b < 1.f; }      // false for a NaN

// chunks of every tensor with at least one element, or -1 where a numel is negative or the total leaves int32
inline int64_t optim_chunks(const int64_t* numels, int n) {
    int64_t chunks = 0;
    for (int i = 0; i < n; ++i) {
        if (numels[i] < 0 || numels[i] > (1ll << 42)) return -1;
        chunks += ceil_div64(numels[i], OPTIM_CHUNK);
    }
    return chunks < (1ll << 31) - 1 ? chunks : -1;
}

}  // namespace

extern "C" {

int64_t radad_optim_workspace_bytes(const int64_t* numels, int n_tensors) {
    if (n_tensors < 0 || n_tensors > RADAD_OPTIM_MAX_TENSORS || (n_tensors > 0 && !numels)) return -1;
    const int64_t chunks = optim_chunks(numels, n_tensors);
    if (chunks < 0) return -1;
    return (int64_t)OptimWs(chunks).total;
}

int radad_bce_logits(const float* logits_dev, const float* labels_dev, int64_t n, float pos_weight, const float* scale_dev,
                     float* loss_out_dev, float* dlogits_out_dev, int32_t* correct_out_dev, int device, void* stream) {
    const char* who = "radad_bce_logits";
    RADAD_REQUIRE(n > 0, "%s: n must be at least 1 (the mean of no losses is not a number), got %lld", who, (long long)n);
    RADAD_REQUIRE(pos_weight > 0.f, "%s: pos_weight must be positive, got %g", who, (double)pos_weight);
    RADAD_REQUIRE(logits_dev && labels_dev && loss_out_dev && dlogits_out_dev && correct_out_dev, "%s: NULL buffer", who);
    DeviceGuard g(device);
    hipLaunchKernelGGL(k_bce_logits, dim3(1), dim3(BCE_THREADS), 0, (hipStream_t)stream, logits_dev, labels_dev, n, pos_weight,
                       scale_dev, loss_out_dev, dlogits_out_dev, correct_out_dev);
    RADAD_HIP_CHECK(hipGetLastError());
    return RADAD_OK;
}

int radad_optim_step(const radad_optim_tensor* tensors_host, int n_tensors, const radad_optim_group* groups_host, int n_groups,
                     const radad_optim_state* state, float growth, float backoff, int growth_interval, void* ws_dev,
                     int64_t ws_bytes, int device, void* stream) {
    const char* who = "radad_optim_step";
    RADAD_REQUIRE(n_tensors >= 0 && n_tensors <= RADAD_OPTIM_MAX_TENSORS, "%s: n_tensors %d outside 0..%d", who, n_tensors,
                  RADAD_OPTIM_MAX_TENSORS);
    RADAD_REQUIRE(n_groups >= 1 && n_groups <= RADAD_OPTIM_MAX_GROUPS, "%s: n_groups %d outside 1..%d", who, n_groups,
                  RADAD_OPTIM_MAX_GROUPS);
    RADAD_REQUIRE(groups_host && state && (tensors_host || n_tensors == 0), "%s: NULL struct", who);
    RADAD_REQUIRE(state->steps && state->grad_norm && state->found_inf, "%s: NULL state pointer (steps, grad_norm, found_inf)", who);
    RADAD_REQUIRE((state->scale == nullptr) == (state->growth_tracker == nullptr), "%s: scale / growth_tracker half NULL", who);
    if (state->scale)
        RADAD_REQUIRE(growth >= 1.f && backoff > 0.f && backoff <= 1.f && growth_interval >= 1,
                      "%s: loss scale needs growth >= 1, 0 < backoff <= 1 and growth_interval >= 1, got %g, %g, %d", who,
                      (double)growth, (double)backoff, growth_interval);
    OptimGroups G{};
    G.n = n_groups;
    for (int i = 0; i < n_groups; ++i) {
        const radad_optim_group& h = groups_host[i];
        RADAD_REQUIRE(unit_open(h.beta1) && unit_open(h.beta2), "%s: group %d: betas (%g, %g) outside [0, 1)", who, i,
                      (double)h.beta1, (double)h.beta2);
        RADAD_REQUIRE(h.eps > 0.f, "%s: group %d: eps must be positive, got %g", who, i, (double)h.eps);
        RADAD_REQUIRE(h.lr >= 0.f, "%s: group %d: lr must not be negative, got %g", who, i, (double)h.lr);
        RADAD_REQUIRE(h.weight_decay >= 0.f, "%s: group %d: weight_decay must not be negative, got %g", who, i,
                      (double)h.weight_decay);
        RADAD_REQUIRE(h.max_norm == h.max_norm, "%s: group %d: max_norm is not a number", who, i);
        G.lr[i] = h.lr; G.beta1[i] = h.beta1; G.beta2[i] = h.beta2; G.eps[i] = h.eps; G.wd[i] = h.weight_decay;
        G.max_norm[i] = h.max_norm;
    }
    int64_t numels[RADAD_OPTIM_MAX_TENSORS];
    for (int i = 0; i < n_tensors; ++i) {
        const radad_optim_tensor& h = tensors_host[i];
        RADAD_REQUIRE(h.group >= 0 && h.group < n_groups, "%s: tensor %d: group %d outside 0..%d", who, i, h.group, n_groups - 1);
        RADAD_REQUIRE(h.numel >= 0, "%s: tensor %d: numel %lld is negative", who, i, (long long)h.numel);
        RADAD_REQUIRE(!h.grad || h.numel == 0 || (h.param && h.exp_avg && h.exp_avg_sq),
                      "%s: tensor %d: NULL param / exp_avg / exp_avg_sq beside a gradient", who, i);
        numels[i] = h.numel;
    }
    const int64_t need = radad_optim_workspace_bytes(numels, n_tensors);
    RADAD_REQUIRE(need >= 0, "%s: more than 2^31 - 2 chunks of %d elements", who, OPTIM_CHUNK);
    RADAD_REQUIRE(ws_dev, "%s: NULL workspace", who);
    RADAD_REQUIRE(ws_bytes >= need, "%s: workspace too small (%lld < %lld bytes)", who, (long long)ws_bytes, (long long)need);
    // the live tensors, group by group in the caller's order
    OptimTable T{};
    int n = 0;
    int32_t chunks = 0;
    for (int gi = 0; gi < n_groups; ++gi) {
        G.chunk_lo[gi] = chunks;
        for (int i = 0; i < n_tensors; ++i) {
            const radad_optim_tensor& h = tensors_host[i];
            if (h.group != gi || !h.grad || h.numel == 0) continue;
            T.p[n] = h.param; T.g[n] = h.grad; T.m[n] = h.exp_avg; T.v[n] = h.exp_avg_sq;
            T.numel[n] = h.numel; T.group[n] = gi; T.chunk0[n] = chunks;
            chunks += (int32_t)ceil_div64(h.numel, OPTIM_CHUNK);
            ++n;
        }
        G.chunk_hi[gi] = chunks;
    }
    T.chunk0[n] = chunks;
    T.n = n;
    DeviceGuard guard(device);
    hipStream_t st = (hipStream_t)stream;
    char* ws = reinterpret_cast<char*>(ws_dev);
    const OptimWs L(chunks);
    OptimScalars* scal = reinterpret_cast<OptimScalars*>(ws);
    double* partial = reinterpret_cast<double*>(ws + L.partial);
    int32_t* flag = reinterpret_cast<int32_t*>(ws + L.flag);
    if (chunks > 0) {
        hipLaunchKernelGGL(k_optim_sumsq, dim3((unsigned)chunks), dim3(OPTIM_THREADS), 0, st, T, (const float*)state->scale, partial,
                           flag);
        RADAD_HIP_CHECK(hipGetLastError());
    }
    OptimFinishParams fp{G, state->scale, state->growth_tracker, state->steps, state->grad_norm, state->found_inf, growth, backoff,
                         growth_interval, partial, flag, scal};
    hipLaunchKernelGGL(k_optim_finish, dim3(1), dim3(OPTIM_FINISH_THREADS), 0, st, fp);
    RADAD_HIP_CHECK(hipGetLastError());
    if (chunks > 0) {
        hipLaunchKernelGGL(k_adam_clip, dim3((unsigned)chunks), dim3(OPTIM_THREADS), 0, st, T, G, (const OptimScalars*)scal);
        RADAD_HIP_CHECK(hipGetLastError());
    }
    return RADAD_OK;
}

}  // extern "C"
