// logmel_h.inc -- the log-mel front-end on the f16 matrix pipe (included by embed.hip inside its anonymous namespace).
//
// k_logmel (above) runs the folded DFT on v_mfma_f32_32x32x2_f32, 1/16 of the f16 MFMA rate.  Here every fp32 product
// is taken in split form instead (DESIGN 4.0): x = (hi + lo) 2^-e with hi, lo in f16, and
//     C.x ~= C_hi.x_hi + C_hi.x_lo + C_lo.x_hi          (fp32 accumulate, exact products; dropped term < 2^-22 |C||x|)
// on v_mfma_f32_32x32x16_f16: 16 taps per instruction at half the cycles of a 2-tap fp32 MFMA.  At that rate the
// fold (x[n] +- x[400-n]) would cost more VALU time than it saves matrix time, so the DFT runs unfolded (K = 400 =
// 25 steps of 16 taps) on the segment stored ONCE in LDS as two f16 planes (hi, lo: 4 bytes per sample, as before):
// the B operand of a step is 8 consecutive samples of the lane's frame = one aligned ds_read_b128 per plane, no VALU.
// The A operand comes from ONE stream in global memory (840 KB, L2-resident, fragment order): per bin tile 25 basis groups
// [cos_hi, cos_lo, sin_hi, sin_lo], then the bin tile's mel filter-bank groups, then padding up to a round of the queue --
// read straight into a 5-step register queue (fixed registers, hand-counted waits: see the kernel); NO barrier and no LDS ring
// in the main loop.
// TWO workgroups per segment (round 2; round 1: one), each with 4 waves (one frame tile of 32 frames per wave) and its own
// LDS planes of only the samples its frames touch: workgroup b takes frames [0, F0), workgroup b + 8 (same XCD: the second
// reader of the segment's samples finds them in that L2) frames [F0, nf) (F0 = 96 of 200: 71 KB of planes each instead of
// 137 KB for the whole segment).  Two workgroups are resident per CU and every SIMD hosts two waves.  Both read the WHOLE
// segment for the statistics (mean / variance / max are the segment's) and keep only their part; the segment max is combined
// by the atomic the kernel already used.  Scales are powers of two (segment: max|x| -> [2^10, 2^11), basis: 2^11): un-scaling
// is exact.  The DFT loop runs at the matrix pipe's roof for the clock the chip sustains; the kernel's other third is its staging
// phase and its stores, which barely overlap with it: measurements and the variants tried (de-phasing, mirrored bins) in DESIGN 4.2.
constexpr int LH_WAVES = 4;
constexpr int LH_THREADS = LH_WAVES * 64;
constexpr int LH_STEPS = N_FFT / 16;             // 25
constexpr int LH_Q = 5;                          // basis steps in flight per wave
constexpr int LH_GPB = LH_STEPS + LH_Q;           // fragment groups per bin tile in the stream: 25 DFT steps, NMT mel tiles, padding
constexpr int LH_NG = NBT * LH_GPB;              // 210 groups of 4 fragments
static_assert(NMT <= LH_Q && LH_STEPS % LH_Q == 0, "the mel tiles of a bin tile ride in one round of the queue");
constexpr int LH_FRAME_STRIDE = FFT_HOP + 8;     // halfs between frame starts in LDS: +8 per 160 keeps b128 reads conflict-free
constexpr int LH_SIG_HALFS = 34192;              // plane for a whole segment: p(160 * 201 + 399) + 8, rounded to 16 (upper bound)
constexpr int LH_FREE_VGPRS = 176;               // registers the compiler may allocate; v[176:255] are the basis queue's (see the kernel)
constexpr int LH_TILES = 1;                      // 32-frame tiles per wave
constexpr int LH_WG_FRAMES = 32 * LH_TILES * LH_WAVES;   // frames one workgroup can take
constexpr float LH_BASIS_SCALE = 2048.f;
constexpr int LH_FB_SHIFT = 16;                 // mel filter weights (<= ~0.03) are split after scaling by 2^16

__device__ __forceinline__ int lh_pos(int c) { return c + 8 * (c / FFT_HOP); }

// halfs per LDS plane for a workgroup that owns `frames` frames: every sample position its frames touch, with the +8 per 160 stride
constexpr int lh_plane_halfs(int frames) {
    const int c = FFT_HOP * (frames - 1) + N_FFT;              // positions [0, c)
    return ((c + 8 * (c / FFT_HOP) + 8) + 15) / 16 * 16;
}
constexpr size_t logmel_h_lds_bytes(int frames) { return sizeof(_Float16) * 2 * lh_plane_halfs(frames) + sizeof(float) * 16; }
// frames of the first workgroup of a segment: everything when one workgroup suffices, else the multiple of 32 nearest below half
inline int lh_split_f0(int nf) { return nf <= LH_WG_FRAMES ? nf : 32 * (nf / 64); }

__device__ __forceinline__ float block_max4(float v, float* scratch) {   // LH_WAVES waves
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = scratch[0];
    for (int w = 1; w < LH_WAVES; ++w) t = fmaxf(t, scratch[w]);
    return t;
}

// CLIP = false: one (segment, half) per workgroup, as described above (k_logmel_h).
// CLIP = true (k_logmel_h_clip, round 3): the frames of OVERLAPPING segments are transformed once.  With the segment hop a multiple
// of the frame hop, frame f of segment s and frame f - H of segment s + 1 window the SAME samples of the clip (H = segment hop in
// frames); the segments differ only in their normalisation, which is affine -- x^ = (x - m_s) / sd_s -- and passes through the DFT:
//     X^_s[k] = (X'[k] + (c - m_s) W[k]) / sd_s,      X' = DFT of the windowed (x - c),  W = DFT of the window itself = (200, -100, 0, ..)
// for ANY pivot c.  Bin 0 has no weight in the Slaney filter bank (its first filter starts at 0 Hz), so the power spectrum of segment s
// is that of x - c scaled by 1 / sd_s^2 except in bin 1, which reaches mel bands 0 and 1 only.  Bin 1 therefore stays OUT of the
// shared sums mel' and every owner adds its own:
//     mel_s[m] = (mel'[m] + fb[1][m] ((Re X'[1] + d)^2 + Im X'[1]^2)) / sd_s^2,   d = -100 (c - m_s)
// and log10 of it is log10 mel' - 2 log10 sd_s for the other 78 bands.  (The expanded form mel' + fb[1][m] (2 d Re X'[1] + d^2) with
// bin 1 inside mel' is the same number on paper and was the first form here: three large terms that cancel when d is large against
// what the frame holds in bin 1 -- a loud passage before a quiet one, a DC step inside a clip, digital silence after sound: bands 0-1
// were off by 1e-3 .. 1 in final units, tests/test_gpu_logmel_designed.py.)  c is the mean of the segment the chunk starts in (d = 0
// for that owner; for its neighbours d is the difference of two overlapping segments' means -- a DC offset cancels).  What is
// NOT shared: a segment's frames 0, 1 and T - 1, whose windows reach past the segment and see its reflection.  So the work list is
//     per clip:    its INTERIOR clip frames j in [2, (S - 1) H + T - 2], in chunks of LH_CLIP_FRAMES = 104 consecutive frames (one workgroup
//                  each: the planes hold the 16 880 samples the chunk touches), every frame written to each segment s that owns it
//                  (2 <= j - s H <= T - 2) with that segment's scale and correction;
//                  plus the clip's 3 S EDGE frames in the clip's last, partly filled chunk(s) (clip_chunking below): every one staged as
//                  its own reflected 400-sample window of x - c behind the chunk's samples and written to its one owner like any other
//                  frame (the affine argument does not care which samples a window holds).
// k_seg_stats supplies mean and 1 / sd of every segment.  At the benchmark's shape (T = 200, H = 100, 3 segments per clip) a clip is
// 3 chunks of 104 frames + one of 85 + 9 edge frames (397 interior frames in all) instead of the 600 frames of three segments; segment samples are read once
// by k_seg_stats and once here instead of twice here.
constexpr int LH_CLIP_FRAMES = 104;              // interior frames of a full chunk: what the planes of two workgroups per CU hold
constexpr int LH_EDGE_STRIDE = 424;              // halfs between edge windows in LDS (>= 416 = lh_pos(399) + 1; same bank residue as 168)
constexpr int LH_EDGE_CHUNK = 32;                // edge frames of an edge-only chunk: one tile
constexpr int LH_CLIP_PLANE_HALFS = 20272;       // halfs per LDS plane of a chunk workgroup: two workgroups per CU
constexpr size_t logmel_h_clip_lds_bytes() { return sizeof(_Float16) * 2 * LH_CLIP_PLANE_HALFS + sizeof(float) * 16; }
static_assert(2 * logmel_h_clip_lds_bytes() <= 160 * 1024, "two chunk workgroups per CU");
static_assert(lh_plane_halfs(LH_CLIP_FRAMES) <= LH_CLIP_PLANE_HALFS && LH_EDGE_CHUNK * LH_EDGE_STRIDE <= LH_CLIP_PLANE_HALFS, "planes fit");

// How a clip of S segments (T frames each, hop H frames) is cut into chunks: its ni = (S - 1) H + T - 3 interior frames in FULL chunks of
// LH_CLIP_FRAMES = 104 (no edge frames), then ONE tail chunk with the remaining r < 104 interior frames and as many of the clip's 3 S
// edge frames as its lanes (128) and its planes hold, then edge-only chunks of 32.  (Balanced chunks leave a wave of every workgroup with a few live lanes
// of 32, and the kernel's time follows the number of wave tiles: hence full chunks first, one partly filled chunk per clip.)
struct ClipChunks { int n_full, r, e_tail, n_edge_chunks; };
__host__ __device__ inline ClipChunks clip_chunking(int S, int T, int H) {
    ClipChunks c{0, 0, 0, 0};
    if (S <= 0) return c;
    const int ni = (S - 1) * H + T - 3, E = 3 * S;
    c.n_full = ni / LH_CLIP_FRAMES;
    c.r = ni - c.n_full * LH_CLIP_FRAMES;
    const int planes_r = c.r > 0 ? lh_plane_halfs(c.r) : 0;
    const int fit = (LH_CLIP_PLANE_HALFS - planes_r) / LH_EDGE_STRIDE;
    c.e_tail = E < fit ? E : fit;
    if (c.e_tail > 128 - c.r) c.e_tail = 128 - c.r;
    c.n_edge_chunks = (E - c.e_tail + LH_EDGE_CHUNK - 1) / LH_EDGE_CHUNK;
    return c;
}
__host__ __device__ inline int clip_chunk_count(int S, int T, int H) {
    const ClipChunks c = clip_chunking(S, T, H);
    return S <= 0 ? 0 : c.n_full + 1 + c.n_edge_chunks;
}
constexpr int LH_MAX_OWNERS = 4;                 // segments that can share one interior frame: floor((T - 4) / H) + 1

template <bool CLIP>
__device__ __forceinline__ void logmel_h_body(const LogmelParams& p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    _Float16* shi = reinterpret_cast<_Float16*>(smem);           // [p.plane_halfs]
    _Float16* slo = shi + p.plane_halfs;                         // [p.plane_halfs]
    float* scratch = reinterpret_cast<float*>(slo + p.plane_halfs);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31;
    const int lh = lane >> 5;
    int nfr, f0 = 0, s = 0;
    float unscale;
    // CLIP: what the epilogue needs to know about this workgroup
    int clip_seg0 = 0, clip_S = 0, j0 = 0, nfr_int = 0, e_first = 0, edge_off = 0;
    float pivot = 0.f;
    if constexpr (CLIP) {
        const int T = p.nf, H = p.seg_hop_frames;
        // ---- a chunk: interior frames [j0, j0 + nfr_int) of clip b, then its share of the clip's edge frames --------------------
        const int w = (int)blockIdx.x;
        const int n_chunks = p.n_seg_dev ? p.n_seg_dev[2] : p.n_chunks;
        if (w >= n_chunks) return;
        const ChunkRec rec = p.chunk_rec[w];
        const int cidx = rec.cidx;
        clip_seg0 = rec.seg0;
        clip_S = rec.n_seg;
        const ClipChunks cc = clip_chunking(clip_S, T, H);
        int n_edge;
        j0 = 2 + cidx * LH_CLIP_FRAMES;
        if (cidx < cc.n_full) { nfr_int = LH_CLIP_FRAMES; e_first = 0; n_edge = 0; }
        else if (cidx == cc.n_full) { nfr_int = cc.r; e_first = 0; n_edge = cc.e_tail; }
        else {
            nfr_int = 0;
            e_first = cc.e_tail + (cidx - cc.n_full - 1) * LH_EDGE_CHUNK;
            n_edge = max(0, min(LH_EDGE_CHUNK, 3 * clip_S - e_first));
        }
        const int edge_base = nfr_int > 0 ? lh_plane_halfs(nfr_int) : 0;      // the edge windows follow the chunk's own samples
        edge_off = edge_base;
        nfr = nfr_int + n_edge;
        if (nfr <= 0) return;
        const int64_t beg = rec.beg;
        const int avail = rec.avail;                                // samples of the clip the segments cover
        const int u0 = FFT_HOP * j0 - 200;                          // first clip sample the chunk touches (>= 120)
        const int span = nfr_int > 0 ? FFT_HOP * (nfr_int - 1) + N_FFT : 0;       // samples [u0, u0 + span)
        if (p.normalize) pivot = p.seg_stats[4 * (clip_seg0 + min(clip_S - 1, j0 / H))];
        const float* clip = p.wave + beg;
        const float* src = clip + u0;
        constexpr int UNR = ((FFT_HOP * (LH_CLIP_FRAMES - 1) + N_FFT) / 4 + LH_THREADS - 1) / LH_THREADS;      // 17
        const int nv = span >> 2;
        f32x4 raw[UNR];
        float amax = 0.f;
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int i4 = u * LH_THREADS + tid;
            const int i = u0 + i4 * 4;
            f32x4 t = {0.f, 0.f, 0.f, 0.f};
            if (i4 < nv) {
                if (RADAD_DBG(p.debug, 2)) t = f32x4{1.f, -1.f, 0.5f, 0.25f};
                else if (i + 4 <= avail) t = *reinterpret_cast<const f32x4_a4*>(src + i4 * 4);
                else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) t[e] = i + e < avail ? src[i4 * 4 + e] : 0.f;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) { t[e] -= pivot; amax = fmaxf(amax, fabsf(t[e])); }
            }
            raw[u] = t;
        }
        // edge windows: position q of edge frame k is segment sample |160 f - 200 + q| reflected at the segment's ends (read twice:
        // once for the chunk's scale, once to write -- a few thousand L2 hits)
        const int L = p.seg_len;
        auto edge_sample = [&](int k, int q) {
            const int ee = e_first + k;
            const int sg = ee / 3, kind = ee - 3 * sg;
            int us = FFT_HOP * (kind < 2 ? kind : T - 1) - 200 + q;
            if (us < 0) us = -us;
            if (us >= L) us = 2 * (L - 1) - us;
            const int uc = sg * p.seg_hop + us;                   // the same sample in clip coordinates
            return (uc < avail ? clip[uc] : 0.f) - pivot;
        };
        for (int i = tid; i < n_edge * N_FFT; i += LH_THREADS) {
            const int k = i / N_FFT;
            amax = fmaxf(amax, fabsf(edge_sample(k, i - k * N_FFT)));
        }
        amax = block_max4(amax, scratch);
        // While this workgroup's matrix phase runs HBM idles, and when it ends the next workgroup on this CU starts with a burst of
        // sample loads that nothing hides (0.07 of 0.60 ms).  So the samples of the chunk that will run here next -- about
        // 2 x CUs further down the list -- are touched now: up to three discarded loads per thread (one per 128-byte line) pull them into L2 /
        // the Infinity Cache.  The destination is a register of the basis queue, idle until the queue's first fill; loads return in
        // order, so the fills that follow land after these.
        if (p.prefetch_dist > 0 && w + p.prefetch_dist < n_chunks) {
            const ChunkRec nx = p.chunk_rec[w + p.prefetch_dist];
            const ClipChunks nc = clip_chunking(nx.n_seg, T, H);
            const int nint = nx.cidx < nc.n_full ? LH_CLIP_FRAMES : (nx.cidx == nc.n_full ? nc.r : 0);
            if (nint > 0) {
                const int nu0 = FFT_HOP * (2 + nx.cidx * LH_CLIP_FRAMES) - 200;
                const int nend = min(nu0 + FFT_HOP * (nint - 1) + N_FFT, nx.avail);       // only samples that exist
                const float* nsrc = p.wave + nx.beg;
#pragma unroll
                for (int r2 = 0; r2 < 3; ++r2) {
                    const int i = nu0 + (r2 * LH_THREADS + tid) * 32;        // one load per 128-byte line
                    if (i < nend) asm volatile("global_load_dword v255, %0, off" : : "v"(nsrc + i) : "memory", "v255");
                }
            }
        }
        int ex = 0;
        if (amax > 0.f && amax < INFINITY) {
            int fe;
            (void)frexpf(amax, &fe);
            ex = max(-100, min(100, 11 - fe));
        }
        const float up = ldexpf(1.0f, ex);
        unscale = ldexpf(1.0f, -ex - 11);
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int i4 = u * LH_THREADS + tid;
            if (i4 < nv) {
                f16x4 hi, lo;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float sc = raw[u][e] * up;
                    hi[e] = (_Float16)sc;
                    lo[e] = (_Float16)(sc - (float)hi[e]);
                }
                const int pos = lh_pos(i4 * 4);
                *reinterpret_cast<f16x4*>(shi + pos) = hi;
                *reinterpret_cast<f16x4*>(slo + pos) = lo;
            }
        }
        for (int i = tid; i < n_edge * N_FFT; i += LH_THREADS) {
            const int k = i / N_FFT, q = i - k * N_FFT;
            const float sc = edge_sample(k, q) * up;
            const _Float16 hi = (_Float16)sc;
            const int pos = edge_base + LH_EDGE_STRIDE * k + lh_pos(q);
            shi[pos] = hi;
            slo[pos] = (_Float16)(sc - (float)hi);
        }
        __syncthreads();
    }
    if constexpr (!CLIP) {
    // workgroups b and b + 8 are the two halves of one segment: consecutive workgroups go to consecutive XCDs, so the pair shares
    // an XCD -- and its L2, where the second reader of the segment's samples finds them (grid = 16 ceil(n_seg / 8))
    s = (int)(blockIdx.x >> 4) * 8 + (int)(blockIdx.x & 7);
    const int half = (blockIdx.x >> 3) & 1;
    if (s >= p.n_seg) return;
    if (p.n_seg_dev && s >= *p.n_seg_dev) return;       // device-built plan: the grid is an upper bound on the segments
    // this workgroup's frames [f0, f0 + nfr) and the sample positions they touch, [c0, c_end) in padded coordinates (c = sample + 200)
    f0 = half ? p.split_f0 : 0;
    nfr = half ? p.nf - p.split_f0 : min(p.nf, p.split_f0);
    if (nfr <= 0) return;
    const int c0 = FFT_HOP * f0;
    const int c_end = FFT_HOP * (f0 + nfr - 1) + N_FFT;
    const int L = p.seg_len;
    const float* src = p.wave + p.seg_start[s];
    const int valid = p.seg_valid[s];

    // ---- stage the segment: HBM -> registers -> (stats, normalise, scale) -> two f16 planes in LDS ---------------------
    constexpr int UNR = (MAX_SEG_LEN / 4 + LH_THREADS - 1) / LH_THREADS;      // 32
    const int nv = L >> 2;
    f32x4 raw[UNR];
    {
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int i4 = u * LH_THREADS + tid;
            const int i = i4 * 4;
            f32x4 t = {0.f, 0.f, 0.f, 0.f};
            if (i4 < nv && !RADAD_DBG(p.debug, 2)) {
                if (i + 4 <= valid) t = *reinterpret_cast<const f32x4_a4*>(src + i);     // (dword alignment is all a 128-bit load needs)
                else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) t[e] = i + e < valid ? src[i + e] : 0.f;
                }
            }
            raw[u] = t;
        }
    }
    float mean = 0.f, inv = 1.f;
    if (p.normalize) {
        float lsum = 0.f;
#pragma unroll
        for (int u = 0; u < UNR; ++u) lsum += (raw[u][0] + raw[u][1]) + (raw[u][2] + raw[u][3]);   // lanes past nv hold zeros
        mean = block_sum(lsum, scratch, LH_WAVES) / (float)L;
        float lsq = 0.f;
#pragma unroll
        for (int u = 0; u < UNR; ++u)
            if (u * LH_THREADS + tid < nv) {
#pragma unroll
                for (int e = 0; e < 4; ++e) { const float d = raw[u][e] - mean; lsq += d * d; }
            }
        const float var = block_sum(lsq, scratch, LH_WAVES) / (float)L;
        inv = 1.0f / sqrtf(var + 1e-7f);
    }
    float amax = 0.f;
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
        if (u * LH_THREADS + tid < nv) {
            if (p.normalize) {
#pragma unroll
                for (int e = 0; e < 4; ++e) raw[u][e] = (raw[u][e] - mean) * inv;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) amax = fmaxf(amax, fabsf(raw[u][e]));
        }
    }
    amax = block_max4(amax, scratch);
    int ex = 0;
    if (amax > 0.f && amax < INFINITY) {
        int fe;
        (void)frexpf(amax, &fe);                 // amax = m 2^fe, m in [0.5, 1)
        ex = max(-100, min(100, 11 - fe));       // amax 2^ex in [2^10, 2^11)
    }
    const float up = ldexpf(1.0f, ex);
    unscale = ldexpf(1.0f, -ex - 11);                // undoes the segment scale and the basis scale 2^11
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
        const int i4 = u * LH_THREADS + tid;
        if (i4 < nv) {
            const f32x4 v = raw[u];
            f16x4 hi, lo;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float sc = v[e] * up;
                hi[e] = (_Float16)sc;
                lo[e] = (_Float16)(sc - (float)hi[e]);
            }
            const int c = i4 * 4 + 200;               // 4 | 200, 4 | 160, 4 | c0, 4 | c_end: the four samples share one 160-block
            if (c >= c0 && c < c_end) {               // and lie inside or outside this workgroup's range together
                const int pos = lh_pos(c - c0);
                *reinterpret_cast<f16x4*>(shi + pos) = hi;
                *reinterpret_cast<f16x4*>(slo + pos) = lo;
            }
            if (p.norm_out && half == 0) *reinterpret_cast<f32x4*>(p.norm_out + (int64_t)s * L + i4 * 4) = v;
        }
    }
    __syncthreads();
    // left border (only the workgroup that starts at frame 0 has it): u = c-200 < 0 reflects to i = 200-c  (c in [0,200))
    if (c0 == 0) {
        for (int c = tid; c < 200; c += LH_THREADS) {
            shi[lh_pos(c)] = shi[lh_pos(400 - c)];
            slo[lh_pos(c)] = slo[lh_pos(400 - c)];
        }
    }
    // right border: u >= L, as far as this workgroup's frames reach.  Self mode (P == L): reflect i = 2(L-1)-u (the source
    // lies at most 200 samples left of L, inside this workgroup's range).  Padded mode: zeros.
    for (int c = max(L + 200, c0) + tid; c < c_end; c += LH_THREADS) {
        const int u = c - 200;
        _Float16 vh = (_Float16)0.f, vl = (_Float16)0.f;
        if (p.padded == L) {
            const int i = 2 * (L - 1) - u;
            vh = shi[lh_pos(i + 200 - c0)];
            vl = slo[lh_pos(i + 200 - c0)];
        }
        shi[lh_pos(c - c0)] = vh;
        slo[lh_pos(c - c0)] = vl;
    }
    __syncthreads();
    }   // !CLIP

    // ---- DFT + mel: wave w owns the workgroup's frame tile w; frames are local to the workgroup from here on ----------------
    // which frame tile this wave takes: rotated by the workgroup index, so that the idle waves of partly filled workgroups (a 104-frame
    // chunk has three full tiles and one of 8 frames) are not always the same wave slot
    const int wtile = CLIP ? ((wave + (int)blockIdx.x) & (LH_WAVES - 1)) : wave;
    if (32 * wtile >= nfr) return;                     // wave-uniform (no barrier below this line)
    f32x16 zacc[NMT];
#pragma unroll
    for (int m = 0; m < NMT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) zacc[m][r] = 0.f;

    // ---- the basis queue: LH_Q slots of four 128-bit fragments in FIXED registers v[176:255] --------------------------------
    // hipcc's waitcnt pass loses count of loads that are in flight across a loop back edge and falls back to vmcnt(0), which
    // drains the queue every iteration (measured in round 1: 51 % MFMA busy).  So the queue's loads and waits are counted by
    // hand in inline asm -- and so are the registers: the kernel is compiled with amdgpu_num_vgpr(176), which keeps the
    // register allocator out of v176..v255 altogether, and every instruction that touches a slot (the load that fills it,
    // the s_waitcnt that awaits it, the MFMAs that read it) names those registers literally.  (Round 1 and the first round-2
    // build kept the slots in C++ variables behind "=v"/"+v" asm operands.  That holds only while the allocator happens to
    // keep each slot in one register for the whole loop nest: when it places a refill's result elsewhere and copies it back
    // -- it did, once the loop nest changed -- the copy reads a register whose load has not landed, and the compiler then
    // reuses the source register while the load is still due to write into it: garbage powers in one build, a GPU memory
    // fault in another.  tools/check_asm_queue.py lints the generated code for exactly that.)
    // Slot d is refilled right after its last use, so when its turn comes again exactly the 4 (LH_Q - 1) = 16 loads of the
    // other slots are younger: s_waitcnt vmcnt(16).  Vector-memory operations retire in order.
#define LH_QCLOB "v176", "v177", "v178", "v179", "v180", "v181", "v182", "v183", "v184", "v185", "v186", "v187", "v188", "v189", "v190", "v191", "v192", "v193", "v194", "v195", "v196", "v197", "v198", "v199", "v200", "v201", "v202", "v203", "v204", "v205", "v206", "v207", "v208", "v209", "v210", "v211", "v212", "v213", "v214", "v215", "v216", "v217", "v218", "v219", "v220", "v221", "v222", "v223", "v224", "v225", "v226", "v227", "v228", "v229", "v230", "v231", "v232", "v233", "v234", "v235", "v236", "v237", "v238", "v239", "v240", "v241", "v242", "v243", "v244", "v245", "v246", "v247", "v248", "v249", "v250", "v251", "v252", "v253", "v254", "v255"
#define LH_FILL_(Q0, Q1, Q2, Q3, ptr)                                                                                   \
    asm volatile("global_load_dwordx4 " Q0 ", %0, off\n global_load_dwordx4 " Q1 ", %0, off offset:1024\n"             \
                 "global_load_dwordx4 " Q2 ", %0, off offset:2048\n global_load_dwordx4 " Q3 ", %0, off offset:3072"    \
                 : : "v"(ptr) : "memory", LH_QCLOB)
    // one DFT step: re += cos_lo x_hi + cos_hi x_lo + cos_hi x_hi, im likewise with sin (slot = [cos_hi, cos_lo, sin_hi, sin_lo])
#define LH_DFT_STEP_(Q0, Q1, Q2, Q3, re_, im_, xh_, xl_, ptr)                                                            \
    asm volatile("s_waitcnt vmcnt(16)\n"                                                                               \
                 "v_mfma_f32_32x32x16_f16 %0, " Q1 ", %2, %0\n v_mfma_f32_32x32x16_f16 %1, " Q3 ", %2, %1\n"             \
                 "v_mfma_f32_32x32x16_f16 %0, " Q0 ", %3, %0\n v_mfma_f32_32x32x16_f16 %1, " Q2 ", %3, %1\n"             \
                 "v_mfma_f32_32x32x16_f16 %0, " Q0 ", %2, %0\n v_mfma_f32_32x32x16_f16 %1, " Q2 ", %2, %1\n"             \
                 "global_load_dwordx4 " Q0 ", %4, off\n global_load_dwordx4 " Q1 ", %4, off offset:1024\n"              \
                 "global_load_dwordx4 " Q2 ", %4, off offset:2048\n global_load_dwordx4 " Q3 ", %4, off offset:3072"     \
                 : "+v"(re_), "+v"(im_) : "v"(xh_), "v"(xl_), "v"(ptr) : "memory", LH_QCLOB)
    // one mel tile: t = fb_lo p_hi + fb_hi p_lo + fb_hi p_hi over both k halves (slot = [half 0 hi, lo, half 1 hi, lo]); the
    // s_nops are the wait states a VALU read of an MFMA result needs (the compiler cannot see the MFMAs in here)
#define LH_MEL_STEP_(Q0, Q1, Q2, Q3, t_, ph0, pl0, ph1, pl1, ptr)                                                        \
    asm volatile("s_waitcnt vmcnt(16)\n"                                                                               \
                 "v_mfma_f32_32x32x16_f16 %0, " Q1 ", %1, 0\n v_mfma_f32_32x32x16_f16 %0, " Q0 ", %2, %0\n"             \
                 "v_mfma_f32_32x32x16_f16 %0, " Q0 ", %1, %0\n v_mfma_f32_32x32x16_f16 %0, " Q3 ", %3, %0\n"            \
                 "v_mfma_f32_32x32x16_f16 %0, " Q2 ", %4, %0\n v_mfma_f32_32x32x16_f16 %0, " Q2 ", %3, %0\n"            \
                 "global_load_dwordx4 " Q0 ", %5, off\n global_load_dwordx4 " Q1 ", %5, off offset:1024\n"              \
                 "global_load_dwordx4 " Q2 ", %5, off offset:2048\n global_load_dwordx4 " Q3 ", %5, off offset:3072\n"  \
                 "s_nop 15\n s_nop 3"                                                                                   \
                 : "=&v"(t_) : "v"(ph0), "v"(pl0), "v"(ph1), "v"(pl1), "v"(ptr) : "memory", LH_QCLOB)
    // a slot whose content is not used (an all-zero mel tile, padding): awaited and refilled all the same, to keep the count
#define LH_SKIP_STEP_(Q0, Q1, Q2, Q3, ptr)                                                                              \
    asm volatile("s_waitcnt vmcnt(16)\n"                                                                               \
                 "global_load_dwordx4 " Q0 ", %0, off\n global_load_dwordx4 " Q1 ", %0, off offset:1024\n"              \
                 "global_load_dwordx4 " Q2 ", %0, off offset:2048\n global_load_dwordx4 " Q3 ", %0, off offset:3072"     \
                 : : "v"(ptr) : "memory", LH_QCLOB)
    // (a slot macro expands to four arguments: the wrappers below expand it before the real macro collects its arguments)
#define LH_FILL(...) LH_FILL_(__VA_ARGS__)
#define LH_DFT_STEP(...) LH_DFT_STEP_(__VA_ARGS__)
#define LH_MEL_STEP(...) LH_MEL_STEP_(__VA_ARGS__)
#define LH_SKIP_STEP(...) LH_SKIP_STEP_(__VA_ARGS__)
#define LH_SLOT0 "v[176:179]", "v[180:183]", "v[184:187]", "v[188:191]"
#define LH_SLOT1 "v[192:195]", "v[196:199]", "v[200:203]", "v[204:207]"
#define LH_SLOT2 "v[208:211]", "v[212:215]", "v[216:219]", "v[220:223]"
#define LH_SLOT3 "v[224:227]", "v[228:231]", "v[232:235]", "v[236:239]"
#define LH_SLOT4 "v[240:243]", "v[244:247]", "v[248:251]", "v[252:255]"
    static_assert(LH_Q == 5 && LH_TILES == 1, "the slot macros below are written out for 5 slots and one frame tile per wave");
    const f16x8* bas = reinterpret_cast<const f16x8*>(p.basis_h) + lane;     // fragment w of group g at bas[(g*4 + w) * 64]
    auto group = [&](int g) { return bas + (size_t)min(g, LH_NG - 1) * 4 * 64; };   // past the end: the last group again (never used)
    LH_FILL(LH_SLOT0, group(0));
    LH_FILL(LH_SLOT1, group(1));
    LH_FILL(LH_SLOT2, group(2));
    LH_FILL(LH_SLOT3, group(3));
    LH_FILL(LH_SLOT4, group(4));

    // B operands (8 samples of the lane's frame per plane) are fetched one step ahead, into a second pair of registers, in
    // front of the step's MFMAs: a whole step (192 matrix cycles) covers the LDS latency
    const int tf = min(32 * wtile + l31, nfr - 1);                   // clamped: extra lanes recompute the last frame
    // (CLIP: the lane's frame is an interior frame at the regular stride, or an edge frame in its own window behind the planes)
    const int xoff = (CLIP && tf >= nfr_int) ? edge_off + LH_EDGE_STRIDE * (tf - nfr_int) : LH_FRAME_STRIDE * tf;
    const _Float16* xb_hi = shi + xoff + 8 * lh;
    const _Float16* xb_lo = slo + xoff + 8 * lh;
    float x1re = 0.f, x1im = 0.f;  // CLIP: X'[1] of the lane's frame (lanes 0-31 hold bin 1 in register 1 of bin tile 0)
    f16x8 xh = *reinterpret_cast<const f16x8*>(xb_hi);
    f16x8 xl = *reinterpret_cast<const f16x8*>(xb_lo);
#define LH_STEP(SLOT, d)                                                                                                \
    {                                                                                                                   \
        const int step = sg * LH_Q + d;                                                                                 \
        const int nstep = step + 1 == LH_STEPS ? 0 : step + 1;      /* the next bin tile starts over at tap 0 */        \
        const int noff = 16 * nstep + 8 * (nstep / 10);             /* lh_pos of tap 16 nstep relative to the frame start */ \
        const f16x8 xh_n = *reinterpret_cast<const f16x8*>(xb_hi + noff);                                               \
        const f16x8 xl_n = *reinterpret_cast<const f16x8*>(xb_lo + noff);                                               \
        const f16x8* nxt = group(bt * LH_GPB + step + LH_Q);                                                            \
        LH_DFT_STEP(SLOT, re, im, xh, xl, nxt);                                                                         \
        xh = xh_n;                                                                                                      \
        xl = xl_n;                                                                                                      \
    }
#pragma unroll 1
    for (int bt = 0; bt < (RADAD_DBG(p.debug, 1) ? 0 : NBT); ++bt) {
        f32x16 re, im;
#pragma unroll
        for (int r = 0; r < 16; ++r) { re[r] = 0.f; im[r] = 0.f; }
#pragma unroll 1
        for (int sg = 0; sg < LH_STEPS / LH_Q; ++sg) {
            LH_STEP(LH_SLOT0, 0)
            LH_STEP(LH_SLOT1, 1)
            LH_STEP(LH_SLOT2, 2)
            LH_STEP(LH_SLOT3, 3)
            LH_STEP(LH_SLOT4, 4)
        }
        asm volatile("s_nop 15\n s_nop 3" : "+v"(re), "+v"(im));      // MFMA result -> VALU read wait states (see LH_MEL_STEP)
        if constexpr (CLIP) { if (bt == 0) { x1re = re[1] * unscale; x1im = im[1] * unscale; } }
        // |X|^2 -> mel, also on the f16 pipe: the lane's 16 power values (bins (r&3) + 8(r>>2) + 4lh) are the B operand of
        // two 16-deep MFMAs whose k order is permuted to match (k' = 8lh + j  <->  register 8h + j); the filter bank comes
        // pre-split in that order.  Powers span many decades, so each FRAME (lane pair l, l+32) gets its own power-of-two
        // scale; the scaled partial result is folded into the fp32 mel accumulators by one fma per element.
        f16x8 ph[2], pl[2];
        float down2;
        {
            float pwv[16];
            float m = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float a = re[r] * unscale, b = im[r] * unscale;
                pwv[r] = a * a + b * b;
                if (CLIP && r == 1) pwv[r] = (bt == 0 && lh == 0) ? 0.f : pwv[r];    // bin 1 stays out of the shared sums (see above)
                m = fmaxf(m, pwv[r]);
            }
            m = fmaxf(m, __shfl_xor(m, 32));
            int e = 0;
            if (m > 0.f && m < INFINITY) {
                int fe;
                (void)frexpf(m, &fe);
                e = max(-100, min(100, 14 - fe));        // m 2^e in [2^13, 2^14)
            }
            const float up2 = ldexpf(1.0f, e);
            down2 = ldexpf(1.0f, -e - LH_FB_SHIFT);
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float sc = pwv[8 * h + j] * up2;
                    ph[h][j] = (_Float16)sc;
                    pl[h][j] = (_Float16)(sc - (float)ph[h][j]);
                }
        }
        // The filter-bank fragments of this bin tile's NMT mel tiles are the next groups of the SAME stream (LH_STEPS ..
        // LH_STEPS + NMT - 1 of the bin tile, then padding up to a full round): they were fetched LH_Q steps ago like any
        // basis step and sit in slots 0 .. NMT-1 (as separate loads they cost 4-5 exposed L2 round trips per bin tile:
        // 0.14 of 0.84 ms).  Every slot of the round is awaited and refilled in order, whether its tile is all zero or not.
#define LH_MEL(SLOT, d)                                                                                                 \
    {                                                                                                                   \
        const f16x8* nxt = group(bt * LH_GPB + LH_STEPS + d + LH_Q);                                                    \
        if (d < NMT && ((p.nzmask >> (bt * NMT + d)) & 1u) && !RADAD_DBG(p.debug, 4)) {      /* wave-uniform */          \
            f32x16 t;                                                                                                   \
            LH_MEL_STEP(SLOT, t, ph[0], pl[0], ph[1], pl[1], nxt);                                                      \
            _Pragma("unroll") for (int r = 0; r < 16; ++r) zacc[d < NMT ? d : 0][r] = fmaf(t[r], down2, zacc[d < NMT ? d : 0][r]); \
        } else {                                                                                                        \
            LH_SKIP_STEP(SLOT, nxt);                                                                                    \
        }                                                                                                               \
    }
        LH_MEL(LH_SLOT0, 0)
        LH_MEL(LH_SLOT1, 1)
        LH_MEL(LH_SLOT2, 2)
        LH_MEL(LH_SLOT3, 3)
        LH_MEL(LH_SLOT4, 4)
    }
    asm volatile("s_waitcnt vmcnt(0)" : : : "memory", LH_QCLOB);     // the queue's trailing (unused) refills
#undef LH_QCLOB
#undef LH_FILL
#undef LH_FILL_
#undef LH_DFT_STEP
#undef LH_DFT_STEP_
#undef LH_MEL_STEP
#undef LH_MEL_STEP_
#undef LH_SKIP_STEP
#undef LH_SKIP_STEP_
#undef LH_STEP
#undef LH_MEL
#undef LH_SLOT0
#undef LH_SLOT1
#undef LH_SLOT2
#undef LH_SLOT3
#undef LH_SLOT4

    // ---- log10, segment max, store [frame][mel] --------------------------------------------------------
    if (RADAD_DBG(p.debug, 8)) return;
    if constexpr (!CLIP) {
    float lmax = -INFINITY;
    {
        const bool fvalid = 32 * wave + l31 < nfr;
        float* orow = p.logmel + ((int64_t)s * p.nf + f0 + tf) * N_MELS;
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int m0 = 32 * mt + 8 * g + 4 * lh;       // registers 4g..4g+3 = mels m0..m0+3
                if (m0 < N_MELS) {
                    f32x4 v;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        v[i] = fmaxf(log10f(zacc[mt][4 * g + i]), -10.f);     // log10(max(mel, 1e-10)), the floor exactly -10 (fmaxf drops the NaN of a rounding-negative sum)
                        if (fvalid) lmax = fmaxf(lmax, v[i]);
                    }
                    if (fvalid) *reinterpret_cast<f32x4*>(orow + m0) = v;
                }
            }
    }
    lmax = wave_max(lmax);
    if (lane == 0 && lmax > -INFINITY) atomic_max_float(p.seg_max + s, lmax);
    } else {
        // every owner of the lane's frame gets the frame's row: log10 mel' + 2 log10(1 / sd_s) (floored at -10 like
        // log10(max(mel, 1e-10))), bands 0 and 1 from the corrected linear value
        const bool fvalid = 32 * wtile + l31 < nfr;
        const int T = p.nf, H = p.seg_hop_frames;
        const bool edge = tf >= nfr_int;
        int s_lo, s_hi, jf = 0, e_kind = 0;             // owners [s_lo, s_hi] (segment indices of the launch), this frame's clip index
        if (edge) {
            const int ee = e_first + (tf - nfr_int);
            s_lo = s_hi = clip_seg0 + ee / 3;
            e_kind = ee - 3 * (ee / 3);
        } else {
            jf = j0 + tf;
            // 2 <= jf - s H <= T - 2
            const int lo = jf - (T - 2);
            s_lo = clip_seg0 + (lo <= 0 ? 0 : (lo + H - 1) / H);
            s_hi = clip_seg0 + min(clip_S - 1, (jf - 2) / H);
        }
        if (!fvalid) s_hi = s_lo - 1;
        // the owners' statistics first, all of them in flight together (behind the stores of an earlier owner the compiler would not
        // hoist them: 1-2 exposed L2 round trips per owner)
        f32x4 st_o[LH_MAX_OWNERS];
#pragma unroll
        for (int o = 0; o < LH_MAX_OWNERS; ++o) {
            st_o[o] = f32x4{0.f, 1.f, 1.f, 0.f};
            if (p.normalize && s_lo + o <= s_hi) st_o[o] = reinterpret_cast<const f32x4*>(p.seg_stats)[s_lo + o];
        }
        const float z0 = zacc[0][0], z1 = zacc[0][1];  // linear mel' of bands 0, 1 without bin 1 (lanes 0-31)
        // log10 mel' once, in place
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) zacc[mt][r] = log10f(zacc[mt][r]);       // (0 -> -inf, floored below; the hardware log alone changes nothing: measured)
        float lmax_o[LH_MAX_OWNERS];
#pragma unroll
        for (int o = 0; o < LH_MAX_OWNERS; ++o) {
            lmax_o[o] = -INFINITY;
            const int sg = s_lo + o;
            if (sg <= s_hi) {
                const int fl = edge ? (e_kind < 2 ? e_kind : T - 1) : jf - (sg - clip_seg0) * H;
                const float g2 = st_o[o][2], lg = st_o[o][3];
                const float d = p.normalize ? -100.f * (pivot - st_o[o][0]) : 0.f;
                float* orow = p.logmel + ((int64_t)sg * T + fl) * N_MELS;
                const float p1 = fmaf(x1re + d, x1re + d, x1im * x1im);    // |X'[1] + d|^2: bin 1 of this owner, before its 1 / sd^2
#pragma unroll
                for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int m0 = 32 * mt + 8 * g + 4 * lh;
                        if (m0 < N_MELS) {
                            f32x4 v;
#pragma unroll
                            for (int i = 0; i < 4; ++i) v[i] = fmaxf(zacc[mt][4 * g + i] + lg, -10.f);
                            if (mt == 0 && g == 0 && lh == 0) {
                                v[0] = fmaxf(log10f(fmaf(p.fb1[0], p1, z0) * g2), -10.f);
                                v[1] = fmaxf(log10f(fmaf(p.fb1[1], p1, z1) * g2), -10.f);
                            }
#pragma unroll
                            for (int i = 0; i < 4; ++i) lmax_o[o] = fmaxf(lmax_o[o], v[i]);
                            if (!RADAD_DBG(p.debug, 16)) *reinterpret_cast<f32x4*>(orow + m0) = v;
                        }
                    }
            }
        }
        // segment maxima: the wave's frames touch a few consecutive segments
        int w_lo = fvalid ? s_lo : 0x7fffffff, w_hi = fvalid ? s_hi : -1;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            w_lo = min(w_lo, __shfl_xor(w_lo, o));
            w_hi = max(w_hi, __shfl_xor(w_hi, o));
        }
        for (int sg = w_lo; sg <= w_hi; ++sg) {
            float m = -INFINITY;
#pragma unroll
            for (int o = 0; o < LH_MAX_OWNERS; ++o)
                if (sg == s_lo + o && sg <= s_hi) m = lmax_o[o];
            m = wave_max(m);
            if (lane == 0 && m > -INFINITY) atomic_max_float(p.seg_max + sg, m);
        }
    }
}

__global__ __launch_bounds__(LH_THREADS, 2) __attribute__((amdgpu_num_vgpr(LH_FREE_VGPRS))) void k_logmel_h(LogmelParams p) {
    logmel_h_body<false>(p);
}
__global__ __launch_bounds__(LH_THREADS, 2) __attribute__((amdgpu_num_vgpr(LH_FREE_VGPRS))) void k_logmel_h_clip(LogmelParams p) {
    logmel_h_body<true>(p);
}

// [S][4]: mean, inv = 1 / sqrt(var + 1e-7), inv^2 and 2 log10(inv) of every segment (zero padded to L), mean and variance as
// k_logmel_h's prologue computes them: two passes from registers.  A segment whose variance is exactly zero -- every sample equals the
// mean: digital silence inside a live clip -- normalises to zeros whatever 1 / sqrt(1e-7) is, and the per-segment kernels give it
// log10(1e-10) in every cell.  The shared transform of x - c cannot: its rounding noise around a pivot taken from a live neighbour,
// times 1 / 1e-7, rises above 1e-10.  Such a segment therefore gets inv^2 = 0 and 2 log10(inv) = -inf: every owner row of it is the floor.
__global__ __launch_bounds__(LH_THREADS) void k_seg_stats(const float* __restrict__ wave, const int64_t* __restrict__ seg_start,
                                                          const int* __restrict__ seg_valid, int L, int n_seg,
                                                          const int* __restrict__ n_seg_dev, float* __restrict__ stats,
                                                          float* __restrict__ seg_max, float seg_max_init) {
    __shared__ float scratch[16];
    const int tid = threadIdx.x;
    // Workgroups are dealt to the 8 XCDs round-robin.  Consecutive segments of a clip overlap (50 %: every sample belongs to two), so
    // three CONSECUTIVE segments go to the SAME XCD -- workgroups i, i + 8, i + 16 of a block of 24 -- and the second reader of a
    // sample finds it in that XCD's L2 instead of fetching it again (FETCH_SIZE was 394 MB for the benchmark's 262 MB batch).
    int s = blockIdx.x;
    {
        const int blk = s / 24, l = s % 24;
        if (blk * 24 + 24 <= n_seg) s = blk * 24 + (l & 7) * 3 + (l >> 3);
    }
    if (s >= n_seg || (n_seg_dev && s >= *n_seg_dev)) return;
    const float* src = wave + seg_start[s];
    const int valid = seg_valid[s];
    constexpr int UNR = (MAX_SEG_LEN / 4 + LH_THREADS - 1) / LH_THREADS;
    const int nv = L >> 2;
    f32x4 raw[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
        const int i4 = u * LH_THREADS + tid;
        const int i = i4 * 4;
        f32x4 t = {0.f, 0.f, 0.f, 0.f};
        if (i4 < nv) {
            if (i + 4 <= valid) t = *reinterpret_cast<const f32x4_a4*>(src + i);
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) t[e] = i + e < valid ? src[i + e] : 0.f;
            }
        }
        raw[u] = t;
    }
    float lsum = 0.f;
#pragma unroll
    for (int u = 0; u < UNR; ++u) lsum += (raw[u][0] + raw[u][1]) + (raw[u][2] + raw[u][3]);
    const float mean = block_sum(lsum, scratch, LH_WAVES) / (float)L;
    float lsq = 0.f;
#pragma unroll
    for (int u = 0; u < UNR; ++u)
        if (u * LH_THREADS + tid < nv) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float dd = raw[u][e] - mean; lsq += dd * dd; }
        }
    const float var = block_sum(lsq, scratch, LH_WAVES) / (float)L;
    if (tid == 0) {
        const float inv = 1.0f / sqrtf(var + 1e-7f);
        const bool flat = var == 0.f;
        reinterpret_cast<f32x4*>(stats)[s] = f32x4{mean, inv, flat ? 0.f : inv * inv, flat ? -INFINITY : 2.f * log10f(inv)};
        seg_max[s] = seg_max_init;                      // the running maximum k_logmel_h_clip raises (saves the fill launch)
    }
}
