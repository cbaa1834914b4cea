// logmel_fft.inc -- the log-mel front-end as a radix FFT on the vector ALU (included by embed.hip inside its anonymous namespace).
//
// The transform the reference calls IS an FFT (feature_extractor.py:94-97 -> transformers' WhisperFeatureExtractor,
// feature_extraction_whisper.py:135-168: hann 400 / hop 160, |X|^2, Slaney mel 201 -> 80, log10).  k_logmel_h / k_logmel_h_clip
// (logmel_h.inc) compute it as a 400 x 402 DFT-as-GEMM on the f16 matrix pipe in split form: ~100 x the arithmetic a radix FFT
// needs.  Here a frame is ONE 200-point complex FFT of the packed real frame, in native fp32:
//
//     z[q] = g[2q] + i g[2q+1],  g = hann . (x - c)           q = 8 m + r:  8 lanes per frame, lane r holds z[8m + r], m = 0..24
//     Y_r[k1] = sum_m W25^(m k1) z[8m + r]                     a 25-point FFT in the lane's registers (5 x 5, two radix-5 passes)
//     Z[k1 + 25 k2] = sum_r W8^(r k2) W200^(r k1) Y_r[k1]      per-lane twiddle, then a radix-8 step ACROSS the 8 lanes: three
//                                                              exchange stages (partner 7 - p, p ^ 2, p ^ 1 -- all DPP patterns),
//                                                              one v_fmac_f32_dpp per real number and stage
//     X[k] = ((Z[k] + Z*[200-k]) - i W400^k (Z[k] - Z*[200-k])) / 2     the real-input split; lane p ends with block k2 = bitrev3(p)
//                                                              and lane 7 - p (row_half_mirror) with block 7 - k2: its partner
//     mel[b] += fb[k][b] |X[k]|^2                              SPARSE: a bin feeds two adjacent bands (triangular filters) and the
//                                                              band index never falls along a lane's 25 bins: two running sums per
//                                                              lane, shifted when the band advances, every step's sum stored to the
//                                                              lane's own slots of the frame's LDS row (the last store of a slot is
//                                                              the complete sum; where the band index skips one -- the bank's linear
//                                                              part: 37.2 Hz bands under 40 Hz bins -- both sums are stored: a
//                                                              wave-uniform step mask); bands that straddle two lanes are added up by the
//                                                              epilogue.  (ds_add_f32 into a shared row was the first form: LDS
//                                                              float atomics run at ~2 cycles per LANE -- 0.72 of 1.07 ms.)
//
// so a wave transforms 8 frames at a time (two such octets interleaved: the per-lane constant tables are read once for both) and a
// workgroup of 4 waves a chunk of 64 frame slots.  The work list, the pivot c, the owners of a frame and the per-owner correction
// are those of k_logmel_h_clip (logmel_h.inc: frames that overlapping segments share are transformed once per clip); only the
// chunk size differs (fc_chunking).  ~1 250 vector instructions per lane and octet = ~10 k lane-operations per frame against
// ~1.2 M matrix-pipe FLOPs per frame of the DFT-as-GEMM.
constexpr int FC_SLOTS = 64;                       // frame slots of a chunk workgroup
constexpr int FC_WAVES = 4;
constexpr int FC_THREADS = FC_WAVES * 64;
constexpr int FC_OCT = 2;                          // octets (8 frames) a wave transforms together
static_assert(FC_OCT == 2 && FC_WAVES * FC_OCT * 8 == FC_SLOTS, "every slot has a lane octet; the two octets of a wave are the two halves of a packed fp32 pair");
constexpr int FC_CAP = FFT_HOP * (FC_SLOTS - 1) + N_FFT;     // floats of sample storage: 64 consecutive frames
constexpr int FC_EDGE_CHUNK = FC_CAP / N_FFT;      // edge frames of an edge-only chunk (each its own 400-sample window)
constexpr int FC_LMS = 112;                        // floats per row of the LDS mel tile: the 8 lanes' band slots, X'[1], a zero
constexpr int FC_ROW_X1IM = 109, FC_ROW_X1 = 110, FC_ROW_ZERO = 111;  // (floats) where a row keeps Im and Re X'[1], and a slot nobody writes after it was zeroed
constexpr int FC_TABK = 80;                        // floats per k1 of the lane tables: [window 2][W200 2][W400 2][mel 4] x 8 lanes
constexpr int FC_NET = 25 * FC_TABK;               // then 8 floats x 8 lanes of exchange-stage constants
constexpr int FC_COMB = FC_NET + 64;               // then per band the byte offsets of the (at most two) slots that add up to it
constexpr int FC_TAB_FLOATS = FC_COMB + 2 * N_MELS;
constexpr int FC_STATS = 32;                       // segments whose statistics a workgroup keeps in LDS for its epilogue
constexpr size_t logmel_fft_lds_bytes() { return sizeof(float) * (FC_CAP + FC_TAB_FLOATS + FC_SLOTS * FC_LMS + 4 * FC_STATS); }
static_assert(2 * logmel_fft_lds_bytes() <= 160 * 1024, "two chunk workgroups per CU");

// How a clip of S segments is cut into chunks of FC_SLOTS frame slots (same scheme as clip_chunking: full chunks of interior
// frames, one tail chunk with the rest plus as many edge frames as its slots and its sample storage hold, then edge-only chunks)
__host__ __device__ inline ClipChunks fc_chunking(int S, int T, int H) {
    ClipChunks c{0, 0, 0, 0};
    if (S <= 0) return c;
    const int ni = (S - 1) * H + T - 3, E = 3 * S;
    c.n_full = ni / FC_SLOTS;
    c.r = ni - c.n_full * FC_SLOTS;
    const int span_r = c.r > 0 ? FFT_HOP * (c.r - 1) + N_FFT : 0;
    const int fit = (FC_CAP - span_r) / N_FFT;
    c.e_tail = E < fit ? E : fit;
    if (c.e_tail > FC_SLOTS - c.r) c.e_tail = FC_SLOTS - c.r;
    c.n_edge_chunks = (E - c.e_tail + FC_EDGE_CHUNK - 1) / FC_EDGE_CHUNK;
    return c;
}
__host__ __device__ inline int fc_chunk_count(int S, int T, int H) {
    const ClipChunks c = fc_chunking(S, T, H);
    return S <= 0 ? 0 : c.n_full + 1 + c.n_edge_chunks;
}
// geometry 0: k_logmel_h_clip (104 interior frames per chunk), 1: k_logmel_fft_clip (64)
__host__ __device__ inline int chunk_count_g(int geom, int S, int T, int H) {
    return geom == 1 ? fc_chunk_count(S, T, H) : clip_chunk_count(S, T, H);
}

// ---- lane primitives --------------------------------------------------------------------------------------------------------
// The vector ALU of a gfx950 SIMD is 16 lanes wide: a wave64 instruction takes 4 cycles whatever it does, and the first build of this
// kernel -- 3 400 scalar fp32 instructions per wave -- ran at exactly that rate.  The packed fp32 forms (v_pk_fma_f32, v_pk_mul_f32,
// v_pk_add_f32) do two operations per lane in the same 4 cycles, so the two octets a wave transforms together live in ONE stream of
// float pairs: element x = octet 0, element y = octet 1, every constant shared (op_sel broadcast, no extra move).  Only the DPP
// instructions stay scalar (one per octet).
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 fc_fma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f32x2 fc_fma(float a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma((f32x2)(a), b, c); }
__device__ __forceinline__ float fc_dpp_hm(float v) {          // value of lane 7 - p (inside every group of 8 lanes)
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, true));
}
__device__ __forceinline__ f32x2 fc_dpp_hm(f32x2 v) { return f32x2{fc_dpp_hm(v.x), fc_dpp_hm(v.y)}; }
// own <- own + g * partner(own) for five complex numbers of one octet (ten registers) at once.  v_fmac_f32_dpp is one instruction
// where the compiler would emit v_mov_b32_dpp + v_fma_f32; the leading s_nop 1 gives the 2 wait states a DPP read needs after a VALU
// write of the same register (the compiler pads nothing inside an asm statement).  No register is read through DPP after it was
// written inside the block: every instruction reads and writes its own.
#define FC_BFLY10(CTRL, g, a0, a1, a2, a3, a4, a5, a6, a7, a8, a9)                                                         \
    asm volatile("s_nop 1\n"                                                                                               \
                 "v_fmac_f32_dpp %0, %0, %10 " CTRL " row_mask:0xf bank_mask:0xf\n"                                         \
                 "v_fmac_f32_dpp %1, %1, %10 " CTRL " row_mask:0xf bank_mask:0xf\n"                                         \
                 "v_fmac_f32_dpp %2, %2, %10 " CTRL " row_mask:0xf bank_mask:0xf\n"                                         \
                 "v_fmac_f32_dpp %3, %3, %10 " CTRL " row_mask:0xf bank_mask:0xf\n"                                         \
                 "v_fmac_f32_dpp %4, %4, %10 " CTRL " row_mask:0xf bank_mask:0xf\n"                                         \
                 "v_fmac_f32_dpp %5, %5, %10 " CTRL " row_mask:0xf bank_mask:0xf\n"                                         \
                 "v_fmac_f32_dpp %6, %6, %10 " CTRL " row_mask:0xf bank_mask:0xf\n"                                         \
                 "v_fmac_f32_dpp %7, %7, %10 " CTRL " row_mask:0xf bank_mask:0xf\n"                                         \
                 "v_fmac_f32_dpp %8, %8, %10 " CTRL " row_mask:0xf bank_mask:0xf\n"                                         \
                 "v_fmac_f32_dpp %9, %9, %10 " CTRL " row_mask:0xf bank_mask:0xf"                                           \
                 : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7), "+v"(a8), "+v"(a9)     \
                 : "v"(g))
#define FC_CTRL_HM "row_half_mirror"
#define FC_CTRL_X2 "quad_perm:[2,3,0,1]"
#define FC_CTRL_X1 "quad_perm:[1,0,3,2]"

// in-place 5-point DFT (forward, W5 = e^(-2 pi i / 5)) of five complex numbers (of both octets): 36 packed operations
__device__ __forceinline__ void fc_radix5(f32x2& r0, f32x2& i0, f32x2& r1, f32x2& i1, f32x2& r2, f32x2& i2, f32x2& r3, f32x2& i3,
                                          f32x2& r4, f32x2& i4) {
    constexpr float C1 = 0.30901699437494742f, C2 = -0.80901699437494742f;     // cos 72, cos 144
    constexpr float S1 = 0.95105651629515357f, S2 = 0.58778525229247313f;      // sin 72, sin 144
    const f32x2 t1r = r1 + r4, t1i = i1 + i4, t2r = r2 + r3, t2i = i2 + i3;
    const f32x2 t3r = r1 - r4, t3i = i1 - i4, t4r = r2 - r3, t4i = i2 - i3;
    const f32x2 m1r = fc_fma(C2, t2r, fc_fma(C1, t1r, r0)), m1i = fc_fma(C2, t2i, fc_fma(C1, t1i, i0));
    const f32x2 m2r = fc_fma(C1, t2r, fc_fma(C2, t1r, r0)), m2i = fc_fma(C1, t2i, fc_fma(C2, t1i, i0));
    const f32x2 n1r = fc_fma(S2, t4r, S1 * t3r), n1i = fc_fma(S2, t4i, S1 * t3i);
    const f32x2 n2r = fc_fma(-S1, t4r, S2 * t3r), n2i = fc_fma(-S1, t4i, S2 * t3i);
    r0 = r0 + t1r + t2r;
    i0 = i0 + t1i + t2i;
    r1 = m1r + n1i; i1 = m1i - n1r;          // m1 - i n1
    r4 = m1r - n1i; i4 = m1i + n1r;          // m1 + i n1
    r2 = m2r + n2i; i2 = m2i - n2r;
    r3 = m2r - n2i; i3 = m2i + n2r;
}

// position of Y[k1] after the two in-place radix-5 passes (k1 = j1 + 5 j2 lives where V[m2 = j2][j1] lived: 5 j1 + j2)
__host__ __device__ constexpr int fc_pos(int k1) { return 5 * (k1 % 5) + k1 / 5; }

// W25^e = cos - i sin, as compile-time constants of the wave-uniform twiddles between the two radix-5 passes
__device__ __forceinline__ constexpr float fc_w25c(int e) {
    constexpr float c[25] = {1.f, 0.96858316112863108f, 0.87630668004386358f, 0.72896862742141155f, 0.53582679497899666f,
                             0.30901699437494742f, 0.062790519529313374f, -0.18738131458572463f, -0.42577929156507272f,
                             -0.63742398974868975f, -0.80901699437494742f, -0.92977648588825146f, -0.99211470131447788f,
                             -0.99211470131447788f, -0.92977648588825146f, -0.80901699437494742f, -0.63742398974868975f,
                             -0.42577929156507272f, -0.18738131458572463f, 0.062790519529313374f, 0.30901699437494742f,
                             0.53582679497899666f, 0.72896862742141155f, 0.87630668004386358f, 0.96858316112863108f};
    return c[e % 25];
}
__device__ __forceinline__ constexpr float fc_w25s(int e) {          // sin(2 pi e / 25)
    constexpr float s[25] = {0.f, 0.24868988716485479f, 0.48175367410171532f, 0.68454710592868873f, 0.84432792550201508f,
                             0.95105651629515357f, 0.99802672842827156f, 0.98228725072868872f, 0.90482705246601958f,
                             0.77051324277578925f, 0.58778525229247313f, 0.36812455268467797f, 0.12533323356430426f,
                             -0.12533323356430426f, -0.36812455268467797f, -0.58778525229247313f, -0.77051324277578925f,
                             -0.90482705246601958f, -0.98228725072868872f, -0.99802672842827156f, -0.95105651629515357f,
                             -0.84432792550201508f, -0.68454710592868873f, -0.48175367410171532f, -0.24868988716485479f};
    return s[e % 25];
}

// 25-point FFT of xr/xi[0..24] (index m = 5 m1 + m2) in place; Y[k1] ends at fc_pos(k1)
__device__ __forceinline__ void fc_fft25(f32x2 (&xr)[25], f32x2 (&xi)[25]) {
#pragma unroll
    for (int m2 = 0; m2 < 5; ++m2)
        fc_radix5(xr[m2], xi[m2], xr[5 + m2], xi[5 + m2], xr[10 + m2], xi[10 + m2], xr[15 + m2], xi[15 + m2], xr[20 + m2], xi[20 + m2]);
#pragma unroll
    for (int j1 = 1; j1 < 5; ++j1)
#pragma unroll
        for (int m2 = 1; m2 < 5; ++m2) {                  // V[m2][j1] *= W25^(m2 j1)
            const float c = fc_w25c(m2 * j1), s = fc_w25s(m2 * j1);
            const f32x2 a = xr[5 * j1 + m2], b = xi[5 * j1 + m2];
            xr[5 * j1 + m2] = fc_fma(s, b, c * a);        // (a + i b)(c - i s)
            xi[5 * j1 + m2] = fc_fma(-s, a, c * b);
        }
#pragma unroll
    for (int j1 = 0; j1 < 5; ++j1)
        fc_radix5(xr[5 * j1], xi[5 * j1], xr[5 * j1 + 1], xi[5 * j1 + 1], xr[5 * j1 + 2], xi[5 * j1 + 2], xr[5 * j1 + 3], xi[5 * j1 + 3],
                  xr[5 * j1 + 4], xi[5 * j1 + 4]);
}

// one exchange stage over all 25 complex numbers of both octets: own <- (own + g partner) (c + i s)
#define FC_STAGE(CTRL, g, c, s, TWIDDLE)                                                                                    \
    _Pragma("unroll") for (int q = 0; q < 25; q += 5) {                                                                     \
        float lr0 = xr[q].x, li0 = xi[q].x, lr1 = xr[q + 1].x, li1 = xi[q + 1].x, lr2 = xr[q + 2].x, li2 = xi[q + 2].x,      \
              lr3 = xr[q + 3].x, li3 = xi[q + 3].x, lr4 = xr[q + 4].x, li4 = xi[q + 4].x;                                    \
        float hr0 = xr[q].y, hi0 = xi[q].y, hr1 = xr[q + 1].y, hi1 = xi[q + 1].y, hr2 = xr[q + 2].y, hi2 = xi[q + 2].y,      \
              hr3 = xr[q + 3].y, hi3 = xi[q + 3].y, hr4 = xr[q + 4].y, hi4 = xi[q + 4].y;                                    \
        FC_BFLY10(CTRL, g, lr0, li0, lr1, li1, lr2, li2, lr3, li3, lr4, li4);                                               \
        FC_BFLY10(CTRL, g, hr0, hi0, hr1, hi1, hr2, hi2, hr3, hi3, hr4, hi4);                                               \
        xr[q] = f32x2{lr0, hr0}; xi[q] = f32x2{li0, hi0}; xr[q + 1] = f32x2{lr1, hr1}; xi[q + 1] = f32x2{li1, hi1};          \
        xr[q + 2] = f32x2{lr2, hr2}; xi[q + 2] = f32x2{li2, hi2}; xr[q + 3] = f32x2{lr3, hr3}; xi[q + 3] = f32x2{li3, hi3};  \
        xr[q + 4] = f32x2{lr4, hr4}; xi[q + 4] = f32x2{li4, hi4};                                                           \
        if (TWIDDLE) {                                                                                                      \
            _Pragma("unroll") for (int e = 0; e < 5; ++e) {                                                                 \
                const f32x2 a = xr[q + e], b = xi[q + e];                                                                   \
                xr[q + e] = fc_fma(-(s), b, (c) * a);                                                                       \
                xi[q + e] = fc_fma((s), a, (c) * b);                                                                        \
            }                                                                                                               \
        }                                                                                                                   \
    }

// one chunk of the work list: interior frames [j0, j0 + nfr_int) of a clip, then its share of the clip's edge frames (logmel_h.inc)
struct FcGeom {
    int nfr_int, e_first, n_edge, nfr;
    int span, edge_base;         // clip samples [u0, u0 + span) sit at the start of the sample storage, the edge windows behind them
    int u0, j0, avail;
    int clip_seg0, clip_S, sc_base;      // the clip's segments; the first segment (relative) whose statistics the epilogue keeps in LDS
    const float* clip;
    bool whole;                  // every sample of the chunk exists (the clip does not end inside it): plain vector loads
};
// A chunk record through the scalar cache.  The records are written by k_build_plan, never by this kernel, so the constant
// address space is legitimate; without it hipcc loads them with vector loads inside the loop (a store may alias), and the wait for
// such a load -- vmcnt counts in order -- also waits for every store of the previous chunk's epilogue.
__device__ __forceinline__ ChunkRec fc_rec(const ChunkRec* recs, int w) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) ChunkRec* crec_p;
    return *((crec_p)(uintptr_t)(recs + w));
#else
    return recs[w];
#endif
}
// (the same for a segment's mean: written by k_seg_stats, never by this kernel)
__device__ __forceinline__ float fc_scalar_f32(const float* ptr) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) float* cf_p;
    return *((cf_p)(uintptr_t)ptr);
#else
    return *ptr;
#endif
}
__device__ __forceinline__ bool fc_geom(const LogmelParams& p, bool exists, const ChunkRec& rec, FcGeom& g) {
    g.nfr = 0;
    if (!exists) return false;
    const int T = p.nf, H = p.seg_hop_frames;
    const int cidx = rec.cidx;
    g.clip_seg0 = rec.seg0; g.clip_S = rec.n_seg;
    const ClipChunks cc = fc_chunking(g.clip_S, T, H);
    g.j0 = 2 + cidx * FC_SLOTS;
    if (cidx < cc.n_full) { g.nfr_int = FC_SLOTS; g.e_first = 0; g.n_edge = 0; }
    else if (cidx == cc.n_full) { g.nfr_int = cc.r; g.e_first = 0; g.n_edge = cc.e_tail; }
    else {
        g.nfr_int = 0;
        g.e_first = cc.e_tail + (cidx - cc.n_full - 1) * FC_EDGE_CHUNK;
        g.n_edge = max(0, min(FC_EDGE_CHUNK, 3 * g.clip_S - g.e_first));
    }
    g.span = g.nfr_int > 0 ? FFT_HOP * (g.nfr_int - 1) + N_FFT : 0;
    g.edge_base = g.span;
    g.nfr = g.nfr_int + g.n_edge;
    g.avail = rec.avail;
    g.u0 = FFT_HOP * g.j0 - 200;
    g.clip = p.wave + rec.beg;
    // segments whose statistics the epilogue needs: the owners of the interior frames, the segments of the edge frames
    g.sc_base = g.nfr_int > 0 ? max(0, (g.j0 - (T - 2) + H - 1) / H) : g.e_first / 3;
    g.whole = g.span > 0 && g.u0 + g.span <= g.avail && !RADAD_DBG(p.debug, 2);
    return g.nfr > 0;
}
constexpr int FC_RAW = (FC_CAP / 4 + FC_THREADS - 1) / FC_THREADS;        // 128-bit sample loads per thread and chunk: 11

// transform + epilogue of the chunk whose samples (minus `pivot`), edge windows and segment statistics are staged in LDS
__device__ __forceinline__ void fc_process(const LogmelParams& p, const FcGeom& g, float pivot, const float* smp, const float* tab,
                                           float* lm, const float* sstat, int lane, int wave) {
    const int T = p.nf, H = p.seg_hop_frames;
    // ---- transform: lane (f, pl) of octet o works on slot 16 wave + 8 o + f ----------------------------------------------------
    const int pl = lane & 7, fo = lane >> 3;
    const int slot0 = 16 * wave;
    if (slot0 < g.nfr && !RADAD_DBG(p.debug, 1)) {           // wave-uniform (no workgroup barrier below this line)
        const int rr = pl < 4 ? pl : 11 - pl;              // the lane's residue class: it holds z[8 m + rr]
        f32x2 xr[25], xi[25];                              // element x: octet 0 (slot 16 wave + f), element y: octet 1 (+ 8)
        int rowb[FC_OCT];                                  // byte offset of the slot's row in the mel tile
        {
            const float* src[FC_OCT];
#pragma unroll
            for (int o = 0; o < FC_OCT; ++o) {
                const int slot = slot0 + 8 * o + fo;
                const int tf = min(slot, g.nfr - 1);         // clamped: slots past the chunk's frames recompute the last one (never stored)
                const int base = tf < g.nfr_int ? FFT_HOP * tf : g.edge_base + N_FFT * (tf - g.nfr_int);
                src[o] = smp + base + 2 * rr;
                rowb[o] = slot * FC_LMS * 4;
            }
            // hann window: g[n], n = 16 m + 2 rr (+ 1)
#pragma unroll
            for (int m = 0; m < 25; ++m) {
                const float2 v0 = *reinterpret_cast<const float2*>(src[0] + 16 * m), v1 = *reinterpret_cast<const float2*>(src[1] + 16 * m);
                const float2 wv = *reinterpret_cast<const float2*>(tab + m * FC_TABK + 2 * pl);
                // four scalar multiplies, each straight into its half of a pair: pairing the loaded values first would cost three
                // moves per pair (the empty asm keeps the compiler from re-forming `pair x constant`)
                float r0 = wv.x * v0.x, r1 = wv.x * v1.x, i0 = wv.y * v0.y, i1 = wv.y * v1.y;
                asm volatile("" : "+v"(r0), "+v"(r1), "+v"(i0), "+v"(i1));
                xr[m] = f32x2{r0, r1};
                xi[m] = f32x2{i0, i1};
            }
        }
        if (!RADAD_DBG(p.debug, 32)) fc_fft25(xr, xi);
        // per-lane twiddle W200^(rr k1) (k1 = 0: 1)
#pragma unroll
        for (int k1 = 1; k1 < 25; ++k1) {
            const float2 tw = *reinterpret_cast<const float2*>(tab + k1 * FC_TABK + 16 + 2 * pl);      // cos, sin of 2 pi rr k1 / 200
            const int q = fc_pos(k1);
            const f32x2 a = xr[q], b = xi[q];
            xr[q] = fc_fma(tw.y, b, tw.x * a);             // (a + i b)(cos - i sin)
            xi[q] = fc_fma(-tw.y, a, tw.x * b);
        }
        // radix-8 across the octet's lanes: own <- (own + g partner) tw, three stages (tools/fft_design.py derives the constants)
        if (!RADAD_DBG(p.debug, 16)) {
            const float* net = tab + FC_NET + 8 * pl;
            const f32x4 n0 = *reinterpret_cast<const f32x4*>(net), n1 = *reinterpret_cast<const f32x4*>(net + 4);
            const float g1 = n0[0], c1 = n0[1], s1 = n0[2], g2 = n0[3], c2 = n1[0], s2 = n1[1], g3 = n1[2];
            FC_STAGE(FC_CTRL_HM, g1, c1, s1, true)
            FC_STAGE(FC_CTRL_X2, g2, c2, s2, true)
            FC_STAGE(FC_CTRL_X1, g3, 1.f, 0.f, false)
        }
        // real-input split against the mirrored lane, |X|^2, sparse mel.  Lane pl holds Z[25 k2 + k1] (k2 = bitrev3(pl)) at fc_pos(k1);
        // its partner Z[200 - k] sits in lane 7 - pl at fc_pos(25 - k1) -- except k1 = 0, whose partner Z[25 (8 - k2)] is a different lane
        const int perm0 = pl < 2 ? pl : (pl < 4 ? (pl ^ 1) : 11 - pl);
        const int src0 = (lane & ~7) | perm0;
        f32x2 a0 = f32x2{0.f, 0.f}, a1 = f32x2{0.f, 0.f};  // running sums of the lane's current band and the next one
        int soff_last = 0;
        char* const rowp0 = reinterpret_cast<char*>(lm) + rowb[0];
        char* const rowp1 = reinterpret_cast<char*>(lm) + rowb[1];
#pragma unroll
        for (int k1 = 0; k1 < (RADAD_DBG(p.debug, 64) ? 0 : 25); ++k1) {
            const float2 pw = *reinterpret_cast<const float2*>(tab + k1 * FC_TABK + 32 + 2 * pl);       // cos, sin of 2 pi k / 400
            const f32x4 ml = *reinterpret_cast<const f32x4*>(tab + k1 * FC_TABK + 48 + 4 * pl);         // fb[k][b] / 4, fb[k][b + 1] / 4, slot, advance
            const float soff_f = ml[2], adv_f = ml[3];         // (a bit_cast of the vector ELEMENT reads element 0: hipcc 7.2)
            const int soff = __float_as_int(soff_f);           // byte offset of band b's slot in the row
            const int adv = __float_as_int(adv_f);             // the next bin's first band is b + adv (0, 1; 2 only where fft_adv2 says)
            const bool two = (p.fft_adv2 >> k1) & 1;           // wave-uniform
            soff_last = soff;
            const int qa = fc_pos(k1), qb = fc_pos(k1 == 0 ? 0 : 25 - k1);
            const f32x2 ar = xr[qa], ai = xi[qa];
            f32x2 br, bi;
            if (k1 == 0) {
                br = f32x2{__shfl(ar.x, src0, 64), __shfl(ar.y, src0, 64)};
                bi = f32x2{__shfl(ai.x, src0, 64), __shfl(ai.y, src0, 64)};
            } else { br = fc_dpp_hm(xr[qb]); bi = fc_dpp_hm(xi[qb]); }
            const f32x2 e1 = ar + br, o1 = ar - br, e2 = ai + bi, o2 = ai - bi;
            const f32x2 re2 = fc_fma(-pw.y, o1, fc_fma(pw.x, e2, e1));      // 2 Re X
            const f32x2 im2 = fc_fma(-pw.y, e2, fc_fma(-pw.x, o1, o2));     // 2 Im X
            f32x2 pw4 = fc_fma(re2, re2, im2 * im2);                        // 4 |X|^2
            // bin 1 (k1 = 1 of lane 0) stays out of the shared sums: every owner adds it with its own mean folded in (epilogue)
            if (k1 == 1) pw4 = pl == 0 ? f32x2{0.f, 0.f} : pw4;
            a0 = fc_fma(ml[0], pw4, a0);
            a1 = fc_fma(ml[1], pw4, a1);
            if (!RADAD_DBG(p.debug, 4)) {
                *reinterpret_cast<float*>(rowp0 + soff) = a0.x;
                *reinterpret_cast<float*>(rowp1 + soff) = a0.y;
            }
            // shift the running sums by adv bands: exact (the factors are 0 or 1)
            const float keep = adv == 0 ? 1.f : 0.f;
            if (two) {                                         // some lane is done with BOTH its bands after this bin
                *reinterpret_cast<float*>(rowp0 + soff + 4) = a1.x;
                *reinterpret_cast<float*>(rowp1 + soff + 4) = a1.y;
                const float take = adv == 1 ? 1.f : 0.f;
                a0 = fc_fma(take, a1, keep * a0);
            } else a0 = fc_fma(1.f - keep, a1, keep * a0);
            a1 = keep * a1;
            if (k1 == 1 && pl == 0) {                          // X'[1]
                reinterpret_cast<float*>(rowp0)[FC_ROW_X1] = 0.5f * re2.x;
                reinterpret_cast<float*>(rowp1)[FC_ROW_X1] = 0.5f * re2.y;
                reinterpret_cast<float*>(rowp0)[FC_ROW_X1IM] = 0.5f * im2.x;
                reinterpret_cast<float*>(rowp1)[FC_ROW_X1IM] = 0.5f * im2.y;
            }
        }
        // (the table marks the last bin as advancing: a0 now holds the band after the last bin's first one)
        *reinterpret_cast<float*>(rowp0 + soff_last + 4) = a0.x;
        *reinterpret_cast<float*>(rowp1 + soff_last + 4) = a0.y;
    }
    // ---- epilogue, per wave over its own 16 rows: every owner of a slot's frame gets the frame's row (logmel_h.inc) ------------
    // lane = (row 16 wave + (lane >> 2), band groups (lane & 3) + 4 i, i = 0..4: 64 contiguous bytes of four lanes per store)
    {
        const int row = slot0 + (lane >> 2);
        const int gq = lane & 3;
        const bool fvalid = row < g.nfr;
        const bool edge = row >= g.nfr_int;
        int s_lo, s_hi, jf = 0, e_kind = 0;
        if (edge) {
            const int ee = g.e_first + (row - g.nfr_int);
            s_lo = s_hi = g.clip_seg0 + ee / 3;
            e_kind = ee - 3 * (ee / 3);
        } else {
            jf = g.j0 + row;
            const int lo = jf - (T - 2);                        // owners: 2 <= jf - s H <= T - 2
            s_lo = g.clip_seg0 + (lo <= 0 ? 0 : (lo + H - 1) / H);
            s_hi = g.clip_seg0 + min(g.clip_S - 1, (jf - 2) / H);
        }
        if (!fvalid) s_hi = s_lo - 1;
        f32x4 st_o[LH_MAX_OWNERS];
#pragma unroll
        for (int o = 0; o < LH_MAX_OWNERS; ++o) {
            st_o[o] = f32x4{0.f, 1.f, 1.f, 0.f};
            if (p.normalize && s_lo + o <= s_hi) {
                const int ci = s_lo + o - g.clip_seg0 - g.sc_base;          // (the staging phase parked the usual ones in LDS)
                st_o[o] = (ci >= 0 && ci < FC_STATS) ? reinterpret_cast<const f32x4*>(sstat)[ci]
                                                     : reinterpret_cast<const f32x4*>(p.seg_stats)[s_lo + o];
            }
        }
        const float* lrow = lm + row * FC_LMS;
        const char* lrowb = reinterpret_cast<const char*>(lrow);
        f32x4 z[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            // band m = the sum of two slots (one of them the row's zero unless the band straddles two lanes)
            const int* cb = reinterpret_cast<const int*>(tab + FC_COMB) + 8 * (gq + 4 * i);
            const int4 c0 = *reinterpret_cast<const int4*>(cb), c1 = *reinterpret_cast<const int4*>(cb + 4);
            z[i][0] = *reinterpret_cast<const float*>(lrowb + c0.x) + *reinterpret_cast<const float*>(lrowb + c0.y);
            z[i][1] = *reinterpret_cast<const float*>(lrowb + c0.z) + *reinterpret_cast<const float*>(lrowb + c0.w);
            z[i][2] = *reinterpret_cast<const float*>(lrowb + c1.x) + *reinterpret_cast<const float*>(lrowb + c1.y);
            z[i][3] = *reinterpret_cast<const float*>(lrowb + c1.z) + *reinterpret_cast<const float*>(lrowb + c1.w);
        }
        const float z0 = z[0][0], z1 = z[0][1];              // linear mel' of bands 0, 1 without bin 1 (lanes gq == 0)
        const float x1re = lrow[FC_ROW_X1], x1im = lrow[FC_ROW_X1IM];
#pragma unroll
        for (int i = 0; i < 5; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) z[i][e] = __log10f(z[i][e]);    // v_log_f32: 1 ulp of log2, < 2e-6 here (0 -> -inf, floored below)
        float lmax_o[LH_MAX_OWNERS];
#pragma unroll
        for (int o = 0; o < LH_MAX_OWNERS; ++o) {
            lmax_o[o] = -INFINITY;
            const int sg = s_lo + o;
            if (sg <= s_hi) {
                const int fl = edge ? (e_kind < 2 ? e_kind : T - 1) : jf - (sg - g.clip_seg0) * H;
                const float g2 = st_o[o][2], lg = st_o[o][3];
                const float d = p.normalize ? -100.f * (pivot - st_o[o][0]) : 0.f;
                const float p1 = fmaf(x1re + d, x1re + d, x1im * x1im);    // |X'[1] + d|^2: bin 1 of this owner, before its 1 / sd^2
                float* orow = p.logmel + ((int64_t)sg * T + fl) * N_MELS;
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(z[i][e] + lg, -10.f);
                    if (i == 0 && gq == 0) {
                        v[0] = fmaxf(log10f(fmaf(p.fb1[0], p1, z0) * g2), -10.f);
                        v[1] = fmaxf(log10f(fmaf(p.fb1[1], p1, z1) * g2), -10.f);
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) lmax_o[o] = fmaxf(lmax_o[o], v[e]);
                    if (!RADAD_DBG(p.debug, 8)) *reinterpret_cast<f32x4*>(orow + 4 * (gq + 4 * i)) = v;
                }
            }
        }
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

// Persistent workgroups (two per CU), each walking the chunk list with a stride of the grid.  The global loads of the NEXT chunk --
// its samples into registers, its pivot and segment statistics -- are issued before the current chunk's transform and land while
// it runs (~6 us of vector-ALU work over ~2 us of HBM latency); the lane tables are loaded once per workgroup.  (One chunk per
// workgroup, the first form, ran its phases back to back: every workgroup of the chip staged at the same time, transformed at the
// same time, stored at the same time -- 0.14 ms of HBM time next to 0.12 ms of ALU time, nothing overlapped.)
__global__ __launch_bounds__(FC_THREADS, 2) void k_logmel_fft_clip(LogmelParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* smp = reinterpret_cast<float*>(smem);          // [FC_CAP] the chunk's samples minus the pivot, then its edge windows
    float* tab = smp + FC_CAP;                            // [FC_TAB_FLOATS] lane tables
    float* lm = tab + FC_TAB_FLOATS;                      // [FC_SLOTS][FC_LMS] the mel tile: every slot's band sums by lane
    float* sstat = lm + FC_SLOTS * FC_LMS;                // [FC_STATS][4] statistics of the segments around the chunk (k_seg_stats)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int T = p.nf, H = p.seg_hop_frames;
    const int n_chunks = p.n_seg_dev ? p.n_seg_dev[2] : p.n_chunks;
    int w = (int)blockIdx.x;
    if (w >= n_chunks) return;

    // what the next chunk needs from global memory, in flight across the current chunk's transform
    f32x4 raw[FC_RAW];
    f32x4 statv = f32x4{0.f, 1.f, 1.f, 0.f};
    float pivot_n = 0.f;
    auto issue = [&](const FcGeom& g) {
        // The small loads FIRST.  hipcc's wait-count pass is conservative about registers a load of the previous iteration wrote: a
        // `default, then load under a condition`, or an address computed in such a register, makes it wait for every load in flight.
        // Behind the sample loads that wait would sit in front of the transform and undo the prefetch; in front of them it is free.
        if (p.normalize) {
            statv = reinterpret_cast<const f32x4*>(p.seg_stats)[g.clip_seg0 + min(g.sc_base + min(tid, FC_STATS - 1), g.clip_S - 1)];
            pivot_n = fc_scalar_f32(p.seg_stats + 4 * (g.clip_seg0 + min(g.clip_S - 1, g.j0 / H)));
        }
        if (g.whole) {
            const float* src = g.clip + g.u0;
            const int nv = g.span >> 2;
#pragma unroll
            for (int u = 0; u < FC_RAW; ++u) raw[u] = *reinterpret_cast<const f32x4_a4*>(src + min(u * FC_THREADS + tid, nv - 1) * 4);
        }
    };
    // ... and into LDS once the previous chunk is done with it
    auto land = [&](const FcGeom& g, float pivot) {
        const int nv = g.span >> 2;
        if (g.whole) {
#pragma unroll
            for (int u = 0; u < FC_RAW; ++u) {
                const int i4 = u * FC_THREADS + tid;
                if (i4 < nv) {
                    f32x4 t = raw[u];
#pragma unroll
                    for (int e = 0; e < 4; ++e) t[e] -= pivot;
                    reinterpret_cast<f32x4*>(smp)[i4] = t;
                }
            }
        } else {                                                  // the clip ends inside the chunk (its last one): sample by sample
            const float* src = g.clip + g.u0;
#pragma unroll 1
            for (int i4 = tid; i4 < nv; i4 += FC_THREADS) {
                const int i = g.u0 + i4 * 4;
                f32x4 t;
#pragma unroll
                for (int e = 0; e < 4; ++e) t[e] = (RADAD_DBG(p.debug, 2) ? 1.f : (i + e < g.avail ? src[i4 * 4 + e] : 0.f)) - pivot;
                reinterpret_cast<f32x4*>(smp)[i4] = t;
            }
        }
        // edge windows: position q of edge frame k is segment sample |160 f - 200 + q| reflected at the segment's ends
        const int L = p.seg_len;
#pragma unroll 1
        for (int i = tid; i < g.n_edge * N_FFT; i += FC_THREADS) {
            const int k = i / N_FFT, q = i - k * N_FFT;
            const int ee = g.e_first + k;
            const int sg = ee / 3, kind = ee - 3 * sg;
            int us = FFT_HOP * (kind < 2 ? kind : T - 1) - 200 + q;
            if (us < 0) us = -us;
            if (us >= L) us = 2 * (L - 1) - us;
            const int uc = sg * p.seg_hop + us;                   // the same sample in clip coordinates
            smp[g.edge_base + i] = (uc < g.avail ? g.clip[uc] : 0.f) - pivot;
        }
        if (tid < FC_STATS) reinterpret_cast<f32x4*>(sstat)[tid] = statv;
    };

    const int stride = (int)gridDim.x;
    FcGeom g;
    bool have = fc_geom(p, true, fc_rec(p.chunk_rec, w), g);
    // prologue: the lane tables and the first chunk; every load is issued before the first is waited for
    {
        constexpr int TAB_UNR = (FC_TAB_FLOATS / 4 + FC_THREADS - 1) / FC_THREADS;          // 3
        f32x4 tabv[TAB_UNR];
#pragma unroll
        for (int u = 0; u < TAB_UNR; ++u) tabv[u] = reinterpret_cast<const f32x4*>(p.fft_tab)[min(u * FC_THREADS + tid, FC_TAB_FLOATS / 4 - 1)];
        issue(g);
#pragma unroll
        for (int u = 0; u < TAB_UNR; ++u) {
            const int i = u * FC_THREADS + tid;
            if (i < FC_TAB_FLOATS / 4) reinterpret_cast<f32x4*>(tab)[i] = tabv[u];
        }
        // (only the rows' zero slots need clearing, once: every other slot a band is read from is stored by the transform)
        if (tid < FC_SLOTS) lm[tid * FC_LMS + FC_ROW_ZERO] = 0.f;
    }
    float pivot = pivot_n;
    land(g, pivot);
    __syncthreads();
    while (true) {
        w += stride;
        FcGeom gn;
        const bool have_n = fc_geom(p, w < n_chunks, fc_rec(p.chunk_rec, min(w, n_chunks - 1)), gn);
        if (have_n) issue(gn);
        if (have) fc_process(p, g, pivot, smp, tab, lm, sstat, lane, wave);
        if (w >= n_chunks) break;                         // (a chunk without frames does not end the walk: the list goes on behind it)
        __syncthreads();                                  // every wave is done with this chunk's samples, rows and statistics
        if (have_n) { pivot = pivot_n; land(gn, pivot); }
        __syncthreads();
        g = gn;
        have = have_n;
    }
}
#undef FC_STAGE
#undef FC_BFLY10
