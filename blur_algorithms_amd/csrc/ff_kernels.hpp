// ff_kernels.hpp -- the fused matrix-core kernel for float32, u16, float16 and bfloat16 images of 1, 3 or 4 channels, every window class (NKB = 3 .. 23
// blocks of 16 positions: pad <= 168).
//
// The structure is fw_kernels.hpp's: a workgroup handles ONE channel of a strip of 128 pixel columns (channel fastest in the task
// list), stages its window through LDS, runs the row pass, the hand-off inside the registers, the sliding column-pass accumulators
// and the emission.  What a float input changes:
//   * range: each frame gets a power-of-two scale s = 2^e (ff_scale_exp) with max|x| s B <= 2^14, B = 1 + |dr| (cols + 2 pad) the
//     bound of the row pass's quirk term relative to max|x| (none without the quirk).  Every V of the hand-off is then below 2^14,
//     inside binary16's normal range with 4x headroom.  max|x| comes from the pre-pass on the device (an integer atomicMax on the
//     bits of |x|: the same result in any order); nothing waits for the host;
//   * staging: x s is split into hi = f16(x s) and lo = f16(x s - hi); the window in LDS is two binary16 planes (hi, lo);
//   * row pass: x_hi t_hi + x_hi t_lo + x_lo t_hi per window block, three products where the u8 kernels take two (x_lo t_lo is
//     dropped, as the column pass drops V_lo t_lo).  The taps keep their 2^14 scaling: every product of two binary16 values is exact
//     in the f32 accumulator, and V = acc 2^-14;
//   * emission: out = tfin 2^-14 / s + the column term (unscaled), stored as f32: no + 0.5f, no clamping;
//   * loads: CH = 1 one dwordx4 per group of 4 pixels; CH = 3 / 4 the channel's four floats of the group (strided dwords; the
//     channel tasks of a strip meet in L2);  stores: one dword per lane and output row (32 lanes: 128 contiguous bytes for CH = 1);
//   * the quirk's sums are floating point: f32 products summed in double, every reduction in a fixed order (no float atomics), so
//     a frame gives the same bits alone and inside a batch.
// The accumulator budget is fw_kernels.hpp's: (NKB - 1) / 2 <= 11 tiles of one channel.
//
// The kernel is a template over the pixel type T: float32, or u16 (blur_gaussian_u16_*).  What a u16 input changes, and nothing else:
//   * range: known from the type, so the scale is a constant of the call, e = ff_scale_exp(65535, B): no max|x| pass, no mbits;
//   * staging: a u16 sample splits EXACTLY into hi + lo (16 bits into 11 + 5), so the dropped x_lo t_lo is the row pass's only
//     truncation, as for floats;
//   * loads: CH = 1 one 8-byte load per group of 4 pixels (two registers per group where the float kernel holds four); CH = 3 / 4
//     the channel's four strided 16-bit loads, and so CH = 2, which u16 alone has (the Cb/Cr plane of a P016 surface).  Loads from the image stay inside a row (the edge chunks read strips), so none
//     leaves the buffer resource whatever the row's byte count;
//   * emission: (uint16_t)((uint32_t)(int32_t)(v + 0.5f) & 0xffff) of the float result v: add 0.5, truncate, keep the low 16 bits, no
//     clamping (chan_pack<uint8_t>'s rule, 16 bits wide), one 16-bit store per lane and output row at stride CH.  (CH = 1: dword
//     stores after a lane-pair exchange were measured 4 % slower than the shorts: DESIGN.md section 2.3);
//   * the quirk's sums: the same code as for floats.  Every term is an integer below 2^53 in a double (|Z| <= 4 x 65535 rows cols,
//     and a frame's bytes fit 32 bits), so every sum is exact and the same in any order; no limit beyond the frame limit follows.
//
// T = ff_f16 (IEEE binary16) or ff_bf16 (bfloat16): blur_gaussian_f16_* / blur_gaussian_bf16_*.  The storage is 16 bits, so the loads,
// stores and strips are the u16 instantiation's; the range comes from the content, so the scale and the pre-pass are the float
// instantiation's (max|x| on the widened sample).  What is the half types' own:
//   * staging: a binary16 sample times 2^e is a binary16 value, and a bfloat16 sample (8 significant bits) times 2^e fits
//     binary16's 11: x s = hi, lo = 0.  ONE binary16 plane per window buffer (FfCfg<NKB, 1>), no remainder.  Only |x s| < 2^-14
//     (a sample more than 2^27 / B below the frame's maximum) rounds, to a binary16 subnormal: at most 2^-25 in scaled units;
//   * row pass: x_hi t_hi + x_hi t_lo, two products per window block (what the u8 kernels do);
//   * emission: the float result v rounded ONCE to the sample type, to nearest even: binary16 by v_cvt_f16_f32 (|v| past 65504 gives
//     +-Inf), bfloat16 by the conversion of float to __bf16 (v_cvt_pk_bf16_f32 on gfx950).  No + 0.5, no clamping.
#pragma once
#include <cstdint>
#include <type_traits>
#include "fw_kernels.hpp"

namespace blur_amd {

// The scale exponent of a frame: e with M B 2^e in [2^13, 2^14) (M = max|x| > 0), clamped to [-125, 125] so that 2^e and 2^-e are
// normal floats; M = 0 (and NaN) take e = 0.
__host__ __device__ inline int ff_scale_exp(float maxabs, double bscale)
{
    if (!(maxabs > 0.f)) return 0;
    int k = 0;
    (void)frexp(static_cast<double>(maxabs) * bscale, &k);          // M B = m 2^k, m in [0.5, 1)
    const int e = 14 - k;
    return e < -125 ? -125 : (e > 125 ? 125 : e);
}

// What the fused float kernel reads besides the image:
//   mbits[frame]                        bits of max|x| over the frame (the pre-pass)
//   srow [frame][row][CH]               Srow(r, c) = sum_x wx(x) img[r][x][c]                  (ff_finalize)
//   cpart[frame][band][cpitch]          sum over the band's rows of wy(r) img[r][x][c] at CH x + c
//   zsum [frame][CH]                    Z(c) = sum_r wy(r) Srow(r, c)                          (ff_finalize)
struct FfQuirk {
    const unsigned* mbits;
    const double* srow;
    const double* cpart;
    const double* zsum;
    const float* taps;          // the 2 pad + 1 taps of the row pass, centre at pad
    int nbands, cpitch;
    float dr, dc;
    double bscale;              // B of ff_scale_exp
};

constexpr float kFfRowUnscale = 1.f / 16384.f;      // V = acc 2^-14 (the taps' scaling)

// the pixel types of 16-bit floating-point frames: tags over the bit pattern (uint16_t is the u16 instantiation's)
struct ff_f16 { uint16_t bits; };
struct ff_bf16 { uint16_t bits; };
template <typename T> inline constexpr bool ff_is_half_v = std::is_same_v<T, ff_f16> || std::is_same_v<T, ff_bf16>;
template <typename T> inline constexpr bool ff_is_pixel_v = std::is_same_v<T, float> || std::is_same_v<T, uint16_t> || ff_is_half_v<T>;

// a half-type sample (its bits in the low 16 of `bits`) as f32: exact for both types
template <typename T> __device__ __forceinline__ float ff_half_widen(uint32_t bits)
{
    if constexpr (std::is_same_v<T, ff_f16>) return static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(bits)));
    else return __uint_as_float(bits << 16);
}
// f32 -> the half type, one rounding to nearest even (binary16: overflow to +-Inf, subnormals kept)
template <typename T> __device__ __forceinline__ uint16_t ff_half_round(float v)
{
    if constexpr (std::is_same_v<T, ff_f16>) return __builtin_bit_cast(uint16_t, static_cast<_Float16>(v));
    else return __builtin_bit_cast(uint16_t, static_cast<__bf16>(v));
}

// NP: binary16 planes per window buffer (2: hi and lo; 1: the half types, whose staged samples have no lo)
template <int NKB, int NP = 2> struct FfCfg {
    using W = FwCfg<NKB>;
    static constexpr int PADA = W::PADA, WIN = W::WIN, GPR = W::GPR, PER = W::PER, PW = W::PW, NT = W::NT;
    static constexpr int BUF = W::BUF;                                // one binary16 plane of one window
    // window buffer b, plane p (0 hi, 1 lo) at (NP b + p) BUF
    static constexpr int TLOFF = 2 * NP * BUF;
    static constexpr int QOFF = TLOFF + NKB * 64 * 16;
    static constexpr int LDS = QOFF + 2 * 2 * 32 * 4;
    static_assert(LDS <= 160 * 1024, "the LDS of one CU");
};

// qc[xl] (xl = 0 .. 127) = the column term of pixel x0 + xl in channel c0 (unscaled), 0 right of the image.  256 threads; `scratch`
// = LDS for (128 + 2 pad) + 2 pad + 1 doubles; ends with a barrier.
template <int CH>
__device__ __forceinline__ void ff_quirk_cols_tile(unsigned char* scratch, float* qc, const FfQuirk& q, int f, int x0, int c0, int cols, int pad, int tid)
{
    const int win = kFxChunk + 2 * pad, ntap = 2 * pad + 1;
    double* cc = reinterpret_cast<double*>(scratch);
    double* tp = cc + win;
    const double* base = q.cpart + static_cast<size_t>(f) * q.nbands * q.cpitch + c0;
    for (int p = tid; p < win; p += 256) {
        const double* cp = base + CH * mx_refl(x0 - pad + p, cols);
        double sum = 0.0;
        for (int b = 0; b < q.nbands; ++b) sum += cp[static_cast<size_t>(b) * q.cpitch];
        cc[p] = sum;
    }
    for (int i = tid; i < ntap; i += 256) tp[i] = static_cast<double>(q.taps[i]);
    __syncthreads();
    const double sp = (pad & 1) ? -1.0 : 1.0, z = q.zsum[static_cast<size_t>(f) * CH + c0];
    if (tid < kFxChunk) {
        const int x = x0 + tid;
        float out = 0.f;
        if (x < cols) {
            const double* ccx = cc + tid;
            double acc[4] = { 0, 0, 0, 0 };
            int t = 0;
            for (; t + 8 <= ntap; t += 8) {
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j & 3] = __builtin_fma(tp[t + j], ccx[t + j], acc[j & 3]);
            }
            for (; t < ntap; ++t) acc[t & 3] = __builtin_fma(tp[t], ccx[t], acc[t & 3]);
            const double sx = ((x + pad) & 1) ? -1.0 : 1.0;
            out = static_cast<float>(static_cast<double>(q.dc) * sp * (((acc[0] + acc[1]) + (acc[2] + acc[3])) + static_cast<double>(q.dr) * sx * z));
        }
        qc[tid] = out;
    }
    __syncthreads();
}

// One workgroup per (frame, segment of output tiles, chunk of 128 pixel columns, channel), channel fastest.
template <typename T, int NKB, bool QUIRK, int CH>
__global__ __launch_bounds__(256, 1) void ff_blur(const T* __restrict__ src, T* __restrict__ dst, const mx_half8* __restrict__ frags, FxGeom g,
                                                  int chunks, int tps, int nseg, int ntasks, FfQuirk qk, const T* __restrict__ strips, FwChSel chsel, FwPitch pt,
                                                  const FwFrame* __restrict__ ft)
{
    static_assert(CH == 1 || CH == 3 || CH == 4 || (CH == 2 && std::is_same_v<T, uint16_t>), "one, three or four channels; u16 also two (the chroma plane of a P016 surface)");
    static_assert(ff_is_pixel_v<T>, "float32, u16, float16 or bfloat16 pixels");
    constexpr bool U16 = std::is_same_v<T, uint16_t>, HALF = ff_is_half_v<T>, W16 = U16 || HALF;      // W16: 16-bit storage
    constexpr uint32_t ES = sizeof(T);                              // bytes per sample
    constexpr int NP = HALF ? 1 : 2;                                // binary16 planes per window buffer
    using C = FfCfg<NKB, NP>;
    constexpr int PADA = C::PADA, PW = C::PW, NT = C::NT, PER = C::PER;
    constexpr int RS = NKB;                                        // row-pass slots
    constexpr int CS = NKB > 9 ? NKB : 9;                         // column-pass slots: hand-off 0 .. 7, emission 1 .. 4, staging from 5
    constexpr int IPS = (PER + CS - 6) / (CS - 5);                // staging items per column-pass slot from slot 5 on
    extern __shared__ __attribute__((aligned(16))) unsigned char ff_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = lane & 31, h = lane >> 5;

    const int nx = g.nxcd, xcd = blockIdx.x % nx, in_xcd = blockIdx.x / nx, per_xcd = (ntasks + nx - 1) / nx, task = xcd * per_xcd + in_xcd;
    if (in_xcd >= per_xcd || task >= ntasks) return;
    // the launch's active channels (FwChSel, fw_kernels.hpp; all CH of them: c = task % CH)
    const int nact = CH == 1 ? 1 : fw_chsel_count(chsel), c = CH == 1 ? 0 : static_cast<int>((chsel >> (4 + 2 * (task % nact))) & 3u);
    const int xc = (task / nact) % chunks, seg = (task / (nact * chunks)) % nseg, f = task / (nact * chunks * nseg);
    const int x0 = xc * kFxChunk;
    const int tile0 = seg * tps, tile1 = min(tile0 + tps, g.ntiles);
    // a launch over frames with their own sigmas (FwFrame, fw_kernels.hpp): everything below that depends on sigma is replaced here,
    // once.  (mbits, like the sums and the strips, is the group's pre-pass's: indexed by the position f in the list)
    int fr = f;
    if (ft) {
        const FwFrame e = ft[f];
        fr = e.frame;
        g.pad = e.pad;
        frags += e.frags;
        qk.taps += e.taps;
        qk.dr = e.dr;
        qk.dc = e.dc;
        qk.bscale = e.bscale;
    }
    // (FwPitch, fw_kernels.hpp: pitches and frame strides in bytes, multiples of the sample's size)
    const T* img = reinterpret_cast<const T*>(reinterpret_cast<const unsigned char*>(src) + static_cast<size_t>(fr) * pt.src_frame);
    T* out = reinterpret_cast<T*>(reinterpret_cast<unsigned char*>(dst) + static_cast<size_t>(fr) * pt.dst_frame);

    // the frame's scale (ff_scale_exp): s = 2^e on the staged values, 2^-e on the results (u16: from the type's range, mbits is not read)
    const int sexp = U16 ? ff_scale_exp(65535.f, qk.bscale) : ff_scale_exp(__uint_as_float(qk.mbits[f]), qk.bscale);
    const float scale = ldexpf(1.f, sexp), unscale = ldexpf(1.f, -sexp);

    constexpr int TLR = FW_TL_REGS < NKB ? FW_TL_REGS : NKB;
    mx_half8 th[NKB], tlr[TLR > 0 ? TLR : 1];
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) th[kb] = frags[kb * 64 + lane];
#pragma unroll
    for (int kb = 0; kb < TLR; ++kb) tlr[kb] = frags[(NKB + kb) * 64 + lane];
    {
        mx_half8* tls = reinterpret_cast<mx_half8*>(ff_lds + C::TLOFF);
        for (int i = tid; i < NKB * 64; i += 256) tls[i] = frags[NKB * 64 + i];
    }
    const mx_half8* tlp = reinterpret_cast<const mx_half8*>(ff_lds + C::TLOFF) + lane;
    auto tlo = [&](int kb) __attribute__((always_inline)) { return kb < TLR ? tlr[kb < TLR ? kb : 0] : tlp[kb * 64]; };

    float cpos = 0.f, cneg = 0.f;
    if (QUIRK) {
        static_assert(C::BUF >= 8 * (C::WIN + 2 * C::PADA + 1) && C::BUF >= 4 * kFxChunk, "ff_quirk_cols_tile's scratch and result fit the window buffers");
        float* qc = reinterpret_cast<float*>(ff_lds + C::BUF);
        ff_quirk_cols_tile<CH>(ff_lds, qc, qk, f, x0, c, g.cols, g.pad, tid);
        const float v = qc[32 * wave + m];
        cpos = v;
        cneg = -v;
        __syncthreads();
    }
    const int qrows = 32 * (g.ntiles + NT);
    const double qrs = QUIRK ? static_cast<double>(qk.dr) * ((g.pad & 1) ? -1.0 : 1.0) * static_cast<double>(scale) : 0.0;

    const mx_float16 zero = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
    mx_float16 acc[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) acc[k] = zero;
    mx_float16 arow = zero, tfin = zero;
    uint32_t hl[2][2][8];

    const int s0 = tile0, s1 = tile1 + NT;
    constexpr int NLEFT = fx_left_strips(PADA);
    const int sidx = xc < NLEFT ? xc : (xc >= chunks - g.nright ? NLEFT + xc - (chunks - g.nright) : -1);      // uniform
    // byte offsets: a frame's bytes fit 32 bits (the engine's frame limit)
    const uint32_t pitch = sidx >= 0 ? static_cast<uint32_t>(ES * CH * C::WIN) : pt.src_pitch;
    const T* wbase = sidx >= 0 ? strips + (static_cast<size_t>(f) * (NLEFT + g.nright) + sidx) * g.rows * (CH * C::WIN) : img + CH * (x0 - PADA);
    const uint32_t wbytes = sidx >= 0 ? static_cast<uint32_t>(g.rows) * static_cast<uint32_t>(ES * CH * C::WIN)
                                      : static_cast<uint32_t>(g.rows - 1) * pt.src_pitch + static_cast<uint32_t>(g.cols - (x0 - PADA)) * static_cast<uint32_t>(ES * CH);
    const __amdgpu_buffer_rsrc_t rimg = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(wbase), 0, wbytes, kMxRsrcWord3);
    const int srow = 8 * (tid >> 6) + ((tid >> 4) & 3) + 4 * ((tid >> 3) & 1), g0 = tid & 7;      // (fx_kernels.hpp: the staging map)
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    constexpr int NR = W16 && CH == 1 ? 2 : 4;                     // 16-bit samples, 1 channel: a group's 4 samples in 2 registers
    uint32_t raw[PER][NR];
    double qv = 0.0;
    // the window of step s: thread t moves channel c of the groups of 4 pixels g0 + 8 k of row srow, all requested at once
    auto issue_window = [&](int s) __attribute__((always_inline)) {
        const int r = mx_refl(32 * s - PADA + srow, g.rows);
        const uint32_t off = static_cast<uint32_t>(r) * pitch + ES * static_cast<uint32_t>(4 * CH * g0 + c);
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const bool in = (C::GPR % 8 == 0) || k < PER - 1 || g0 < C::GPR % 8;
            const uint32_t o = in ? off + ES * static_cast<uint32_t>(32 * CH * k) : off;
            if constexpr (W16) {
                if constexpr (CH == 1) {
                    typedef uint32_t u2 __attribute__((ext_vector_type(2)));
                    const u2 t = __builtin_amdgcn_raw_buffer_load_b64(rimg, o, 0, 0);
                    raw[k][0] = t[0];
                    raw[k][1] = t[1];
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) raw[k][j] = __builtin_amdgcn_raw_buffer_load_b16(rimg, o + static_cast<uint32_t>(2 * CH * j), 0, 0);
                }
            } else if (CH == 1) {
                const u4 t = __builtin_amdgcn_raw_buffer_load_b128(rimg, o, 0, 0);
#pragma unroll
                for (int j = 0; j < 4; ++j) raw[k][j] = t[j];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) raw[k][j] = __builtin_amdgcn_raw_buffer_load_b32(rimg, o + static_cast<uint32_t>(4 * CH * j), 0, 0);
            }
        }
        if (QUIRK)              // the row term of row re of V (= image row refl(re - PADA)); every thread (row tid & 31: eight copies of each value)
            qv = qk.srow[(static_cast<size_t>(f) * g.rows + mx_refl(min(32 * s + (tid & 31), qrows - 1) - PADA, g.rows)) * CH + c];
    };
    // group k: x s -> hi + lo binary16 -> the two planes in LDS (one ds_write_b64 each); the half types: x s = hi, one plane
    auto commit_item = [&](int buf, int k) __attribute__((always_inline)) {
        if (k >= PER) return;
        _Float16* base = reinterpret_cast<_Float16*>(ff_lds + NP * buf * C::BUF) + srow * PW + 4 * g0 + 32 * k;
        typedef float f2 __attribute__((ext_vector_type(2)));
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        if constexpr (HALF) {
            uint32_t hp[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                f2 vv;
                if constexpr (CH == 1) vv = f2{ ff_half_widen<T>(raw[k][j] & 0xffffu) * scale, ff_half_widen<T>(raw[k][j] >> 16) * scale };
                else vv = f2{ ff_half_widen<T>(raw[k][2 * j]) * scale, ff_half_widen<T>(raw[k][2 * j + 1]) * scale };
                hp[j] = __builtin_bit_cast(uint32_t, __builtin_convertvector(vv, h2));
            }
            *reinterpret_cast<uint2*>(base) = make_uint2(hp[0], hp[1]);
        } else {
            uint32_t hp[2], lp[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                f2 vv;
                if constexpr (!U16) vv = f2{ __uint_as_float(raw[k][2 * j]) * scale, __uint_as_float(raw[k][2 * j + 1]) * scale };
                else if constexpr (CH == 1) vv = f2{ static_cast<float>(raw[k][j] & 0xffffu) * scale, static_cast<float>(raw[k][j] >> 16) * scale };
                else vv = f2{ static_cast<float>(raw[k][2 * j]) * scale, static_cast<float>(raw[k][2 * j + 1]) * scale };
                hp[j] = __builtin_bit_cast(uint32_t, __builtin_convertvector(vv, h2));
                float r0, r1;
                mx_remainder(hp[j], vv[0], vv[1], r0, r1);
                const f2 rem = { r0, r1 };
                lp[j] = __builtin_bit_cast(uint32_t, __builtin_convertvector(rem, h2));
            }
            *reinterpret_cast<uint2*>(base) = make_uint2(hp[0], hp[1]);
            *reinterpret_cast<uint2*>(base + C::BUF / 2) = make_uint2(lp[0], lp[1]);
        }
    };
    auto commit_q = [&](int buf) __attribute__((always_inline)) {
        if (QUIRK) {
            const float qraw = static_cast<float>(qrs * qv);
            float* qs = reinterpret_cast<float*>(ff_lds + C::QOFF) + buf * 64 + (tid & 31);
            qs[0] = qraw;
            qs[32] = -qraw;
        }
    };
    // R: the window in buffer `buf` -> arow; `beside(kb)` runs after the products of slot kb
    auto rowpass = [&](int buf, auto beside) __attribute__((always_inline)) {
        const _Float16* base = reinterpret_cast<const _Float16*>(ff_lds + NP * buf * C::BUF) + m * PW + wave * 32 + 8 * h;
        const _Float16* lbase = base + C::BUF / 2;                // (the half types have no lo plane: not read)
        mx_float16 a = zero;
        mx_half8 x[3], xl[3], tq[3];
#pragma unroll
        for (int kb = 0; kb < 2 && kb < NKB; ++kb) {
            x[kb] = *reinterpret_cast<const mx_half8*>(base + 16 * kb);
            if constexpr (!HALF) xl[kb] = *reinterpret_cast<const mx_half8*>(lbase + 16 * kb);
        }
        tq[0] = tlo(0);
        tq[1] = tlo(1);
#pragma unroll
        for (int kb = 0; kb < RS; ++kb) {
            if (kb + 2 < NKB) {
                x[(kb + 2) % 3] = *reinterpret_cast<const mx_half8*>(base + 16 * (kb + 2));
                if constexpr (!HALF) xl[(kb + 2) % 3] = *reinterpret_cast<const mx_half8*>(lbase + 16 * (kb + 2));
                tq[(kb + 2) % 3] = tlo(kb + 2);
            }
            a = __builtin_amdgcn_mfma_f32_32x32x16_f16(x[kb % 3], th[kb], a, 0, 0, 0);
            a = __builtin_amdgcn_mfma_f32_32x32x16_f16(x[kb % 3], tq[kb % 3], a, 0, 0, 0);
            if constexpr (!HALF) a = __builtin_amdgcn_mfma_f32_32x32x16_f16(xl[kb % 3], th[kb], a, 0, 0, 0);
            asm volatile("" : "+a"(a));
            beside(kb);
            __builtin_amdgcn_sched_barrier(0);
        }
        arow = a;
    };
    // S: arow -> V (+ quirk), split into hi + lo, exchange with lane ^ 32 -> hl[hb] (fw_kernels.hpp: split_piece)
    float sv[16];
    auto split_piece = [&](int buf, int hb, int piece) __attribute__((always_inline)) {
        const int hf = piece >> 2, sub = piece & 3;
        uint32_t (&hp)[8] = hl[hb][0];
        uint32_t (&lp)[8] = hl[hb][1];
        if (sub == 0) {
            if (QUIRK) {
                const float* qs4 = reinterpret_cast<const float*>(ff_lds + C::QOFF) + buf * 64 + (m & 1) * 32 + 4 * h;
#pragma unroll
                for (int k = 2 * hf; k < 2 * hf + 2; ++k) {
                    const float4 t4 = *reinterpret_cast<const float4*>(qs4 + 8 * k);
                    sv[4 * k] = __builtin_fmaf(arow[4 * k], kFfRowUnscale, t4.x);
                    sv[4 * k + 1] = __builtin_fmaf(arow[4 * k + 1], kFfRowUnscale, t4.y);
                    sv[4 * k + 2] = __builtin_fmaf(arow[4 * k + 2], kFfRowUnscale, t4.z);
                    sv[4 * k + 3] = __builtin_fmaf(arow[4 * k + 3], kFfRowUnscale, t4.w);
                }
            } else {
#pragma unroll
                for (int k = 8 * hf; k < 8 * hf + 8; ++k) sv[k] = arow[k] * kFfRowUnscale;
            }
        } else if (sub == 1 || sub == 2) {
#pragma unroll
            for (int k = 4 * hf + 2 * (sub - 1); k < 4 * hf + 2 * sub; ++k) {
                typedef float f2 __attribute__((ext_vector_type(2)));
                typedef _Float16 h2 __attribute__((ext_vector_type(2)));
                const f2 vv = { sv[2 * k], sv[2 * k + 1] };
                hp[k] = __builtin_bit_cast(uint32_t, __builtin_convertvector(vv, h2));
                float r0, r1;
                mx_remainder(hp[k], vv[0], vv[1], r0, r1);
                const f2 rem = { r0, r1 };
                lp[k] = __builtin_bit_cast(uint32_t, __builtin_convertvector(rem, h2));
            }
        } else {
            fx_swap4(hp[4 * hf], hp[4 * hf + 2], hp[4 * hf + 1], hp[4 * hf + 3], lp[4 * hf], lp[4 * hf + 2], lp[4 * hf + 1], lp[4 * hf + 3]);
        }
    };
    // E + F: rows 8 gq + 4 h + 0 .. 3 of the lane's pixel column of the finished tile -> f32 (16-bit types: rounded), stored at once.  Buffer
    // stores: rows past the image, pixels right of it (an explicit x < cols: the bytes between two rows of a pitched frame lie inside
    // the resource) and tiles that do not exist get an offset outside the resource
    const __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc(out, 0, static_cast<uint32_t>(g.rows - 1) * pt.dst_pitch + static_cast<uint32_t>(g.cols) * (ES * CH), kMxRsrcWord3);
    // (the pitch and the store group's row as values the compiler cannot see through: fw_kernels.hpp, store_group)
    uint32_t rowstep_ = pt.dst_pitch;
    asm volatile("" : "+s"(rowstep_));
    const uint32_t rowstep = rowstep_;
    const int xcol = x0 + 32 * wave + m;
    auto emit_store = [&](int tile, bool valid, int gq) __attribute__((always_inline)) {
        int row0 = 32 * tile + 8 * gq + 4 * h;
        asm volatile("" : "+v"(row0));
        const uint32_t base = static_cast<uint32_t>(row0) * rowstep + ES * (static_cast<uint32_t>(xcol) * CH + static_cast<uint32_t>(c));
        if constexpr (W16) {
            uint32_t u[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int reg = 4 * gq + k;
                const float v = __builtin_fmaf(tfin[reg] * kMxUnscale, unscale, (reg & 1) ? cneg : cpos);
                if constexpr (HALF) u[k] = ff_half_round<T>(v);                               // one rounding to nearest even
                else u[k] = static_cast<uint32_t>(static_cast<int>(v + 0.5f)) & 0xffffu;     // add 0.5, truncate, keep the low 16 bits
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool ok = valid && xcol < g.cols && row0 + k < g.rows;
                __builtin_amdgcn_raw_buffer_store_b16(static_cast<uint16_t>(u[k]), rout, ok ? base + k * rowstep : 0xfffffff0u, 0, 0);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int reg = 4 * gq + k;
                const float v = __builtin_fmaf(tfin[reg] * kMxUnscale, unscale, (reg & 1) ? cneg : cpos);
                const bool ok = valid && xcol < g.cols && row0 + k < g.rows;
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rout, ok ? base + k * rowstep : 0xfffffff0u, 0, 0);
            }
        }
    };
    auto colpass = [&](int qs, int hb, int ri, auto beside) __attribute__((always_inline)) {
        mx_half8 v1[2], v2[2];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const u4 w1 = { hl[hb][0][4 * b], hl[hb][0][4 * b + 1], hl[hb][0][4 * b + 2], hl[hb][0][4 * b + 3] };
            const u4 w2 = { hl[hb][1][4 * b], hl[hb][1][4 * b + 1], hl[hb][1][4 * b + 2], hl[hb][1][4 * b + 3] };
            v1[b] = __builtin_bit_cast(mx_half8, w1);
            v2[b] = __builtin_bit_cast(mx_half8, w2);
        }
        auto dof = [](int it) { return it == 0 ? NKB - 1 : (it >= NKB - 2 ? it - (NKB - 2) : it + 1); };
        mx_half8 tq[3];
        tq[0] = tlo(dof(0));
        if (NKB > 1) tq[1] = tlo(dof(1));
#pragma unroll
        for (int it = 0; it < CS; ++it) {
            if (it < NKB) {
                const int d = dof(it);
                const int b = d & 1, a2 = d >> 1, slot = (qs - a2 + 2 * NT) % NT;
                if (it + 2 < NKB) tq[(it + 2) % 3] = tlo(dof(it + 2));
                if (ri < 0 || a2 <= ri) {
                    mx_float16 t = d == 0 ? zero : acc[slot];
                    t = __builtin_amdgcn_mfma_f32_32x32x16_f16(th[d], v1[b], t, 0, 0, 0);
                    t = __builtin_amdgcn_mfma_f32_32x32x16_f16(tq[it % 3], v1[b], t, 0, 0, 0);
                    t = __builtin_amdgcn_mfma_f32_32x32x16_f16(th[d], v2[b], t, 0, 0, 0);
                    asm volatile("" : "+a"(t));
                    if (it == 0) tfin = t; else acc[slot] = t;
                }
            }
            beside(it);
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    // prologue: windows s0 and s0 + 1 in LDS, the first row pass and its hand-off done
    issue_window(s0);
#pragma unroll
    for (int k = 0; k < PER; ++k) commit_item(0, k);
    commit_q(0);
    issue_window(s0 + 1);
#pragma unroll
    for (int k = 0; k < PER; ++k) commit_item(1, k);
    commit_q(1);
    __syncthreads();
    rowpass(0, [](int) {});
#pragma unroll
    for (int p = 0; p < 8; ++p) split_piece(0, 0, p);
    __syncthreads();

    // step s: the row pass of step s + 1, then the column pass of step s (which finishes tile s - NT), the vector work beside the products
    auto step = [&](int s, int qs, int ri) __attribute__((always_inline)) {
        const int par = (s - s0) & 1;
        const int ftile = s - NT;
        const bool fvalid = ftile >= tile0;
        issue_window(s + 2);
        rowpass(par ^ 1, [](int) {});
        colpass(qs, 0, ri, [&](int it) __attribute__((always_inline)) {
            if (it < 8) split_piece(par ^ 1, 1, it);
            if (it >= 1 && it <= 4) emit_store(ftile, fvalid, it - 1);
            if (it >= 5) {
#pragma unroll
                for (int i = 0; i < IPS; ++i) commit_item(par, IPS * (it - 5) + i);
            }
            if (it == CS - 1) commit_q(par);
        });
#pragma unroll
        for (int k = 0; k < 8; ++k) { hl[0][0][k] = hl[1][0][k]; hl[0][1][k] = hl[1][1][k]; }
        __syncthreads();                                   // window s + 2 complete, window s + 1 no longer read
    };
#pragma unroll
    for (int j = 0; j < NT; ++j) step(s0 + j, j, j);
    for (int sb = s0 + NT; sb < s1; sb += NT) {
#pragma unroll
        for (int qs = 0; qs < NT; ++qs) {
            const int s = sb + qs;
            if (s >= s1) break;
            step(s, qs, -1);
        }
    }
}

// The classes that are instantiated: all but NKB = 23 with 3 or 4 channels, whose strided loads leave no registers for the window
// (768 bytes of scratch per lane); those take the plane fallback
__host__ __device__ constexpr bool ff_class_ok(int nkb, int ch) { return !(nkb >= 23 && ch != 1); }
// u16: every class fits (NKB 23 with 3 / 4 channels: 256 VGPRs, 234 / 223 AGPRs, no scratch); the half types hold the same loads
// and one window operand fewer: every class fits
template <typename T> __host__ __device__ constexpr bool ff_class_ok_t(int nkb, int ch)
{
    return std::is_same_v<T, uint16_t> || ff_is_half_v<T> || ff_class_ok(nkb, ch);
}
// The classes the library's own choice takes.  The f32 accumulation over 2 x 3 products per window block reaches 1.02e-6 (NKB 19)
// and 1.11e-6 (NKB 21, 23) of max|x| where the output is as large as max|x| over an area (steps, constants), and 1.19e-6 at NKB 17
// with max|x| = 0.7e30, past the contract's 1e-6; NKB <= 15 was measured within it (9.0e-7).  AUTO takes the plane fallback for pad
// 105 .. 168; FUSED still runs the kernel.
__host__ __device__ constexpr bool ff_class_in_contract(int nkb) { return nkb <= 15; }

template <typename T> struct FfEntryT {
    int nkb;
    // ch: 1, 3 or 4; quirk: whether the quirk's sums in qk are there (float and the half types: qk.mbits always is; u16: never read);
    // chsel: the channels to blur; pt: where the rows and frames lie (FwPitch); ft: the frame list of a launch over frames with their
    // own sigmas, or null (FwFrame)
    hipError_t (*blur)(hipStream_t, const T* src, T* dst, const void* frags, FxGeom g, int ch, int num_cus, const FfQuirk& qk, bool quirk, const T* strips,
                       FwChSel chsel, FwPitch pt, const FwFrame* ft);
};

template <typename T, int NKB, int CH> hipError_t ff_launch_ch(hipStream_t st, const T* src, T* dst, const void* frags, FxGeom g, int num_cus, const FfQuirk& qk,
                                                               bool quirk, const T* strips, FwChSel chsel, FwPitch pt, const FwFrame* ft)
{
    using C = FfCfg<NKB, ff_is_half_v<T> ? 1 : 2>;
    const int nact = fw_chsel_count(chsel);
    if (nact < 1 || nact > CH) return hipErrorInvalidValue;
    for (int i = 0; i < nact; ++i)
        if (static_cast<int>((chsel >> (4 + 2 * i)) & 3u) >= CH) return hipErrorInvalidValue;
    const FxLaunch l = fx_plan_launch(g, nact, C::NT, num_cus);
    if (l.ntasks == 0) return hipSuccess;
    static std::atomic<unsigned long long> attr_done{ 0 };
    const hipError_t e = fx_set_lds(attr_done, C::LDS, ff_blur<T, NKB, true, CH>, ff_blur<T, NKB, false, CH>);
    if (e != hipSuccess) return e;
    if (quirk)
        hipLaunchKernelGGL((ff_blur<T, NKB, true, CH>), l.grid, dim3(256), C::LDS, st, src, dst, static_cast<const mx_half8*>(frags), g, l.chunks, l.tps,
                           l.nseg, static_cast<int>(l.ntasks), qk, strips, chsel, pt, ft);
    else
        hipLaunchKernelGGL((ff_blur<T, NKB, false, CH>), l.grid, dim3(256), C::LDS, st, src, dst, static_cast<const mx_half8*>(frags), g, l.chunks, l.tps,
                           l.nseg, static_cast<int>(l.ntasks), qk, strips, chsel, pt, ft);
    return hipGetLastError();
}

template <typename T, int NKB> hipError_t ff_launch(hipStream_t st, const T* src, T* dst, const void* frags, FxGeom g, int ch, int num_cus, const FfQuirk& qk,
                                                    bool quirk, const T* strips, FwChSel chsel, FwPitch pt, const FwFrame* ft)
{
    if (ch == 1) return ff_launch_ch<T, NKB, 1>(st, src, dst, frags, g, num_cus, qk, quirk, strips, chsel, pt, ft);
    if constexpr (ff_class_ok_t<T>(NKB, 3)) {
        if (ch == 3) return ff_launch_ch<T, NKB, 3>(st, src, dst, frags, g, num_cus, qk, quirk, strips, chsel, pt, ft);
        if (ch == 4) return ff_launch_ch<T, NKB, 4>(st, src, dst, frags, g, num_cus, qk, quirk, strips, chsel, pt, ft);
    }
    // two channels: u16 only (the interleaved Cb/Cr plane of a P016 surface, blur_gaussian_p016_*: no public entry takes channels = 2)
    if constexpr (std::is_same_v<T, uint16_t>) {
        if (ch == 2) return ff_launch_ch<T, NKB, 2>(st, src, dst, frags, g, num_cus, qk, quirk, strips, chsel, pt, ft);
    }
    return hipErrorInvalidValue;
}

// ff_conv.hip makes the entries: FfEntryT<T> for every window class and pixel type

// ---- what runs before the fused kernel (engine.hip) ------------------------------------------------------------------
// strips[f][strip][row][CH (128 + 2 pada)] samples: the window of an edge chunk with the mirrored pixels in place.  A thread moves
// one sample.
template <typename T, int CH>
__device__ __forceinline__ void ff_edge_strips_body(const T* __restrict__ src, T* __restrict__ strips, int rows, int cols, int pada, int chunks,
                                                    int nright, int bx, int sidx, int f, uint32_t spitch, size_t sframe)
{
    const int win = kFxChunk + 2 * pada, fpr = CH * win;                // samples per strip row
    const int nleft = fx_left_strips(pada);
    const int xc = sidx < nleft ? sidx : chunks - nright + sidx - nleft, x0 = kFxChunk * xc;
    const int i = bx * 256 + threadIdx.x;
    if (i >= rows * fpr) return;
    const int r = i / fpr, e = i - r * fpr, p = e / CH, ch = e - p * CH;
    const T* line = reinterpret_cast<const T*>(reinterpret_cast<const unsigned char*>(src) + static_cast<size_t>(f) * sframe + static_cast<size_t>(r) * spitch);
    strips[((static_cast<size_t>(f) * (nleft + nright) + sidx) * rows + r) * fpr + e] = line[CH * mx_refl(x0 - pada + p, cols) + ch];
}

// The pre-pass's sums for a CH-channel float image: workgroup (band of band_rows rows, batch of G BS elements of a row, frame), BS =
// 256 (CH = 1, 4) or 255 (CH = 3): element j BS + t of the batch belongs to thread t, so that all of a thread's elements are of
// channel t mod CH.  Always: max|x| of the frame into mbits (integer atomicMax on the bits: order-free).  With `sums`: the parts of
// Srow per batch (spart[f][batch][row][CH]) and the column sums per band (cpart), f32 products summed in double, every sum in a
// fixed order.  u16 samples: no max (mbits is not touched); the sums hold integers below 2^53, exact in any order.  float16 /
// bfloat16 samples: widened to f32 (exact), then as float samples.  spitch, sframe: the source's row pitch and frame stride in bytes
// (FwPitch); the outputs stay packed and the partition depends on rows, cols and CH only.
constexpr int kFfSumRows = 16;
__host__ __device__ constexpr int ff_batch_stride(int ch) { return ch == 3 ? 255 : 256; }
inline int ff_groups_per_thread(int cols, int ch)
{
    const int ne = cols * ch, bs = ff_batch_stride(ch);
    return ne <= bs ? 1 : (ne <= 2 * bs ? 2 : 4);
}

template <typename T, int CH, int G>
__device__ __forceinline__ void ff_altsums_body(const T* __restrict__ src, unsigned* __restrict__ mbits, double* __restrict__ spart, double* __restrict__ cpart,
                                                int rows, int cols, int pad, int nbands, int nbatches, int cpitch, int band, int batch, int f, int band_rows, bool sums,
                                                uint32_t spitch, size_t sframe)
{
    constexpr int BS = ff_batch_stride(CH);
    constexpr bool U16 = std::is_same_v<T, uint16_t>;
    if constexpr (U16) {
        if (!sums) return;
    }
    __shared__ double red[kFfSumRows][256];
    __shared__ double red2[kFfSumRows][16][CH];
    __shared__ float wmax[4];
    const int tid = threadIdx.x;
    const uint32_t ne = static_cast<uint32_t>(cols) * CH;
    const __amdgpu_buffer_rsrc_t rimg = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned char*>(reinterpret_cast<const unsigned char*>(src) + static_cast<size_t>(f) * sframe), 0,
        static_cast<uint32_t>(rows - 1) * spitch + ne * static_cast<uint32_t>(sizeof(T)), kMxRsrcWord3);
    const int r0 = band * band_rows, r1 = min(r0 + band_rows, rows);
    int dj[G], wx[G];
    bool own[G];
    double col[G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
        dj[j] = (batch * G + j) * BS + tid;
        own[j] = tid < BS && dj[j] < static_cast<int>(ne);
        wx[j] = own[j] ? mx_alt_weight(dj[j] / CH, cols, pad) : 0;
        col[j] = 0.0;
    }
    float amax = 0.f;
    for (int rs = r0; rs < r1; rs += kFfSumRows) {
        const int re = min(rs + kFfSumRows, r1);
#pragma unroll 4
        for (int r = rs; r < re; ++r) {
            float v[G];
#pragma unroll
            for (int j = 0; j < G; ++j) {
                if constexpr (U16) v[j] = static_cast<float>(__builtin_amdgcn_raw_buffer_load_b16(rimg, own[j] ? static_cast<uint32_t>(r) * spitch + 2u * dj[j] : 0xfffffff0u, 0, 0));
                else if constexpr (ff_is_half_v<T>)
                    v[j] = ff_half_widen<T>(__builtin_amdgcn_raw_buffer_load_b16(rimg, own[j] ? static_cast<uint32_t>(r) * spitch + 2u * dj[j] : 0xfffffff0u, 0, 0));
                else v[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rimg, own[j] ? static_cast<uint32_t>(r) * spitch + 4u * dj[j] : 0xfffffff0u, 0, 0));
            }
            if constexpr (!U16) {
#pragma unroll
                for (int j = 0; j < G; ++j) amax = fmaxf(amax, fabsf(v[j]));
            }
            if (sums) {
                const int wy = mx_alt_weight(r, rows, pad);
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < G; ++j) {
                    s = __builtin_fma(static_cast<double>(wx[j]), static_cast<double>(v[j]), s);
                    col[j] = __builtin_fma(static_cast<double>(wy), static_cast<double>(v[j]), col[j]);
                }
                red[r - rs][tid] = s;
            }
        }
        if (!sums) continue;
        __syncthreads();
        {   // thread (row, part): the 16 entries of its part, by channel; then the 16 parts of (row, channel) in order
            const int rr = tid >> 4, part = tid & 15;
            double pc[CH];
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) pc[ch] = 0.0;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int t = 16 * part + k;
                if (t < BS) pc[t % CH] += red[rr][t];
            }
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) red2[rr][part][ch] = pc[ch];
        }
        __syncthreads();
        if (tid < (re - rs) * CH) {
            const int rr = tid / CH, ch = tid - rr * CH;
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < 16; ++k) v += red2[rr][k][ch];
            spart[((static_cast<size_t>(f) * nbatches + batch) * rows + rs + rr) * CH + ch] = v;
        }
        __syncthreads();
    }
    if (sums) {
#pragma unroll
        for (int j = 0; j < G; ++j)
            if (own[j]) cpart[(static_cast<size_t>(f) * nbands + band) * cpitch + dj[j]] = col[j];
    }
    if constexpr (!U16) {
        // the workgroup's max|x| (NaN: the largest bits) -> one integer atomicMax
        unsigned mb = __float_as_uint(amax);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mb = max(mb, static_cast<unsigned>(__shfl_xor(static_cast<int>(mb), o)));
        if ((tid & 63) == 0) wmax[tid >> 6] = __uint_as_float(mb);
        __syncthreads();
        if (tid == 0) {
            unsigned m4 = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) m4 = max(m4, __float_as_uint(wmax[w]));
            atomicMax(mbits + f, m4);
        }
    }
}

// One launch: the max and (with sums) the quirk's parts (n_alt = bands x batches x frames workgroups), then the edge strips
// (strip_blocks x nstrips x frames workgroups).  Float: mbits must be zero before the launch; u16: mbits is not touched.
template <typename T, int CH, int G>
__global__ __launch_bounds__(256) void ff_prepass(const T* __restrict__ src, unsigned* __restrict__ mbits, double* __restrict__ spart, double* __restrict__ cpart,
                                                  T* __restrict__ strips, int rows, int cols, int pad, int pada, int nbands, int nbatches, int cpitch, int n_alt,
                                                  int chunks, int nright, int strip_blocks, int band_rows, int sums, uint32_t spitch, size_t sframe)
{
    int b = blockIdx.x;
    if (b < n_alt) {
        const int band = b % nbands, batch = (b / nbands) % nbatches, f = b / (nbands * nbatches);
        ff_altsums_body<T, CH, G>(src, mbits, spart, cpart, rows, cols, pad, nbands, nbatches, cpitch, band, batch, f, band_rows, sums != 0, spitch, sframe);
    } else {
        b -= n_alt;
        const int nstrips = fx_left_strips(pada) + nright, bx = b % strip_blocks, sidx = (b / strip_blocks) % nstrips, f = b / (strip_blocks * nstrips);
        ff_edge_strips_body<T, CH>(src, strips, rows, cols, pada, chunks, nright, bx, sidx, f, spitch, sframe);
    }
}

// ff_prepass for a launch over frames with their own sigmas (FwFrame, fw_kernels.hpp: fc_prepass_frames): workgroup frame f of the
// grid is entry f of the list `ft`, the sums are weighted with that frame's pad and read its frame of the source
template <typename T, int CH, int G>
__global__ __launch_bounds__(256) void ff_prepass_frames(const T* __restrict__ src, unsigned* __restrict__ mbits, double* __restrict__ spart, double* __restrict__ cpart,
                                                         T* __restrict__ strips, int rows, int cols, int pada, int nbands, int nbatches, int cpitch, int n_alt,
                                                         int chunks, int nright, int strip_blocks, int band_rows, int sums, uint32_t spitch, size_t sframe,
                                                         const FwFrame* __restrict__ ft)
{
    int b = blockIdx.x;
    const bool alt = b < n_alt;
    if (!alt) b -= n_alt;
    const int nstrips = fx_left_strips(pada) + nright;
    const int f = alt ? b / (nbands * nbatches) : b / (strip_blocks * nstrips);
    // (the bodies address the source as src + f sframe: the frame's own offset less that)
    const T* s = reinterpret_cast<const T*>(reinterpret_cast<const unsigned char*>(src) + (static_cast<ptrdiff_t>(ft[f].frame) - f) * static_cast<ptrdiff_t>(sframe));
    if (alt) {
        const int band = b % nbands, batch = (b / nbands) % nbatches;
        ff_altsums_body<T, CH, G>(s, mbits, spart, cpart, rows, cols, ft[f].pad, nbands, nbatches, cpitch, band, batch, f, band_rows, sums != 0, spitch, sframe);
    } else {
        const int bx = b % strip_blocks, sidx = (b / strip_blocks) % nstrips;
        ff_edge_strips_body<T, CH>(s, strips, rows, cols, pada, chunks, nright, bx, sidx, f, spitch, sframe);
    }
}

// Srow complete (the batches' parts in order) and Z = sum_r wy(r) Srow(r) (a fixed tree): one workgroup per frame
template <int CH>
__device__ __forceinline__ void ff_finalize_body(const double* __restrict__ spart, double* __restrict__ srow, double* __restrict__ zsum, int rows, int pad, int nbatches)
{
    __shared__ double zr[CH][256];
    const int tid = threadIdx.x, f = blockIdx.x;
    double z[CH];
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) z[ch] = 0.0;
    for (int r = tid; r < rows; r += 256) {
        const double wy = static_cast<double>(mx_alt_weight(r, rows, pad));
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) {
            double s = 0.0;
            for (int b = 0; b < nbatches; ++b) s += spart[((static_cast<size_t>(f) * nbatches + b) * rows + r) * CH + ch];
            srow[(static_cast<size_t>(f) * rows + r) * CH + ch] = s;
            z[ch] = __builtin_fma(wy, s, z[ch]);
        }
    }
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) zr[ch][tid] = z[ch];
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w)
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) zr[ch][tid] += zr[ch][tid + w];
        __syncthreads();
    }
    if (tid < CH) zsum[static_cast<size_t>(f) * CH + tid] = zr[tid][0];
}
template <int CH>
__global__ __launch_bounds__(256) void ff_finalize(const double* __restrict__ spart, double* __restrict__ srow, double* __restrict__ zsum, int rows, int pad, int nbatches)
{
    ff_finalize_body<CH>(spart, srow, zsum, rows, pad, nbatches);
}
// the same with the pad of the workgroup's frame from the list of a launch over frames with their own sigmas
template <int CH>
__global__ __launch_bounds__(256) void ff_finalize_frames(const double* __restrict__ spart, double* __restrict__ srow, double* __restrict__ zsum, int rows, int nbatches,
                                                          const FwFrame* __restrict__ ft)
{
    ff_finalize_body<CH>(spart, srow, zsum, rows, ft[blockIdx.x].pad, nbatches);
}

}  // namespace blur_amd
