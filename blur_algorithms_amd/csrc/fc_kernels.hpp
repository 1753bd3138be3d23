// fc_kernels.hpp -- the fused matrix-core kernel for 1- and 4-channel u8 images (grayscale, BGRA / RGBA), every window class
// (NKB = 3 .. 23 blocks of 16 positions: pad <= 168).
//
// The structure is fw_kernels.hpp's: a workgroup handles ONE channel of a strip of 128 pixel columns (the task list has the channel
// as its fastest dimension), stages its window through LDS as binary16 subnormals, runs the row pass, the hand-off inside the
// registers, the sliding column-pass accumulators and the + 0.5f truncation.  What the channel count CH changes:
//   * staging: a group of 4 pixels is 4 CH bytes -- one dword (CH = 1: the bytes are the four values, no deinterleaving) or one
//     dwordx4 (CH = 4: byte c of each of the four dwords) -- instead of three dwords;
//   * stores: CH = 1 transposes a finished tile's bytes inside lane quads (fx_quad_transpose) so that a lane owns 4 adjacent pixels
//     of one row: one dword store per lane and row group instead of four byte stores.  CH = 4 stores single bytes as fw_blur_u8 does
//     (the four channel tasks' stores of a strip meet in L2);
//   * narrow windows: fw_blur_u8 hands the vector work of a step out over the column pass's NKB triples (the hand-off in slots
//     0 .. 7, the emission in 1 .. 4, the staging from slot 5 on) and the stores over the row pass's first four blocks.  Below
//     NKB = 9 there are fewer slots than that: the loops run on past the products, max(NKB, 9) and max(NKB, 4) slots, the ones
//     beyond NKB holding only vector work;
//   * the quirk's sums come from fc_prepass (C channels, below) in a simpler layout: Srow and Z complete (integer atomics), the
//     column sums in parts per band of rows.
// The accumulator budget is fw_kernels.hpp's: (NKB - 1) / 2 <= 11 tiles of one channel.
#pragma once
#include "fw_kernels.hpp"

namespace blur_amd {

// Whole-frame partial sums of the quirk for a CH-channel image (fc_prepass), read by fc_blur_u8:
//   srow [frame][row][CH]             Srow(r, c) = sum_x wx(x) img[r][x][c]          (complete: the batches add with atomics)
//   cpart[frame][band][cpitch]        sum over the band's rows of wy(r) img[r][x][c] at CH x + c
//   zsum [frame][CH]                  Z(c) = sum_r wy(r) Srow(r, c)                  (complete, 64-bit)
struct FcQuirk {
    const int* srow;
    const int* cpart;
    const long long* zsum;
    const float* taps;          // the 2 pad + 1 taps of the row pass, centre at pad
    int nbands, cpitch;
    float dr, dc;
};

// dwords of a row per pre-pass thread: batches of 256 G dwords (G = 1, 2, 4); as many batches as the row needs
inline int fc_groups_per_thread(int cols, int ch)
{
    const int dw = (cols * ch + 3) / 4;
    return dw <= 256 ? 1 : (dw <= 512 ? 2 : 4);
}

// qc[xl] (xl = 0 .. 127) = the column term of pixel x0 + xl in channel c0, 0 right of the image (fx_quirk_cols_tile for a
// CH-channel layout and one channel).  256 threads; `scratch` = LDS for (128 + 2 pad) + 2 pad + 1 doubles; ends with a barrier.
template <int CH>
__device__ __forceinline__ void fc_quirk_cols_tile(unsigned char* scratch, float* qc, const FcQuirk& q, int f, int x0, int c0, int cols, int pad, int tid)
{
    const int win = kFxChunk + 2 * pad, ntap = 2 * pad + 1;
    double* cc = reinterpret_cast<double*>(scratch);
    double* tp = cc + win;
    const int* base = q.cpart + static_cast<size_t>(f) * q.nbands * q.cpitch + c0;
    for (int p = tid; p < win; p += 256) {
        const int* cp = base + CH * mx_refl(x0 - pad + p, cols);
        int sum = 0;
        int b = 0;
        for (; b + 8 <= q.nbands; b += 8) {
            int t[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) t[j] = cp[static_cast<size_t>(b + j) * q.cpitch];
#pragma unroll
            for (int j = 0; j < 8; ++j) sum += t[j];
        }
        for (; b < q.nbands; ++b) sum += cp[static_cast<size_t>(b) * q.cpitch];
        cc[p] = static_cast<double>(sum);
    }
    for (int i = tid; i < ntap; i += 256) tp[i] = static_cast<double>(q.taps[i]);
    __syncthreads();
    const double sp = (pad & 1) ? -1.0 : 1.0, z = static_cast<double>(q.zsum[static_cast<size_t>(f) * CH + c0]);
    if (tid < kFxChunk) {
        const int x = x0 + tid;
        float out = 0.f;
        if (x < cols) {
            const double* ccx = cc + tid;                                    // tap t = -pad sits here
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
template <int NKB, bool QUIRK, int CH>
__global__ __launch_bounds__(256, 1) void fc_blur_u8(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const mx_half8* __restrict__ frags, FxGeom g,
                                                     int chunks, int tps, int nseg, int ntasks, FcQuirk qk, const uint8_t* __restrict__ strips)
{
    static_assert(CH == 1 || CH == 4, "one or four channels (three: fx_blur_u8 / fw_blur_u8)");
    using C = FwCfg<NKB>;
    constexpr int PADA = C::PADA, PW = C::PW, NT = C::NT, PER = C::PER;
    constexpr int RS = NKB > 4 ? NKB : 4;                         // row-pass slots: the stores of the previous tile need four
    constexpr int CS = NKB > 9 ? NKB : 9;                         // column-pass slots: hand-off 0 .. 7, emission 1 .. 4, staging from 5
    constexpr int IPS = (PER + CS - 6) / (CS - 5);                // staging items per column-pass slot from slot 5 on
    extern __shared__ __attribute__((aligned(16))) unsigned char fc_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = lane & 31, h = lane >> 5;

    const int nx = g.nxcd, xcd = blockIdx.x % nx, in_xcd = blockIdx.x / nx, per_xcd = (ntasks + nx - 1) / nx, task = xcd * per_xcd + in_xcd;
    if (in_xcd >= per_xcd || task >= ntasks) return;
    const int c = task % CH, xc = (task / CH) % chunks, seg = (task / (CH * chunks)) % nseg, f = task / (CH * chunks * nseg);
    const int x0 = xc * kFxChunk;
    const int tile0 = seg * tps, tile1 = min(tile0 + tps, g.ntiles);
    const uint8_t* img = src + static_cast<size_t>(f) * g.rows * g.cols * CH;
    uint8_t* out = dst + static_cast<size_t>(f) * g.rows * g.cols * CH;

    constexpr int TLR = FW_TL_REGS < NKB ? FW_TL_REGS : NKB;
    mx_half8 th[NKB], tlr[TLR > 0 ? TLR : 1];
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) th[kb] = frags[kb * 64 + lane];
#pragma unroll
    for (int kb = 0; kb < TLR; ++kb) tlr[kb] = frags[(NKB + kb) * 64 + lane];
    {
        mx_half8* tls = reinterpret_cast<mx_half8*>(fc_lds + C::TLOFF);
        for (int i = tid; i < NKB * 64; i += 256) tls[i] = frags[NKB * 64 + i];
    }
    const mx_half8* tlp = reinterpret_cast<const mx_half8*>(fc_lds + C::TLOFF) + lane;
    auto tlo = [&](int kb) __attribute__((always_inline)) { return kb < TLR ? tlr[kb < TLR ? kb : 0] : tlp[kb * 64]; };

    float cpos = 0.5f, cneg = 0.5f;
    if (QUIRK) {
        static_assert(C::BUF >= 8 * (C::WIN + 2 * C::PADA + 1) && C::BUF >= 4 * kFxChunk, "fc_quirk_cols_tile's scratch and result fit the window buffers");
        float* qc = reinterpret_cast<float*>(fc_lds + C::BUF);
        fc_quirk_cols_tile<CH>(fc_lds, qc, qk, f, x0, c, g.cols, g.pad, tid);
        const float v = qc[32 * wave + m];
        cpos = 0.5f + v;
        cneg = 0.5f - v;
        __syncthreads();
    }
    const int qrows = 32 * (g.ntiles + NT);
    const double qrs = QUIRK ? static_cast<double>(qk.dr) * ((g.pad & 1) ? -1.0 : 1.0) : 0.0;

    const mx_float16 zero = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
    mx_float16 acc[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) acc[k] = zero;
    mx_float16 arow = zero, tfin = zero;
    uint32_t hl[2][2][8];
    uint32_t rr[4];

    const int s0 = tile0, s1 = tile1 + NT;
    constexpr int NLEFT = fx_left_strips(PADA);
    const int sidx = xc < NLEFT ? xc : (xc >= chunks - g.nright ? NLEFT + xc - (chunks - g.nright) : -1);      // uniform
    const uint32_t pitch = sidx >= 0 ? static_cast<uint32_t>(CH * C::WIN) : static_cast<uint32_t>(CH) * static_cast<uint32_t>(g.cols);
    const uint8_t* wbase = sidx >= 0 ? strips + (static_cast<size_t>(f) * (NLEFT + g.nright) + sidx) * g.rows * (CH * C::WIN) : img + CH * (x0 - PADA);
    const uint32_t wbytes = sidx >= 0 ? static_cast<uint32_t>(g.rows) * static_cast<uint32_t>(CH * C::WIN)
                                      : (static_cast<uint32_t>(g.rows) * g.cols - static_cast<uint32_t>(x0 - PADA)) * static_cast<uint32_t>(CH);
    const __amdgpu_buffer_rsrc_t rimg = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(wbase), 0, wbytes, kMxRsrcWord3);
    const int srow = 8 * (tid >> 6) + ((tid >> 4) & 3) + 4 * ((tid >> 3) & 1), g0 = tid & 7;      // (fx_kernels.hpp: the staging map)
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    uint32_t raw[PER][CH];
    int qv = 0;
    // the window of step s: thread t moves the groups of 4 pixels g0 + 8 k of row srow, all requested at once
    auto issue_window = [&](int s) __attribute__((always_inline)) {
        const int r = mx_refl(32 * s - PADA + srow, g.rows);
        const uint32_t off = static_cast<uint32_t>(r) * pitch + static_cast<uint32_t>(4 * CH * g0);
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const bool in = (C::GPR % 8 == 0) || k < PER - 1 || g0 < C::GPR % 8;
            const uint32_t o = in ? off + static_cast<uint32_t>(32 * CH * k) : off;
            if (CH == 1) {
                raw[k][0] = __builtin_amdgcn_raw_buffer_load_b32(rimg, o, 0, 0);
            } else {
                const u4 t = __builtin_amdgcn_raw_buffer_load_b128(rimg, o, 0, 0);
#pragma unroll
                for (int j = 0; j < CH; ++j) raw[k][j] = t[j];
            }
        }
        if (QUIRK)              // the row term of row re of V (= image row refl(re - PADA)); every thread (row tid & 31: eight copies of each value)
            qv = qk.srow[(static_cast<size_t>(f) * g.rows + mx_refl(min(32 * s + (tid & 31), qrows - 1) - PADA, g.rows)) * CH + c];
    };
    // channel c of group k -> binary16 subnormals -> LDS: two v_perm_b32 and one ds_write_b64
    const uint32_t sel4 = 0x0c000c00u | (static_cast<uint32_t>(4 + c) << 16) | static_cast<uint32_t>(c);
    auto commit_item = [&](int buf, int k) __attribute__((always_inline)) {
        if (k >= PER) return;
        _Float16* base = reinterpret_cast<_Float16*>(fc_lds + buf * C::BUF) + srow * PW + 4 * g0;
        uint2 wd;
        if (CH == 1) {
            wd.x = __builtin_amdgcn_perm(0u, raw[k][0], 0x0c010c00u);
            wd.y = __builtin_amdgcn_perm(0u, raw[k][0], 0x0c030c02u);
        } else {
            wd.x = __builtin_amdgcn_perm(raw[k][1 % CH], raw[k][0], sel4);
            wd.y = __builtin_amdgcn_perm(raw[k][3 % CH], raw[k][2 % CH], sel4);
        }
        *reinterpret_cast<uint2*>(base + 32 * k) = wd;
    };
    auto commit_q = [&](int buf) __attribute__((always_inline)) {
        if (QUIRK) {
            const float qraw = static_cast<float>(qrs * qv);
            float* qs = reinterpret_cast<float*>(fc_lds + C::QOFF) + buf * 64 + (tid & 31);
            qs[0] = qraw;
            qs[32] = -qraw;
        }
    };
    // R: the window in buffer `buf` -> arow; `beside(kb)` runs after the products of slot kb
    auto rowpass = [&](int buf, auto beside) __attribute__((always_inline)) {
        const _Float16* base = reinterpret_cast<const _Float16*>(fc_lds + buf * C::BUF) + m * PW + wave * 32 + 8 * h;
        mx_float16 a = zero;
        mx_half8 x[4], tq[3];
#pragma unroll
        for (int kb = 0; kb < 3 && kb < NKB; ++kb) x[kb] = *reinterpret_cast<const mx_half8*>(base + 16 * kb);
        tq[0] = tlo(0);
        tq[1] = tlo(1);
#pragma unroll
        for (int kb = 0; kb < RS; ++kb) {
            if (kb < NKB) {
                if (kb + 3 < NKB) x[(kb + 3) & 3] = *reinterpret_cast<const mx_half8*>(base + 16 * (kb + 3));
                if (kb + 2 < NKB) tq[(kb + 2) % 3] = tlo(kb + 2);
                a = __builtin_amdgcn_mfma_f32_32x32x16_f16(x[kb & 3], th[kb], a, 0, 0, 0);
                a = __builtin_amdgcn_mfma_f32_32x32x16_f16(x[kb & 3], tq[kb % 3], a, 0, 0, 0);
                asm volatile("" : "+a"(a));
            }
            beside(kb);
            __builtin_amdgcn_sched_barrier(0);
        }
        arow = a;
    };
    // S: arow -> scale (+ quirk), split into hi + lo, exchange with lane ^ 32 -> hl[hb] (fw_kernels.hpp: split_piece)
    float sv[16];
    auto split_piece = [&](int buf, int hb, int piece) __attribute__((always_inline)) {
        const int hf = piece >> 2, sub = piece & 3;
        uint32_t (&hp)[8] = hl[hb][0];
        uint32_t (&lp)[8] = hl[hb][1];
        if (sub == 0) {
            if (QUIRK) {
                const float* qs4 = reinterpret_cast<const float*>(fc_lds + C::QOFF) + buf * 64 + (m & 1) * 32 + 4 * h;
#pragma unroll
                for (int k = 2 * hf; k < 2 * hf + 2; ++k) {
                    const float4 t4 = *reinterpret_cast<const float4*>(qs4 + 8 * k);
                    sv[4 * k] = __builtin_fmaf(arow[4 * k], kFxRowUnscale, t4.x);
                    sv[4 * k + 1] = __builtin_fmaf(arow[4 * k + 1], kFxRowUnscale, t4.y);
                    sv[4 * k + 2] = __builtin_fmaf(arow[4 * k + 2], kFxRowUnscale, t4.z);
                    sv[4 * k + 3] = __builtin_fmaf(arow[4 * k + 3], kFxRowUnscale, t4.w);
                }
            } else {
#pragma unroll
                for (int k = 8 * hf; k < 8 * hf + 8; ++k) sv[k] = arow[k] * kFxRowUnscale;
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
    // E: rows 8 gq + 4 h + 0 .. 3 of the lane's pixel column -> bytes.  CH = 1: then transposed inside the lane quad: lane q of quad
    // Q holds row 8 gq + 4 h + q, pixels 4 Q .. 4 Q + 3 of the wave's 32
    const uint32_t sel1 = (lane & 1) ? 0x03070105u : 0x06020400u, sel2 = (lane & 2) ? 0x03020706u : 0x05040100u;
    auto emit_piece = [&](int gq) __attribute__((always_inline)) {
        float fv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int reg = 4 * gq + k;
            fv[k] = __builtin_fmaf(tfin[reg], kMxUnscale, (reg & 1) ? cneg : cpos);
        }
        // (uint8_t)(v + 0.5f) of the reference (Utils.hpp:189,204-206): truncate, keep the low byte
        const uint32_t b0 = static_cast<uint32_t>(static_cast<int>(fv[0])) & 0xffu, b1 = static_cast<uint32_t>(static_cast<int>(fv[1])) & 0xffu;
        const uint32_t b2 = static_cast<uint32_t>(static_cast<int>(fv[2])) & 0xffu, b3 = static_cast<uint32_t>(static_cast<int>(fv[3]));
        const uint32_t pk = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
        rr[gq] = CH == 1 ? fx_quad_transpose(pk, sel1, sel2) : pk;
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
    // F: the finished tile's bytes.  Buffer stores: rows past the image, pixels right of it and tiles that do not exist get an
    // offset outside the resource
    const __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc(out, 0, static_cast<uint32_t>(g.rows) * g.cols * static_cast<uint32_t>(CH), kMxRsrcWord3);
    const uint32_t rowstep = static_cast<uint32_t>(g.cols) * CH;
    const int xcol = x0 + 32 * wave + m;                                  // CH = 4: the lane's pixel column
    const int xq = x0 + 32 * wave + 4 * (m >> 2), q = m & 3;                // CH = 1: first pixel of the lane's quad, its row in the row group
    const bool ragged = (g.cols & 3) != 0;                                // (uniform) CH = 1: the quad cut by the right edge leaves as bytes
    const int qn = xq >= g.cols ? 0 : min(4, g.cols - xq);                // pixels of the lane's quad inside the image
    auto store_group = [&](int tile, bool valid, int gq) __attribute__((always_inline)) {
        const uint32_t v = rr[gq];
        if (CH == 1) {
            const int row = 32 * tile + 8 * gq + 4 * h + q;
            const bool rok = valid && row < g.rows;
            const uint32_t o = static_cast<uint32_t>(row) * rowstep + static_cast<uint32_t>(xq);
            __builtin_amdgcn_raw_buffer_store_b32(v, rout, rok && qn == 4 ? o : 0xfffffff0u, 0, 0);
            if (ragged) {
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    __builtin_amdgcn_raw_buffer_store_b8(static_cast<uint8_t>(v >> (8 * k)), rout, rok && qn < 4 && k < qn ? o + k : 0xfffffff0u, 0, 0);
            }
        } else {
            const int row0 = 32 * tile + 8 * gq + 4 * h;
            const uint32_t base = (static_cast<uint32_t>(row0) * g.cols + static_cast<uint32_t>(xcol)) * CH + static_cast<uint32_t>(c);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool ok = valid && xcol < g.cols && row0 + k < g.rows;
                __builtin_amdgcn_raw_buffer_store_b8(static_cast<uint8_t>(v >> (8 * k)), rout, ok ? base + k * rowstep : 0xfffffff0u, 0, 0);
            }
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

    // step s: the row pass of step s + 1, then the column pass of step s, the vector work beside the products (fw_kernels.hpp)
    auto step = [&](int s, int qs, int ri) __attribute__((always_inline)) {
        const int par = (s - s0) & 1;
        const int ptile = s - 1 - NT;
        const bool pvalid = ptile >= tile0 && s > s0;
        issue_window(s + 2);
        rowpass(par ^ 1, [&](int kb) __attribute__((always_inline)) {
            if (kb < 4) store_group(ptile, pvalid, kb);
        });
        colpass(qs, 0, ri, [&](int it) __attribute__((always_inline)) {
            if (it < 8) split_piece(par ^ 1, 1, it);
            if (it >= 1 && it <= 4) emit_piece(it - 1);
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
    {
        const int ltile = s1 - 1 - NT;
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) store_group(ltile, ltile >= tile0, gq);
    }
}

struct FcEntry {
    int nkb;
    // ch: 1 or 4; qk: the quirk's sums (null: nyquist_quirk = 0)
    hipError_t (*blur_u8)(hipStream_t, const uint8_t* src, uint8_t* dst, const void* frags, FxGeom g, int ch, int num_cus, const FcQuirk* qk, const uint8_t* strips);
};

template <int NKB, int CH> hipError_t fc_launch_ch(hipStream_t st, const uint8_t* src, uint8_t* dst, const void* frags, FxGeom g, int num_cus, const FcQuirk* qk,
                                                   const uint8_t* strips)
{
    using C = FwCfg<NKB>;
    const FxLaunch l = fx_plan_launch(g, CH, C::NT, num_cus);
    if (l.ntasks == 0) return hipSuccess;
    static std::atomic<unsigned long long> attr_done{ 0 };
    const hipError_t e = fx_set_lds(attr_done, C::LDS, fc_blur_u8<NKB, true, CH>, fc_blur_u8<NKB, false, CH>);
    if (e != hipSuccess) return e;
    if (qk)
        hipLaunchKernelGGL((fc_blur_u8<NKB, true, CH>), l.grid, dim3(256), C::LDS, st, src, dst, static_cast<const mx_half8*>(frags), g, l.chunks, l.tps,
                           l.nseg, static_cast<int>(l.ntasks), *qk, strips);
    else
        hipLaunchKernelGGL((fc_blur_u8<NKB, false, CH>), l.grid, dim3(256), C::LDS, st, src, dst, static_cast<const mx_half8*>(frags), g, l.chunks, l.tps,
                           l.nseg, static_cast<int>(l.ntasks), FcQuirk{}, strips);
    return hipGetLastError();
}

template <int NKB> hipError_t fc_launch_u8(hipStream_t st, const uint8_t* src, uint8_t* dst, const void* frags, FxGeom g, int ch, int num_cus, const FcQuirk* qk,
                                           const uint8_t* strips)
{
    if (ch == 1) return fc_launch_ch<NKB, 1>(st, src, dst, frags, g, num_cus, qk, strips);
    if (ch == 4) return fc_launch_ch<NKB, 4>(st, src, dst, frags, g, num_cus, qk, strips);
    return hipErrorInvalidValue;
}

#define BLUR_FC(NKB_)                                                                                       \
    namespace blur_amd {                                                                                    \
    const FcEntry* fc_entry_##NKB_()                                                                        \
    {                                                                                                       \
        static const FcEntry e = { NKB_, fc_launch_u8<NKB_> };                                              \
        return &e;                                                                                          \
    }                                                                                                       \
    }

// ---- what runs before the fused kernel (engine.hip) ------------------------------------------------------------------
// strips[f][strip][row][CH (128 + 2 pada)]: the window of an edge chunk with the mirrored pixels in place (fx_edge_strips_body for
// CH channels; the CH-channel kernel reads the whole window of an edge chunk from its strip).  A thread writes one dword.
template <int CH>
__device__ __forceinline__ void fc_edge_strips_body(const uint8_t* __restrict__ src, uint8_t* __restrict__ strips, int rows, int cols, int pada, int chunks,
                                                    int nright, int bx, int sidx, int f)
{
    const int win = kFxChunk + 2 * pada, dpr = CH * win / 4;            // dwords per strip row (win is a multiple of 4)
    const int nleft = fx_left_strips(pada);
    const int xc = sidx < nleft ? sidx : chunks - nright + sidx - nleft, x0 = kFxChunk * xc;
    const int i = bx * 256 + threadIdx.x;
    if (i >= rows * dpr) return;
    const int r = i / dpr, d = i - r * dpr;
    const uint8_t* line = src + (static_cast<size_t>(f) * rows + r) * cols * CH;
    uint32_t o = 0;
    const int X = x0 - pada + (CH == 1 ? 4 * d : d);                   // first pixel of the dword's window position
    if (CH == 4) o = *reinterpret_cast<const uint32_t*>(line + 4 * mx_refl(X, cols));
    else if (X >= 0 && X + 3 < cols) o = *reinterpret_cast<const uint32_t*>(line + X);
    else {                                                             // a mirrored pixel (or past one reflection): byte by byte
#pragma unroll
        for (int k = 0; k < 4; ++k) o |= static_cast<uint32_t>(line[mx_refl(X + k, cols)]) << (8 * k);
    }
    *reinterpret_cast<uint32_t*>(strips + ((static_cast<size_t>(f) * (nleft + nright) + sidx) * rows + r) * (CH * win) + 4 * d) = o;
}

// The quirk's sums (FcQuirk) for a CH-channel image: workgroup (band of band_rows rows, batch of 256 G dwords of a row, frame).
// A thread owns G dwords of every row of the band: CH = 1 four pixels, CH = 4 one pixel's four channels.  Exact integers; srow and
// zsum must be zero before the launch (they are completed with atomics).  sred[row][channel][lane]: lane l of every wave adds
// into slot l (fx_altsums_body).
constexpr int kFcSumRows = 32;
template <int CH, int G>
__device__ __forceinline__ void fc_altsums_body(const uint8_t* __restrict__ src, int* __restrict__ srow, int* __restrict__ cpart, long long* __restrict__ zsum,
                                                int rows, int cols, int pad, int nbands, int cpitch, int band, int batch, int f, int (*sred)[CH][64], int band_rows)
{
    const int tid = threadIdx.x;
    const uint32_t rowbytes = static_cast<uint32_t>(cols) * CH;
    const __amdgpu_buffer_rsrc_t rimg = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(src + static_cast<size_t>(f) * rows * rowbytes), 0,
                                                                          static_cast<uint32_t>(rows) * rowbytes, kMxRsrcWord3);
    const int ndw = static_cast<int>((rowbytes + 3) / 4), r0 = band * band_rows, r1 = min(r0 + band_rows, rows);
    // a row that is no multiple of 4 bytes (cols * CH >= 4): its last dword is loaded `over` bytes early and shifted down, so that no
    // load reaches past the row (the last row's would leave the buffer resource, which returns 0 for the WHOLE dword)
    const int over = 4 * ndw - static_cast<int>(rowbytes);
    int dj[G], wx[G][4], col[G][4], back[G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
        dj[j] = (batch * G + j) * 256 + tid;
        back[j] = dj[j] == ndw - 1 ? over : 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int b = 4 * dj[j] + k, x = CH == 1 ? b : dj[j];          // pixel of byte k of the dword
            wx[j][k] = dj[j] < ndw && b < static_cast<int>(rowbytes) ? mx_alt_weight(x, cols, pad) : 0;
            col[j][k] = 0;
        }
    }
    for (int rs = r0; rs < r1; rs += kFcSumRows) {
        const int re = min(rs + kFcSumRows, r1);
        for (int i = tid; i < kFcSumRows * CH * 64; i += 256) (&sred[0][0][0])[i] = 0;
        __syncthreads();
        constexpr int RB = G == 1 ? 8 : (G == 2 ? 4 : 2);                  // rows of loads in flight
        for (int rb = rs; rb < re; rb += RB) {
            uint32_t d[RB][G];
#pragma unroll
            for (int i = 0; i < RB; ++i) {
                const uint32_t roff = static_cast<uint32_t>(min(rb + i, re - 1)) * rowbytes;
#pragma unroll
                for (int j = 0; j < G; ++j)
                    d[i][j] = __builtin_amdgcn_raw_buffer_load_b32(rimg, dj[j] < ndw ? roff + 4u * dj[j] - back[j] : 0xfffffff0u, 0, 0) >> (8 * back[j]);
            }
#pragma unroll
            for (int i = 0; i < RB; ++i) {
                const int r = rb + i;
                if (r >= re) break;                                                // uniform
                const int wy = mx_alt_weight(r, rows, pad);
                int s[CH];
#pragma unroll
                for (int ch = 0; ch < CH; ++ch) s[ch] = 0;
#pragma unroll
                for (int j = 0; j < G; ++j)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int v = wx[j][k] != 0 ? static_cast<int>((d[i][j] >> (8 * k)) & 0xffu) : 0;      // (bytes of the next row: weight 0)
                        s[CH == 1 ? 0 : k % CH] += wx[j][k] * v;
                        col[j][k] += wy * v;
                    }
#pragma unroll
                for (int ch = 0; ch < CH; ++ch) atomicAdd(&sred[r - rs][ch][tid & 63], s[ch]);
            }
        }
        __syncthreads();
        if (tid < (re - rs) * CH) {
            const int rr = tid / CH, ch = tid - rr * CH;
            const int* p64 = &sred[rr][ch][0];
            int v = 0;
#pragma unroll 8
            for (int k = 0; k < 64; ++k) v += p64[(k + tid) & 63];
            atomicAdd(&srow[(static_cast<size_t>(f) * rows + rs + rr) * CH + ch], v);
            atomicAdd(reinterpret_cast<unsigned long long*>(&zsum[static_cast<size_t>(f) * CH + ch]),
                      static_cast<unsigned long long>(static_cast<long long>(mx_alt_weight(rs + rr, rows, pad)) * v));
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < G; ++j)
        if (4 * dj[j] < cpitch)
            *reinterpret_cast<int4*>(cpart + (static_cast<size_t>(f) * nbands + band) * cpitch + 4 * dj[j]) = make_int4(col[j][0], col[j][1], col[j][2], col[j][3]);
}

// One launch: the quirk's sums (n_alt = bands x batches x frames workgroups, none with nyquist_quirk = 0), then the edge strips
// (strip_blocks x nstrips x frames workgroups)
template <int CH, int G>
__global__ __launch_bounds__(256) void fc_prepass(const uint8_t* __restrict__ src, int* __restrict__ srow, int* __restrict__ cpart, long long* __restrict__ zsum,
                                                  uint8_t* __restrict__ strips, int rows, int cols, int pad, int pada, int nbands, int nbatches, int cpitch, int n_alt,
                                                  int chunks, int nright, int strip_blocks, int band_rows)
{
    __shared__ int sred[kFcSumRows][CH][64];
    int b = blockIdx.x;
    if (b < n_alt) {
        const int band = b % nbands, batch = (b / nbands) % nbatches, f = b / (nbands * nbatches);
        fc_altsums_body<CH, G>(src, srow, cpart, zsum, rows, cols, pad, nbands, cpitch, band, batch, f, sred, band_rows);
    } else {
        b -= n_alt;
        const int nstrips = fx_left_strips(pada) + nright, bx = b % strip_blocks, sidx = (b / strip_blocks) % nstrips, f = b / (strip_blocks * nstrips);
        fc_edge_strips_body<CH>(src, strips, rows, cols, pada, chunks, nright, bx, sidx, f);
    }
}

}  // namespace blur_amd
