// fw_kernels.hpp -- the fused matrix-core kernel that gives a workgroup ONE channel of its strip: u8 images of CH = 1, 2, 3 or 4
// channels (grayscale, the interleaved Cb/Cr plane of an NV12 surface, BGR, BGRA / RGBA), every window class (NKB = 3 .. 23 blocks
// of 16 positions: pad <= 168).  Whole BGR frames with one sigma take CH = 3 for the WIDE windows only (NKB = 13 .. 23: pad 73 .. 168; narrower BGR windows run on fx_blur_u8); the
// narrow CH = 3 instantiations serve the launches over a subset of the channels (one sigma per channel: FwChSel, Fw3Entry).
//
// fx_kernels.hpp keeps (NKB - 1) / 2 column-pass accumulator tiles per channel and a wave carries all three channels: 240 AGPRs at
// NKB = 11 and no room beyond.  Here a workgroup handles ONE channel of its strip of 128 pixel columns -- the task list has the
// channel as its fastest dimension, so the CH channel tasks of a strip run at the same time on neighbouring CUs of one XCD and
// share the window's cache lines -- which leaves (NKB - 1) / 2 <= 11 tiles = 176 AGPRs.  Everything else is the structure of
// fx_kernels.hpp: window of the next step staged through LDS (binary16 subnormals straight from the bytes), row pass
// D[32 rows][32 pixels] = window x Toeplitz fragments, hand-off inside the registers (scale, quirk term, hi + lo split,
// v_permlane32_swap), sliding column-pass accumulators, emission with + 0.5f truncation.  Differences:
//   * the hi halves of the fragments live in registers (4 NKB of them), the lo halves in LDS (one ds_read_b128 per use);
//   * one product per step instead of three, and it is long (5 NKB = 115 matrix instructions at NKB = 23): the vector work of a
//     step (staging, the hand-off, the emission) is handed out between the products in a few places instead of instruction by
//     instruction.
// What the channel count CH selects, at compile time:
//   * staging: a group of 4 pixels is 4 CH bytes: one dword (CH = 1: the bytes are the four values), three dwords (CH = 3: two
//     v_perm_b32 with run-time selectors, the channel is the task's), one dwordx4 (CH = 4: byte c of each dword) or one dwordx2
//     (CH = 2: bytes c and 2 + c of each dword);
//   * the quirk's sums: CH = 3 reads fx_prepass's (struct FxQuirk: Srow in parts per batch, the column term by
//     fx_quirk_cols_tile), CH = 1, 2 and 4 those of fc_prepass below (struct FcQuirk: Srow complete, fc_quirk_cols_tile);
//   * stores: CH = 1 transposes a finished tile's bytes inside lane quads (fx_quad_transpose) so that a lane owns 4 adjacent pixels
//     of one row: one dword store per lane and row group.  CH = 2, 3 and 4 store single bytes: the output bytes of one channel are
//     every CH-th byte of the image (the channel tasks' stores meet in L2 before the lines go to memory);
//   * narrow windows: the vector work of a step goes out over the column pass's NKB triples (the hand-off in
//     slots 0 .. 7, the emission in 1 .. 4, the staging from slot 5 on) and the stores over the row pass's first four blocks.
//     Below NKB = 9 there are fewer slots than that: the loops run on past the products, max(NKB, 9) and max(NKB, 4) slots, the
//     ones beyond NKB holding only vector work.
#pragma once
#include "fx_kernels.hpp"
#include <cstddef>
#include <type_traits>

#ifndef FW_TL_REGS
#define FW_TL_REGS 12     // lo halves of the fragments kept in registers (the others are read from LDS at every use; 8 -> 12 in round 4: +1.5 % at 4K, 16 the same)
#endif

namespace blur_amd {

// The channels a launch works on (blur_gaussian_*_sigmas_*: the channels that share one sigma), packed into one kernel argument
// (uniform: it stays in scalar registers): the count n in bits 0 .. 2, the i-th active channel in bits 4 + 2 i, 5 + 2 i.  The task
// list runs over (frame, segment, chunk, active channel); the layout's stride stays CH and the quirk's sums are indexed by the real
// channel.  fw_chsel_all(CH) gives the task order of a launch over every channel.
typedef uint32_t FwChSel;
constexpr FwChSel fw_chsel_all(int ch) { return static_cast<FwChSel>(ch) | (ch > 1 ? 0xe40u : 0u); }      // channels 0, 1, 2, 3 in order
inline FwChSel fw_chsel_mask(unsigned mask, int ch)
{
    FwChSel s = 0;
    int n = 0;
    for (int c = 0; c < ch; ++c)
        if (mask >> c & 1u) s |= static_cast<FwChSel>(c) << (4 + 2 * n++);
    return s | static_cast<FwChSel>(n);
}
__host__ __device__ constexpr int fw_chsel_count(FwChSel s) { return static_cast<int>(s & 7u); }
inline unsigned fw_chsel_bits(FwChSel s)                                                                   // bit c: channel c is active
{
    unsigned m = 0;
    for (int i = 0; i < fw_chsel_count(s); ++i) m |= 1u << ((s >> (4 + 2 * i)) & 3u);
    return m;
}

// Where the rows and the frames of a launch lie, in bytes (fw_blur_u8, ff_blur and their pre-passes): row r of frame f of the
// source starts at f src_frame + r src_pitch, of the destination at f dst_frame + r dst_pitch.  A packed frame has pitch = cols CH
// ES and frame = rows pitch; a pitched surface or a region of interest inside a larger image has more.  The pitches go into the
// 32-bit offsets of the buffer resources (a frame's span, (rows - 1) pitch + cols CH ES, fits them), the frame strides into the
// 64-bit base.  The bytes between two rows lie INSIDE the resources: loads may return them (they land where the next row's bytes
// land in a packed frame: in padding, or under a weight of 0), stores are masked by x < cols and never reach them.
struct FwPitch {
    uint32_t src_pitch, dst_pitch;
    size_t src_frame, dst_frame;
};
inline FwPitch fw_pitch_packed(int rows, int cols, int ch, int es)
{
    const uint32_t pitch = static_cast<uint32_t>(cols) * static_cast<uint32_t>(ch * es);
    return FwPitch{ pitch, pitch, static_cast<size_t>(rows) * pitch, static_cast<size_t>(rows) * pitch };
}

// One frame of a launch over frames that each have their own sigma (blur_gaussian_*_frame_sigmas_*: the frames of one window class
// share a launch).  The launch's frame list `ft` has one entry per task frame; a null list is a launch with one sigma, whose pad,
// fragments, taps and gains are the launch-wide arguments.  The kernels read the entry once, in the prologue, with scalar loads (the
// task's frame is uniform); the step loop knows the window class only.  Position f in the list indexes everything the group's
// pre-pass made (strips, the quirk's sums, max|x|); `frame` is the frame's index in the call and addresses the source and destination.
// The fragments and taps of every frame of a call lie in one table: `frags` (in mx_half8) and `taps` (in floats) count from its start,
// which the launch passes where a launch with one sigma passes the fragments and the taps.
struct FwFrame {
    int frame;
    int pad;
    uint32_t frags, taps;
    float dr, dc;               // the quirk's gains for this sigma (FcQuirk, FxQuirk, FfQuirk)
    double bscale;              // float frames: B of ff_scale_exp (FfQuirk)
};
static_assert(sizeof(FwFrame) == 32, "eight dwords: one scalar load");

template <int NKB> struct FwCfg {
    static constexpr int PADA = 8 * (NKB - 2), WIN = kFxChunk + 2 * PADA, GPR = WIN / 4, PER = (GPR + 7) / 8;
    // halfs per LDS row of the window: every thread commits PER groups of 4 positions, 32 apart, without a lane mask (fx_kernels.hpp:
    // FxCfg -- a masked commit is a branch in the middle of a slice of matrix instructions), so a row holds 32 PER positions; the
    // pitch is 4 mod 8 dwords (conflict-free ds_read_b128, and ds_write_b64 with the staging rows of a 16-lane group 4 apart)
    static constexpr int fw_pitch() { int dw = 16 * PER; while ((dw & 7) != 4) ++dw; return 2 * dw; }
    static constexpr int PW = fw_pitch();
    static constexpr int NT = (NKB - 1) / 2;                          // live accumulator tiles = steps per unrolled round
    static constexpr int BUF = 32 * PW * 2;                           // bytes of one window buffer (one channel)
    static constexpr int TLOFF = 2 * BUF;                             // lo halves of the fragments: [NKB][64 lanes] x 16 bytes
    static constexpr int QOFF = TLOFF + NKB * 64 * 16;                // qrow stage: [2 buffers][x even, odd: +q, -q][32] floats
    static constexpr int LDS = QOFF + 2 * 2 * 32 * 4;
};

// Whole-frame partial sums of the quirk for a 1-, 2- or 4-channel image (fc_prepass), read by fw_blur_u8<NKB, true, 1 / 2 / 4>:
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

// the quirk's sums the kernel reads: fx_prepass's for three channels, fc_prepass's for one, two and four
template <int CH> using FwQuirk = std::conditional_t<CH == 3, FxQuirk, FcQuirk>;

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
// FRAMES: a launch over frames with their own sigmas (FwFrame), its list in `ft`; without, `ft` is an empty argument and the kernel
// is the one it was.  Two instantiations and not one kernel with a nullable list (as ff_blur has it, at no cost): that form cost the
// quirk instantiations here 1 .. 10 more spilled scalar registers each (they sit at the limit of 106 with 25 .. 32 spilled), and so
// did a shared inlined body under two kernels.
struct FwNoFrames {};
template <bool FRAMES> using FwFrameList = std::conditional_t<FRAMES, const FwFrame*, FwNoFrames>;
template <int NKB, bool QUIRK, int CH, bool FRAMES = false>
__global__ __launch_bounds__(256, 1) void fw_blur_u8(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const mx_half8* __restrict__ frags, FxGeom g,
                                                     int chunks, int tps, int nseg, int ntasks, FwQuirk<CH> qk, const uint8_t* __restrict__ strips, FwChSel chsel, FwPitch pt,
                                                     FwFrameList<FRAMES> ft)
{
    static_assert(CH >= 1 && CH <= 4, "one to four channels");
    using C = FwCfg<NKB>;
    constexpr int PADA = C::PADA, PW = C::PW, NT = C::NT, PER = C::PER;
    constexpr int RS = NKB > 4 ? NKB : 4;                         // row-pass slots: the stores of the previous tile need four
    constexpr int CS = NKB > 9 ? NKB : 9;                         // column-pass slots: hand-off 0 .. 7, emission 1 .. 4, staging from 5
    constexpr int IPS = (PER + CS - 6) / (CS - 5);                // staging items per column-pass slot from slot 5 on
    extern __shared__ __attribute__((aligned(16))) unsigned char fw_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = lane & 31, h = lane >> 5;

    const int nx = g.nxcd, xcd = blockIdx.x % nx, in_xcd = blockIdx.x / nx, per_xcd = (ntasks + nx - 1) / nx, task = xcd * per_xcd + in_xcd;
    if (in_xcd >= per_xcd || task >= ntasks) return;
    // the launch's active channels (FwChSel; all CH of them: c = task % CH)
    const int nact = CH == 1 ? 1 : fw_chsel_count(chsel), c = CH == 1 ? 0 : static_cast<int>((chsel >> (4 + 2 * (task % nact))) & 3u);
    const int xc = (task / nact) % chunks, seg = (task / (nact * chunks)) % nseg, f = task / (nact * chunks * nseg);
    const int x0 = xc * kFxChunk;
    const int tile0 = seg * tps, tile1 = min(tile0 + tps, g.ntiles);
    // a launch over frames with their own sigmas (FwFrame): everything below that depends on sigma is replaced here, once
    int fr = f;
    if constexpr (FRAMES) {
        const FwFrame e = ft[f];
        fr = e.frame;
        g.pad = e.pad;
        frags += e.frags;
        qk.taps += e.taps;
        qk.dr = e.dr;
        qk.dc = e.dc;
    }
    const uint8_t* img = src + static_cast<size_t>(fr) * pt.src_frame;
    uint8_t* out = dst + static_cast<size_t>(fr) * pt.dst_frame;

    // fragments: hi halves in registers; of the lo halves the first TLR in registers too, the rest in LDS (the row pass reads a
    // window fragment per block already: with every lo half from LDS as well its two products would wait for the LDS pipe)
    constexpr int TLR = FW_TL_REGS < NKB ? FW_TL_REGS : NKB;
    mx_half8 th[NKB], tlr[TLR > 0 ? TLR : 1];
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) th[kb] = frags[kb * 64 + lane];
#pragma unroll
    for (int kb = 0; kb < TLR; ++kb) tlr[kb] = frags[(NKB + kb) * 64 + lane];
    {
        mx_half8* tls = reinterpret_cast<mx_half8*>(fw_lds + C::TLOFF);
        for (int i = tid; i < NKB * 64; i += 256) tls[i] = frags[NKB * 64 + i];
    }
    const mx_half8* tlp = reinterpret_cast<const mx_half8*>(fw_lds + C::TLOFF) + lane;
    auto tlo = [&](int kb) __attribute__((always_inline)) { return kb < TLR ? tlr[kb < TLR ? kb : 0] : tlp[kb * 64]; };

    float cpos = 0.5f, cneg = 0.5f;
    if (QUIRK) {
        // the column term of this chunk's pixels in the task's channel (the window buffers are not in use yet: scratch in buffer 0,
        // the result in buffer 1)
        float* qc = reinterpret_cast<float*>(fw_lds + C::BUF);
        if constexpr (CH == 3) {
            static_assert(C::BUF >= 8 * (C::WIN + 2 * C::PADA + 1 + 6) + 4 * (3 * C::WIN + 4), "fx_quirk_cols_tile's scratch fits window buffer 0");
            fx_quirk_cols_tile<1>(fw_lds, qc, qk, f, x0, c, g.cols, g.pad, tid);
        } else {
            static_assert(C::BUF >= 8 * (C::WIN + 2 * C::PADA + 1) && C::BUF >= 4 * kFxChunk, "fc_quirk_cols_tile's scratch and result fit the window buffers");
            fc_quirk_cols_tile<CH>(fw_lds, qc, qk, f, x0, c, g.cols, g.pad, tid);
        }
        const float v = qc[32 * wave + m];
        cpos = 0.5f + v;
        cneg = 0.5f - v;
        __syncthreads();                                   // before the staging writes windows over it
    }
    const int qrows = 32 * (g.ntiles + NT);
    const double qrs = QUIRK ? static_cast<double>(qk.dr) * ((g.pad & 1) ? -1.0 : 1.0) : 0.0;

    const mx_float16 zero = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
    mx_float16 acc[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) acc[k] = zero;
    mx_float16 arow = zero, tfin = zero;
    uint32_t hl[2][2][8];               // hand-off, two of them (the next step's is made while this step's is consumed): [hi, lo][packed row pairs], block b = entries 4 b .. 4 b + 3
    uint32_t rr[4];                     // finished tile per row group: the channel's bytes of 4 rows of the lane's pixel column (CH = 1: transposed)

    const int s0 = tile0, s1 = tile1 + NT;
    // the window's source: the image, or (edge chunks) a strip with the mirrored pixels in place -- as in fx_kernels.hpp
    constexpr int NLEFT = fx_left_strips(PADA);                // two chunks at the left edge once the window is wider than a chunk either side
    const int sidx = xc < NLEFT ? xc : (xc >= chunks - g.nright ? NLEFT + xc - (chunks - g.nright) : -1);      // uniform
    const uint32_t pitch = sidx >= 0 ? static_cast<uint32_t>(CH * C::WIN) : pt.src_pitch;
    const uint8_t* wbase = sidx >= 0 ? strips + (static_cast<size_t>(f) * (NLEFT + g.nright) + sidx) * g.rows * (CH * C::WIN) : img + CH * (x0 - PADA);
    const uint32_t wbytes = sidx >= 0 ? static_cast<uint32_t>(g.rows) * static_cast<uint32_t>(CH * C::WIN)
                                      : static_cast<uint32_t>(g.rows - 1) * pt.src_pitch + static_cast<uint32_t>(g.cols - (x0 - PADA)) * static_cast<uint32_t>(CH);
    const __amdgpu_buffer_rsrc_t rimg = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(wbase), 0, wbytes, kMxRsrcWord3);
    const int srow = 8 * (tid >> 6) + ((tid >> 4) & 3) + 4 * ((tid >> 3) & 1), g0 = tid & 7;      // (fx_kernels.hpp: the staging map)
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    uint32_t raw[PER][CH];
    int qpart[CH == 3 ? kFxMaxBatches : 1] = {};      // the row term's Srow: CH = 3 in fx_prepass's parts per batch, CH = 1, 4 complete
    // the window of step s: thread t moves the groups of 4 pixels g0 + 8 k of row srow, all requested at once (consumed one
    // matrix-heavy pass later).  (CH = 3: a mapping with 2 rows x 384 contiguous bytes per wave load instead of 8 x 96 changed nothing.)
    auto issue_window = [&](int s) __attribute__((always_inline)) {
        const int r = mx_refl(32 * s - PADA + srow, g.rows);
        const uint32_t off = static_cast<uint32_t>(r) * pitch + static_cast<uint32_t>(4 * CH * g0);
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const bool in = (C::GPR % 8 == 0) || k < PER - 1 || g0 < C::GPR % 8;
            // (CH = 3 spells the offset out in its load: through `o` the compiler schedules that kernel differently)
            const uint32_t o = in ? off + static_cast<uint32_t>(32 * CH * k) : off;
            if constexpr (CH == 1) {
                raw[k][0] = __builtin_amdgcn_raw_buffer_load_b32(rimg, o, 0, 0);
            } else if constexpr (CH == 2) {
                typedef uint32_t u2 __attribute__((ext_vector_type(2)));
                const u2 t = __builtin_amdgcn_raw_buffer_load_b64(rimg, o, 0, 0);
                raw[k][0] = t[0]; raw[k][1] = t[1];
            } else if constexpr (CH == 3) {
                typedef uint32_t u3 __attribute__((ext_vector_type(3)));
                const u3 t = __builtin_amdgcn_raw_buffer_load_b96(rimg, in ? off + 32u * CH * k : off, 0, 0);
                raw[k][0] = t[0]; raw[k][1] = t[1]; raw[k][2] = t[2];
            } else {
                const u4 t = __builtin_amdgcn_raw_buffer_load_b128(rimg, o, 0, 0);
                raw[k][0] = t[0]; raw[k][1] = t[1]; raw[k][2] = t[2]; raw[k][3] = t[3];
            }
        }
        if (QUIRK) {                    // the row term of row re of V (= image row refl(re - PADA)): dr (-1)^pad Srow; every thread (row tid & 31:
                                        // eight copies of each value) -- a test on tid would be a branch in the middle of a slice of matrix instructions
            if constexpr (CH == 3) {
                const int* sp = qk.srow_part + (static_cast<size_t>(f) * qk.nbatches * g.rows + mx_refl(min(32 * s + (tid & 31), qrows - 1) - PADA, g.rows)) * 3 + c;
#pragma unroll
                for (int b = 0; b < kFxMaxBatches; ++b) qpart[b] = sp[static_cast<size_t>(min(b, qk.nbatches - 1)) * g.rows * 3];      // (fx_kernels.hpp: issue_chunk)
            } else {
                qpart[0] = qk.srow[(static_cast<size_t>(f) * g.rows + mx_refl(min(32 * s + (tid & 31), qrows - 1) - PADA, g.rows)) * CH + c];
            }
        }
    };
    // channel c of group k -> binary16 subnormals -> LDS: two v_perm_b32 and one ds_write_b64.  CH = 3: pixels (0, 1) of the group
    // are bytes (c, 3 + c), pixels (2, 3) bytes (6 + c, 9 + c) of its three dwords; CH = 4: byte c of each dword; CH = 2: one
    // v_perm_b32 per dword, bytes (c, 2 + c) of it
    const uint32_t selA = CH == 3 ? (c == 0 ? 0x0c030c00u : (c == 1 ? 0x0c040c01u : 0x0c050c02u))                 // operands (d1, d0)
                                  : 0x0c000c00u | (static_cast<uint32_t>(4 + c) << 16) | static_cast<uint32_t>(c);  // CH = 4: (d1, d0), (d3, d2)
    const uint32_t selB = c == 0 ? 0x0c050c02u : (c == 1 ? 0x0c060c03u : 0x0c070c00u);                             // CH = 3: (d2, d1) / c == 2: (d2, d2)
    const uint32_t selC = 0x0c000c00u | (static_cast<uint32_t>(2 + c) << 16) | static_cast<uint32_t>(c);             // CH = 2: (0, d0), (0, d1)
    auto commit_item = [&](int buf, int k) __attribute__((always_inline)) {
        if (k >= PER) return;
        // (groups past the window's GPR of the last k hold whatever their clamped load returned: they land in the row's padding)
        _Float16* base = reinterpret_cast<_Float16*>(fw_lds + buf * C::BUF) + srow * PW + 4 * g0;
        uint2 wd;
        if constexpr (CH == 1) {
            wd.x = __builtin_amdgcn_perm(0u, raw[k][0], 0x0c010c00u);
            wd.y = __builtin_amdgcn_perm(0u, raw[k][0], 0x0c030c02u);
        } else if constexpr (CH == 2) {
            wd.x = __builtin_amdgcn_perm(0u, raw[k][0], selC);
            wd.y = __builtin_amdgcn_perm(0u, raw[k][1], selC);
        } else if constexpr (CH == 3) {
            wd.x = __builtin_amdgcn_perm(raw[k][1], raw[k][0], selA);
            wd.y = __builtin_amdgcn_perm(raw[k][2], c == 2 ? raw[k][2] : raw[k][1], selB);
        } else {
            wd.x = __builtin_amdgcn_perm(raw[k][1], raw[k][0], selA);
            wd.y = __builtin_amdgcn_perm(raw[k][3], raw[k][2], selA);
        }
        *reinterpret_cast<uint2*>(base + 32 * k) = wd;
    };
    auto commit_q = [&](int buf) __attribute__((always_inline)) {
        if (QUIRK) {                     // (every thread: the eight threads of a row store the same value to the same place)
            int v = qpart[0];
            if constexpr (CH == 3) {
#pragma unroll
                for (int b = 1; b < kFxMaxBatches; ++b) v += b < qk.nbatches ? qpart[b] : 0;
            }
            const float qraw = static_cast<float>(qrs * v);
            float* qs = reinterpret_cast<float*>(fw_lds + C::QOFF) + buf * 64 + (tid & 31);
            qs[0] = qraw;            // the term enters as qrow (-1)^x: lanes of even x read this copy,
            qs[32] = -qraw;          // lanes of odd x this one
        }
    };
    // R: the window in buffer `buf` -> arow; `beside(kb)` runs after the products of slot kb
    auto rowpass = [&](int buf, auto beside) __attribute__((always_inline)) {
        const _Float16* base = reinterpret_cast<const _Float16*>(fw_lds + buf * C::BUF) + m * PW + wave * 32 + 8 * h;
        mx_float16 a = zero;
        mx_half8 x[4], tq[3];                      // window fragments three blocks ahead, LDS-resident lo halves two blocks ahead
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
                asm volatile("" : "+a"(a));          // pins the two products between this block's fences
            }
            beside(kb);
            __builtin_amdgcn_sched_barrier(0);       // the vector work handed out beside slot kb stays beside slot kb
        }
        arow = a;
    };
    // S: arow -> scale (+ quirk), split into hi + lo, exchange with lane ^ 32 -> hl[hb] (fx_kernels.hpp: split_piece), in eight pieces:
    // rows 0..15 / 16..31 of the tile x {read + scale, convert row pairs 0 1, convert row pairs 2 3, exchange}
    float sv[16];
    auto split_piece = [&](int buf, int hb, int piece) __attribute__((always_inline)) {
        const int hf = piece >> 2, sub = piece & 3;
        uint32_t (&hp)[8] = hl[hb][0];
        uint32_t (&lp)[8] = hl[hb][1];
        if (sub == 0) {
            if (QUIRK) {
                const float* qs4 = reinterpret_cast<const float*>(fw_lds + C::QOFF) + buf * 64 + (m & 1) * 32 + 4 * h;
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
            // regs (0..3, 4..7) of the half = rows (0..3, 8..11) + 4 h of its 16-row block -> the lane wants rows 8 h .. 8 h + 7
            fx_swap4(hp[4 * hf], hp[4 * hf + 2], hp[4 * hf + 1], hp[4 * hf + 3], lp[4 * hf], lp[4 * hf + 2], lp[4 * hf + 1], lp[4 * hf + 3]);
        }
    };
    // E: four registers of the finished tile (rows 8 gq + 4 h + 0 .. 3 of the lane's pixel column) -> bytes, kept in rr[gq].  CH = 2, 3,
    // 4: no transposes, the lane keeps its COLUMN, so a store instruction covers 2 rows x 32 pixels.  CH = 1: transposed inside the
    // lane quad: lane q of quad Q holds row 8 gq + 4 h + q, pixels 4 Q .. 4 Q + 3 of the wave's 32
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
    // C: column pass of step slot qs from hl (fx_kernels.hpp: colpass): first the tile that FINISHES, last the tile that STARTS
    // `ri`: step ri of the segment's first NT (-1: a later step) -- the triples of tiles above the segment (a2 > ri) are left out
    // statically (fx_kernels.hpp: colpass)
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
                    asm volatile("" : "+a"(t));      // pins the three products between this triple's fences
                    if (it == 0) tfin = t; else acc[slot] = t;
                }
            }
            beside(it);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    // F: the finished tile's bytes.  Buffer stores: rows past the image, pixels right of it (an explicit x < cols: the bytes between
    // two rows of a pitched frame lie inside the resource) and tiles that do not exist get an offset outside the resource
    const __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc(out, 0, static_cast<uint32_t>(g.rows - 1) * pt.dst_pitch + static_cast<uint32_t>(g.cols) * CH, kMxRsrcWord3);
    const int xcol = x0 + 32 * wave + m;                                  // CH = 3, 4: the lane's pixel column
    // CH = 3: byte c of the lane's pixel in row 4 h (the stores add the row group's offset to it; CH = 4 computes each offset whole.
    // The two spellings keep each kernel's code as it was tuned: either one in the other kernel changes its registers and schedule)
    const uint32_t lane_out = CH == 3 ? static_cast<uint32_t>(4 * h) * pt.dst_pitch + static_cast<uint32_t>(xcol) * CH + static_cast<uint32_t>(c) : 0u;
    // (the pitch as a value the compiler cannot see through, and below the row of a CH = 4 store group likewise: with a plain scalar
    // pitch it splits every store offset into a per-step scalar and per-lane parts that it keeps in registers across the whole step
    // loop -- 80 to 95 more registers at NKB 7 .. 11, parked in AGPRs -- where the packed kernels multiplied by cols CH in place)
    uint32_t rowstep_ = pt.dst_pitch;
    asm volatile("" : "+s"(rowstep_));
    const uint32_t rowstep = rowstep_;
    const int xq = x0 + 32 * wave + 4 * (m >> 2), q = m & 3;                // CH = 1: first pixel of the lane's quad, its row in the row group
    const bool ragged = (g.cols & 3) != 0;                                // (uniform) CH = 1: the quad cut by the right edge leaves as bytes
    const int qn = xq >= g.cols ? 0 : min(4, g.cols - xq);                // pixels of the lane's quad inside the image
    auto store_group = [&](int tile, bool valid, int gq) __attribute__((always_inline)) {
        const uint32_t v = rr[gq];
        if constexpr (CH == 1) {
            const int row = 32 * tile + 8 * gq + 4 * h + q;
            const bool rok = valid && row < g.rows;
            const uint32_t o = static_cast<uint32_t>(row) * rowstep + static_cast<uint32_t>(xq);
            __builtin_amdgcn_raw_buffer_store_b32(v, rout, rok && qn == 4 ? o : 0xfffffff0u, 0, 0);
            if (ragged) {
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    __builtin_amdgcn_raw_buffer_store_b8(static_cast<uint8_t>(v >> (8 * k)), rout, rok && qn < 4 && k < qn ? o + k : 0xfffffff0u, 0, 0);
            }
        } else {                                                          // byte c of every pixel, rows 8 gq + 4 h + k of the lane's column
            int row0 = 32 * tile + 8 * gq + 4 * h;
            if constexpr (CH == 4 || CH == 2) asm volatile("" : "+v"(row0));
            const uint32_t base = CH == 3 ? lane_out + static_cast<uint32_t>(32 * tile + 8 * gq) * rowstep
                                          : static_cast<uint32_t>(row0) * rowstep + static_cast<uint32_t>(xcol) * CH + static_cast<uint32_t>(c);
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
    __syncthreads();                                           // window s0 may be overwritten (row pass s0 has read it)

    // Step s: the row pass of step s + 1 (window s + 1), then the column pass of step s.  The step's vector work rides beside the
    // products, a few instructions per slot (a slot = the two products of a window block / the three of a column-pass triple; a
    // block of vector instructions longer than a slot's matrix time would leave the matrix pipe idle):
    //   row pass    the stores of the tile the PREVIOUS step finished (slots 0 .. 3); the loads of window s + 2 are requested before it
    //   column pass the hand-off of step s + 1 (slots 0 .. 7, into hl[1]; copied to hl[0] at the end of the step), the emission of
    //               the tile this step finishes (slots 1 .. 4), window s + 2 group by group into the buffer window s left (from slot 5)
    // The step loop is unrolled NT times: the accumulator rotation is static, the window buffers alternate through a run-time offset.
    auto step = [&](int s, int qs, int ri) __attribute__((always_inline)) {
        const int par = (s - s0) & 1;                          // window s: buffer par; window s + 1: the other one
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
        __syncthreads();                                       // window s + 2 complete, window s + 1 no longer read
    };
    // the first NT steps of a segment as their own copy of the body, without the column products of the tiles above the segment (about
    // half the column pass of these steps: NT = 11 for the widest window, where a single image's segments are 14 .. 20 steps long)
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
        const int ltile = s1 - 1 - NT;                         // the tile the last step finished
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) store_group(ltile, ltile >= tile0, gq);
    }
}

// ft: the launch's frame list (device; g.nframes entries) or null (FwFrame)
template <int NKB, int CH> hipError_t fw_launch(hipStream_t st, const uint8_t* src, uint8_t* dst, const void* frags, FxGeom g, int num_cus, const FwQuirk<CH>* qk,
                                               const uint8_t* strips, FwChSel chsel, FwPitch pt, const FwFrame* ft)
{
    using C = FwCfg<NKB>;
    const int nact = fw_chsel_count(chsel);
    if (nact < 1 || nact > CH) return hipErrorInvalidValue;
    for (int i = 0; i < nact; ++i)
        if (static_cast<int>((chsel >> (4 + 2 * i)) & 3u) >= CH) return hipErrorInvalidValue;
    const FxLaunch l = fx_plan_launch(g, nact, C::NT, num_cus);
    if (l.ntasks == 0) return hipSuccess;
    static std::atomic<unsigned long long> attr_done{ 0 };
    const hipError_t e = fx_set_lds(attr_done, C::LDS, fw_blur_u8<NKB, true, CH>, fw_blur_u8<NKB, false, CH>, fw_blur_u8<NKB, true, CH, true>,
                                    fw_blur_u8<NKB, false, CH, true>);
    if (e != hipSuccess) return e;
    const mx_half8* fr = static_cast<const mx_half8*>(frags);
    const int nt = static_cast<int>(l.ntasks);
    if (ft) {
        if (qk) hipLaunchKernelGGL((fw_blur_u8<NKB, true, CH, true>), l.grid, dim3(256), C::LDS, st, src, dst, fr, g, l.chunks, l.tps, l.nseg, nt, *qk, strips, chsel, pt, ft);
        else hipLaunchKernelGGL((fw_blur_u8<NKB, false, CH, true>), l.grid, dim3(256), C::LDS, st, src, dst, fr, g, l.chunks, l.tps, l.nseg, nt, FwQuirk<CH>{}, strips, chsel, pt, ft);
    } else {
        if (qk) hipLaunchKernelGGL((fw_blur_u8<NKB, true, CH>), l.grid, dim3(256), C::LDS, st, src, dst, fr, g, l.chunks, l.tps, l.nseg, nt, *qk, strips, chsel, pt, FwNoFrames{});
        else hipLaunchKernelGGL((fw_blur_u8<NKB, false, CH>), l.grid, dim3(256), C::LDS, st, src, dst, fr, g, l.chunks, l.tps, l.nseg, nt, FwQuirk<CH>{}, strips, chsel, pt, FwNoFrames{});
    }
    return hipGetLastError();
}

// the three-channel entry (FxEntry; fx_registry.hpp: find_entry_for_pad) of the wide windows
template <int NKB> hipError_t fw_launch_u8c3(hipStream_t st, const uint8_t* src, uint8_t* dst, const void* frags, FxGeom g, int num_cus, const FxQuirk* qk,
                                             const uint8_t* strips, float* vdump, unsigned long long* stamps)
{
    if (vdump || stamps) return hipErrorNotSupported;            // the row-pass dump and the phase stamps are builds of fx_blur_u8 only
    return fw_launch<NKB, 3>(st, src, dst, frags, g, num_cus, qk, strips, fw_chsel_all(3), fw_pitch_packed(g.rows, g.cols, 3, 1), nullptr);
}

struct FcEntry {
    int nkb;
    // ch: 1, 2 or 4; qk: the quirk's sums (null: nyquist_quirk = 0); chsel: the channels to blur; pt: where the rows and frames lie;
    // ft: the frame list of a launch over frames with their own sigmas, or null (FwFrame)
    hipError_t (*blur_u8)(hipStream_t, const uint8_t* src, uint8_t* dst, const void* frags, FxGeom g, int ch, int num_cus, const FcQuirk* qk, const uint8_t* strips,
                          FwChSel chsel, FwPitch pt, const FwFrame* ft);
};

// three channels, a subset of them per launch (one sigma per channel), every window class: the strips are whole windows (fx_prepass
// with narrow = 0) and the quirk's sums fx_prepass's, as for the wide three-channel entry
struct Fw3Entry {
    int nkb;
    hipError_t (*blur_u8)(hipStream_t, const uint8_t* src, uint8_t* dst, const void* frags, FxGeom g, int num_cus, const FxQuirk* qk, const uint8_t* strips, FwChSel chsel,
                          FwPitch pt, const FwFrame* ft);
};
template <int NKB> hipError_t fw_launch_u8c3_sel(hipStream_t st, const uint8_t* src, uint8_t* dst, const void* frags, FxGeom g, int num_cus, const FxQuirk* qk,
                                                 const uint8_t* strips, FwChSel chsel, FwPitch pt, const FwFrame* ft)
{
    return fw_launch<NKB, 3>(st, src, dst, frags, g, num_cus, qk, strips, chsel, pt, ft);
}

// the one-, two- and four-channel entry (FcEntry; fx_registry.hpp: find_entry) of every window class (two channels: the chroma plane
// of an NV12 surface -- blur_gaussian_nv12_*, with a frame list blur_gaussian_nv12_frame_sigmas_*; no public entry takes channels = 2)
template <int NKB> hipError_t fw_launch_u8c14(hipStream_t st, const uint8_t* src, uint8_t* dst, const void* frags, FxGeom g, int ch, int num_cus, const FcQuirk* qk,
                                              const uint8_t* strips, FwChSel chsel, FwPitch pt, const FwFrame* ft)
{
    if (ch == 1) return fw_launch<NKB, 1>(st, src, dst, frags, g, num_cus, qk, strips, chsel, pt, ft);
    if (ch == 4) return fw_launch<NKB, 4>(st, src, dst, frags, g, num_cus, qk, strips, chsel, pt, ft);
    if (ch == 2) return fw_launch<NKB, 2>(st, src, dst, frags, g, num_cus, qk, strips, chsel, pt, ft);
    return hipErrorInvalidValue;
}

// fw_conv.hip makes the entries: FcEntry and Fw3Entry for every window class, FxEntry as well for the wide ones (whole BGR frames)

// ---- what runs before the 1- and 4-channel kernels (engine.hip) ------------------------------------------------------
// strips[f][strip][row][CH (128 + 2 pada)]: the window of an edge chunk with the mirrored pixels in place (fx_edge_strips_body for
// CH channels; the CH-channel kernel reads the whole window of an edge chunk from its strip).  A thread writes one dword.
template <int CH>
__device__ __forceinline__ void fc_edge_strips_body(const uint8_t* __restrict__ src, uint8_t* __restrict__ strips, int rows, int cols, int pada, int chunks,
                                                    int nright, int bx, int sidx, int f, uint32_t spitch, size_t sframe)
{
    const int win = kFxChunk + 2 * pada, dpr = CH * win / 4;            // dwords per strip row (win is a multiple of 4)
    const int nleft = fx_left_strips(pada);
    const int xc = sidx < nleft ? sidx : chunks - nright + sidx - nleft, x0 = kFxChunk * xc;
    const int i = bx * 256 + threadIdx.x;
    if (i >= rows * dpr) return;
    const int r = i / dpr, d = i - r * dpr;
    const uint8_t* line = src + static_cast<size_t>(f) * sframe + static_cast<size_t>(r) * spitch;
    uint32_t o = 0;
    if constexpr (CH == 2) {                                           // two pixels per dword, each mirrored on its own, byte by byte
        const int X2 = x0 - pada + 2 * d;
#pragma unroll
        for (int k = 0; k < 4; ++k) o |= static_cast<uint32_t>(line[2 * mx_refl(X2 + (k >> 1), cols) + (k & 1)]) << (8 * k);
        *reinterpret_cast<uint32_t*>(strips + ((static_cast<size_t>(f) * (nleft + nright) + sidx) * rows + r) * (CH * win) + 4 * d) = o;
        return;
    }
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
// A thread owns G dwords of every row of the band: CH = 1 four pixels, CH = 2 two pixels' two channels (byte k of the dword: pixel
// k / 2, channel k % 2), CH = 4 one pixel's four channels.  Exact integers; srow and
// zsum must be zero before the launch (they are completed with atomics).  sred[row][channel][lane]: lane l of every wave adds
// into slot l (fx_altsums_body).  chmask: the channels whose sums the launch that follows reads (bit c; one sigma per channel: a
// subset) -- the row sums of the others are neither reduced nor added up (srow and zsum stay 0 for them).
// spitch, sframe: the source's row pitch and frame stride in bytes (FwPitch); every output stays packed and the partition depends
// on rows, cols and CH only, so a pitched frame gives the sums of its packed copy.
constexpr int kFcSumRows = 32;
template <int CH, int G>
__device__ __forceinline__ void fc_altsums_body(const uint8_t* __restrict__ src, int* __restrict__ srow, int* __restrict__ cpart, long long* __restrict__ zsum,
                                                int rows, int cols, int pad, int nbands, int cpitch, int band, int batch, int f, int (*sred)[CH][64], int band_rows,
                                                unsigned chmask, uint32_t spitch, size_t sframe)
{
    const int tid = threadIdx.x;
    const uint32_t rowbytes = static_cast<uint32_t>(cols) * CH;
    const __amdgpu_buffer_rsrc_t rimg = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(src + static_cast<size_t>(f) * sframe), 0,
                                                                          static_cast<uint32_t>(rows - 1) * spitch + rowbytes, kMxRsrcWord3);
    const int ndw = static_cast<int>((rowbytes + 3) / 4), r0 = band * band_rows, r1 = min(r0 + band_rows, rows);
    // a row that is no multiple of 4 bytes (cols * CH >= 4): its last dword is loaded `over` bytes early and shifted down, so that no
    // load reaches past the row's cols CH bytes (the last row's would leave the buffer resource, which returns 0 for the WHOLE dword)
    const int over = 4 * ndw - static_cast<int>(rowbytes);
    int dj[G], wx[G][4], col[G][4], back[G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
        dj[j] = (batch * G + j) * 256 + tid;
        back[j] = dj[j] == ndw - 1 ? over : 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int b = 4 * dj[j] + k, x = CH == 1 ? b : (CH == 2 ? b >> 1 : dj[j]);          // pixel of byte k of the dword (CH = 2: two pixels per dword)
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
                const uint32_t roff = static_cast<uint32_t>(min(rb + i, re - 1)) * spitch;
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
                for (int ch = 0; ch < CH; ++ch)
                    if (chmask >> ch & 1u) atomicAdd(&sred[r - rs][ch][tid & 63], s[ch]);                  // uniform
            }
        }
        __syncthreads();
        if (tid < (re - rs) * CH && (chmask >> (tid % CH) & 1u)) {
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
                                                  int chunks, int nright, int strip_blocks, int band_rows, unsigned chmask, uint32_t spitch, size_t sframe)
{
    __shared__ int sred[kFcSumRows][CH][64];
    int b = blockIdx.x;
    if (b < n_alt) {
        const int band = b % nbands, batch = (b / nbands) % nbatches, f = b / (nbands * nbatches);
        fc_altsums_body<CH, G>(src, srow, cpart, zsum, rows, cols, pad, nbands, cpitch, band, batch, f, sred, band_rows, chmask, spitch, sframe);
    } else {
        b -= n_alt;
        const int nstrips = fx_left_strips(pada) + nright, bx = b % strip_blocks, sidx = (b / strip_blocks) % nstrips, f = b / (strip_blocks * nstrips);
        fc_edge_strips_body<CH>(src, strips, rows, cols, pada, chunks, nright, bx, sidx, f, spitch, sframe);
    }
}

// fc_prepass for a launch over frames with their own sigmas: workgroup frame f of the grid is entry f of the list `ft`; the sums are
// weighted with that frame's pad and read its frame of the source (the outputs are indexed by f, as the fused launch reads them)
template <int CH, int G>
__global__ __launch_bounds__(256) void fc_prepass_frames(const uint8_t* __restrict__ src, int* __restrict__ srow, int* __restrict__ cpart, long long* __restrict__ zsum,
                                                         uint8_t* __restrict__ strips, int rows, int cols, int pada, int nbands, int nbatches, int cpitch, int n_alt,
                                                         int chunks, int nright, int strip_blocks, int band_rows, unsigned chmask, uint32_t spitch, size_t sframe,
                                                         const FwFrame* __restrict__ ft)
{
    __shared__ int sred[kFcSumRows][CH][64];
    int b = blockIdx.x;
    if (b < n_alt) {
        const int band = b % nbands, batch = (b / nbands) % nbatches, f = b / (nbands * nbatches);
        // (the bodies address the source as src + f sframe: the frame's own offset less that)
        const uint8_t* s = src + (static_cast<ptrdiff_t>(ft[f].frame) - f) * static_cast<ptrdiff_t>(sframe);
        fc_altsums_body<CH, G>(s, srow, cpart, zsum, rows, cols, ft[f].pad, nbands, cpitch, band, batch, f, sred, band_rows, chmask, spitch, sframe);
    } else {
        b -= n_alt;
        const int nstrips = fx_left_strips(pada) + nright, bx = b % strip_blocks, sidx = (b / strip_blocks) % nstrips, f = b / (strip_blocks * nstrips);
        const uint8_t* s = src + (static_cast<ptrdiff_t>(ft[f].frame) - f) * static_cast<ptrdiff_t>(sframe);
        fc_edge_strips_body<CH>(s, strips, rows, cols, pada, chunks, nright, bx, sidx, f, spitch, sframe);
    }
}

// fc_prepass_frames<2, G> on `nblocks` workgroups (G = 1, 2, 4): instantiated and launched in fc_frames2.hip, which says why
hipError_t fc_prepass_frames2_launch(int G, unsigned nblocks, hipStream_t st, const uint8_t* src, int* srow, int* cpart, long long* zsum, uint8_t* strips, int rows, int cols,
                                     int pada, int nbands, int nbatches, int cpitch, int n_alt, int chunks, int nright, int strip_blocks, int band_rows, unsigned chmask,
                                     uint32_t spitch, size_t sframe, const FwFrame* ft);

#ifdef BLUR_FX_QUIRK_KERNELS
// fx_prepass (three channels: fx_kernels.hpp) for a launch over frames with their own sigmas, as fc_prepass_frames
template <int G>
__global__ __launch_bounds__(256) void fx_prepass_frames(const uint8_t* __restrict__ src, int* __restrict__ srow_part, int* __restrict__ cpart, long long* __restrict__ zpart,
                                                         uint8_t* __restrict__ strips, int rows, int cols, int pada, int nbands, int nbatches, int n_alt, int chunks,
                                                         int nright, int strip_blocks, int band_rows, int narrow, uint32_t spitch, size_t sframe,
                                                         const FwFrame* __restrict__ ft)
{
    __shared__ int sred[kFxSumRows][3][64];
    int b = blockIdx.x;
    if (b < n_alt) {
        const int band = b % nbands, batch = (b / nbands) % nbatches, f = b / (nbands * nbatches);
        const uint8_t* s = src + (static_cast<ptrdiff_t>(ft[f].frame) - f) * static_cast<ptrdiff_t>(sframe);
        fx_altsums_body<G>(s, srow_part, cpart, zpart, rows, cols, ft[f].pad, nbands, nbatches, band, batch, f, sred, band_rows, spitch, sframe);
    } else {
        b -= n_alt;
        const int nstrips = fx_left_strips(pada) + nright, bx = b % strip_blocks, sidx = (b / strip_blocks) % nstrips, f = b / (strip_blocks * nstrips);
        const uint8_t* s = src + (static_cast<ptrdiff_t>(ft[f].frame) - f) * static_cast<ptrdiff_t>(sframe);
        fx_edge_strips_body(s, strips, rows, cols, pada, chunks, nright, bx, sidx, f, narrow, spitch, sframe);
    }
}
#endif  // BLUR_FX_QUIRK_KERNELS

}  // namespace blur_amd
