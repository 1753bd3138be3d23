// engine.hip -- HIP kernels (gfx950) and the C ABI of include/blur_amd.h.
//
// Data path of pffft_() (Source.cpp:429-570) on the GPU, per frame:
//
//   rowpass_kernel   u8 BGR interleaved (or one f32 plane)  --->  3 float planes, row-major
//       deinterleave_BGR (Utils.hpp:159-184) + per-row reflect-101 pad (Source.cpp:525-529)
//       + FFT / pointwise / inverse FFT (:531-533) + crop (:536), two image rows per
//       complex line, one workgroup per (row pair, channel).
//   colpass_kernel   3 float planes  --->  u8 BGR interleaved (or one f32 plane)
//       a workgroup owns a strip of G adjacent columns and reads it straight out of the
//       row-major planes (the transposes flip_block of :540,562 never materialise), pads
//       by reflection along the column (:549-551), FFT / pointwise / inverse FFT (:553-555),
//       crops (:558) and applies interleave_BGR's "+0.5f, truncate" (Utils.hpp:189,204-206),
//       staging the three channels in LDS so that the strip is written as whole pixels.
//
// HBM traffic per pixel: 3 B in + 12 B intermediate out, 12 B intermediate in + 3 B out.
#include <hip/hip_runtime.h>

#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <list>
#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "../../include/blur_amd.h"
#include "fast_registry.hpp"
#include "fft_engine.hpp"
#include "host_math.hpp"
#define BLUR_MX_QUIRK_KERNELS
#include "mx_kernels.hpp"
#define BLUR_FX_QUIRK_KERNELS
#include "fw_kernels.hpp"
#include "fx_registry.hpp"
#include "bx_box.hpp"
#include "wr_registry.hpp"

using namespace blur_amd;

namespace {

constexpr int kThreads = 256;
constexpr size_t kLdsLimit = 160 * 1024;

// Blocks b and b + nx share an XCD (and its L2; nx = hipDeviceAttributeNumberOfXccs, 8 on MI355X).  Give each XCD a contiguous
// run of work items so that neighbours (which touch the same 128-byte lines) meet in one L2.
__device__ __forceinline__ int xcd_contiguous(int b, int nwg, int nx)
{
    if (nx < 1) nx = 8;
    const int q = nwg / nx, r = nwg - q * nx, x = b % nx;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + b / nx;
}

// reflect-101 source index of padded position p (Source.cpp:525-529); -1 = trailing zero
__device__ __forceinline__ int reflect_src(int p, int pad, int len)
{
    const int i = p - pad;
    if (i < 0) return -i;
    if (i < len) return i;
    if (i < len + pad) return 2 * (len - 1) - i;
    return -1;
}

template <typename T> __device__ __forceinline__ float load_px(const T* p) { return static_cast<float>(*p); }

// ------------------------------------------------------------------------------------
// row pass: one workgroup = rows (2q, 2q+1) of channel c
// ------------------------------------------------------------------------------------
template <typename InT, int CH, int T = kThreads>
__global__ __launch_bounds__(T) void rowpass_kernel(const InT* __restrict__ src, float* __restrict__ planes,
                                                           int rows, int cols, int pad, DevPlan plan,
                                                           const float2* __restrict__ tw, const float* __restrict__ mperm, int gshift)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* z = reinterpret_cast<float2*>(smem);
    const int item = xcd_contiguous(blockIdx.x, gridDim.x, plan.nxcd);
    const int pair = item / CH, c = item - pair * CH;
    const int r0 = 2 * pair;
    const bool two = r0 + 1 < rows;
    const int n = plan.n;
    const InT* row_a = src + (static_cast<size_t>(r0) * cols) * CH + c;
    const InT* row_b = src + (static_cast<size_t>(r0 + (two ? 1 : 0)) * cols) * CH + c;

    // unconditional loads (clamped index, value masked afterwards): a load under a branch costs one
    // memory round trip per iteration, unconditional ones overlap across the unrolled iterations
#pragma unroll 8
    for (int p = threadIdx.x; p < n; p += T) {
        const int x = reflect_src(p, pad, cols);
        const size_t xi = static_cast<size_t>(x >= 0 ? x : 0) * CH;
        const float a = load_px(row_a + xi), b = load_px(row_b + xi);
        z[phys(p)] = make_float2(x >= 0 ? a : 0.f, (x >= 0 && two) ? b : 0.f);
    }
    __syncthreads();
    fftconv_lines<1>(z, 0, plan, tw, mperm);

    if (gshift > 0) {
        // strip-major intermediate (gshift = log2 of the G columns a column-pass workgroup takes): [channel][strip x / G][row][G], so
        // that the column pass reads its strip as ONE contiguous block instead of 4 G bytes out of every row of the plane
        const int G = 1 << gshift, nstrips = (cols + G - 1) >> gshift;
        float* base = planes + static_cast<size_t>(c) * nstrips * rows * G + static_cast<size_t>(r0) * G;
        for (int x = threadIdx.x; x < cols; x += T) {
            const float2 v = z[phys(pad + x)];
            float* o = base + static_cast<size_t>(x >> gshift) * rows * G + (x & (G - 1));
            o[0] = v.x;
            if (two) o[G] = v.y;
        }
        return;
    }
    float* out_a = planes + (static_cast<size_t>(c) * rows + r0) * cols;
    float* out_b = out_a + cols;
    for (int x = threadIdx.x; x < cols; x += T) {
        const float2 v = z[phys(pad + x)];
        out_a[x] = v.x;
        if (two) out_b[x] = v.y;
    }
}

// ------------------------------------------------------------------------------------
// column pass: one workgroup = columns [x0, x0 + 2C) of all CH channels
// ------------------------------------------------------------------------------------
__device__ __forceinline__ void store_out(float* p, float v) { *p = v; }

template <typename OutT, int CH, int C, int T = kThreads>
__global__ __launch_bounds__(T) void colpass_kernel(const float* __restrict__ planes, OutT* __restrict__ dst,
                                                           int rows, int cols, int pad, DevPlan plan,
                                                           const float2* __restrict__ tw, const float* __restrict__ mperm, int strips)
{
    constexpr int G = 2 * C;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* z = reinterpret_cast<float2*>(smem);
    const int n = plan.n;
    const int zs = line_stride(n);
    uint8_t* stage = reinterpret_cast<uint8_t*>(z + static_cast<size_t>(C) * zs);   // [rows][G][CH] bytes (u8 output only)
    const int strip = xcd_contiguous(blockIdx.x, gridDim.x, plan.nxcd);
    const int x0 = strip * G;

    for (int c = 0; c < CH; ++c) {
        // strips: the intermediate is [channel][strip][row][G] (rowpass_kernel), this workgroup's strip one contiguous block
        const int nstrips = (cols + G - 1) / G;
        const float* plane = strips ? planes + (static_cast<size_t>(c) * nstrips + strip) * rows * G : planes + static_cast<size_t>(c) * rows * cols;
        // gather the strip: position p of line l  <-  plane[reflect(p)][x0 + 2l, x0 + 2l + 1]
#pragma unroll 4
        for (int idx = threadIdx.x; idx < n * C; idx += T) {
            const int p = idx / C, l = idx - p * C;
            const int r = reflect_src(p, pad, rows);
            const int col = x0 + 2 * l;
            const float* s = strips ? plane + static_cast<size_t>(r >= 0 ? r : 0) * G - x0 : plane + static_cast<size_t>(r >= 0 ? r : 0) * cols;
            const float a = strips ? s[col] : s[col < cols ? col : cols - 1], b = strips ? s[col + 1] : s[col + 1 < cols ? col + 1 : cols - 1];   // unconditional
            z[l * zs + phys(p)] = make_float2((r >= 0 && col < cols) ? a : 0.f, (r >= 0 && col + 1 < cols) ? b : 0.f);
        }
        __syncthreads();
        fftconv_lines<C>(z, zs, plan, tw, mperm);

        if constexpr (sizeof(OutT) == 1) {
            // interleave_BGR<uint8_t,float>: (uint8_t)(value + 0.5f)   Utils.hpp:189,204-206
            for (int idx = threadIdx.x; idx < rows * C; idx += T) {
                const int r = idx / C, l = idx - r * C;
                const float2 v = z[l * zs + phys(pad + r)];
                uint8_t* s = stage + (static_cast<size_t>(r) * G + 2 * l) * CH + c;
                s[0] = static_cast<uint8_t>(static_cast<int>(v.x + 0.5f));
                s[CH] = static_cast<uint8_t>(static_cast<int>(v.y + 0.5f));
            }
        } else {
            for (int idx = threadIdx.x; idx < rows * C; idx += T) {
                const int r = idx / C, l = idx - r * C;
                const float2 v = z[l * zs + phys(pad + r)];
                const int col = x0 + 2 * l;
                OutT* d = dst + (static_cast<size_t>(r) * cols + col) * CH + c;
                if (col < cols) d[0] = v.x;
                if (col + 1 < cols) d[CH] = v.y;
            }
        }
        __syncthreads();
    }

    if constexpr (sizeof(OutT) == 1) {
        const int wbytes = (min(G, cols - x0)) * CH;      // valid bytes per row of the strip
        for (int idx = threadIdx.x; idx < rows * G * CH; idx += T) {
            const int r = idx / (G * CH), b = idx - r * (G * CH);
            if (b < wbytes) dst[(static_cast<size_t>(r) * cols + x0) * CH + b] = stage[idx];
        }
    }
}

// ------------------------------------------------------------------------------------
// the pieces: flip_block, de/interleave
// ------------------------------------------------------------------------------------
// flip_block<float,1>: out[x*h + y] = in[y*w + x]; 64x64 tiles through LDS, both sides coalesced
__global__ __launch_bounds__(256) void flip_block_kernel(const float* __restrict__ in, float* __restrict__ out, int w, int h)
{
    __shared__ float tile[64][65];
    const int tiles_x = (w + 63) / 64;
    const int t = blockIdx.x;
    const int tx = (t % tiles_x) * 64, ty = (t / tiles_x) * 64;
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    for (int yy = ly; yy < 64; yy += 4) {
        const int x = tx + lx, y = ty + yy;
        if (x < w && y < h) tile[yy][lx] = in[static_cast<size_t>(y) * w + x];
    }
    __syncthreads();
    for (int xx = ly; xx < 64; xx += 4) {
        const int x = tx + xx, y = ty + lx;
        if (x < w && y < h) out[static_cast<size_t>(x) * h + y] = tile[lx][xx];
    }
}

__global__ __launch_bounds__(256) void deinterleave_kernel(const uint8_t* __restrict__ in, float* __restrict__ planes, uint32_t total)
{
    for (uint32_t x = blockIdx.x * 256u + threadIdx.x; x < total; x += gridDim.x * 256u) {
        planes[x] = in[3 * static_cast<size_t>(x)];
        planes[static_cast<size_t>(total) + x] = in[3 * static_cast<size_t>(x) + 1];
        planes[2 * static_cast<size_t>(total) + x] = in[3 * static_cast<size_t>(x) + 2];
    }
}

__global__ __launch_bounds__(256) void interleave_kernel(const float* __restrict__ planes, uint8_t* __restrict__ out, uint32_t total)
{
    for (uint32_t x = blockIdx.x * 256u + threadIdx.x; x < total; x += gridDim.x * 256u) {
        out[3 * static_cast<size_t>(x)] = static_cast<uint8_t>(static_cast<int>(planes[x] + 0.5f));
        out[3 * static_cast<size_t>(x) + 1] = static_cast<uint8_t>(static_cast<int>(planes[static_cast<size_t>(total) + x] + 0.5f));
        out[3 * static_cast<size_t>(x) + 2] = static_cast<uint8_t>(static_cast<int>(planes[2 * static_cast<size_t>(total) + x] + 0.5f));
    }
}

// ------------------------------------------------------------------------------------
// tiled wave-resident path (run_wr_tiled): the Nyquist-slot quirk's two term vectors from fx_prepass's integer sums
//   e[f][c][x] = dc Ccol(x, c)                                                (x < pitch; 0 right of the image)
//   h[f][c][r] = dr (colconv(Srow)(r, c) + dc (-1)^(r + pad) Z(c))            (the column convolution with reflect-101, in double)
// grid (ne + nh blocks of 256 outputs, frames): the first ne = ceil(pitch / 256) blocks make e, the others h
// dynamic LDS: 3 (256 + 2 pad) + 2 pad + 1 + 3 + 3 x 256 doubles
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tl_terms_kernel(const int* __restrict__ srow_part, const int* __restrict__ cpart, const long long* __restrict__ zpart,
                                                       const float* __restrict__ taps, float* __restrict__ e, float* __restrict__ h, int rows, int cols, int pad,
                                                       int pitch, int nbatches, int nbands, int cpitch, float dr, float dc, int ne)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char tl_lds[];
    const int f = blockIdx.y, tid = threadIdx.x;
    if (static_cast<int>(blockIdx.x) < ne) {
        const int x = blockIdx.x * 256 + tid;
        if (x >= pitch) return;
        // the bands' parts in batches of eight independent loads per channel (a band's part is below 2^31 / nbands: exact in int)
        const int* cp = cpart + static_cast<size_t>(f) * nbands * cpitch + 3 * (x < cols ? x : 0);
        long long tot[3] = { 0, 0, 0 };
        for (int b0 = 0; b0 < nbands; b0 += 8) {
            int t[8][3];
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int c = 0; c < 3; ++c) t[j][c] = cp[static_cast<size_t>(b0 + j < nbands ? b0 + j : nbands - 1) * cpitch + c];
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int c = 0; c < 3; ++c) tot[c] += b0 + j < nbands ? t[j][c] : 0;
        }
        for (int c = 0; c < 3; ++c)
            e[(static_cast<size_t>(f) * 3 + c) * pitch + x] = x < cols ? static_cast<float>(static_cast<double>(dc) * static_cast<double>(tot[c])) : 0.f;
        return;
    }
    const int r0 = (blockIdx.x - ne) * 256, win = 256 + 2 * pad, ntap = 2 * pad + 1;
    double* sr = reinterpret_cast<double*>(tl_lds);            // [3][win]
    double* tp = sr + 3 * win;
    double* zs = tp + ntap;                                    // [3]
    double* zr = zs + 3;                                       // [3][256] partial sums of Z
    for (int i = tid; i < 3 * win; i += 256) {
        const int c = i / win, p = i - c * win;
        const int r = mx_refl(r0 - pad + p, rows);
        long long v = 0;
        for (int b = 0; b < nbatches; ++b) v += srow_part[((static_cast<size_t>(f) * nbatches + b) * rows + r) * 3 + c];
        sr[i] = static_cast<double>(v);
    }
    for (int i = tid; i < ntap; i += 256) tp[i] = static_cast<double>(taps[i]);
    {
        const int nz = nbands * nbatches;
        long long z[3] = { 0, 0, 0 };
        for (int i = tid; i < nz; i += 256)
            for (int c = 0; c < 3; ++c) z[c] += zpart[(static_cast<size_t>(f) * nz + i) * 3 + c];
        for (int c = 0; c < 3; ++c) zr[c * 256 + tid] = static_cast<double>(z[c]);      // (exact: |Z| < 2^53)
    }
    __syncthreads();
    if (tid < 3) {
        double z = 0;
        for (int i = 0; i < 256; ++i) z += zr[tid * 256 + i];
        zs[tid] = z;
    }
    __syncthreads();
    const int r = r0 + tid;
    if (r >= rows) return;
    const double sg = ((r + pad) & 1) ? -1.0 : 1.0;
    for (int c = 0; c < 3; ++c) {
        const double* s = sr + c * win + tid;
        double acc[4] = { 0, 0, 0, 0 };
        int t = 0;
        for (; t + 4 <= ntap; t += 4) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __builtin_fma(tp[t + j], s[t + j], acc[j]);
        }
        for (; t < ntap; ++t) acc[0] = __builtin_fma(tp[t], s[t], acc[0]);
        h[(static_cast<size_t>(f) * 3 + c) * rows + r] =
            static_cast<float>(static_cast<double>(dr) * (((acc[0] + acc[1]) + (acc[2] + acc[3])) + static_cast<double>(dc) * sg * zs[c]));
    }
}

// ------------------------------------------------------------------------------------
// fastboxblur: one sweep of the sliding accumulator along lines of length n.
// Element (line l, position x, channel c) at buf[l*lstride + x*xstride + c].
// A wave owns 64 adjacent (line, channel) accumulators; along the line it walks
// sequentially (the accumulator recurrence), so for the vertical sweep (xstride = row
// pitch) the 64 lanes read 64 adjacent bytes, and for the horizontal sweep the lines are
// first brought through LDS in chunks.  V1: direct global accesses, L2 absorbs the reuse.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ int refl101(int i, int n)
{
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
    return i;
}

__global__ __launch_bounds__(256) void boxsweep_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int nlines, int n,
                                                       size_t lstride, size_t xstride, int C, int r, int seg_len)
{
    // work item = (segment, line*C + c); segments split long lines so the grid fills the chip
    const int lc_total = nlines * C;
    const int nseg = (n + seg_len - 1) / seg_len;
    const long long gid = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (gid >= static_cast<long long>(lc_total) * nseg) return;
    const int lc = static_cast<int>(gid % lc_total), seg = static_cast<int>(gid / lc_total);
    const int l = lc / C, c = lc - l * C;
    const uint8_t* ip = in + static_cast<size_t>(l) * lstride + c;
    uint8_t* op = out + static_cast<size_t>(l) * lstride + c;
    const float iarr = 1.f / static_cast<float>(r + r + 1);
    const int xs = seg * seg_len, xe = min(n, xs + seg_len);
    int acc = 0;
    for (int d = -r; d <= r; ++d) acc += ip[static_cast<size_t>(refl101(xs + d, n)) * xstride];
    op[static_cast<size_t>(xs) * xstride] = static_cast<uint8_t>(static_cast<int>(static_cast<float>(acc) * iarr + 0.5f));
    for (int x = xs + 1; x < xe; ++x) {
        acc += ip[static_cast<size_t>(refl101(x + r, n)) * xstride];
        acc -= ip[static_cast<size_t>(refl101(x - r - 1, n)) * xstride];
        op[static_cast<size_t>(x) * xstride] = static_cast<uint8_t>(static_cast<int>(static_cast<float>(acc) * iarr + 0.5f));
    }
}

// Vertical sweep, four adjacent bytes (column-channels) per thread: dword loads/stores, lanes
// cover 256 contiguous bytes of an image row, the walk along y is the accumulator recurrence.
// Segments along y give the grid enough threads; each pays 2r+1 loads to start its window.
__global__ __launch_bounds__(256) void boxcol4_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                      int h, int pitch4 /* dwords per row */, int r, int seg_len, int nseg)
{
    const long long gid = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (gid >= static_cast<long long>(pitch4) * nseg) return;
    const int xq = static_cast<int>(gid % pitch4), seg = static_cast<int>(gid / pitch4);
    const uint32_t* ip = reinterpret_cast<const uint32_t*>(in) + xq;
    uint32_t* op = reinterpret_cast<uint32_t*>(out) + xq;
    const float iarr = 1.f / static_cast<float>(r + r + 1);
    const int ys = seg * seg_len, ye = min(h, ys + seg_len);
    if (ys >= ye) return;
    int a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    auto add = [&](int y, int sgn) {
        const uint32_t v = ip[static_cast<size_t>(refl101(y, h)) * pitch4];
        a0 += sgn * static_cast<int>(v & 0xffu);
        a1 += sgn * static_cast<int>((v >> 8) & 0xffu);
        a2 += sgn * static_cast<int>((v >> 16) & 0xffu);
        a3 += sgn * static_cast<int>(v >> 24);
    };
    auto emit = [&](int y) {
        const uint32_t b0 = static_cast<uint32_t>(static_cast<int>(static_cast<float>(a0) * iarr + 0.5f)) & 0xffu;
        const uint32_t b1 = static_cast<uint32_t>(static_cast<int>(static_cast<float>(a1) * iarr + 0.5f)) & 0xffu;
        const uint32_t b2 = static_cast<uint32_t>(static_cast<int>(static_cast<float>(a2) * iarr + 0.5f)) & 0xffu;
        const uint32_t b3 = static_cast<uint32_t>(static_cast<int>(static_cast<float>(a3) * iarr + 0.5f)) & 0xffu;
        op[static_cast<size_t>(y) * pitch4] = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
    };
    for (int d = -r; d <= r; ++d) add(ys + d, 1);
    emit(ys);
    int y = ys + 1;
    if (ys - r - 1 >= 0 && ye + r < h) {                // interior segment: loads of four rows in flight together
        for (; y + 4 <= ye; y += 4) {
            uint32_t vi[4], vo[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                vi[i] = ip[static_cast<size_t>(y + i + r) * pitch4];
                vo[i] = ip[static_cast<size_t>(y + i - r - 1) * pitch4];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                a0 += static_cast<int>(vi[i] & 0xffu) - static_cast<int>(vo[i] & 0xffu);
                a1 += static_cast<int>((vi[i] >> 8) & 0xffu) - static_cast<int>((vo[i] >> 8) & 0xffu);
                a2 += static_cast<int>((vi[i] >> 16) & 0xffu) - static_cast<int>((vo[i] >> 16) & 0xffu);
                a3 += static_cast<int>(vi[i] >> 24) - static_cast<int>(vo[i] >> 24);
                emit(y + i);
            }
        }
    }
    for (; y < ye; ++y) {
        add(y + r, 1);
        add(y - r - 1, -1);
        emit(y);
    }
}

// All `passes` horizontal sweeps of one image row in one go: the row lives in LDS (two byte
// buffers, ping-pong), each thread walks one (channel, segment) with the sliding accumulator,
// u8 rounding after every sweep exactly as the per-sweep kernel does.  HBM sees the row once
// in and once out instead of once per pass.
__global__ __launch_bounds__(256) void boxrow_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                     int w, int C, int r, int passes, int seg_len, int nseg)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int rb = w * C;                               // bytes per row
    const int rb4 = (rb + 3) & ~3;
    uint8_t* a = reinterpret_cast<uint8_t*>(smem);
    uint8_t* b = a + rb4;
    const uint8_t* src = in + static_cast<size_t>(blockIdx.x) * rb;
    uint8_t* dst = out + static_cast<size_t>(blockIdx.x) * rb;
    if ((rb & 3) == 0) {
        for (int i = threadIdx.x; i < rb / 4; i += 256) reinterpret_cast<uint32_t*>(a)[i] = reinterpret_cast<const uint32_t*>(src)[i];
    } else {
        for (int i = threadIdx.x; i < rb; i += 256) a[i] = src[i];
    }
    __syncthreads();
    const float iarr = 1.f / static_cast<float>(r + r + 1);
    for (int p = 0; p < passes; ++p) {
        for (int item = threadIdx.x; item < C * nseg; item += 256) {
            const int c = item % C, seg = item / C;
            const int xs = seg * seg_len, xe = min(w, xs + seg_len);
            if (xs >= xe) continue;
            // restrict: the sweep reads one buffer and writes the other, so the LDS reads of several steps may be
            // issued together instead of one read latency per step behind the previous step's store
            const uint8_t* __restrict__ s = a + c;
            uint8_t* __restrict__ d = b + c;
            int acc = 0;
            if (xs - r - 1 >= 0 && xe + r < w) {        // interior segment: no reflection anywhere
#pragma unroll 8
                for (int x = xs - r; x <= xs + r; ++x) acc += s[x * C];
                d[xs * C] = static_cast<uint8_t>(static_cast<int>(static_cast<float>(acc) * iarr + 0.5f));
                int x = xs + 1;
                for (; x + 8 <= xe; x += 8) {
                    int in_[8], out_[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) { in_[i] = s[(x + i + r) * C]; out_[i] = s[(x + i - r - 1) * C]; }
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        acc += in_[i] - out_[i];
                        d[(x + i) * C] = static_cast<uint8_t>(static_cast<int>(static_cast<float>(acc) * iarr + 0.5f));
                    }
                }
                for (; x < xe; ++x) {
                    acc += s[(x + r) * C] - s[(x - r - 1) * C];
                    d[x * C] = static_cast<uint8_t>(static_cast<int>(static_cast<float>(acc) * iarr + 0.5f));
                }
            } else {
                for (int x = xs - r; x <= xs + r; ++x) acc += s[refl101(x, w) * C];
                d[xs * C] = static_cast<uint8_t>(static_cast<int>(static_cast<float>(acc) * iarr + 0.5f));
                for (int x = xs + 1; x < xe; ++x) {
                    acc += s[refl101(x + r, w) * C] - s[refl101(x - r - 1, w) * C];
                    d[x * C] = static_cast<uint8_t>(static_cast<int>(static_cast<float>(acc) * iarr + 0.5f));
                }
            }
        }
        __syncthreads();
        uint8_t* t = a; a = b; b = t;
    }
    if ((rb & 3) == 0) {
        for (int i = threadIdx.x; i < rb / 4; i += 256) reinterpret_cast<uint32_t*>(dst)[i] = reinterpret_cast<const uint32_t*>(a)[i];
    } else {
        for (int i = threadIdx.x; i < rb; i += 256) dst[i] = a[i];
    }
}

// All `passes` horizontal sweeps of one image row, four pixels per step.  The row sits in LDS with reflect-101
// borders written out physically (r + 1 pixels on each side, refreshed after every sweep), so every segment takes
// the same branch-free path: per group of four pixels the entering and the leaving 4*C bytes are fetched as aligned
// dwords (+ v_alignbyte with a shift that is uniform for the whole launch), the 4*C outputs leave as C dwords.
// Against the byte-wise kernel above: 3.3x fewer LDS instructions in the walk, 2.9x fewer in the window set-up, no
// slow border segments.  Same integer accumulators and the same float rounding, so the bytes are identical.
template <int C>
__global__ __launch_bounds__(256) void boxrow4_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                      int w, int r, int passes, int groups_per_thread, int off0, int buf_bytes)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint8_t* a = reinterpret_cast<uint8_t*>(smem);
    uint8_t* b = a + buf_bytes;
    const int rb = w * C;
    const uint8_t* src = in + static_cast<size_t>(blockIdx.x) * rb;
    uint8_t* dst = out + static_cast<size_t>(blockIdx.x) * rb;
    if ((rb & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 3) == 0) {
        for (int i = threadIdx.x; i < rb / 4; i += 256) reinterpret_cast<uint32_t*>(a + off0)[i] = reinterpret_cast<const uint32_t*>(src)[i];
    } else {
        for (int i = threadIdx.x; i < rb; i += 256) a[off0 + i] = src[i];
    }
    const float iarr = 1.f / static_cast<float>(r + r + 1);
    const int xs = static_cast<int>(threadIdx.x) * groups_per_thread * 4;
    const int ngroups = xs < w ? min(groups_per_thread, (w - xs + 3) / 4) : 0;
    // byte offsets (mod 4) of the two streams: uniform because xs is a multiple of 4
    const int sh_in = (r * C) & 3, sh_out = ((-(r + 1)) * C) & 3;
    for (int p = 0; p < passes; ++p) {
        __syncthreads();                                     // the row (or the previous sweep) is complete
        // reflect-101 borders: pixels -(r+1) .. -1 and w .. w+r (the outermost one on the left only ever cancels out)
        for (int i = threadIdx.x; i < 2 * (r + 1) * C; i += 256) {
            const int side = i / ((r + 1) * C), k = i - side * (r + 1) * C;
            const int px = k / C, c = k - px * C;
            const int x = side ? w + px : -(px + 1);
            int m = x < 0 ? -x : 2 * (w - 1) - x;
            m = m < 0 ? 0 : (m > w - 1 ? w - 1 : m);
            a[off0 + x * C + c] = a[off0 + m * C + c];
        }
        __syncthreads();
        if (ngroups > 0) {
            const uint32_t* __restrict__ s32 = reinterpret_cast<const uint32_t*>(a);
            uint32_t* __restrict__ d32 = reinterpret_cast<uint32_t*>(b);
            // aligned dword index of the byte where a stream's group starts
            auto stream = [&](int byte_off, int sh, uint32_t (&g)[C]) {
                const int q = (off0 + byte_off - sh) >> 2;
                uint32_t t[C + 1];
#pragma unroll
                for (int k = 0; k <= C; ++k) t[k] = s32[q + k];
#pragma unroll
                for (int k = 0; k < C; ++k) g[k] = __builtin_amdgcn_alignbyte(t[k + 1], t[k], sh);
            };
            auto byte_of = [](const uint32_t (&g)[C], int k) -> int { return static_cast<int>((g[k >> 2] >> (8 * (k & 3))) & 0xffu); };
            int acc[C];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = 0;
            // window centred on pixel xs - 1: pixels xs-1-r .. xs-1+r = 2r+1 pixels from the "leaving" stream position
            {
                const int np = 2 * r + 1;
                int px = 0;
                for (; px + 4 <= np; px += 4) {
                    uint32_t g[C];
                    stream((xs - 1 - r + px) * C, sh_out, g);
#pragma unroll
                    for (int k = 0; k < 4 * C; ++k) acc[k % C] += byte_of(g, k);
                }
                for (; px < np; ++px) {
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[c] += a[off0 + (xs - 1 - r + px) * C + c];
                }
            }
            for (int gi = 0; gi < ngroups; ++gi) {
                const int x = xs + 4 * gi;
                uint32_t gin[C], gout[C], res[C];
                stream((x + r) * C, sh_in, gin);
                stream((x - r - 1) * C, sh_out, gout);
#pragma unroll
                for (int k = 0; k < C; ++k) res[k] = 0;
#pragma unroll
                for (int k = 0; k < 4 * C; ++k) {
                    acc[k % C] += byte_of(gin, k) - byte_of(gout, k);
                    const uint32_t v = static_cast<uint32_t>(static_cast<int>(static_cast<float>(acc[k % C]) * iarr + 0.5f)) & 0xffu;
                    res[k >> 2] |= v << (8 * (k & 3));
                }
#pragma unroll
                for (int k = 0; k < C; ++k) d32[((off0 + x * C) >> 2) + k] = res[k];
            }
        }
        uint8_t* t = a; a = b; b = t;
    }
    __syncthreads();
    if ((rb & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
        for (int i = threadIdx.x; i < rb / 4; i += 256) reinterpret_cast<uint32_t*>(dst)[i] = reinterpret_cast<const uint32_t*>(a + off0)[i];
    } else {
        for (int i = threadIdx.x; i < rb; i += 256) dst[i] = a[off0 + i];
    }
}


// ------------------------------------------------------------------------------------
// Whole-image 2D transform path: pocketfft_2D (Source.cpp:143-277) and its DFT_image branch (:235-252).
//
// The padded image (Reflect_101 on all four sides, :178-180) is transformed as ONE 2D FFT.  Two colour planes ride in
// one complex image z = a + i b (the kernel spectrum is real, so they never mix in the blur; for the spectrum image
// they are separated with F_a[k] = (Z[k] + conj Z[-k]) / 2).  Spectra stay in the position order of the plans along
// both axes; nothing is reordered in memory.
//
//   img2d_rows_fwd   u8 image -> z rows: reflect-101 + deinterleave + pack fused into the load, forward FFT along x
//   img2d_cols<true> strip of G columns: (x Krow[pos_x]) -> forward along y -> x Kcol[pos_y] -> inverse along y  (:255-260)
//   img2d_cols<false>                    forward along y only (DFT_image keeps the spectrum)
//   img2d_rows_inv   rows of the crop: inverse along x, "+0.5f, truncate", crop (:263-276) -> u8 image
//   img2d_logspec    fftshift + 20 log10(|Re F| + 1e-5) with the reference's index arithmetic (:238-251), crop
// ------------------------------------------------------------------------------------
struct Img2dGeom { int rows, cols, s0, s1, top, left; };

__global__ __launch_bounds__(256) void img2d_rows_fwd_kernel(const uint8_t* __restrict__ src, float2* __restrict__ z, Img2dGeom g, int ca, int cb,
                                                             DevPlan plan, const float2* __restrict__ tw)
{
    extern __shared__ float2 lds2d[];
    const int zs = line_stride(plan.n);
    const int y = blockIdx.x;
    const uint8_t* row = src + static_cast<size_t>(refl101(y - g.top, g.rows)) * g.cols * 3;
    for (int x = threadIdx.x; x < g.s1; x += blockDim.x) {
        const uint8_t* px = row + 3 * refl101(x - g.left, g.cols);
        lds2d[phys(x)] = make_float2(static_cast<float>(px[ca]), cb >= 0 ? static_cast<float>(px[cb]) : 0.f);
    }
    __syncthreads();
    fft_forward_lines<1>(lds2d, zs, plan, tw);
    float2* out = z + static_cast<size_t>(y) * g.s1;
    for (int pos = threadIdx.x; pos < g.s1; pos += blockDim.x) out[pos] = lds2d[phys(pos)];
}

template <int G, bool CONV>
__global__ __launch_bounds__(256) void img2d_cols_kernel(float2* __restrict__ z, int s0, int s1, DevPlan plan, const float2* __restrict__ tw,
                                                         const float* __restrict__ mcol, const float* __restrict__ krow_pos)
{
    extern __shared__ float2 lds2d[];
    const int zs = line_stride(plan.n);
    const int x0 = blockIdx.x * G;
    for (int idx = threadIdx.x; idx < s0 * G; idx += blockDim.x) {
        const int y = idx / G, c = idx - y * G, x = x0 + c;
        float2 v = make_float2(0.f, 0.f);
        if (x < s1) {
            v = z[static_cast<size_t>(y) * s1 + x];
            if (CONV) v = cscale(v, krow_pos[x]);
        }
        lds2d[c * zs + phys(y)] = v;
    }
    __syncthreads();
    if (CONV) fftconv_lines<G>(lds2d, zs, plan, tw, mcol);
    else fft_forward_lines<G>(lds2d, zs, plan, tw);
    for (int idx = threadIdx.x; idx < s0 * G; idx += blockDim.x) {
        const int y = idx / G, c = idx - y * G, x = x0 + c;
        if (x < s1) z[static_cast<size_t>(y) * s1 + x] = lds2d[c * zs + phys(y)];
    }
}

__global__ __launch_bounds__(256) void img2d_rows_inv_kernel(const float2* __restrict__ z, uint8_t* __restrict__ dst, float* __restrict__ planes, Img2dGeom g,
                                                             int ca, int cb, DevPlan plan, const float2* __restrict__ tw)
{
    extern __shared__ float2 lds2d[];
    const int zs = line_stride(plan.n);
    const int i = blockIdx.x;                                   // row of the cropped image
    const float2* in = z + static_cast<size_t>(i + g.top) * g.s1;
    for (int pos = threadIdx.x; pos < g.s1; pos += blockDim.x) lds2d[phys(pos)] = in[pos];
    __syncthreads();
    fft_inverse_lines<1>(lds2d, zs, plan, tw);
    const size_t plane = static_cast<size_t>(g.rows) * g.cols;
    for (int j = threadIdx.x; j < g.cols; j += blockDim.x) {
        const float2 v = lds2d[phys(j + g.left)];
        const size_t px = static_cast<size_t>(i) * g.cols + j;
        dst[3 * px + ca] = static_cast<uint8_t>(static_cast<int>(v.x + 0.5f));
        if (cb >= 0) dst[3 * px + cb] = static_cast<uint8_t>(static_cast<int>(v.y + 0.5f));
        if (planes) {
            planes[ca * plane + px] = v.x;
            if (cb >= 0) planes[cb * plane + px] = v.y;
        }
    }
}

__global__ __launch_bounds__(256) void img2d_logspec_kernel(const float2* __restrict__ z, uint8_t* __restrict__ dst, float* __restrict__ planes, Img2dGeom g,
                                                            int ca, int cb, const int* __restrict__ pos_of_freq_y, const int* __restrict__ pos_of_freq_x)
{
    const size_t plane = static_cast<size_t>(g.rows) * g.cols;
    for (size_t px = blockIdx.x * 256u + threadIdx.x; px < plane; px += static_cast<size_t>(gridDim.x) * 256u) {
        const int i = static_cast<int>(px / g.cols), j = static_cast<int>(px - static_cast<size_t>(i) * g.cols);
        const int row = i + g.top, col = j + g.left;
        // FFTSHIFT, "odd/even treated as in matlab" (Source.cpp:239-241)
        const int fy = (row + (g.s0 % 2 == 0 ? g.s0 : g.s0 + 1) / 2) % g.s0;
        const int col_ = (col + (g.s1 % 2 == 0 ? g.s1 : g.s1 + 1) / 2) % g.s1;
        // "Reverse reading from end to the beginning after reached (sizes[1] / 2 + 1)" (:243): the reference indexes
        // its HALF spectrum, so the right half shows column s1/2 - col_ % (s1/2) of the SAME row
        const int fx = col_ < g.s1 / 2 + 1 ? col_ : g.s1 / 2 - col_ % (g.s1 / 2);
        const float2 p = z[static_cast<size_t>(pos_of_freq_y[fy]) * g.s1 + pos_of_freq_x[fx]];
        const float2 q = z[static_cast<size_t>(pos_of_freq_y[(g.s0 - fy) % g.s0]) * g.s1 + pos_of_freq_x[(g.s1 - fx) % g.s1]];
        const float va = 20.f * log10f(fabsf(0.5f * (p.x + q.x)) + 0.00001f);
        dst[3 * px + ca] = static_cast<uint8_t>(static_cast<int>(va + 0.5f));
        if (planes) planes[ca * plane + px] = va;
        if (cb >= 0) {
            const float vb = 20.f * log10f(fabsf(0.5f * (p.y + q.y)) + 0.00001f);
            dst[3 * px + cb] = static_cast<uint8_t>(static_cast<int>(vb + 0.5f));
            if (planes) planes[cb * plane + px] = vb;
        }
    }
}

// 16 bytes per lane, grid-stride: the access shape of the engines' wide loads and stores (blur_copy_bandwidth)
__global__ __launch_bounds__(256) void copy16_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t n16)
{
    for (size_t i = blockIdx.x * 256ull + threadIdx.x; i < n16; i += static_cast<size_t>(gridDim.x) * 256ull) dst[i] = src[i];
}

// Reflect_101<uint8_t, C> (Utils.hpp:212-243) as a piece: out[(rows+top+bottom) x (cols+left+right) x C]
__global__ __launch_bounds__(256) void reflect101_u8_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int rows, int cols, int C,
                                                            int top, int left, int out_rows, int out_cols)
{
    const size_t total = static_cast<size_t>(out_rows) * out_cols;
    for (size_t px = blockIdx.x * 256u + threadIdx.x; px < total; px += static_cast<size_t>(gridDim.x) * 256u) {
        const int y = static_cast<int>(px / out_cols), x = static_cast<int>(px - static_cast<size_t>(y) * out_cols);
        const uint8_t* s = in + (static_cast<size_t>(refl101(y - top, rows)) * cols + refl101(x - left, cols)) * C;
        for (int c = 0; c < C; ++c) out[px * C + c] = s[c];
    }
}

}  // namespace

// ======================================================================================
// host side: context, caches, launches
// ======================================================================================
struct DevicePlan {
    FftPlan host;
    DevPlan dev{};
    float2* d_tw = nullptr;
    const FastEntry* fast = nullptr;   // compile-time specialised kernels for this length, if any
    int key = 0;
    int* d_pos_of_freq = nullptr;      // inverse of freq_of_pos, uploaded on first use (whole-image 2D path)
};

// staging for blur_gaussian_u8c3_host_batch: frame i+1 travels to the device and frame i-1 back to the host
// while frame i is in the kernels (three slots, two copy streams beside the context's kernel stream)
struct HostPipe {
    static constexpr int S = 3;
    hipStream_t h2d = nullptr, d2h = nullptr;
    uint8_t* buf[S] = { nullptr, nullptr, nullptr };
    size_t bytes = 0;
    hipEvent_t in_done[S] = {}, comp_done[S] = {}, out_done[S] = {};
    bool ready = false;
};

struct MxTables {
    void* frags_row = nullptr;   // [2][nkb][64][8] binary16 (host_math.hpp: mx_fragments)
    void* frags_col = nullptr;
    float* taps_row = nullptr;   // 2 pad + 1 floats, centre at pad (the same taps serve both axes)
    float dr = 0.f, dc = 0.f;    // m[0] - m[N/2] of the reference's row / column transform length (the quirk's gain)
};

struct blur_ctx {
    int device = 0;
    HostPipe pipe;
    hipStream_t stream = nullptr;
    std::string err;
    std::map<int, std::unique_ptr<DevicePlan>> plans;   // key: 4*n + role (0 generic, 1 specialised row, 2 specialised column)
    // (plan key, ksize, quirk, sigma bits) -> device multiplier table in position order
    std::map<std::tuple<int, int, int, uint64_t>, float*> spectra;
    std::map<int, float*> last_spectrum;   // n -> most recent table (diagnostic stamp read-back)
    int num_cus = 256;           // hipDeviceProp_t::multiProcessorCount
    int num_xcds = 8;            // hipDeviceAttributeNumberOfXccs
    // wave-resident engine (wr_kernels.hpp): shared 256-point twiddles, pass-0 twiddles per R0, multiplier tables
    float2* d_w256 = nullptr;
    std::map<int, float2*> wr_tw0;
    std::map<std::tuple<int, int, int, int, uint64_t>, float*> wr_spectra;   // (n, n_ref, ksize | -1, quirk, sigma bits | hash)
    struct LinesTable { uint64_t hash; std::vector<float> host; float* dev; };
    std::list<LinesTable> lines_tables;                                     // blur_convolve_lines_c32_dev: caller tables, LRU, bounded
    // matrix-core engine (mx_kernels.hpp): Toeplitz fragments + taps per kernel, integer sums and float terms of the quirk
    std::map<std::tuple<int, int, int, int, int, uint64_t>, MxTables> mx_tables;   // (ksize | -1, pad, nkb, n_row, n_col, sigma bits | hash)
    uint8_t* fx_strips = nullptr;   // fused kernel: the edge chunks' windows with the mirrored pixels in place
    size_t fx_strips_bytes = 0;
    int* fx_sums = nullptr;         // fused kernel, quirk: the pre-pass's partial sums (run_fx_u8c3)
    size_t fx_sums_bytes = 0;
    // tiled wave-resident path: the quirk's sums and term vectors of one frame, a copy of an in-place frame, the taps per kernel
    int* tl_sums = nullptr;
    size_t tl_sums_bytes = 0;
    float* tl_terms = nullptr;
    size_t tl_terms_bytes = 0;
    uint8_t* tl_copy = nullptr;
    size_t tl_copy_bytes = 0;
    std::map<std::pair<uint64_t, int>, float*> tl_taps;      // (sigma bits, kSize) -> 2 pad + 1 taps on the device
    int* mx_sums = nullptr;
    size_t mx_sums_bytes = 0;
    float* mx_terms = nullptr;
    size_t mx_terms_bytes = 0;
    float* work = nullptr;       // float planes of one frame
    size_t work_bytes = 0;
    float* work2 = nullptr;      // second set of planes: very tall images only (column pass without the LDS pixel stage)
    size_t work2_bytes = 0;
    uint8_t* box_tmp = nullptr;
    float* ch_planes = nullptr;      // 1- / 4-channel plane fallback: the frame's f32 planes
    size_t ch_planes_bytes = 0;
    uint8_t* ch_copy = nullptr;      // 1- / 4-channel images: a copy of overlapping source frames
    size_t ch_copy_bytes = 0;
    void* ff_sums = nullptr;         // float32 / u16 / half images, fused kernel: max|x| per frame (not u16) and the quirk's sums (run_ff)
    size_t ff_sums_bytes = 0;
    void* ff_strips = nullptr;       // float32 / u16 / half images, fused kernel: the edge chunks' windows (samples of the frame's type)
    size_t ff_strips_bytes = 0;
    // one sigma per frame (blur_ch_frame_sigmas_batch_impl): the call's frame list, fragments and taps on the device, and the pinned
    // host memory they are uploaded from; fs_uploaded is recorded behind the upload that last read the staging memory
    void* fs_table = nullptr;
    size_t fs_table_bytes = 0;
    void* fs_stage = nullptr;
    size_t fs_stage_bytes = 0;
    hipEvent_t fs_uploaded = nullptr;
    bool fs_pending = false;
    size_t box_bytes = 0;
    std::string engine_note;      // BLUR_ENGINE_AUTO: why the last call's choice passed over a faster engine ("" if it did not)
    int last_family = -1;         // kernels the last u8c3 blur used: 0 run-time plans, 1 specialised rows-first, 2 wave-resident, 3 whole-image 2D, 4 matrix-core (two kernels), 6 fused matrix-core
    void* host_stage = nullptr;   // device staging of the host-pointer entry points (kept between calls: no allocation per frame)
    size_t host_stage_bytes = 0;
    int timing = 0;              // 0 off, 1 every timed launch, 2 slot 0 only (blur_ctx_timing_enable)
    std::vector<std::tuple<hipEvent_t, hipEvent_t, int, int>> ev_busy;   // start, stop, kernel (0 row / 1 column), frames
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_free;
    double ms[2] = { 0, 0 };
    int launches[2] = { 0, 0 };
    int frames[2] = { 0, 0 };
};

static thread_local std::string g_create_err;

#define HIP_TRY(ctx, call)                                                                          \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                         \
            return BLUR_ERR_HIP;                                                                    \
        }                                                                                           \
    } while (0)

static int fail(blur_ctx* ctx, int code, const char* msg)
{
    if (ctx) ctx->err = msg;
    return code;
}

static int get_plan(blur_ctx* ctx, int n, bool want_fast, bool column_role, DevicePlan** out)
{
    const FastEntry* fe = want_fast ? find_fast_entry(n, column_role) : nullptr;
    const int key = 4 * n + (fe ? (column_role ? 2 : 1) : 0);
    auto it = ctx->plans.find(key);
    if (it != ctx->plans.end()) { *out = it->second.get(); return BLUR_OK; }
    auto dp = std::make_unique<DevicePlan>();
    dp->fast = fe;
    dp->key = key;
    const bool ok = fe ? make_plan_radices(n, fe->radix, fe->npass, dp->host) : make_plan(n, dp->host);
    if (!ok) return fail(ctx, BLUR_ERR_UNSUPPORTED, "FFT length is not 2^a 3^b 5^c");
    dp->dev.n = n;
    dp->dev.npass = dp->host.npass;
    for (int i = 0; i < dp->host.npass; ++i) {
        dp->dev.radix[i] = dp->host.radix[i];
        dp->dev.m[i] = dp->host.m[i];
        dp->dev.tw_off[i] = dp->host.tw_off[i];
    }
    const size_t bytes = std::max<size_t>(dp->host.tw.size() * sizeof(float), 16);
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&dp->d_tw), bytes));
    if (!dp->host.tw.empty())
        HIP_TRY(ctx, hipMemcpy(dp->d_tw, dp->host.tw.data(), dp->host.tw.size() * sizeof(float), hipMemcpyHostToDevice));
    *out = dp.get();
    ctx->plans[key] = std::move(dp);
    return BLUR_OK;
}

static int get_spectrum(blur_ctx* ctx, const DevicePlan& plan, double sigma, int ksize, bool quirk, float** out)
{
    uint64_t bits;
    std::memcpy(&bits, &sigma, sizeof bits);
    const auto key = std::make_tuple(plan.key, ksize, quirk ? 1 : 0, bits);
    auto it = ctx->spectra.find(key);
    if (it != ctx->spectra.end()) { *out = it->second; return BLUR_OK; }
    const int n = plan.dev.n;
    std::vector<float> m(n / 2 + 1), mp(n);
    kernel_multipliers(sigma, ksize, n, m.data());
    permuted_multipliers(plan.host, m.data(), quirk, mp.data());
    float* d = nullptr;
    // the tail behind the table is only written by -DFK_STAMPS diagnostic builds
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&d), sizeof(float) * (n + kStampTailFloats)));
    HIP_TRY(ctx, hipMemset(d, 0, sizeof(float) * (n + kStampTailFloats)));
    HIP_TRY(ctx, hipMemcpy(d, mp.data(), sizeof(float) * n, hipMemcpyHostToDevice));
    ctx->spectra[key] = d;
    ctx->last_spectrum[plan.key] = d;
    *out = d;
    return BLUR_OK;
}

// multiplier table of a caller-supplied n-periodic kernel (box/tent mode, user kernels); cached by content
static int get_spectrum_custom(blur_ctx* ctx, const DevicePlan& plan, const std::vector<float>& karr, bool quirk, float** out)
{
    uint64_t h = 1469598103934665603ull;                         // FNV-1a over the kernel bytes
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(karr.data());
    for (size_t i = 0; i < karr.size() * sizeof(float); ++i) { h ^= bytes[i]; h *= 1099511628211ull; }
    const auto key = std::make_tuple(plan.key, -1, quirk ? 1 : 0, h);
    auto it = ctx->spectra.find(key);
    if (it != ctx->spectra.end()) { *out = it->second; return BLUR_OK; }
    const int n = plan.dev.n;
    std::vector<float> m(n / 2 + 1), mp(n);
    kernel_multipliers_from_array(karr.data(), n, m.data());
    permuted_multipliers(plan.host, m.data(), quirk, mp.data());
    float* d = nullptr;
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&d), sizeof(float) * (n + kStampTailFloats)));
    HIP_TRY(ctx, hipMemset(d, 0, sizeof(float) * (n + kStampTailFloats)));
    HIP_TRY(ctx, hipMemcpy(d, mp.data(), sizeof(float) * n, hipMemcpyHostToDevice));
    ctx->spectra[key] = d;
    ctx->last_spectrum[plan.key] = d;
    *out = d;
    return BLUR_OK;
}

// device staging buffer of the host-pointer entry points, grown on demand and kept in the context
static int ensure_host_stage(blur_ctx* ctx, size_t bytes, void** out)
{
    if (ctx->host_stage_bytes < bytes) {
        if (ctx->host_stage) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); HIP_TRY(ctx, hipFree(ctx->host_stage)); ctx->host_stage = nullptr; ctx->host_stage_bytes = 0; }
        HIP_TRY(ctx, hipMalloc(&ctx->host_stage, bytes ? bytes : 1));
        ctx->host_stage_bytes = bytes;
    }
    *out = ctx->host_stage;
    return BLUR_OK;
}

// The float workspace sits between two guard bands of kWorkGuard bytes filled with 0xA5 when it is allocated;
// blur_debug_check_workspace_guards() counts the guard bytes that no longer hold it (redzone tests).
constexpr size_t kWorkGuard = 4096;
static int ensure_work(blur_ctx* ctx, size_t bytes)
{
    if (ctx->work_bytes >= bytes) return BLUR_OK;
    if (ctx->work) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipFree(reinterpret_cast<char*>(ctx->work) - kWorkGuard));
        ctx->work = nullptr;
        ctx->work_bytes = 0;
    }
    char* base = nullptr;
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&base), bytes + 2 * kWorkGuard));
    HIP_TRY(ctx, hipMemset(base, 0xA5, kWorkGuard));
    HIP_TRY(ctx, hipMemset(base + kWorkGuard + bytes, 0xA5, kWorkGuard));
    ctx->work = reinterpret_cast<float*>(base + kWorkGuard);
    ctx->work_bytes = bytes;
    return BLUR_OK;
}

// ---- event timing -----------------------------------------------------------------
static int timing_drain(blur_ctx* ctx)
{
    for (auto& t : ctx->ev_busy) {
        hipEvent_t a = std::get<0>(t), b = std::get<1>(t);
        HIP_TRY(ctx, hipEventSynchronize(b));
        float ms = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, a, b));
        ctx->ms[std::get<2>(t)] += ms;
        ctx->launches[std::get<2>(t)] += 1;
        ctx->frames[std::get<2>(t)] += std::get<3>(t);
        ctx->ev_free.emplace_back(a, b);
    }
    ctx->ev_busy.clear();
    return BLUR_OK;
}

struct TimedLaunch {
    blur_ctx* ctx; int which; int nframes; hipEvent_t a = nullptr, b = nullptr; bool on;
    TimedLaunch(blur_ctx* c, int w, int nf = 1) : ctx(c), which(w), nframes(nf), on(c->timing == 1 || (c->timing == 2 && w == 0))
    {
        if (!on) return;
        if (ctx->ev_busy.size() >= 8192) timing_drain(ctx);
        if (ctx->ev_free.empty()) {
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { on = false; return; }
        } else { a = ctx->ev_free.back().first; b = ctx->ev_free.back().second; ctx->ev_free.pop_back(); }
        (void)hipEventRecord(a, ctx->stream);
    }
    ~TimedLaunch()
    {
        if (!on) return;
        (void)hipEventRecord(b, ctx->stream);
        ctx->ev_busy.emplace_back(a, b, which, nframes);
    }
};

// ---- launches ---------------------------------------------------------------------
static size_t row_lds_bytes(int n) { return static_cast<size_t>(line_stride(n)) * sizeof(float2); }
static size_t col_lds_bytes(int n, int C, int rows, int out_bytes_per_px)
{
    return static_cast<size_t>(C) * line_stride(n) * sizeof(float2) + (out_bytes_per_px ? static_cast<size_t>(rows) * 2 * C * out_bytes_per_px : 0) + 16;
}

// threads per workgroup of the run-time-planned kernels by the LDS a workgroup takes (BLUR_GENERIC_THREADS overrides: developer
// knob).  Measured on single images of the reference's sweep (4000 x 6000 sigma 77.5 / 7600 x 11400 sigma 106.8; 256, 512, 1024
// threads): column kernel 908 / 606 / 622 and 3517 / 2673 / 2694 us -- long lines leave room for one or two workgroups per CU and
// four waves per CU hide nothing of the strip gather; row kernel 367 / 459 / 437 and 1641 / 1263 / 1210 us -- better only for the
// longest lines.
static int generic_threads(size_t lds, bool column_pass)
{
    static const int forced = [] { const char* e = getenv("BLUR_GENERIC_THREADS"); return e && *e ? atoi(e) : 0; }();
    if (forced == 256 || forced == 512 || forced == 1024) return forced;
    if (column_pass) return lds > 40 * 1024 ? 512 : 256;
    return lds > 80 * 1024 ? 1024 : 256;
}

template <typename K> static int set_lds(blur_ctx* ctx, K kernel, size_t bytes)
{
    if (bytes > 64 * 1024)
        HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes)));
    return BLUR_OK;
}

template <typename InT, int CH>
static int launch_rowpass(blur_ctx* ctx, const InT* src, float* planes, int rows, int cols, int pad,
                          const DevicePlan& plan, const float* mperm, int gshift = 0)
{
    const size_t lds = row_lds_bytes(plan.dev.n);
    DevPlan dv = plan.dev;
    dv.nxcd = ctx->num_xcds;
    if (lds > kLdsLimit) return fail(ctx, BLUR_ERR_UNSUPPORTED, "row FFT length exceeds LDS capacity");
    const int grid = ((rows + 1) / 2) * CH;
    // long lines leave room for one or two workgroups per CU only: four times the threads then (the passes are loops over
    // butterflies with a barrier each, and 4 waves per CU hide nothing)
    const int threads = generic_threads(lds, false);
    TimedLaunch t(ctx, 0);
    if (threads == 1024) {
        if (int rc = set_lds(ctx, rowpass_kernel<InT, CH, 1024>, lds)) return rc;
        hipLaunchKernelGGL((rowpass_kernel<InT, CH, 1024>), dim3(grid), dim3(1024), lds, ctx->stream, src, planes, rows, cols, pad, dv, plan.d_tw, mperm, gshift);
    } else if (threads == 512) {
        if (int rc = set_lds(ctx, rowpass_kernel<InT, CH, 512>, lds)) return rc;
        hipLaunchKernelGGL((rowpass_kernel<InT, CH, 512>), dim3(grid), dim3(512), lds, ctx->stream, src, planes, rows, cols, pad, dv, plan.d_tw, mperm, gshift);
    } else {
        if (int rc = set_lds(ctx, rowpass_kernel<InT, CH>, lds)) return rc;
        hipLaunchKernelGGL((rowpass_kernel<InT, CH>), dim3(grid), dim3(kThreads), lds, ctx->stream, src, planes, rows, cols, pad, dv, plan.d_tw, mperm, gshift);
    }
    HIP_TRY(ctx, hipGetLastError());
    return BLUR_OK;
}

template <typename OutT, int CH, int C>
static int launch_colpass_c(blur_ctx* ctx, const float* planes, OutT* dst, int rows, int cols, int pad,
                            const DevicePlan& plan, const float* mperm, int strips)
{
    const size_t lds = col_lds_bytes(plan.dev.n, C, rows, sizeof(OutT) == 1 ? CH : 0);
    DevPlan dv = plan.dev;
    dv.nxcd = ctx->num_xcds;
    const int grid = (cols + 2 * C - 1) / (2 * C);
    const int threads = generic_threads(lds, true);
    TimedLaunch t(ctx, 1);
    if (threads == 1024) {
        if (int rc = set_lds(ctx, colpass_kernel<OutT, CH, C, 1024>, lds)) return rc;
        hipLaunchKernelGGL((colpass_kernel<OutT, CH, C, 1024>), dim3(grid), dim3(1024), lds, ctx->stream, planes, dst, rows, cols, pad, dv, plan.d_tw, mperm, strips);
    } else if (threads == 512) {
        if (int rc = set_lds(ctx, colpass_kernel<OutT, CH, C, 512>, lds)) return rc;
        hipLaunchKernelGGL((colpass_kernel<OutT, CH, C, 512>), dim3(grid), dim3(512), lds, ctx->stream, planes, dst, rows, cols, pad, dv, plan.d_tw, mperm, strips);
    } else {
        if (int rc = set_lds(ctx, colpass_kernel<OutT, CH, C>, lds)) return rc;
        hipLaunchKernelGGL((colpass_kernel<OutT, CH, C>), dim3(grid), dim3(kThreads), lds, ctx->stream, planes, dst, rows, cols, pad, dv, plan.d_tw, mperm, strips);
    }
    HIP_TRY(ctx, hipGetLastError());
    return BLUR_OK;
}

// complex lines (pairs of columns) a column-pass workgroup takes: as many as the options ask for and LDS holds; 0 = not even one
static int colpass_lines(int n, int rows, int col_group, int obpp)
{
    int C = col_group > 0 ? col_group / 2 : 4;
    if (C >= 8) C = 8; else if (C >= 4) C = 4; else if (C >= 2) C = 2; else C = 1;
    while (C > 1 && col_lds_bytes(n, C, rows, obpp) > kLdsLimit) C /= 2;
    return col_lds_bytes(n, C, rows, obpp) > kLdsLimit ? 0 : C;
}

// strips: the intermediate is strip-major with strips of 2 C columns (rowpass_kernel's gshift = log2(2 C))
template <typename OutT, int CH>
static int launch_colpass(blur_ctx* ctx, const float* planes, OutT* dst, int rows, int cols, int pad,
                          const DevicePlan& plan, const float* mperm, int col_group, int strips = 0)
{
    const int C = colpass_lines(plan.dev.n, rows, col_group, sizeof(OutT) == 1 ? CH : 0);
    if (!C) return fail(ctx, BLUR_ERR_UNSUPPORTED, "column FFT length exceeds LDS capacity");
    switch (C) {
    case 8: return launch_colpass_c<OutT, CH, 8>(ctx, planes, dst, rows, cols, pad, plan, mperm, strips);
    case 4: return launch_colpass_c<OutT, CH, 4>(ctx, planes, dst, rows, cols, pad, plan, mperm, strips);
    case 2: return launch_colpass_c<OutT, CH, 2>(ctx, planes, dst, rows, cols, pad, plan, mperm, strips);
    default: return launch_colpass_c<OutT, CH, 1>(ctx, planes, dst, rows, cols, pad, plan, mperm, strips);
    }
}

struct Prepared {
    Sizing sz;
    DevicePlan *row = nullptr, *col = nullptr;
    float *m_row = nullptr, *m_col = nullptr;
    int col_group = 0;
    int col_fast_c = 0;     // > 0: complex lines per workgroup of the specialised column kernel
    int tile_w = 0;         // > 0: both passes specialised, the float intermediate uses the strip layout
    size_t frame_elems = 0; // floats of intermediate per frame
    int gen_gshift = 0;     // run-time-planned kernel pair: log2 of the strip width of their strip-major intermediate (0: row-major planes)
    // wave-resident kernels (columns first, then rows) when both passes have one
    const WrEntry *wr_col = nullptr, *wr_row = nullptr;
    float2 *wr_tw0_col = nullptr, *wr_tw0_row = nullptr;
    float *wr_m_col = nullptr, *wr_m_row = nullptr;
    // matrix-core kernels (both passes)
    const MxEntry* mx = nullptr;
    const FxEntry* fx = nullptr;      // fused kernel (fx_kernels.hpp); taps and quirk gains shared with the two-kernel matrix engine
    const MxTables* mxt = nullptr;
    int mx_vpitch = 0;
    bool mx_quirk = false;
    // tiled wave-resident path (run_wr_tiled): bands of rows for the column pass, tiles of columns for the row pass
    struct Span { int in0, in1, padmode, v0, v1; };      // lines [in0, in1) go in (padmode = pad: reflect-101 at both ends; 0: none), [v0, v1) are kept
    std::vector<Span> bands, tiles;
    const WrEntry *tl_col = nullptr;                      // one column kernel for every band
    std::vector<const WrEntry*> tl_row;                   // a row kernel per tile
    std::vector<float*> tl_m_row;
    std::vector<float2*> tl_tw0_row;
    float* tl_m_col = nullptr;
    float2* tl_tw0_col = nullptr;
    float tl_dr = 0.f, tl_dc = 0.f;
    float* tl_taps = nullptr;                             // device: the 2 pad + 1 taps
    bool tiled = false, tl_quirk = false;
};

// a caller-supplied separable kernel instead of the Gaussian: taps (odd count, centre in the middle)
// or, for the tent mode, the reference's box_kernel arrays; pad as the caller's mode defines it
struct CustomKernel {
    const float* taps = nullptr;
    int ksize = 0;
    int pad = 0;
    int box_klen = 0;      // > 0: build the arrays with box_kernel_1d(klen) instead of from taps
};

// ---- wave-resident engine: tables --------------------------------------------------------------
static int wr_get_tables(blur_ctx* ctx, const WrEntry* e, float2** tw0)
{
    if (!ctx->d_w256) {
        std::vector<float> w(512);
        wr_w256(w.data());
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->d_w256), w.size() * sizeof(float)));
        HIP_TRY(ctx, hipMemcpy(ctx->d_w256, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    auto it = ctx->wr_tw0.find(e->r0);
    if (it == ctx->wr_tw0.end()) {
        std::vector<float> t(static_cast<size_t>(e->r0 - 1) * kWrS * 2 + 2);
        wr_tw0(e->r0, t.data());
        float2* d = nullptr;
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&d), t.size() * sizeof(float)));
        HIP_TRY(ctx, hipMemcpy(d, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
        it = ctx->wr_tw0.emplace(e->r0, d).first;
    }
    *tw0 = it->second;
    return BLUR_OK;
}

// multiplier table (natural order, n floats) of the n-periodic kernel `karr`; cached by `key`
static int wr_get_spectrum(blur_ctx* ctx, const std::tuple<int, int, int, int, uint64_t>& key, const std::vector<float>& karr, int n, int n_ref, bool quirk, float** out)
{
    auto it = ctx->wr_spectra.find(key);
    if (it != ctx->wr_spectra.end()) { *out = it->second; return BLUR_OK; }
    std::vector<float> m(n);
    wr_multipliers(karr.data(), n, n_ref, quirk, m.data());
    float* d = nullptr;
    // the tail behind the table is only written by -DWR_STAMPS diagnostic builds
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&d), sizeof(float) * (n + kWrStampTailFloats)));
    HIP_TRY(ctx, hipMemset(d, 0, sizeof(float) * (n + kWrStampTailFloats)));
    HIP_TRY(ctx, hipMemcpy(d, m.data(), sizeof(float) * n, hipMemcpyHostToDevice));
    ctx->wr_spectra[key] = d;
    ctx->last_spectrum[-n] = d;
    *out = d;
    return BLUR_OK;
}

static uint64_t fnv1a(const void* data, size_t bytes)
{
    uint64_t h = 1469598103934665603ull;
    const unsigned char* b = static_cast<const unsigned char*>(data);
    for (size_t i = 0; i < bytes; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}

// ---- matrix-core engine: tables ----------------------------------------------------------------------------------
// What the matrix-core kernels read for one kernel, as the host makes it from (sigma | a caller's kernel, Sizing, nkb) alone:
// mx_get_tables uploads and caches it per context; the one-sigma-per-frame entries (blur_ch_frame_sigmas_batch_impl) put the tables
// of a whole call into one upload instead, from this same code: what a frame is blurred with cannot differ between the two.
struct MxHostTables {
    std::vector<uint16_t> frags[2];   // row axis, column axis: [2][nkb][64][8] binary16 (host_math.hpp: mx_fragments)
    std::vector<float> taps_row;      // 2 pad + 1 floats, centre at pad (the same taps serve both axes)
    float dr = 0.f, dc = 0.f;         // m[0] - m[N/2] of the reference's row / column transform length (the quirk's gain)
};

// the reference's n-periodic kernel arrays (centre at index 0) of the row axis (n_row) and the column axis (n_col)
static int mx_kernel_arrays(double sigma, const Sizing& sz, const CustomKernel* ck, std::vector<float> (&karr)[2], const char** why)
{
    const int nn[2] = { sz.n_row, sz.n_col };
    for (int ax = 0; ax < 2; ++ax) {
        const int n = nn[ax];
        if (ck) {
            karr[ax].assign(n, 0.f);
            if (ck->box_klen > 0) box_kernel_1d(karr[ax].data(), ck->box_klen, n);
            else {
                if (ck->ksize > n) { *why = "kernel longer than the padded line"; return BLUR_ERR_INVALID; }
                const int c = ck->ksize / 2;
                for (int t = 0; t < ck->ksize; ++t) karr[ax][(t - c + n) % n] += ck->taps[t];
            }
        } else {
            karr[ax].assign(std::max(n, sz.kSize), 0.f);
            get_gaussian(karr[ax].data(), sigma, sz.kSize, n);    // Source.cpp:75-102
        }
    }
    return BLUR_OK;
}

// taps of one axis from the kernel array: taps[t + pad] = karr[(t + n) % n]; fragments, taps and gains of both axes.  Host only.
// col_frags = false: the column axis is checked and its gain made, its fragments are not (the fused kernels read the row axis')
static int mx_host_tables(const std::vector<float> (&karr)[2], const Sizing& sz, int nkb, MxHostTables& t, const char** why, bool col_frags = true)
{
    const int pad = sz.pad;
    const int nn[2] = { sz.n_row, sz.n_col };
    for (int ax = 0; ax < 2; ++ax) {
        const int n = nn[ax];
        std::vector<float> taps(2 * pad + 1);
        for (int k = -pad; k <= pad; ++k) taps[k + pad] = karr[ax][(k + n) % n];
        // anything of the kernel array outside +-pad would be lost here: the Toeplitz band is 2 pad + 1 wide
        for (int i = pad + 1; i < n - pad; ++i)
            if (karr[ax][i] != 0.f) { *why = "matrix-core engine: kernel wider than 2 pad + 1"; return BLUR_ERR_UNSUPPORTED; }
        // the 24-bit intermediate of the two-kernel engine (mx_kernels.hpp) covers [0, 256): non-negative taps with sum <= 1 keep the
        // row pass inside 0..255.13 (the quirk's terms are added in f32 after it is decoded: no bound on them)
        {
            double sum = 0;
            bool neg = false;
            for (float v : taps) { sum += v; neg = neg || v < 0.f; }
            if (neg || sum > 1.0005) { *why = "matrix-core engine: taps must be non-negative with sum <= 1"; return BLUR_ERR_UNSUPPORTED; }
        }
        if (ax == 0 || col_frags) {
            t.frags[ax].resize(static_cast<size_t>(2) * nkb * 512);
            mx_fragments(taps.data(), pad, nkb, t.frags[ax].data());
        }
        // m[0] and m[n/2] as host_math's kernel_multipliers computes them: float(Re DFT) * (1.f / n)
        long double k0 = 0, kalt = 0;
        for (int i = 0; i < n; ++i) { k0 += karr[ax][i]; kalt += (i & 1) ? -static_cast<long double>(karr[ax][i]) : static_cast<long double>(karr[ax][i]); }
        const float scaler = 1.f / n;
        const float m0 = static_cast<float>(k0) * scaler, mh = static_cast<float>(kalt) * scaler;
        (ax ? t.dc : t.dr) = m0 - mh;
        if (ax == 0) t.taps_row = std::move(taps);               // the taps themselves: the fused engine's quirk terms convolve with them
    }
    return BLUR_OK;
}

// The tables of one kernel on the device, cached in the context (the scalar entries: a few sigmas per context).
// quiet: a kernel the engine cannot hold is reported by the return value only (the caller falls back to another engine)
static int mx_get_tables(blur_ctx* ctx, int nkb, double sigma, const Sizing& sz, const CustomKernel* ck, const MxTables** out, bool quiet = false)
{
    auto refuse = [&](int code, const char* msg) { return quiet ? code : fail(ctx, code, msg); };
    std::vector<float> karr[2];                                  // row axis (n_row), column axis (n_col)
    const int nn[2] = { sz.n_row, sz.n_col };
    const char* why = nullptr;
    uint64_t tag;
    int kkey;
    // the Gaussian's key needs no kernel array: look it up before building one
    if (ck) {
        if (int rc = mx_kernel_arrays(sigma, sz, ck, karr, &why)) return refuse(rc, why);
        kkey = -1;
        tag = fnv1a(karr[0].data(), nn[0] * sizeof(float)) ^ (fnv1a(karr[1].data(), nn[1] * sizeof(float)) * 3);
    } else { kkey = sz.kSize; std::memcpy(&tag, &sigma, sizeof tag); }
    // (pad and nkb are part of the key: the same taps with another pad, or the two-kernel and the fused engine with different
    // window sizes for one pad, have different fragment tables)
    const auto key = std::make_tuple(kkey, sz.pad, nkb, nn[0], nn[1], tag);
    auto it = ctx->mx_tables.find(key);
    if (it != ctx->mx_tables.end()) { *out = &it->second; return BLUR_OK; }
    if (!ck) { if (int rc = mx_kernel_arrays(sigma, sz, ck, karr, &why)) return refuse(rc, why); }
    MxHostTables h;
    if (int rc = mx_host_tables(karr, sz, nkb, h, &why)) return refuse(rc, why);
    MxTables t;
    t.dr = h.dr;
    t.dc = h.dc;
    auto upload = [](void** d, const void* src, size_t bytes) {
        hipError_t e = hipMalloc(d, bytes);
        if (e == hipSuccess) e = hipMemcpy(*d, src, bytes, hipMemcpyHostToDevice);
        return e;
    };
    hipError_t e = upload(&t.frags_row, h.frags[0].data(), h.frags[0].size() * sizeof(uint16_t));
    if (e == hipSuccess) e = upload(reinterpret_cast<void**>(&t.taps_row), h.taps_row.data(), h.taps_row.size() * sizeof(float));
    if (e == hipSuccess) e = upload(&t.frags_col, h.frags[1].data(), h.frags[1].size() * sizeof(uint16_t));
    if (e != hipSuccess) {
        // a failure on a later table must not leak the earlier ones
        if (t.frags_row) (void)hipFree(t.frags_row);
        if (t.frags_col) (void)hipFree(t.frags_col);
        if (t.taps_row) (void)hipFree(t.taps_row);
        (void)hipGetLastError();          // clear it: under AUTO the caller falls back to another engine, whose first launch check would pick it up
        if (!quiet) ctx->err = std::string("matrix-core tables: ") + hipGetErrorString(e);
        return BLUR_ERR_HIP;
    }
    *out = &(ctx->mx_tables[key] = t);
    return BLUR_OK;
}

// ptrs_aligned: the frame pointers of the call are 4-byte aligned (no engine depends on it any more: the fused kernels take any
// width and alignment since round 4)
// The one rule both the matrix-core branch and the FFT branch of prepare() consult: do the wave-resident FFT kernels pay for this
// frame?  Both passes need a kernel (N = 256 R0 >= line + 2 pad) whose LDS holds the image; where the rows-first family has
// compile-time kernels for BOTH reference lengths as well (the six BASELINE (length, role) pairs) the wave-resident pair must fill
// its waves (R0 >= 8 / 12, lines at least 3/4 of N), elsewhere it competes with the run-time-planned kernels and wins as soon as the
// lines are at least half of N.  (Measured, us per frame wave-resident / rows-first: 4K sigma 20 106 / 107; 1080p sigma 20 41 / 36;
// 1000 x 1500 sigma 38.7 32 / 144; 1300 x 1950 sigma 44 83 / 87.)
struct FftFamilyChoice {
    const WrEntry* wc = nullptr;       // wave-resident column kernel / row kernel, where they exist and fit
    const WrEntry* wr = nullptr;
    bool fits = false;                 // both exist and their LDS holds the image
    bool old_both = false;             // the rows-first family has compile-time kernels for both reference lengths
    bool wr_pays = false;
};
static FftFamilyChoice fft_family_choice(int rows, int cols, const Sizing& sz)
{
    FftFamilyChoice c;
    c.wc = find_wr_entry(rows + 2 * sz.pad, true);
    c.wr = find_wr_entry(cols + 2 * sz.pad, false);
    c.old_both = find_fast_entry(sz.n_col, true) && find_fast_entry(sz.n_row, false);
    c.fits = c.wc && c.wr && c.wc->col_lds(rows) <= kLdsLimit && c.wr->row_lds(cols) <= kLdsLimit;
    if (c.fits) {
        const int need_c = rows + 2 * sz.pad, need_r = cols + 2 * sz.pad, nc = c.wc->r0 * kWrS, nr = c.wr->r0 * kWrS;
        c.wr_pays = c.old_both ? (c.wc->r0 >= 8 && c.wr->r0 >= 12 && 4 * need_c >= 3 * nc && 4 * need_r >= 3 * nr) : (2 * need_c >= nc && 2 * need_r >= nr);
    }
    return c;
}

// ---- tiled wave-resident path: spans along one axis --------------------------------------------------------------------------
// Cuts `len` lines with a kernel of half width `pad` into spans a transform of at most `nmax` points and `in_max` input lines can take.
// The first and the last span end at an image border and are padded by the kernel itself (reflect-101, padmode = pad: in + 2 pad
// points); the spans between are circular convolutions of real pixels only (padmode = 0: in points) whose first `halo` (= pad rounded
// up to `align`, so that the kept part starts at a multiple of `align`) and last pad results are not kept.  False: pad too wide.
static bool plan_spans(int len, int pad, int nmax, int in_max, int align, std::vector<Prepared::Span>& out, bool equal_middle = false, bool edge_max = false)
{
    out.clear();
    if (in_max > nmax) in_max = nmax;
    if (len + 2 * pad <= nmax && len <= in_max) { out.push_back({ 0, len, pad, 0, len }); return true; }
    const int halo = (pad + align - 1) / align * align;
    const int le = std::min(nmax - 2 * pad, in_max), lm = in_max;
    int ve = (le - halo) / align * align, vm = (lm - halo - pad) / align * align;        // most kept lines of an edge / a middle span
    if (ve <= 0 || vm <= 0) return false;
    // boundaries: as few spans as possible, evened out (one or two more where the even split breaks a limit)
    int nsp0 = 2;
    if (len > 2 * ve) nsp0 += (len - 2 * ve + vm - 1) / vm;
    std::vector<int> b;
    int nsp = 0, sm_equal = 0;
    for (int tries = 0; tries < 4 && nsp == 0; ++tries) {
        const int n = nsp0 + tries;
        b.assign(n + 1, 0);
        b[n] = len;
        // edge spans take the same share as the middle ones where that fits their limit
        int e = edge_max ? ve : static_cast<int>(static_cast<long long>(len) / n) / align * align;      // (edge_max: the edge spans as long as they go)
        if (e > ve) e = ve;
        if (2 * e >= len) e = (len / 2) / align * align;
        if (e < align) e = align;
        b[1] = e;
        const int rest = len - 2 * e;
        if (equal_middle && n > 2) {
            // middle spans of ONE length (a multiple of 2 and of align), so that they can run as the "frames" of one launch; the last of
            // them may reach into the last span's rows (written twice, by both)
            const int unit = align % 2 == 0 ? align : 2 * align;
            const int sm = ((rest + (n - 2) - 1) / (n - 2) + unit - 1) / unit * unit;
            if (sm > vm || e + (n - 2) * sm + pad > len) continue;
            for (int i = 2; i < n; ++i) b[i] = e + (i - 1) * sm;
            b[n - 1] = len - e;                                                               // the last span keeps its own e lines
            if (b[n - 1] <= b[n - 2] - sm) continue;
            nsp = n;
            sm_equal = sm;
            break;
        }
        for (int i = 2; i < n; ++i) b[i] = (e + static_cast<int>(static_cast<long long>(rest) * (i - 1) / (n - 2))) / align * align;
        b[n - 1] = std::max(b[n - 1], (len - ve + align - 1) / align * align);             // the last span's limit
        bool ok = len - b[n - 1] <= ve && len - b[n - 1] > 0 && b[1] <= ve;
        for (int i = 1; i < n && ok; ++i) ok = b[i] > b[i - 1];
        for (int i = 1; i + 1 < n && ok; ++i) ok = b[i + 1] - b[i] <= vm;
        if (ok) nsp = n;
    }
    if (nsp == 0) return false;
    for (int i = 0; i < nsp; ++i) {
        Prepared::Span sp;
        sp.v0 = b[i];
        sp.v1 = b[i + 1];
        if (i == 0) { sp.in0 = 0; sp.in1 = std::min(len, sp.v1 + pad); sp.padmode = pad; }
        else if (i == nsp - 1) { sp.in0 = sp.v0 - halo; sp.in1 = len; sp.padmode = pad; }
        else {
            if (sm_equal > 0) sp.v1 = sp.v0 + sm_equal;            // (the last middle span may reach into the last span's lines)
            sp.in0 = sp.v0 - halo; sp.in1 = std::min(len, sp.v1 + pad); sp.padmode = 0;
        }
        if (sp.in0 < 0 || sp.in1 - sp.in0 + 2 * sp.padmode > nmax || sp.in1 - sp.in0 > in_max || sp.padmode > sp.in1 - sp.in0 - 1) return false;
        out.push_back(sp);
    }
    return true;
}

// m[0] - m[n / 2] of the n-periodic kernel array as host_math's kernel_multipliers computes the two: float(Re DFT) * (1.f / n)
static float quirk_gain(const float* karr, int n)
{
    long double k0 = 0, kalt = 0;
    for (int i = 0; i < n; ++i) { k0 += karr[i]; kalt += (i & 1) ? -static_cast<long double>(karr[i]) : static_cast<long double>(karr[i]); }
    const float scaler = 1.f / n;
    return static_cast<float>(k0) * scaler - static_cast<float>(kalt) * scaler;
}

// the tiled wave-resident path for this frame: the column kernel and its bands, the row kernels and their tiles, the tables
// (multipliers WITHOUT the quirk: it enters as the terms of tl_terms_kernel).  tile_points > 0 (tests): no transform longer than that.
static int plan_tiled(blur_ctx* ctx, int rows, int cols, double sigma, bool quirk, int tile_points, Prepared& p)
{
    const int pad = p.sz.pad;
    // one column kernel for all bands: the candidate that transforms the fewest points per column
    long long best = -1;
    for (int r0 : { 16, 15, 12, 10, 9, 8, 6, 5, 4, 3 }) {
        const int n = r0 * kWrS;
        if (tile_points > 0 && n > tile_points) continue;
        const WrEntry* e = find_wr_entry(n, true);
        if (!e || e->r0 != r0) continue;
        int in_max = n;
        while (in_max > 0 && e->col_lds(in_max) > kLdsLimit) in_max -= 8;
        std::vector<Prepared::Span> sp;
        if (in_max <= 0 || !plan_spans(rows, pad, n, in_max, 1, sp, true)) continue;
        const long long cost = static_cast<long long>(sp.size()) * n;
        if (best < 0 || cost < best) { best = cost; p.bands = sp; p.tl_col = e; }
    }
    if (best < 0) return BLUR_ERR_UNSUPPORTED;
    best = -1;
    for (int r0 : { 16, 15, 12, 10, 9, 8, 6, 5, 4, 3 }) {
        const int n = r0 * kWrS;
        if (tile_points > 0 && n > tile_points) continue;
        const WrEntry* e = find_wr_entry(n, false);
        if (!e || e->r0 != r0) continue;
        int in_max = n;
        while (in_max > 0 && e->row_lds(in_max) > kLdsLimit) in_max -= 16;
        if (in_max <= 0) continue;
        for (int variant = 0; variant < 2; ++variant) {
            std::vector<Prepared::Span> sp;
            if (!plan_spans(cols, pad, n, in_max, 16, sp, false, variant == 1)) continue;
            // every tile runs on the smallest kernel that holds it: the cost is the transform points per row
            long long cost = 0;
            for (const Prepared::Span& t : sp) {
                const WrEntry* te = find_wr_entry(t.in1 - t.in0 + 2 * t.padmode, false);
                cost += te ? te->r0 * kWrS : 1 << 20;
            }
            if (best < 0 || cost < best) { best = cost; p.tiles = sp; }
        }
    }
    if (best < 0) return BLUR_ERR_UNSUPPORTED;
    uint64_t bits;
    std::memcpy(&bits, &sigma, sizeof bits);
    auto spectrum = [&](int n, float** out) -> int {
        const auto key = std::make_tuple(n, 0, p.sz.kSize, 0, bits);            // n_ref 0: no quirk in the table
        std::vector<float> karr(n, 0.f);
        if (ctx->wr_spectra.find(key) == ctx->wr_spectra.end()) {
            std::vector<float> k(std::max(n, p.sz.kSize));
            get_gaussian(k.data(), sigma, p.sz.kSize, n);                       // Source.cpp:75-102: taps rotated to index 0
            std::copy(k.begin(), k.begin() + n, karr.begin());
        }
        return wr_get_spectrum(ctx, key, karr, n, n, false, out);
    };
    if (int rc = wr_get_tables(ctx, p.tl_col, &p.tl_tw0_col)) return rc;
    if (int rc = spectrum(p.tl_col->r0 * kWrS, &p.tl_m_col)) return rc;
    p.tl_row.clear(); p.tl_m_row.clear(); p.tl_tw0_row.clear();
    for (const Prepared::Span& t : p.tiles) {
        const WrEntry* e = find_wr_entry(t.in1 - t.in0 + 2 * t.padmode, false);
        while (e && e->row_lds(t.in1 - t.in0) > kLdsLimit) e = find_wr_entry(e->r0 * kWrS + 1, false);
        if (!e || (tile_points > 0 && e->r0 * kWrS > tile_points)) return BLUR_ERR_UNSUPPORTED;
        float2* tw0 = nullptr;
        float* m = nullptr;
        if (int rc = wr_get_tables(ctx, e, &tw0)) return rc;
        if (int rc = spectrum(e->r0 * kWrS, &m)) return rc;
        p.tl_row.push_back(e); p.tl_tw0_row.push_back(tw0); p.tl_m_row.push_back(m);
    }
    // the quirk's gains at the REFERENCE's transform lengths (Source.cpp:420-425), and the taps
    {
        std::vector<float> k(std::max(std::max(p.sz.n_row, p.sz.n_col), p.sz.kSize));
        get_gaussian(k.data(), sigma, p.sz.kSize, p.sz.n_row);
        p.tl_dr = quirk_gain(k.data(), p.sz.n_row);
        std::vector<float> taps(2 * pad + 1);
        for (int t = -pad; t <= pad; ++t) taps[t + pad] = k[(t + p.sz.n_row) % p.sz.n_row];
        get_gaussian(k.data(), sigma, p.sz.kSize, p.sz.n_col);
        p.tl_dc = quirk_gain(k.data(), p.sz.n_col);
        const auto tk = std::make_pair(bits, p.sz.kSize);
        auto it = ctx->tl_taps.find(tk);
        if (it == ctx->tl_taps.end()) {
            float* d = nullptr;
            HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&d), taps.size() * sizeof(float)));
            HIP_TRY(ctx, hipMemcpy(d, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice));
            it = ctx->tl_taps.emplace(tk, d).first;
        }
        p.tl_taps = it->second;
    }
    p.frame_elems = 0;
    for (const Prepared::Span& b : p.bands) p.frame_elems = std::max(p.frame_elems, wr_frame_floats(b.in1 - b.in0, cols, b.padmode, p.tl_col->g));
    p.tiled = true;
    p.tl_quirk = quirk;
    return BLUR_OK;
}

// the frames the fused kernels cannot take whatever the pad (null: none of these); prepare() and the one-sigma-per-frame entries
static const char* fx_frame_limits(int rows, int cols, bool quirk)
{
    // (0xfffffff0 is the offset the kernels give a dropped store: it must lie outside the frame's buffer resource)
    // (and the left chunk's image resource starts 3 pad bytes before the frame: its size is the frame's plus those)
    if (static_cast<long long>(rows) * cols * 3 > 0xfffff000ll) return "fused matrix-core engine: frame too large for 32-bit offsets";
    if (quirk && fx_groups_per_thread(cols) == 0) return "fused matrix-core engine: image wider than 16384 pixels (the quirk's pre-pass)";
    if (quirk && cols < 4) return "fused matrix-core engine: image narrower than 4 pixels (the quirk's pre-pass)";
    return nullptr;
}

static int prepare(blur_ctx* ctx, int rows, int cols, double sigma, const blur_opts* opts, Prepared& p, bool u8c3 = true,
                   const CustomKernel* ck = nullptr, bool allow_wr = true, bool ptrs_aligned = false)
{
    if (!ctx) return BLUR_ERR_INVALID;
    if (rows <= 0 || cols <= 0 || (!ck && !(sigma > 0))) return fail(ctx, BLUR_ERR_INVALID, "rows, cols and sigma must be positive");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->engine_note.clear();
    if (ck) {
        p.sz = Sizing{};
        p.sz.kSize = ck->box_klen > 0 ? ck->box_klen : ck->ksize;
        p.sz.pad = ck->pad;
        auto fit = [](int want, int& tz) { const int n = is_valid_size(want) ? want : nearest_transform_size(want); tz = n - want; return n; };
        p.sz.n_col = fit(rows + 2 * ck->pad, p.sz.tz_col);          // Source.cpp:445-457
        p.sz.n_row = fit(cols + 2 * ck->pad, p.sz.tz_row);
    } else
    p.sz = pffft_sizing(rows, cols, sigma);
    if (p.sz.pad > rows - 1 || p.sz.pad > cols - 1)
        return fail(ctx, BLUR_ERR_UNSUPPORTED, "pad > min(rows, cols) - 1: reflect-101 would read outside the image (README.md:33-38)");
    const bool quirk = opts ? opts->nyquist_quirk != 0 : true;
    p.col_group = opts ? opts->col_group : 0;
    const bool allow_fast = u8c3 && !(opts && opts->force_generic == 1);   // force the generic kernels (tests)
    // Engine choice (enum blur_engine).  The library's own policy, BLUR_ENGINE_AUTO, in the order it is applied:
    //   | engine                      | where                                                   | measured (MI355X, 8 frames per call)            |
    //   | fused matrix-core kernel    | pad <= 72 (sigma <~ 22), non-negative taps with sum <= 1 | 4K sigma 20: 45 us per frame against 70 for the  |
    //   |                             | (any width, any pointer alignment)                      | two kernels and 105 for the FFT kernels          |
    //   | fused kernel, wide windows  | pad 73 .. 168 on frames >= 1 MP (not where the next row | 4K sigma 30: 98 GP/s against 85 / 70; 8K sigma 40 |
    //   |                             | applies), same conditions                               | single frame 79 against 54 / 26                   |
    //   | FFT, compile-time families  | frames < 1 MP, or pad > 136 on frames >= 6 MP           | 1080p sigma 20 single frame 72 / 78 us;          |
    //   |                             |                                                         | 4K sigma 50: 72 GP/s against 63                  |
    //   | two-kernel matrix engine    | pad <= 168, non-negative taps with sum <= 1             | 4K sigma 26 / 30 / 36: 103 / 87 / 80 GP/s (FFT 76)|
    //   | FFT kernels                 | everything else                                         |                                                   |
    // The choice depends on the frame and the kernel only, never on the number of frames.
    const int choice = opts ? opts->engine : BLUR_ENGINE_AUTO;
    // (allow_wr = false: the caller wants the rows-first float planes themselves, blur_rowpass_u8c3_dev)
    // Where the library's own choice (reserved[3] = 0) stays with the FFT kernels although a matrix-core kernel exists -- only
    // when the FFT engine has a compile-time family that its own policy below would pick (the run-time-planned kernels are
    // 3-4 times slower: then the matrix cores win regardless):
    //  * small frames (< 1 MP): the matrix-core path is four launches against two, and one small frame does not fill the chip
    //    either way (one frame per call, us: 1080p sigma 20 78 matrix / 72 FFT; eight per call: 23 / 36 per frame);
    //  * wide kernels (19 window blocks and more, pad > 136): the row kernel's window is then 3-4 times its 128 output pixels and
    //    its fragments leave one workgroup per CU (4K, 8 frames per call, GP/s matrix / FFT: sigma 36 80 / 76, sigma 40 72 / 73,
    //    sigma 44 66 / 72, sigma 50 63 / 72).
    // The choice depends on the frame and the kernel only, never on the number of frames: a frame blurred alone and the same
    // frame inside a batch give the same bytes.
    bool small_fft = false;
    if (choice == 0) {
        const MxEntry* me0 = find_entry_for_pad<MxEntry>(p.sz.pad);
        // (wide: measured on 4K frames only; the 1.5-3.8 MP images of the reference's sweep with sigma 39-49 run 1.0-1.5 times
        // FASTER on the matrix cores than on the wave-resident FFT kernels, so the rule is limited to large frames)
        const bool small = static_cast<long long>(rows) * cols < 1000000ll, wide = me0 && me0->nkb >= 19 && static_cast<long long>(rows) * cols >= 6000000ll;
        if (small || wide) {
            const FftFamilyChoice fc = fft_family_choice(rows, cols, p.sz);
            small_fft = fc.wr_pays || fc.old_both;
        }
    }
    const bool force_tiled = opts && opts->tile_points > 0;       // (tests: straight to the tiled wave-resident path)
    if (!force_tiled && allow_fast && allow_wr && (choice == BLUR_ENGINE_FUSED || choice == BLUR_ENGINE_AUTO)) {
        const FxEntry* fe = find_entry_for_pad<FxEntry>(p.sz.pad);
        // the one-channel-per-workgroup kernels for wide windows (fw_kernels.hpp; measured against the two-kernel engine / the FFT
        // kernels, GP/s: 4K sigma 30 single frame 61 / 50 / 57, eight frames 98 / 85 / 70; 8K sigma 40 single 79 / 54 / 26;
        // 1080p sigma 30 single 29 / 31 / 36, eight 68 / 63 / 59; 1000 x 1500 sigma 38.7 single 17 / 21 / 13; 4K sigma 50 single
        // 39 / 37 / 57, eight 68-73 / 63 / 63-74, sigma 44 eight 76 / 63 / 64): the library's own choice for frames of 6 MP and more,
        // except the widest window (23 blocks, pad > 152) where the FFT engine has a compile-time family for the frame (small_fft
        // above).
        const char* why = nullptr;
        if (fe && fe->nkb > 11 && choice == BLUR_ENGINE_AUTO) {
            // (round 4, segments of any number of tiles: one image per call, GP/s fused / two kernels / FFT: 1000 x 1500 sigma 38.7 21 / 21 / 16,
            // 1600 x 2400 sigma 49 33 / 27 / 32, 1080p sigma 30 35 / 31 / 37, eight of them 69 / 63 / 63: from 1 MP on; rounds 3-4 had 6 MP here)
            if (static_cast<long long>(rows) * cols < 1000000ll) { fe = nullptr; why = "wide fused kernel (pad 73 .. 168): frames below 1 MP run on two kernels or the FFT kernels"; }
            else if (small_fft && fe->nkb >= 23) { fe = nullptr; why = "wide fused kernel: pad > 152 where the FFT engine has a compile-time family for the frame"; }
        }
        if (!fe && !why) why = "fused matrix-core engine: no kernel instantiated for this pad";
        else if (const char* limit = fx_frame_limits(rows, cols, quirk)) why = limit;
        if (why && choice == BLUR_ENGINE_FUSED) return fail(ctx, BLUR_ERR_UNSUPPORTED, why);
        if (why) ctx->engine_note = why;
        if (!why) {
            const int rc = mx_get_tables(ctx, fe->nkb, sigma, p.sz, ck, &p.mxt, choice == BLUR_ENGINE_AUTO);
            if (rc != BLUR_OK && choice == BLUR_ENGINE_FUSED) return rc;
            if (rc == BLUR_OK) {
                p.fx = fe;
                p.mx_quirk = quirk;
                p.frame_elems = 0;
                return BLUR_OK;
            }
        }
    }
    if (!force_tiled && allow_fast && allow_wr && !small_fft && (choice == 0 || choice == 3)) {
        const MxEntry* me = find_entry_for_pad<MxEntry>(p.sz.pad);
        const int vpitch = (3 * cols + 31) & ~31;
        const bool fits = me && static_cast<long long>(mx_vrows(rows, me->nkb)) * vpitch < (1ll << 30) && static_cast<long long>(rows) * cols * 3 < (1ll << 32);
        if (!fits && choice != 0)
            return fail(ctx, BLUR_ERR_UNSUPPORTED, me ? "matrix-core engine: frame too large for 32-bit element offsets" : "matrix-core engine: no kernel instantiated for this pad");
        int rc_tables = BLUR_OK;
        if (fits) rc_tables = mx_get_tables(ctx, me->nkb, sigma, p.sz, ck, &p.mxt, choice == BLUR_ENGINE_AUTO);
        if (fits && rc_tables != BLUR_OK && choice != 0) return rc_tables;
        if (fits && rc_tables == BLUR_OK) {
        p.mx = me;
        p.mx_vpitch = vpitch;
        p.mx_quirk = quirk;
        p.frame_elems = static_cast<size_t>(mx_vrows(rows, me->nkb)) * vpitch;
        return BLUR_OK;
        }
    }
    // Tiled wave-resident path (round 4): lines longer than the longest wave-resident transform -- sigma = sqrt(side) on large images,
    // the reference's own benchmark (Source.cpp:627-635) -- in bands and tiles through the same kernels, instead of the run-time-planned
    // kernels (three to four times slower).  Taken where neither the whole-image wave-resident pair nor the rows-first family's
    // compile-time kernels apply; blur_opts.tile_points > 0 forces it (tests).
    {
        const int tile_points = opts ? opts->tile_points : 0;
        if (allow_fast && allow_wr && u8c3 && !ck && !(opts && opts->engine == BLUR_ENGINE_FFT_ROWS_FIRST)) {
            const FftFamilyChoice fc0 = fft_family_choice(rows, cols, p.sz);
            const bool whole = fc0.fits && ((opts && opts->engine == BLUR_ENGINE_FFT_WAVE_RESIDENT) || fc0.wr_pays);
            // (measured, one image per call, tools/tiled_compare.py: from 17 MP on the tiled path is 1.06 .. 1.76 times faster than the
            // run-time-planned kernels in either orientation; between 10 and 16 MP only where the columns still fit one transform
            // (rows + 2 pad <= 4096: wide images, 29 .. 35 GP/s against 26 .. 28) -- the reference's own sweep has tall images, whose
            // columns then need two bands of 4096 points each: 5 .. 9 % slower than the run-time-planned kernels there)
            const long long mp = static_cast<long long>(rows) * cols;
            const bool pays = mp >= 16000000ll || (mp >= 10000000ll && rows + 2 * p.sz.pad <= 4096);
            if (tile_points > 0 || (!whole && !fc0.old_both && pays)) {
                const int rc = plan_tiled(ctx, rows, cols, sigma, quirk, tile_points, p);
                if (rc == BLUR_OK) return BLUR_OK;
                if (rc != BLUR_ERR_UNSUPPORTED) return rc;
                if (tile_points > 0) return fail(ctx, BLUR_ERR_UNSUPPORTED, "tiled wave-resident path: the kernel is too wide for transforms of tile_points points");
                p.bands.clear(); p.tiles.clear();
            }
        }
    }
    // Wave-resident kernels first (reserved[3] = 1 switches them off): both passes need one, and its LDS must hold the image
    if (allow_fast && allow_wr && !(opts && opts->engine == BLUR_ENGINE_FFT_ROWS_FIRST)) {
        // (BLUR_ENGINE_FFT_WAVE_RESIDENT: wherever the image fits; otherwise the rule of fft_family_choice)
        const FftFamilyChoice fc = fft_family_choice(rows, cols, p.sz);
        const WrEntry* wc = fc.wc;
        const WrEntry* wr = fc.wr;
        const bool pays = (opts && opts->engine == BLUR_ENGINE_FFT_WAVE_RESIDENT) || fc.wr_pays;
        if (fc.fits && pays &&
            wr_frame_floats(rows, cols, p.sz.pad, wc->g) / 3 < (static_cast<size_t>(1) << 30)) {
            if (int rc = wr_get_tables(ctx, wc, &p.wr_tw0_col)) return rc;
            if (int rc = wr_get_tables(ctx, wr, &p.wr_tw0_row)) return rc;
            for (int pass = 0; pass < 2; ++pass) {
                const WrEntry* e = pass ? wc : wr;
                const int n = e->r0 * kWrS, n_ref = pass ? p.sz.n_col : p.sz.n_row;
                std::vector<float> karr(n, 0.f);
                std::tuple<int, int, int, int, uint64_t> key;
                if (ck) {
                    if (ck->box_klen > 0) box_kernel_1d(karr.data(), ck->box_klen, n);
                    else {
                        if (ck->ksize > n) return fail(ctx, BLUR_ERR_INVALID, "kernel longer than the padded line");
                        const int c = ck->ksize / 2;
                        for (int t = 0; t < ck->ksize; ++t) karr[(t - c + n) % n] += ck->taps[t];
                    }
                    key = std::make_tuple(n, n_ref, -1, quirk ? 1 : 0, fnv1a(karr.data(), karr.size() * sizeof(float)));
                } else {
                    uint64_t bits;
                    std::memcpy(&bits, &sigma, sizeof bits);
                    key = std::make_tuple(n, n_ref, p.sz.kSize, quirk ? 1 : 0, bits);
                    if (ctx->wr_spectra.find(key) == ctx->wr_spectra.end()) {
                        std::vector<float> k(std::max(n, p.sz.kSize));
                        get_gaussian(k.data(), sigma, p.sz.kSize, n);          // Source.cpp:75-102: taps rotated to index 0
                        std::copy(k.begin(), k.begin() + n, karr.begin());
                    }
                }
                if (int rc = wr_get_spectrum(ctx, key, karr, n, n_ref, quirk, pass ? &p.wr_m_col : &p.wr_m_row)) return rc;
            }
            p.wr_col = wc;
            p.wr_row = wr;
            p.frame_elems = wr_frame_floats(rows, cols, p.sz.pad, wc->g);
            return BLUR_OK;
        }
    }
    // the specialised column kernel needs its strip (C complex lines + pixel stage) to fit in LDS
    if (allow_fast)
        if (const FastEntry* fe = find_fast_entry(p.sz.n_col, true)) {
            int C = p.col_group > 0 ? (p.col_group >= 8 ? 4 : 2) : 4;
            while (C >= 2 && fe->col_lds_bytes(rows, C) > kLdsLimit) C /= 2;
            p.col_fast_c = C >= 2 ? C : 0;
        }
    // the specialised row kernel addresses a frame's three float planes with 32-bit byte offsets (fk_launch_row_u8)
    const bool row_fast_ok = static_cast<size_t>(rows + 1) * (cols + 8) * 12 < (static_cast<size_t>(1) << 32) && rows < (1 << 20);
    if (int rc = get_plan(ctx, p.sz.n_row, allow_fast && row_fast_ok, false, &p.row)) return rc;
    if (int rc = get_plan(ctx, p.sz.n_col, allow_fast && p.col_fast_c > 0, true, &p.col)) return rc;
    if (ck) {
        for (int pass = 0; pass < 2; ++pass) {
            DevicePlan* pl = pass ? p.col : p.row;
            const int n = pl->dev.n;
            std::vector<float> karr(n, 0.f);
            if (ck->box_klen > 0) box_kernel_1d(karr.data(), ck->box_klen, n);
            else {
                if (ck->ksize > n) return fail(ctx, BLUR_ERR_INVALID, "kernel longer than the padded line");
                const int c = ck->ksize / 2;
                for (int t = 0; t < ck->ksize; ++t) karr[(t - c + n) % n] += ck->taps[t];   // centre at index 0 (README.md:93-101)
            }
            if (int rc = get_spectrum_custom(ctx, *pl, karr, quirk, pass ? &p.m_col : &p.m_row)) return rc;
        }
    } else {
        if (int rc = get_spectrum(ctx, *p.row, sigma, p.sz.kSize, quirk, &p.m_row)) return rc;
        if (int rc = get_spectrum(ctx, *p.col, sigma, p.sz.kSize, quirk, &p.m_col)) return rc;
    }
    // strip layout of the intermediate only when both kernels understand it
    const bool no_tile = opts && opts->row_major_planes == 1;
    p.tile_w = (p.row->fast && p.col->fast && p.col_fast_c == 4 && !no_tile) ? 8 : 0;
    // strip layout: [strip][row pair][8 columns][2 rows] per channel
    p.frame_elems = p.tile_w ? static_cast<size_t>((cols + p.tile_w - 1) / p.tile_w) * ((rows + 1) / 2) * (2 * p.tile_w) * 3
                             : static_cast<size_t>(rows) * cols * 3;
    // both kernels run-time-planned: strip-major intermediate, strips as wide as a column-pass workgroup's share (the column kernel
    // then reads one contiguous block instead of 16 bytes out of every row: 4000 x 6000 sigma 77.5: 593 -> 4xx us)
    p.gen_gshift = 0;
    if (u8c3 && !p.row->fast && !p.col->fast && !no_tile) {
        int C = colpass_lines(p.col->dev.n, rows, p.col_group, 3);
        if (C < 1) C = colpass_lines(p.col->dev.n, rows, p.col_group, 0);        // very tall images: the column pass runs plane by plane (run_colpass_u8c3)
        if (C >= 1) {
            int g = 1;
            while ((1 << g) < 2 * C) ++g;
            p.gen_gshift = g;
            const int G = 1 << g;
            p.frame_elems = static_cast<size_t>((cols + G - 1) / G) * G * rows * 3;
        }
    }
    return BLUR_OK;
}

// nframes frames back to back (planes: 3*rows*cols floats per frame)
static int run_rowpass_u8c3(blur_ctx* ctx, const uint8_t* src, float* planes, int rows, int cols, int nframes, const Prepared& p, int tile_w)
{
    if (p.row->fast) {
        TimedLaunch t(ctx, 0, nframes);
        HIP_TRY(ctx, p.row->fast->row_u8(ctx->stream, src, planes, rows, cols, p.sz.pad, nframes, tile_w < 0 ? 0 : tile_w, p.row->d_tw, p.m_row));
        return BLUR_OK;
    }
    const size_t px = static_cast<size_t>(rows) * cols;
    const int gshift = tile_w < 0 ? 0 : p.gen_gshift;                 // (tile_w < 0: the caller wants row-major planes)
    const size_t fstride = gshift ? p.frame_elems : px * 3;
    for (int f = 0; f < nframes; ++f)
        if (int rc = launch_rowpass<uint8_t, 3>(ctx, src + f * px * 3, planes + f * fstride, rows, cols, p.sz.pad, *p.row, p.m_row, gshift)) return rc;
    return BLUR_OK;
}

static int run_colpass_u8c3(blur_ctx* ctx, const float* planes, uint8_t* dst, int rows, int cols, int nframes, const Prepared& p)
{
    if (p.col->fast) {
        TimedLaunch t(ctx, 1, nframes);
        HIP_TRY(ctx, p.col->fast->col_u8(ctx->stream, planes, dst, rows, cols, p.sz.pad, nframes, p.tile_w ? 1 : 0, p.col->d_tw, p.m_col, p.col_fast_c));
        return BLUR_OK;
    }
    const size_t px = static_cast<size_t>(rows) * cols;
    if (col_lds_bytes(p.col->dev.n, 1, rows, 3) > kLdsLimit && col_lds_bytes(p.col->dev.n, 1, rows, 0) <= kLdsLimit) {
        // Very tall images: one complex line plus the u8 pixel stage no longer fit in LDS.  Run the
        // column pass plane by plane into float planes (no stage) and interleave afterwards:
        // 24 B/px more traffic, but the FFT length limit becomes that of a bare line (N <~ 19800).
        if (ctx->work2_bytes < px * 3 * sizeof(float)) {
            if (ctx->work2) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); HIP_TRY(ctx, hipFree(ctx->work2)); ctx->work2 = nullptr; ctx->work2_bytes = 0; }
            HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->work2), px * 3 * sizeof(float)));
            ctx->work2_bytes = px * 3 * sizeof(float);
        }
        const size_t fstride = p.gen_gshift ? p.frame_elems : px * 3, cstride = fstride / 3;
        for (int f = 0; f < nframes; ++f) {
            for (int c = 0; c < 3; ++c)
                if (int rc = launch_colpass<float, 1>(ctx, planes + f * fstride + c * cstride, ctx->work2 + c * px, rows, cols, p.sz.pad, *p.col, p.m_col, p.col_group,
                                                      p.gen_gshift ? 1 : 0)) return rc;
            const unsigned grid = static_cast<unsigned>(std::min<size_t>((px + 255) / 256, 2048u * 8));
            hipLaunchKernelGGL(interleave_kernel, dim3(grid), dim3(256), 0, ctx->stream, ctx->work2, dst + f * px * 3, static_cast<uint32_t>(px));
            HIP_TRY(ctx, hipGetLastError());
        }
        return BLUR_OK;
    }
    const size_t fstride = p.gen_gshift ? p.frame_elems : px * 3;
    for (int f = 0; f < nframes; ++f)
        if (int rc = launch_colpass<uint8_t, 3>(ctx, planes + f * fstride, dst + f * px * 3, rows, cols, p.sz.pad, *p.col, p.m_col, p.col_group, p.gen_gshift ? 1 : 0)) return rc;
    return BLUR_OK;
}

// ======================================================================================
// 1- and 4-channel u8 images (blur_gaussian_u8_*), float32, u16, float16 and bfloat16 images of 1, 3 or 4 channels
// (blur_gaussian_f32_*, blur_gaussian_u16_*, blur_gaussian_f16_*, blur_gaussian_bf16_*): every channel blurred on its own as pffft_()
// blurs one of its planes (u8 and u16 with the + 0.5f truncation, float32 without, the half types rounded once to nearest even)
// ======================================================================================
#include "ff_kernels.hpp"

// the per-channel entries' pixel types by name (messages)
template <typename T> constexpr const char* ch_type_name()
{
    if constexpr (std::is_same_v<T, uint16_t>) return "u16";
    else if constexpr (std::is_same_v<T, ff_f16>) return "float16";
    else if constexpr (std::is_same_v<T, ff_bf16>) return "bfloat16";
    else if constexpr (std::is_same_v<T, float>) return "float32";
    else return "u8";
}

static int ensure_buf(blur_ctx* ctx, void** buf, size_t* have, size_t bytes)
{
    if (*have >= bytes) return BLUR_OK;
    if (*buf) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipFree(*buf));
        *buf = nullptr;
        *have = 0;
    }
    HIP_TRY(ctx, hipMalloc(buf, bytes));
    *have = bytes;
    return BLUR_OK;
}

// Where the rows and frames of a per-channel call lie, in bytes (blur_gaussian_*_pitched_batch_dev; the packed entries: ch_packed).
// Row r of frame f of the source starts at f sframe + r spitch, of the destination at f dframe + r dpitch.
struct ChLayout {
    size_t spitch, sframe, dpitch, dframe;
};
static ChLayout ch_packed(int rows, int cols, int ch, size_t es)
{
    const size_t pitch = static_cast<size_t>(cols) * ch * es;
    return ChLayout{ pitch, pitch * rows, pitch, pitch * rows };
}
// the bytes from a frame's first to behind its last
static size_t ch_frame_span(int rows, size_t pitch, size_t rowbytes) { return static_cast<size_t>(rows - 1) * pitch + rowbytes; }
// the fused kernels' view of a layout (ch_fused_refusal has checked that a frame's span fits 32-bit offsets)
static FwPitch fw_pitch_of(const ChLayout& L)
{
    return FwPitch{ static_cast<uint32_t>(L.spitch), static_cast<uint32_t>(L.dpitch), L.sframe, L.dframe };
}

static int run_fx_u8c3(blur_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int nframes, int rows, int cols, const Prepared& p, float* vdump, FwChSel chsel,
                       const ChLayout* lay, const FwFrame* ft = nullptr);

// the fused kernel for CH = 1, 2, 4 (fw_kernels.hpp; 2: the chroma plane of an NV12 surface, blur_nv_batch_impl): the pre-pass (the quirk's sums, the edge chunks' strips), then the kernel.
// Frames are disjoint from the destination here (blur_ch_batch_impl copies overlapping ones first).
// chsel: the channels to blur (blur_ch_sigmas_batch_impl: one sigma per channel); the pre-pass reads every channel (a pixel is one
// dword) and completes the quirk's row sums of these channels only
// ft: the frame list of a launch over frames with their own sigmas (blur_ch_frame_sigmas_batch_impl; FwFrame): nframes entries, whose
// pads, fragments, taps and gains replace p's in the kernels
static int run_fc_u8(blur_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int nframes, int rows, int cols, int ch, const Prepared& p, FwChSel chsel, const ChLayout& L,
                     const FwFrame* ft = nullptr)
{
    const FwPitch pt = fw_pitch_of(L);
    const int nkb = p.fx->nkb, pada = 8 * (nkb - 2);
    const FcEntry* fe = find_entry<FcEntry>(nkb);
    if (!fe) return fail(ctx, BLUR_ERR_UNSUPPORTED, "fused kernel for 1 / 4 channels: no kernel instantiated for this pad");
    FxGeom g{ rows, cols, p.sz.pad, nframes, 0, (rows + 31) / 32, fx_right_strips(cols, pada), ctx->num_xcds };
    const int chunks_x = (cols + kFxChunk - 1) / kFxChunk, win = kFxChunk + 2 * pada, nstrips = fx_left_strips(pada) + g.nright;
    if (int rc = ensure_buf(ctx, reinterpret_cast<void**>(&ctx->fx_strips), &ctx->fx_strips_bytes, static_cast<size_t>(nframes) * nstrips * rows * win * ch + 64)) return rc;
    const int strip_blocks = (rows * (ch * win / 4) + 255) / 256;
    const int n_strip = strip_blocks * nstrips * nframes;
    const int G = fc_groups_per_thread(cols, ch), ndw = (cols * ch + 3) / 4, nbatches = (ndw + 256 * G - 1) / (256 * G), cpitch = 4 * ndw;
    int band_rows = 16, nbands = 1, n_alt = 0;
    FcQuirk qk{};
    if (p.mx_quirk) {
        if (static_cast<long long>(rows) * cols >= 4000000ll)
            while (band_rows < 128 && static_cast<long long>(nbatches) * ((rows + 2 * band_rows - 1) / (2 * band_rows)) * nframes >= 4ll * ctx->num_cus) band_rows *= 2;
        nbands = (rows + band_rows - 1) / band_rows;
        n_alt = nbands * nbatches * nframes;
        // [zsum: frames x ch long long][srow: frames x rows x ch][cpart: frames x bands x cpitch] (int4 stores: 16-byte aligned)
        const size_t n_z = static_cast<size_t>(nframes) * ch, n_srow = (static_cast<size_t>(nframes) * rows * ch + 3) & ~static_cast<size_t>(3);
        const size_t n_cpart = static_cast<size_t>(nframes) * nbands * cpitch;
        const size_t zbytes = (n_z * sizeof(long long) + 15) & ~static_cast<size_t>(15);
        if (int rc = ensure_buf(ctx, reinterpret_cast<void**>(&ctx->fx_sums), &ctx->fx_sums_bytes, zbytes + (n_srow + n_cpart) * sizeof(int) + 64)) return rc;
        long long* zsum = reinterpret_cast<long long*>(ctx->fx_sums);
        int* srow = reinterpret_cast<int*>(reinterpret_cast<char*>(ctx->fx_sums) + zbytes);
        HIP_TRY(ctx, hipMemsetAsync(ctx->fx_sums, 0, zbytes + n_srow * sizeof(int), ctx->stream));
        qk.zsum = zsum;
        qk.srow = srow;
        qk.cpart = srow + n_srow;
        qk.taps = p.mxt->taps_row;
        qk.nbands = nbands;
        qk.cpitch = cpitch;
        qk.dr = p.mxt->dr;
        qk.dc = p.mxt->dc;
    }
    {
        TimedLaunch t(ctx, 1, nframes);
        int* srow = const_cast<int*>(qk.srow);
        int* cpart = const_cast<int*>(qk.cpart);
        long long* zsum = const_cast<long long*>(qk.zsum);
        auto kern = ch == 1 ? (G == 1 ? fc_prepass<1, 1> : (G == 2 ? fc_prepass<1, 2> : fc_prepass<1, 4>))
                  : ch == 2 ? (G == 1 ? fc_prepass<2, 1> : (G == 2 ? fc_prepass<2, 2> : fc_prepass<2, 4>))
                            : (G == 1 ? fc_prepass<4, 1> : (G == 2 ? fc_prepass<4, 2> : fc_prepass<4, 4>));
        auto kern_frames = ch == 1 ? (G == 1 ? fc_prepass_frames<1, 1> : (G == 2 ? fc_prepass_frames<1, 2> : fc_prepass_frames<1, 4>))
                                   : (G == 1 ? fc_prepass_frames<4, 1> : (G == 2 ? fc_prepass_frames<4, 2> : fc_prepass_frames<4, 4>));
        if (ft && ch == 2)          // (the two-channel instantiations are fc_frames2.hip's)
            HIP_TRY(ctx, fc_prepass_frames2_launch(G, static_cast<unsigned>(n_alt + n_strip), ctx->stream, d_src, srow, cpart, zsum, ctx->fx_strips, rows, cols, pada, nbands,
                                                   nbatches, cpitch, n_alt, chunks_x, g.nright, strip_blocks, band_rows, fw_chsel_bits(chsel), pt.src_pitch, pt.src_frame, ft));
        else if (ft)
            hipLaunchKernelGGL(kern_frames, dim3(n_alt + n_strip), dim3(256), 0, ctx->stream, d_src, srow, cpart, zsum, ctx->fx_strips, rows, cols, pada, nbands, nbatches,
                               cpitch, n_alt, chunks_x, g.nright, strip_blocks, band_rows, fw_chsel_bits(chsel), pt.src_pitch, pt.src_frame, ft);
        else
            hipLaunchKernelGGL(kern, dim3(n_alt + n_strip), dim3(256), 0, ctx->stream, d_src, srow, cpart, zsum, ctx->fx_strips, rows, cols, p.sz.pad, pada, nbands,
                               nbatches, cpitch, n_alt, chunks_x, g.nright, strip_blocks, band_rows, fw_chsel_bits(chsel), pt.src_pitch, pt.src_frame);
        HIP_TRY(ctx, hipGetLastError());
    }
    TimedLaunch t(ctx, 0, nframes);
    HIP_TRY(ctx, fe->blur_u8(ctx->stream, d_src, d_dst, p.mxt->frags_row, g, ch, ctx->num_cus, p.mx_quirk ? &qk : nullptr, ctx->fx_strips, chsel, pt, ft));
    return BLUR_OK;
}

// the fused kernel (ff_kernels.hpp): the pre-pass (max|x|, the quirk's sums, the edge chunks' strips), the quirk's finalisation,
// then the kernel.  Frames are disjoint from the destination here (blur_ch_batch_impl copies overlapping ones first).  Every
// partition of a sum (bands, batches) depends on the frame's shape only: a frame gives the same bits alone and in a batch.
// T = float, uint16_t, ff_f16 or ff_bf16.  u16: no max|x| (the scale is a constant of the call), and without the quirk no sums at
// all; the half types: as float.  chsel: the channels to blur (the pre-pass covers every channel either way: max|x| is the frame's).
// ft: the frame list of a launch over frames with their own sigmas (run_fc_u8)
template <typename T>
static int run_ff(blur_ctx* ctx, const T* d_src, T* d_dst, int nframes, int rows, int cols, int ch, const Prepared& p, FwChSel chsel, const ChLayout& L,
                  const FwFrame* ft = nullptr)
{
    const FwPitch pt = fw_pitch_of(L);
    constexpr bool u16 = std::is_same_v<T, uint16_t>;
    const int nkb = p.fx->nkb, pada = 8 * (nkb - 2);
    const FfEntryT<T>* fe = find_entry<FfEntryT<T>>(nkb);
    if (!fe || !ff_class_ok_t<T>(nkb, ch))
        return fail(ctx, BLUR_ERR_UNSUPPORTED, (std::string("fused kernel for ") + ch_type_name<T>() + " images: no kernel instantiated for this pad and channel count").c_str());
    FxGeom g{ rows, cols, p.sz.pad, nframes, 0, (rows + 31) / 32, fx_right_strips(cols, pada), ctx->num_xcds };
    const int chunks_x = (cols + kFxChunk - 1) / kFxChunk, win = kFxChunk + 2 * pada, nstrips = fx_left_strips(pada) + g.nright;
    if (int rc = ensure_buf(ctx, &ctx->ff_strips, &ctx->ff_strips_bytes,
                            (static_cast<size_t>(nframes) * nstrips * rows * win * ch + 16) * sizeof(T))) return rc;
    T* strips = static_cast<T*>(ctx->ff_strips);
    const int strip_blocks = static_cast<int>((static_cast<long long>(rows) * ch * win + 255) / 256);
    const int n_strip = strip_blocks * nstrips * nframes;
    const int G = ff_groups_per_thread(cols, ch), ne = cols * ch, nbatches = (ne + ff_batch_stride(ch) * G - 1) / (ff_batch_stride(ch) * G);
    // bands of rows: enough workgroups per frame to read it at the memory's rate (from the frame's shape alone)
    int band_rows = 16;
    while (band_rows < 128 && static_cast<long long>(nbatches) * ((rows + 2 * band_rows - 1) / (2 * band_rows)) >= 512) band_rows *= 2;
    const bool quirk = p.mx_quirk;
    const int nbands = (rows + band_rows - 1) / band_rows, n_alt = u16 && !quirk ? 0 : nbands * nbatches * nframes;
    // [mbits: frames][zsum: frames x ch][srow: frames x rows x ch][spart: frames x batches x rows x ch][cpart: frames x bands x ne]
    const size_t n_m = (static_cast<size_t>(nframes) + 1) / 2, n_z = static_cast<size_t>(nframes) * ch, n_srow = static_cast<size_t>(nframes) * rows * ch;
    const size_t n_spart = quirk ? n_srow * nbatches : 0, n_cpart = quirk ? static_cast<size_t>(nframes) * nbands * ne : 0;
    if (int rc = ensure_buf(ctx, &ctx->ff_sums, &ctx->ff_sums_bytes, (n_m + n_z + (quirk ? n_srow : 0) + n_spart + n_cpart) * sizeof(double) + 64)) return rc;
    double* base = static_cast<double*>(ctx->ff_sums);
    unsigned* mbits = reinterpret_cast<unsigned*>(base);
    double* zsum = base + n_m;
    double* srow = zsum + n_z;
    double* spart = srow + (quirk ? n_srow : 0);
    double* cpart = spart + n_spart;
    if (!u16) HIP_TRY(ctx, hipMemsetAsync(mbits, 0, static_cast<size_t>(nframes) * sizeof(unsigned), ctx->stream));
    FfQuirk qk{};
    qk.mbits = u16 ? nullptr : mbits;
    qk.bscale = 1.0;
    if (quirk) {
        qk.srow = srow;
        qk.cpart = cpart;
        qk.zsum = zsum;
        qk.taps = p.mxt->taps_row;
        qk.nbands = nbands;
        qk.cpitch = ne;
        qk.dr = p.mxt->dr;
        qk.dc = p.mxt->dc;
        qk.bscale = 1.0 + std::fabs(static_cast<double>(p.mxt->dr)) * (static_cast<double>(cols) + 2.0 * p.sz.pad);     // |Srow| <= (cols + 2 pad) max|x|
    }
    {
        TimedLaunch t(ctx, 1, nframes);
        auto pick = [&](auto k1, auto k2, auto k4) { return G == 1 ? k1 : (G == 2 ? k2 : k4); };
        auto kern = ch == 1 ? pick(ff_prepass<T, 1, 1>, ff_prepass<T, 1, 2>, ff_prepass<T, 1, 4>)
                            : (ch == 3 ? pick(ff_prepass<T, 3, 1>, ff_prepass<T, 3, 2>, ff_prepass<T, 3, 4>)
                                       : pick(ff_prepass<T, 4, 1>, ff_prepass<T, 4, 2>, ff_prepass<T, 4, 4>));
        auto kern_frames = ch == 1 ? pick(ff_prepass_frames<T, 1, 1>, ff_prepass_frames<T, 1, 2>, ff_prepass_frames<T, 1, 4>)
                                   : (ch == 3 ? pick(ff_prepass_frames<T, 3, 1>, ff_prepass_frames<T, 3, 2>, ff_prepass_frames<T, 3, 4>)
                                              : pick(ff_prepass_frames<T, 4, 1>, ff_prepass_frames<T, 4, 2>, ff_prepass_frames<T, 4, 4>));
        auto fin = ch == 1 ? ff_finalize<1> : (ch == 3 ? ff_finalize<3> : ff_finalize<4>);
        auto fin_frames = ch == 1 ? ff_finalize_frames<1> : (ch == 3 ? ff_finalize_frames<3> : ff_finalize_frames<4>);
        if constexpr (u16) {                  // two channels (the chroma plane of a P016 surface, blur_nv_batch_impl and blur_nv_frame_sigmas_batch_impl): u16 only
            if (ch == 2) {
                kern = pick(ff_prepass<T, 2, 1>, ff_prepass<T, 2, 2>, ff_prepass<T, 2, 4>);
                kern_frames = pick(ff_prepass_frames<T, 2, 1>, ff_prepass_frames<T, 2, 2>, ff_prepass_frames<T, 2, 4>);
                fin = ff_finalize<2>;
                fin_frames = ff_finalize_frames<2>;
            }
        }
        if (n_alt + n_strip > 0 && ft)
            hipLaunchKernelGGL(kern_frames, dim3(n_alt + n_strip), dim3(256), 0, ctx->stream, d_src, mbits, spart, cpart, strips, rows, cols, pada, nbands, nbatches, ne,
                               n_alt, chunks_x, g.nright, strip_blocks, band_rows, quirk ? 1 : 0, pt.src_pitch, pt.src_frame, ft);
        else if (n_alt + n_strip > 0)
            hipLaunchKernelGGL(kern, dim3(n_alt + n_strip), dim3(256), 0, ctx->stream, d_src, mbits, spart, cpart, strips, rows, cols, p.sz.pad, pada, nbands,
                               nbatches, ne, n_alt, chunks_x, g.nright, strip_blocks, band_rows, quirk ? 1 : 0, pt.src_pitch, pt.src_frame);
        HIP_TRY(ctx, hipGetLastError());
        if (quirk) {
            if (ft) hipLaunchKernelGGL(fin_frames, dim3(nframes), dim3(256), 0, ctx->stream, spart, srow, zsum, rows, nbatches, ft);
            else hipLaunchKernelGGL(fin, dim3(nframes), dim3(256), 0, ctx->stream, spart, srow, zsum, rows, p.sz.pad, nbatches);
            HIP_TRY(ctx, hipGetLastError());
        }
    }
    TimedLaunch t(ctx, 0, nframes);
    HIP_TRY(ctx, fe->blur(ctx->stream, d_src, d_dst, p.mxt->frags_row, g, ch, ctx->num_cus, qk, quirk, strips, chsel, pt, ft));
    return BLUR_OK;
}

// the plane fallback: split a frame into f32 planes, blur each on the f32 plane path, interleave the results
// Float frames are scaled by a power of two on the way in and back on the way out (exact), as the fused kernel scales its frames:
// the plane path's transforms are unnormalised f32, so max|x| near 1e37 overflowed in them and max|x| near 1e-37 lost bits to
// subnormals.  mbits: the bits of max|x| over the frame (an integer atomicMax: the same result in any order); the scale puts
// max|x| into [0.5, 1).  u8 and u16 frames are not scaled (mbits is not read).  float16 / bfloat16 frames are widened to f32 (exact)
// and then treated as float frames; chan_pack rounds the result once to nearest even, as the fused kernel does.
template <typename T> __device__ __forceinline__ float chan_widen(T v)
{
    if constexpr (ff_is_half_v<T>) return ff_half_widen<T>(v.bits);
    else return static_cast<float>(v);
}

// These kernels walk a frame by rows (blockIdx.y, gridDim.y apart) and by pixels of a row (the x dimension): `pitch` is the row
// pitch of the interleaved frame in bytes (a packed frame: cols ch sizeof(T)); the planes are packed.
template <typename T> __device__ __forceinline__ const T* chan_row(const T* base, size_t r, size_t pitch)
{
    return reinterpret_cast<const T*>(reinterpret_cast<const unsigned char*>(base) + r * pitch);
}
template <typename T> __device__ __forceinline__ T* chan_row(T* base, size_t r, size_t pitch)
{
    return reinterpret_cast<T*>(reinterpret_cast<unsigned char*>(base) + r * pitch);
}

template <typename T>
__global__ void chan_maxabs(const T* __restrict__ src, unsigned* __restrict__ mbits, int rows, int cols, int ch, size_t pitch)
{
    unsigned m = 0;
    for (int r = blockIdx.y; r < rows; r += gridDim.y) {
        const T* line = chan_row(src, r, pitch);
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < cols * ch; i += gridDim.x * blockDim.x)
            m = max(m, __float_as_uint(chan_widen(line[i])) & 0x7fffffffu);
    }
    if (m) atomicMax(mbits, m);
}

__device__ inline int chan_scale_exp(unsigned mbits)
{
    const float m = __uint_as_float(mbits);
    if (!(m > 0.f) || mbits >= 0x7f800000u) return 0;              // zero frame, Inf or NaN: no scale
    int k = 0;
    (void)frexpf(m, &k);                                            // m = f 2^k, f in [0.5, 1)
    return -k < -125 ? -125 : (-k > 125 ? 125 : -k);                // 2^e and 2^-e stay normal floats
}

template <typename T>
__global__ void chan_split(const T* __restrict__ src, float* __restrict__ planes, int rows, int cols, int ch, const unsigned* __restrict__ mbits, unsigned mask,
                           size_t pitch)
{
    float scale = 1.f;
    if constexpr (std::is_same_v<T, float> || ff_is_half_v<T>) scale = ldexpf(1.f, chan_scale_exp(*mbits));
    const size_t px = static_cast<size_t>(rows) * cols;
    for (int r = blockIdx.y; r < rows; r += gridDim.y) {
        const T* line = chan_row(src, r, pitch);
        float* prow = planes + static_cast<size_t>(r) * cols;
        for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < cols; x += gridDim.x * blockDim.x)
            for (int c = 0; c < ch; ++c) {
                if (!(mask >> c & 1u)) continue;
                if constexpr (std::is_same_v<T, float>) prow[c * px + x] = line[x * ch + c] * scale;
                else if constexpr (ff_is_half_v<T>) prow[c * px + x] = chan_widen(line[x * ch + c]) * scale;
                else prow[c * px + x] = static_cast<float>(line[x * ch + c]);
            }
    }
}

template <typename T>
__global__ void chan_pack(const float* __restrict__ planes, T* __restrict__ dst, int rows, int cols, int ch, const unsigned* __restrict__ mbits, unsigned mask,
                          size_t pitch)
{
    float unscale = 1.f;
    if constexpr (std::is_same_v<T, float> || ff_is_half_v<T>) unscale = ldexpf(1.f, -chan_scale_exp(*mbits));
    const size_t px = static_cast<size_t>(rows) * cols;
    for (int r = blockIdx.y; r < rows; r += gridDim.y) {
        T* line = chan_row(dst, r, pitch);                   // (only samples x < cols of a row are written)
        const float* prow = planes + static_cast<size_t>(r) * cols;
        for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < cols; x += gridDim.x * blockDim.x)
            for (int c = 0; c < ch; ++c) {
                if (!(mask >> c & 1u)) continue;
                if constexpr (std::is_same_v<T, uint8_t>)  // (uint8_t)(v + 0.5f) of the reference (Utils.hpp:189,204-206): truncate, keep the low byte
                    line[x * ch + c] = static_cast<uint8_t>(static_cast<uint32_t>(static_cast<int>(prow[c * px + x] + 0.5f)) & 0xffu);
                else if constexpr (std::is_same_v<T, uint16_t>)  // the same rule 16 bits wide: truncate, keep the low 16 bits
                    line[x * ch + c] = static_cast<uint16_t>(static_cast<uint32_t>(static_cast<int>(prow[c * px + x] + 0.5f)) & 0xffffu);
                else if constexpr (ff_is_half_v<T>)             // one rounding to nearest even (binary16: overflow to +-Inf)
                    line[x * ch + c] = T{ ff_half_round<T>(prow[c * px + x] * unscale) };
                else
                    line[x * ch + c] = prow[c * px + x] * unscale;
            }
    }
}

// mask: the channels to blur (one sigma per channel: the others are neither split nor packed; max|x| is the whole frame's either way)
template <typename T>
static int run_planes(blur_ctx* ctx, const T* d_src, T* d_dst, int nframes, int rows, int cols, int ch, double sigma, const blur_opts* opts, const ChLayout& L,
                      unsigned mask = 0xfu)
{
    Prepared p;
    if (int rc = prepare(ctx, rows, cols, sigma, opts, p, false)) return rc;
    const size_t px = static_cast<size_t>(rows) * cols;
    if (int rc = ensure_work(ctx, px * sizeof(float))) return rc;
    if (int rc = ensure_buf(ctx, reinterpret_cast<void**>(&ctx->ch_planes), &ctx->ch_planes_bytes, px * ch * sizeof(float) + 16)) return rc;
    unsigned* mbits = reinterpret_cast<unsigned*>(ctx->ch_planes + px * ch);          // behind the planes
    // (as many workgroups as before the kernels walked rows: about 4096, a row's pixels in x and the rows in y)
    const unsigned bx = static_cast<unsigned>(std::min<size_t>((static_cast<size_t>(cols) + 255) / 256, 4096));
    const dim3 blocks(bx, static_cast<unsigned>(std::min<size_t>(rows, std::max<size_t>(1, 4096 / bx))));
    for (int f = 0; f < nframes; ++f) {
        const T* s = reinterpret_cast<const T*>(reinterpret_cast<const char*>(d_src) + static_cast<size_t>(f) * L.sframe);
        T* d = reinterpret_cast<T*>(reinterpret_cast<char*>(d_dst) + static_cast<size_t>(f) * L.dframe);
        if constexpr (std::is_same_v<T, float> || ff_is_half_v<T>) {
            HIP_TRY(ctx, hipMemsetAsync(mbits, 0, sizeof(unsigned), ctx->stream));
            hipLaunchKernelGGL(chan_maxabs<T>, blocks, dim3(256), 0, ctx->stream, s, mbits, rows, cols, ch, L.spitch);
            HIP_TRY(ctx, hipGetLastError());
        }
        hipLaunchKernelGGL(chan_split<T>, blocks, dim3(256), 0, ctx->stream, s, ctx->ch_planes, rows, cols, ch, mbits, mask, L.spitch);
        HIP_TRY(ctx, hipGetLastError());
        for (int c = 0; c < ch; ++c) {
            if (!(mask >> c & 1u)) continue;
            float* plane = ctx->ch_planes + c * px;
            if (int rc = launch_rowpass<float, 1>(ctx, plane, ctx->work, rows, cols, p.sz.pad, *p.row, p.m_row)) return rc;
            if (int rc = launch_colpass<float, 1>(ctx, ctx->work, plane, rows, cols, p.sz.pad, *p.col, p.m_col, p.col_group)) return rc;
        }
        hipLaunchKernelGGL(chan_pack<T>, blocks, dim3(256), 0, ctx->stream, ctx->ch_planes, d, rows, cols, ch, mbits, mask, L.dpitch);
        HIP_TRY(ctx, hipGetLastError());
    }
    return BLUR_OK;
}

// the arguments of every blur_gaussian_{u8,f32,u16,f16,bf16}_* entry, without the device (ctx may be NULL here: the status is the same)
static int check_ch_args(blur_ctx* ctx, const void* src, const void* dst, int nframes, int rows, int cols, int channels, double sigma)
{
    if (channels != 1 && channels != 3 && channels != 4) return fail(ctx, BLUR_ERR_INVALID, "channels must be 1, 3 or 4");
    if (!src || !dst || nframes < 0) return fail(ctx, BLUR_ERR_INVALID, "null frame pointer or negative frame count");
    if (rows <= 0 || cols <= 0 || !(sigma > 0)) return fail(ctx, BLUR_ERR_INVALID, "rows, cols and sigma must be positive");
    const Sizing sz = pffft_sizing(rows, cols, sigma);
    if (sz.pad > rows - 1 || sz.pad > cols - 1)
        return fail(ctx, BLUR_ERR_UNSUPPORTED, "pad > min(rows, cols) - 1: reflect-101 would read outside the image (README.md:33-38)");
    return ctx ? BLUR_OK : BLUR_ERR_INVALID;
}

// the arguments a pitched entry adds (blur_gaussian_*_pitched_batch_dev), without the device: pitches and frame strides in bytes
// src_broadcast: a source frame stride of 0 is accepted for any nframes (the one-sigma-per-frame entries: every frame of the result
// is blurred from the same source frame)
// two_ok: two channels are legal (the chroma plane of an NV12 / P016 surface: blur_nv_batch_impl only)
static int check_ch_layout(blur_ctx* ctx, int nframes, int rows, int cols, int channels, size_t es, const ChLayout& L, bool src_broadcast = false, bool two_ok = false)
{
    if (rows <= 0 || cols <= 0 || (channels != 1 && channels != 3 && channels != 4 && !(two_ok && channels == 2))) return BLUR_OK;       // (refused by the other checks)
    const size_t rowbytes = static_cast<size_t>(cols) * channels * es;
    if (L.spitch < rowbytes || L.dpitch < rowbytes) return fail(ctx, BLUR_ERR_INVALID, "row pitch below cols * channels * sizeof(element)");
    if (L.spitch % es || L.dpitch % es || L.sframe % es || L.dframe % es)
        return fail(ctx, BLUR_ERR_INVALID, "row pitch and frame stride must be multiples of the element size");
    if (nframes > 1 && ((L.sframe < ch_frame_span(rows, L.spitch, rowbytes) && !(src_broadcast && L.sframe == 0)) || L.dframe < ch_frame_span(rows, L.dpitch, rowbytes)))
        return fail(ctx, BLUR_ERR_INVALID, "frame stride below (rows - 1) * pitch + cols * channels * sizeof(element): the frames of the batch would overlap");
    return BLUR_OK;
}

// Overlapping calls read from a packed copy.  The byte spans [base, base + (n - 1) frame + (rows - 1) pitch + rowbytes) of the source
// and the destination are compared: an in-place call and two rectangles of one parent image both intersect.  ch_gather_rows moves
// the source rectangles into the workspace in one launch (V: 16, 4 or 1 bytes per thread, by what the addresses allow).
template <typename V>
__global__ __launch_bounds__(256) void ch_gather_rows(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int rows, size_t rowbytes, size_t spitch,
                                                      size_t sframe)
{
    const size_t nv = rowbytes / sizeof(V);
    const unsigned char* s = src + blockIdx.z * sframe;
    unsigned char* d = dst + blockIdx.z * static_cast<size_t>(rows) * rowbytes;
    for (int r = blockIdx.y; r < rows; r += gridDim.y) {
        const V* sl = reinterpret_cast<const V*>(s + static_cast<size_t>(r) * spitch);
        V* dl = reinterpret_cast<V*>(d + static_cast<size_t>(r) * rowbytes);
        for (size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; i < nv; i += static_cast<size_t>(gridDim.x) * blockDim.x) dl[i] = sl[i];
    }
}

static bool ch_spans_overlap(const void* src, const void* dst, int nframes, int rows, size_t rowbytes, const ChLayout& L)
{
    const char* s0 = static_cast<const char*>(src);
    const char* d0 = static_cast<const char*>(dst);
    const size_t sspan = static_cast<size_t>(nframes - 1) * L.sframe + ch_frame_span(rows, L.spitch, rowbytes);
    const size_t dspan = static_cast<size_t>(nframes - 1) * L.dframe + ch_frame_span(rows, L.dpitch, rowbytes);
    return s0 < d0 + dspan && d0 < s0 + sspan;
}

// Where the spans of the nframes source and destination frames overlap (the fused kernel reads its neighbours' pixels while it
// writes, and the plane path writes frame f before it reads frame f + 1): the first ncopy source rectangles -> ctx->ch_copy, packed;
// *src and the layout's source side then describe the copy
template <typename T>
static int ch_copy_source(blur_ctx* ctx, const T** src, const T* dst, int nframes, int ncopy, int rows, size_t rowbytes, ChLayout& L)
{
    if (!ch_spans_overlap(*src, dst, nframes, rows, rowbytes, L)) return BLUR_OK;
    const size_t fb = rowbytes * rows;
    if (int rc = ensure_buf(ctx, reinterpret_cast<void**>(&ctx->ch_copy), &ctx->ch_copy_bytes, fb * ncopy)) return rc;
    if (L.spitch == rowbytes && (ncopy == 1 || L.sframe == fb)) {
        HIP_TRY(ctx, hipMemcpyAsync(ctx->ch_copy, *src, fb * ncopy, hipMemcpyDeviceToDevice, ctx->stream));
    } else {
        const uintptr_t bits = reinterpret_cast<uintptr_t>(*src) | L.spitch | L.sframe | rowbytes | reinterpret_cast<uintptr_t>(ctx->ch_copy);
        const size_t vb = (bits & 15) == 0 ? 16 : ((bits & 3) == 0 ? 4 : 1);
        const unsigned bx = static_cast<unsigned>(std::min<size_t>((rowbytes / vb + 255) / 256, 64));
        const dim3 grid(bx, static_cast<unsigned>(std::min<size_t>(rows, 1024)), static_cast<unsigned>(ncopy));
        auto kern = vb == 16 ? ch_gather_rows<uint4> : (vb == 4 ? ch_gather_rows<uint32_t> : ch_gather_rows<unsigned char>);
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, ctx->stream, reinterpret_cast<const unsigned char*>(*src), reinterpret_cast<unsigned char*>(ctx->ch_copy), rows,
                           rowbytes, L.spitch, L.sframe);
        HIP_TRY(ctx, hipGetLastError());
    }
    *src = reinterpret_cast<const T*>(ctx->ch_copy);
    L.spitch = rowbytes;
    L.sframe = fb;
    return BLUR_OK;
}

// a call that writes its frames where it reads them
static bool ch_in_place(const void* src, const void* dst, const ChLayout& L) { return src == dst && L.spitch == L.dpitch && L.sframe == L.dframe; }

// An in-place batch that reads from a copy runs in parts of at most 1 GiB (a part's result never touches a later part's source).
// True where the batch is larger than that: body(part, nf, f0) has run on the nf frames from frame f0 on, and *rc is its status
template <typename T, typename Body>
static bool ch_in_place_parts(T* d_dst, int nframes, size_t fb, size_t dframe, int* rc, Body body)
{
    const size_t cap = std::max<size_t>(1, (static_cast<size_t>(1) << 30) / fb);
    if (static_cast<size_t>(nframes) <= cap) return false;
    *rc = BLUR_OK;
    for (int f0 = 0; f0 < nframes && *rc == BLUR_OK; f0 += static_cast<int>(cap)) {
        const int nf = std::min<int>(static_cast<int>(cap), nframes - f0);
        T* part = reinterpret_cast<T*>(reinterpret_cast<char*>(d_dst) + static_cast<size_t>(f0) * dframe);
        *rc = body(part, nf, f0);
    }
    return true;
}

// opts (null: the defaults) with another engine
static blur_opts with_engine(const blur_opts* opts, int engine)
{
    blur_opts o;
    if (opts) o = *opts;
    else blur_opts_default(&o);
    o.engine = engine;
    return o;
}

// The engine a per-channel call asks for (opts null: AUTO).  The fused kernel and the plane path are all these entries have: -1 for
// any other engine, with the call's error set (BLUR_ERR_UNSUPPORTED)
static int ch_engine_choice(blur_ctx* ctx, const blur_opts* opts, const char* who, const char* what)
{
    const int choice = opts ? opts->engine : BLUR_ENGINE_AUTO;
    if (choice != BLUR_ENGINE_AUTO && choice != BLUR_ENGINE_FUSED && choice != BLUR_ENGINE_FFT)
        return fail(ctx, BLUR_ERR_UNSUPPORTED, (std::string(who) + what + ": engine must be AUTO, FUSED or FFT").c_str()), -1;
    return choice;
}

// What takes the fused kernel of window class nkb away from pixel type T (empty: nothing does).  float32 has no kernel for NKB 23
// with 3 or 4 channels (ff_class_ok_t); the own choice of float32 and u16 stops at NKB 15 (ff_class_in_contract: at 16 bits 1e-6 of
// full scale is 0.066 of a grey level); the 32-bit offsets limit the frame's bytes (a pitched frame: its span, (rows - 1) pitch + a
// row's bytes).  own_name: the one-sigma-per-frame driver's wording, which names T where choose_ch_engine's says "float16 /
// bfloat16" of both half types
template <typename T>
static std::string ch_fused_refusal(int nkb, int rows, int cols, int channels, int choice, const ChLayout& L, bool own_name)
{
    constexpr bool u16 = std::is_same_v<T, uint16_t>, half = ff_is_half_v<T>, ffk = !std::is_same_v<T, uint8_t>;      // ffk: the ff_kernels.hpp types
    const size_t rowbytes = static_cast<size_t>(cols) * channels * sizeof(T);
    const std::string fused = "fused kernel for ";
    if (ffk && !ff_class_ok_t<T>(nkb, channels)) return fused + ch_type_name<T>() + " images: pad 153 .. 168 has a kernel for 1 channel only";
    if (ffk && choice == BLUR_ENGINE_AUTO && !ff_class_in_contract(nkb))
        return fused + (half && !own_name ? "float16 / bfloat16" : ch_type_name<T>()) +
               (half ? " images: pad 105 .. 168 is outside the library's own choice, as for float32; ask for it with engine = FUSED"
                : u16 ? " images: pad 105 .. 168 exceeds 1e-6 of full scale on full-scale content (1.2e-6); ask for it with engine = FUSED"
                      : " images: pad 105 .. 168 exceeds 1e-6 max|x| on full-scale content (1.2e-6); ask for it with engine = FUSED");
    if (std::max(ch_frame_span(rows, L.spitch, rowbytes), ch_frame_span(rows, L.dpitch, rowbytes)) > 0xfffff000ull)
        return "fused matrix-core engine: frame too large for 32-bit offsets";
    return std::string();
}

// the fused kernel of the pixel type over the channels in chsel (frames: the list of a launch over frames with their own sigmas)
template <typename T>
static int run_ch_fused(blur_ctx* ctx, const T* d_src, T* d_dst, int nframes, int rows, int cols, int channels, const Prepared& p, FwChSel chsel, const ChLayout& L,
                        const FwFrame* frames = nullptr)
{
    if constexpr (!std::is_same_v<T, uint8_t>) return run_ff<T>(ctx, d_src, d_dst, nframes, rows, cols, channels, p, chsel, L, frames);
    else return channels == 3 ? run_fx_u8c3(ctx, d_src, d_dst, nframes, rows, cols, p, nullptr, chsel, &L, frames)
                              : run_fc_u8(ctx, d_src, d_dst, nframes, rows, cols, channels, p, chsel, L, frames);
}

// The engine of a per-channel blur with one sigma (blur_ch_batch_impl; blur_ch_sigmas_batch_impl: of a group of channels): p.fx set =
// the fused kernel, else the plane fallback, and `note` says why.  choice: AUTO, FUSED or FFT.
template <typename T>
static int choose_ch_engine(blur_ctx* ctx, int rows, int cols, int channels, double sigma, const blur_opts* opts, int choice, Prepared& p, std::string& note,
                            const ChLayout& L)
{
    // The fused kernel wherever it applies (prepare's rules for BLUR_ENGINE_FUSED: a kernel for the pad, the frame and quirk limits; a
    // float32 class instantiated for the channel count; the frame's bytes within 32-bit offsets), the plane fallback elsewhere.  AUTO
    // too: where the u8c3 policy passes the fused engine over for a compile-time FFT family (frames under 1 MP, pad > 152 on 6 MP), the
    // alternative here is the run-time-planned plane path, three to four times slower than the fused kernel (4K sigma 50, 8 frames:
    // 0.146 ms per 1-channel u8 frame, 0.568 per 4-channel one, on the plane path)
    if (choice != BLUR_ENGINE_FFT) {
        const blur_opts fo = with_engine(opts, BLUR_ENGINE_FUSED);
        const int rc = prepare(ctx, rows, cols, sigma, &fo, p, true);
        if (rc == BLUR_ERR_UNSUPPORTED && choice == BLUR_ENGINE_AUTO) {
            p = Prepared{};
            note = ctx->err;
            ctx->err.clear();                    // (not a failure of this call)
        } else if (rc) return rc;
        const std::string why = p.fx ? ch_fused_refusal<T>(p.fx->nkb, rows, cols, channels, choice, L, false) : std::string();
        if (!why.empty()) {
            if (choice == BLUR_ENGINE_FUSED) return fail(ctx, BLUR_ERR_UNSUPPORTED, why.c_str());
            p.fx = nullptr;
            note = why;
        }
    }
    return BLUR_OK;
}

// One driver for the five element types (float16 and bfloat16: in everything below as float32, two bytes per sample).  What differs by type: u8 forwards 3 channels to the u8c3 entry;
// the rules that take the fused kernel away (ch_fused_refusal); the fused kernel (run_ch_fused) and the engine error's text
template <typename T>
static int blur_ch_batch_impl(blur_ctx* ctx, const T* d_src, T* d_dst, int nframes, int rows, int cols, int channels, double sigma, const blur_opts* opts,
                              const ChLayout* lay = nullptr)
{
    constexpr bool u8 = std::is_same_v<T, uint8_t>;
    // lay: the pitched entries' layout (null: packed frames).  Three u8 channels, packed: the u8c3 entry and its kernels; pitched:
    // fw_blur_u8<NKB, Q, 3> over the three channels (Fw3Entry), the route of the one-sigma-per-channel calls
    if (lay)
        if (int rc = check_ch_layout(ctx, nframes, rows, cols, channels, sizeof(T), *lay)) return rc;
    if (int rc = check_ch_args(ctx, d_src, d_dst, nframes, rows, cols, channels, sigma)) return rc;
    if constexpr (u8) {
        if (channels == 3 && !lay) return blur_gaussian_u8c3_batch_dev(ctx, d_src, d_dst, nframes, rows, cols, sigma, opts);
    }
    ChLayout L = lay ? *lay : ch_packed(rows, cols, channels, sizeof(T));
    if (nframes == 1) L.sframe = L.dframe = 0;               // (not used; in-place calls compare the layouts)
    const int choice = ch_engine_choice(ctx, opts, u8 ? "1- and 4-channel" : ch_type_name<T>(), " images");
    if (choice < 0) return BLUR_ERR_UNSUPPORTED;
    Prepared p;
    std::string note;
    if (int rc = choose_ch_engine<T>(ctx, rows, cols, channels, sigma, opts, choice, p, note, L)) return rc;
    if (nframes == 0) return BLUR_OK;
    const size_t rowbytes = static_cast<size_t>(cols) * channels * sizeof(T), fb = rowbytes * rows;
    // an in-place call of the plane path needs no copy (frame f is read whole before it is written); every other overlap reads from one
    const bool in_place = ch_in_place(d_src, d_dst, L);
    if (p.fx || !in_place) {
        int rc;
        if (in_place && ch_in_place_parts(d_dst, nframes, fb, L.dframe, &rc, [&](T* part, int nf, int) {
                return blur_ch_batch_impl(ctx, part, part, nf, rows, cols, channels, sigma, opts, lay);
            }))
            return rc;
        if (int rc = ch_copy_source(ctx, &d_src, d_dst, nframes, nframes, rows, rowbytes, L)) return rc;
    }
    if (p.fx) {
        ctx->last_family = 6;
        return run_ch_fused<T>(ctx, d_src, d_dst, nframes, rows, cols, channels, p, fw_chsel_all(channels), L);
    }
    const blur_opts o = with_engine(opts, BLUR_ENGINE_FFT);
    if (int rc = run_planes(ctx, d_src, d_dst, nframes, rows, cols, channels, sigma, &o, L)) return rc;
    ctx->last_family = 0;
    ctx->engine_note = note;
    return BLUR_OK;
}

// One frame through the context's host staging buffer: in, body(d_src, d_dst) on its two halves (source and destination apart: the
// fused engine reads its neighbours' pixels while it writes and would otherwise copy an in-place frame into its workspace), out
template <typename Body>
static int blur_through_host_stage(blur_ctx* ctx, const void* src, void* dst, size_t bytes, Body body)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t half = (bytes + 255) & ~static_cast<size_t>(255);
    void* dv = nullptr;
    if (int rc0 = ensure_host_stage(ctx, 2 * half, &dv)) return rc0;
    char* d = static_cast<char*>(dv);
    int rc = BLUR_OK;
    hipError_t e = hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) rc = body(d, d + half);
    if (e == hipSuccess && rc == BLUR_OK) e = hipMemcpyAsync(dst, d + half, bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { ctx->err = std::string("host blur: ") + hipGetErrorString(e); return BLUR_ERR_HIP; }
    return rc;
}

// blur_gaussian_{u8,f32,u16,f16,bf16}_host
template <typename T>
static int blur_ch_host(blur_ctx* ctx, const T* src, T* dst, int rows, int cols, int channels, double sigma, const blur_opts* opts)
{
    if (int rc = check_ch_args(ctx, src, dst, 1, rows, cols, channels, sigma)) return rc;
    return blur_through_host_stage(ctx, src, dst, static_cast<size_t>(rows) * cols * channels * sizeof(T), [&](char* s, char* d) {
        return blur_ch_batch_impl(ctx, reinterpret_cast<const T*>(s), reinterpret_cast<T*>(d), 1, rows, cols, channels, sigma, opts);
    });
}

// ======================================================================================
// One sigma per channel (blur_gaussian_{u8,f32,u16,f16,bf16}_sigmas_*): channel c is what the scalar entry returns for sigmas[c];
// sigma = 0 leaves the channel as it is
// ======================================================================================
// The channels of a call by sigma: group g holds the channels in mask[g] with sigma[g] > 0, in the order of their first channel;
// zero_mask: the channels with sigma = 0
struct SigmaGroups {
    int ngroups = 0;
    double sigma[4] = {};
    unsigned mask[4] = {};
    int group_of[4] = { -1, -1, -1, -1 };
    unsigned zero_mask = 0;
};

// The arguments of every blur_gaussian_*_sigmas_* entry, without a context or a device: the status and, where it is not BLUR_OK,
// its text in *why.  Every entry of sigmas is checked here, before anything is launched: a refused call has written nothing.
// two_ok: two channels are legal (the chroma plane of an NV12 / P016 surface: blur_nv_batch_impl only)
static int ch_sigmas_status(const void* src, const void* dst, int nframes, int rows, int cols, int channels, const double* sigmas, SigmaGroups& sg, const char** why,
                            bool two_ok = false)
{
    auto no = [&](int rc, const char* text) { *why = text; return rc; };
    if (channels != 1 && channels != 3 && channels != 4 && !(two_ok && channels == 2)) return no(BLUR_ERR_INVALID, "channels must be 1, 3 or 4");
    if (!src || !dst || nframes < 0) return no(BLUR_ERR_INVALID, "null frame pointer or negative frame count");
    if (rows <= 0 || cols <= 0) return no(BLUR_ERR_INVALID, "rows and cols must be positive");
    if (!sigmas) return no(BLUR_ERR_INVALID, "sigmas must point to one sigma per channel");
    for (int c = 0; c < channels; ++c)
        if (!(sigmas[c] >= 0) || !std::isfinite(sigmas[c])) return no(BLUR_ERR_INVALID, "every sigma must be finite and positive, or 0 for a channel that is left as it is");
    sg = SigmaGroups{};
    for (int c = 0; c < channels; ++c) {
        if (sigmas[c] == 0) { sg.zero_mask |= 1u << c; continue; }
        int g = 0;
        while (g < sg.ngroups && sg.sigma[g] != sigmas[c]) ++g;
        if (g == sg.ngroups) sg.sigma[sg.ngroups++] = sigmas[c];
        sg.mask[g] |= 1u << c;
        sg.group_of[c] = g;
    }
    for (int g = 0; g < sg.ngroups; ++g) {
        const Sizing sz = pffft_sizing(rows, cols, sg.sigma[g]);
        if (sz.pad > rows - 1 || sz.pad > cols - 1)
            return no(BLUR_ERR_UNSUPPORTED, "pad > min(rows, cols) - 1 for one of the sigmas: reflect-101 would read outside the image (README.md:33-38)");
    }
    return BLUR_OK;
}

// the same for an entry with a context: the arguments' status first (ctx = NULL: the status is the same), then the missing context
static int check_ch_sigmas_args(blur_ctx* ctx, const void* src, const void* dst, int nframes, int rows, int cols, int channels, const double* sigmas, SigmaGroups& sg,
                                bool two_ok = false)
{
    const char* why = nullptr;
    if (int rc = ch_sigmas_status(src, dst, nframes, rows, cols, channels, sigmas, sg, &why, two_ok)) return fail(ctx, rc, why);
    return ctx ? BLUR_OK : BLUR_ERR_INVALID;
}

// The sigma = 0 channels of an out-of-place call: the samples (ES bytes each) of the channels in `mask` of a CH-interleaved batch go
// from src to dst.  The call runs before the blurred channels are written, on the same stream, and every channel outside the mask
// is one of them, so the other bytes of dst may hold anything afterwards.  vec (both pointers 16-byte aligned): a lane moves 16
// bytes of src as they are and dst is not read; the samples behind the last whole 16 bytes, and every sample where vec = 0, go
// one by one, the masked channels only.
template <int ES, int CH>
__global__ __launch_bounds__(256) void chan_copy(const uint8_t* __restrict__ src, uint8_t* dst, size_t nbytes, unsigned mask, int vec)
{
    using E = std::conditional_t<ES == 1, uint8_t, std::conditional_t<ES == 2, uint16_t, uint32_t>>;
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x, t0 = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
    const size_t nv = vec ? nbytes / 16 : 0, ne = nbytes / ES;
    for (size_t i = t0; i < nv; i += stride) reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
    for (size_t e = nv * (16 / ES) + t0; e < ne; e += stride)
        if (mask >> static_cast<unsigned>(e % CH) & 1u) reinterpret_cast<E*>(dst)[e] = reinterpret_cast<const E*>(src)[e];
}

// the same for pitched frames, row by row: only the masked channels' samples of the rows' cols pixels are written (frames in z)
template <int ES>
__global__ __launch_bounds__(256) void chan_copy_rows(const uint8_t* __restrict__ src, uint8_t* dst, int rows, int cols, int ch, unsigned mask, ChLayout L)
{
    using E = std::conditional_t<ES == 1, uint8_t, std::conditional_t<ES == 2, uint16_t, uint32_t>>;
    const uint8_t* s = src + blockIdx.z * L.sframe;
    uint8_t* d = dst + blockIdx.z * L.dframe;
    for (int r = blockIdx.y; r < rows; r += gridDim.y) {
        const E* sl = reinterpret_cast<const E*>(s + static_cast<size_t>(r) * L.spitch);
        E* dl = reinterpret_cast<E*>(d + static_cast<size_t>(r) * L.dpitch);
        for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < cols * ch; e += gridDim.x * blockDim.x)
            if (mask >> static_cast<unsigned>(e % ch) & 1u) dl[e] = sl[e];
    }
}

template <typename T>
static int launch_chan_copy_rows(blur_ctx* ctx, const T* src, T* dst, int nframes, int rows, int cols, int ch, unsigned mask, const ChLayout& L)
{
    if (!mask || nframes == 0) return BLUR_OK;
    const unsigned bx = static_cast<unsigned>(std::min<size_t>((static_cast<size_t>(cols) * ch + 255) / 256, 64));
    const dim3 grid(bx, static_cast<unsigned>(std::min<size_t>(rows, 1024)), static_cast<unsigned>(nframes));
    hipLaunchKernelGGL(chan_copy_rows<sizeof(T)>, grid, dim3(256), 0, ctx->stream, reinterpret_cast<const uint8_t*>(src), reinterpret_cast<uint8_t*>(dst), rows, cols, ch,
                       mask, L);
    HIP_TRY(ctx, hipGetLastError());
    return BLUR_OK;
}

template <typename T>
static int launch_chan_copy(blur_ctx* ctx, const T* src, T* dst, size_t nelem, int ch, unsigned mask)
{
    constexpr int ES = sizeof(T);
    const size_t nbytes = nelem * ES;
    if (nbytes == 0 || !mask) return BLUR_OK;
    const int vec = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0 ? 1 : 0;
    const size_t items = vec ? nbytes / 16 + 256 : nelem;
    const unsigned blocks = static_cast<unsigned>(std::min<size_t>((items + 255) / 256, 16384));
    auto kern = ch == 3 ? chan_copy<ES, 3> : (ch == 2 ? chan_copy<ES, 2> : chan_copy<ES, 4>);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, ctx->stream, reinterpret_cast<const uint8_t*>(src), reinterpret_cast<uint8_t*>(dst), nbytes, mask, vec);
    HIP_TRY(ctx, hipGetLastError());
    return BLUR_OK;
}

// One driver for the five element types, next to blur_ch_batch_impl.  The channels are grouped by sigma; one group without zeros is
// the scalar call itself.  Otherwise every group gets the engine blur_ch_batch_impl's rules give its sigma (choose_ch_engine; u8 with
// three channels too: its groups run on fw_blur_u8<NKB, Q, 3> where the scalar u8c3 call has other kernels), all of them before the
// first launch.  Overlapping frames, in place included, are read from one copy by every group.  Then, on the one stream: the copy of
// the sigma = 0 channels (out of place only), and per group the whole pre-pass (the quirk's sums are weighted by the pad's parity and
// the strips are as wide as the pad: both belong to the group) and the fused launch over the group's channels, or the plane path
// over them.  The strips and sums workspaces are reused from group to group.
// part.two_ok (blur_nv_batch_impl: the interleaved Cb/Cr plane of an NV12 / P016 surface): channels = 2 is legal, u8 and u16 only.
struct ChSigmasPart { bool two_ok = false; };

template <typename T>
static int blur_ch_sigmas_batch_impl(blur_ctx* ctx, const T* d_src, T* d_dst, int nframes, int rows, int cols, int channels, const double* sigmas, const blur_opts* opts,
                                     const ChLayout* lay = nullptr, const ChSigmasPart& part = {})
{
    SigmaGroups sg;
    if (lay)
        if (int rc = check_ch_layout(ctx, nframes, rows, cols, channels, sizeof(T), *lay, false, part.two_ok)) return rc;
    if (int rc = check_ch_sigmas_args(ctx, d_src, d_dst, nframes, rows, cols, channels, sigmas, sg, part.two_ok)) return rc;
    // (two channels have no scalar entry: one group over both is a launch of this driver)
    if (sg.ngroups == 1 && !sg.zero_mask && channels != 2) return blur_ch_batch_impl(ctx, d_src, d_dst, nframes, rows, cols, channels, sg.sigma[0], opts, lay);
    ChLayout L = lay ? *lay : ch_packed(rows, cols, channels, sizeof(T));
    if (nframes == 1) L.sframe = L.dframe = 0;
    const int choice = ch_engine_choice(ctx, opts, ch_type_name<T>(), " images, one sigma per channel");
    if (choice < 0) return BLUR_ERR_UNSUPPORTED;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Prepared p[4];
    std::string why[4];
    for (int g = 0; g < sg.ngroups; ++g)
        if (int rc = choose_ch_engine<T>(ctx, rows, cols, channels, sg.sigma[g], opts, choice, p[g], why[g], L)) return rc;
    ctx->engine_note.clear();
    if (nframes == 0) return BLUR_OK;
    const bool in_place = ch_in_place(d_src, d_dst, L);
    if (in_place && sg.ngroups == 0) return BLUR_OK;            // every channel is left as it is
    const size_t rowbytes = static_cast<size_t>(cols) * channels * sizeof(T), fe = static_cast<size_t>(rows) * cols * channels, fb = fe * sizeof(T);
    const bool packed = L.spitch == rowbytes && L.dpitch == rowbytes && (nframes == 1 || (L.sframe == fb && L.dframe == fb));
    int parts_rc;
    if (in_place && ch_in_place_parts(d_dst, nframes, fb, L.dframe, &parts_rc, [&](T* at, int nf, int) {
            return blur_ch_sigmas_batch_impl(ctx, at, at, nf, rows, cols, channels, sigmas, opts, lay, part);
        }))
        return parts_rc;
    if (int rc = ch_copy_source(ctx, &d_src, d_dst, nframes, nframes, rows, rowbytes, L)) return rc;
    if (!in_place) {
        if (!packed) {                  // a pitched destination: the samples of the sigma = 0 channels only, row by row
            if (int rc = launch_chan_copy_rows<T>(ctx, d_src, d_dst, nframes, rows, cols, channels, sg.zero_mask, L)) return rc;
        } else if (sg.ngroups == 0) HIP_TRY(ctx, hipMemcpyAsync(d_dst, d_src, fb * nframes, hipMemcpyDeviceToDevice, ctx->stream));
        else if (int rc = launch_chan_copy<T>(ctx, d_src, d_dst, fe * nframes, channels, sg.zero_mask)) return rc;       // (every other channel is written below)
    }
    const blur_opts fft_opts = with_engine(opts, BLUR_ENGINE_FFT);
    std::string note;
    for (int g = 0; g < sg.ngroups; ++g) {
        if (p[g].fx) {
            if (int rc = run_ch_fused<T>(ctx, d_src, d_dst, nframes, rows, cols, channels, p[g], fw_chsel_mask(sg.mask[g], channels), L)) return rc;
        } else {
            if (int rc = run_planes(ctx, d_src, d_dst, nframes, rows, cols, channels, sg.sigma[g], &fft_opts, L, sg.mask[g])) return rc;
            char head[96];
            std::snprintf(head, sizeof head, "%ssigma %g (channel mask 0x%x) on the plane path: ", note.empty() ? "" : "; ", sg.sigma[g], sg.mask[g]);
            note += head + why[g];
        }
    }
    // family 6: every blurred group ran on the fused kernel; 0: a group took the plane path, and the note names it
    ctx->last_family = note.empty() ? 6 : 0;
    ctx->engine_note = note;
    return BLUR_OK;
}

// blur_gaussian_*_sigmas_host (as blur_ch_host)
template <typename T>
static int blur_ch_sigmas_host(blur_ctx* ctx, const T* src, T* dst, int rows, int cols, int channels, const double* sigmas, const blur_opts* opts)
{
    SigmaGroups sg;
    if (int rc = check_ch_sigmas_args(ctx, src, dst, 1, rows, cols, channels, sigmas, sg)) return rc;
    return blur_through_host_stage(ctx, src, dst, static_cast<size_t>(rows) * cols * channels * sizeof(T), [&](char* s, char* d) {
        return blur_ch_sigmas_batch_impl(ctx, reinterpret_cast<const T*>(s), reinterpret_cast<T*>(d), 1, rows, cols, channels, sigmas, opts);
    });
}

// ======================================================================================
// Decoded video surfaces (blur_gaussian_nv12_*, blur_gaussian_p016_*): a rows x cols luma plane and a rows / 2 x cols / 2 plane of
// interleaved Cb/Cr pairs with the luma's row pitch.  A call is a luma part (one channel, sigmas[0]) and a chroma part (two
// channels, sigmas[1] and sigmas[2]) of blur_ch_sigmas_batch_impl, on the context's stream: grouping by sigma, launches over a
// subset of the channels, the copy of overlapping spans and the plane fallback are that driver's.  Two channels are legal there
// for these calls only (two_ok).
// ======================================================================================
struct NvSurface {
    const void* sy;
    const void* suv;
    void* dy;
    void* duv;
    size_t spitch, sy_frame, suv_frame, dpitch, dy_frame, duv_frame;
};

// The arguments of every blur_gaussian_{nv12,p016}_* entry, without a context or a device (es: bytes per sample): the status and,
// where it is not BLUR_OK, its text in *why.  Layout errors come before BLUR_ERR_UNSUPPORTED.
// nv_layout_status: the part that does not read sigmas (pointers, sizes, pitches, strides); nv_status: a call with one sigma per
// plane and channel; nv_frame_sigmas_status (below): one luma and one chroma sigma per frame
static int nv_layout_status(const NvSurface& s, size_t es, int nframes, int rows, int cols, const double* sigmas, const char** why)
{
    auto no = [&](int rc, const char* text) { *why = text; return rc; };
    if (!s.sy || !s.suv || !s.dy || !s.duv || !sigmas || nframes < 0) return no(BLUR_ERR_INVALID, "null plane or sigmas pointer, or negative frame count");
    if (rows <= 0 || cols <= 0 || (rows & 1) || (cols & 1)) return no(BLUR_ERR_INVALID, "rows and cols must be positive and even (4:2:0 chroma)");
    const size_t rowbytes = static_cast<size_t>(cols) * es;            // of a luma row and of a chroma row (cols / 2 pairs)
    if (s.spitch < rowbytes || s.dpitch < rowbytes) return no(BLUR_ERR_INVALID, "row pitch below cols * sizeof(sample)");
    if (s.spitch % es || s.dpitch % es) return no(BLUR_ERR_INVALID, "row pitch must be a multiple of the sample size");
    if (nframes > 1) {
        if (s.sy_frame % es || s.suv_frame % es || s.dy_frame % es || s.duv_frame % es) return no(BLUR_ERR_INVALID, "frame strides must be multiples of the sample size");
        if (s.sy_frame < ch_frame_span(rows, s.spitch, rowbytes) || s.dy_frame < ch_frame_span(rows, s.dpitch, rowbytes) ||
            s.suv_frame < ch_frame_span(rows / 2, s.spitch, rowbytes) || s.duv_frame < ch_frame_span(rows / 2, s.dpitch, rowbytes))
            return no(BLUR_ERR_INVALID, "frame stride below its plane's span: the planes of the batch would overlap");
    }
    return BLUR_OK;
}

// The n sigmas of a call, every `period` of them one luma sigma and then the chroma sigmas (in chroma pixels): each finite and >= 0,
// and the pad of each positive one within its plane
static int nv_sigmas_status(const double* sigmas, int n, int period, int rows, int cols, const char* luma_pad, const char* chroma_pad, const char** why)
{
    auto no = [&](int rc, const char* text) { *why = text; return rc; };
    for (int i = 0; i < n; ++i)
        if (!(sigmas[i] >= 0) || !std::isfinite(sigmas[i])) return no(BLUR_ERR_INVALID, "every sigma must be finite and positive, or 0 for a plane that is left as it is");
    for (int i = 0; i < n; ++i) {
        if (sigmas[i] == 0) continue;
        const bool chroma = i % period != 0;
        const int r = chroma ? rows / 2 : rows, c = chroma ? cols / 2 : cols;
        const Sizing sz = pffft_sizing(r, c, sigmas[i]);
        if (sz.pad > r - 1 || sz.pad > c - 1) return no(BLUR_ERR_UNSUPPORTED, chroma ? chroma_pad : luma_pad);
    }
    return BLUR_OK;
}

static int nv_status(const NvSurface& s, size_t es, int nframes, int rows, int cols, const double* sigmas, const char** why)
{
    if (int rc = nv_layout_status(s, es, nframes, rows, cols, sigmas, why)) return rc;
    return nv_sigmas_status(sigmas, 3, 3, rows, cols, "luma pad > min(rows, cols) - 1: reflect-101 would read outside the plane",
                            "chroma pad > min(rows / 2, cols / 2) - 1: reflect-101 would read outside the plane (sigmas[1], sigmas[2] are in chroma pixels)", why);
}

// the two planes of a batch of surfaces as the per-channel drivers take them: the layouts, and the chroma plane's size in pairs
struct NvPlanes { ChLayout Ly, Luv; int crows, ccols; };
static NvPlanes nv_planes(NvSurface s, int nframes, int rows, int cols)
{
    if (nframes <= 1) s.sy_frame = s.suv_frame = s.dy_frame = s.duv_frame = 0;           // (a single frame's strides address nothing)
    return NvPlanes{ { s.spitch, s.sy_frame, s.dpitch, s.dy_frame }, { s.spitch, s.suv_frame, s.dpitch, s.duv_frame }, rows / 2, cols / 2 };
}

// The luma part and the chroma part of a call, each a call of a per-channel driver, and what blur_last_engine says of both (blur_y,
// blur_c: the part has a sigma > 0, so it sets the family, and its note is empty where that is 6).  family 6: every blurred plane (of
// every frame) ran on the fused kernel; 0: some took the plane path, and the note names them
template <typename Luma, typename Chroma>
static int nv_run_parts(blur_ctx* ctx, bool blur_y, bool blur_c, const char* luma_prefix, Luma luma, Chroma chroma)
{
    std::string note;
    ctx->engine_note.clear();
    if (int rc = luma()) return rc;
    if (blur_y && ctx->last_family != 6) note = luma_prefix + ctx->engine_note;
    ctx->engine_note.clear();
    if (int rc = chroma()) return rc;
    if (blur_c && ctx->last_family != 6) note += (note.empty() ? "" : "; ") + std::string("chroma: ") + ctx->engine_note;
    ctx->last_family = note.empty() ? 6 : 0;
    ctx->engine_note = note;
    return BLUR_OK;
}

template <typename T>
static int blur_nv_batch_impl(blur_ctx* ctx, NvSurface s, int nframes, int rows, int cols, const double* sigmas, const blur_opts* opts)
{
    const char* why = nullptr;
    if (int rc = nv_status(s, sizeof(T), nframes, rows, cols, sigmas, &why)) return fail(ctx, rc, why);
    if (!ctx) return BLUR_ERR_INVALID;
    const NvPlanes pl = nv_planes(s, nframes, rows, cols);
    const int choice = ch_engine_choice(ctx, opts, "NV12 / P016", " surfaces");
    if (choice < 0) return BLUR_ERR_UNSUPPORTED;
    if (choice == BLUR_ENGINE_FUSED) {          // every plane's engine before the first launch: a refused call has written nothing
        for (int p = 0; p < 3; ++p) {
            if (sigmas[p] == 0 || (p == 2 && sigmas[2] == sigmas[1])) continue;
            Prepared pr;
            std::string note;
            if (int rc = choose_ch_engine<T>(ctx, p ? pl.crows : rows, p ? pl.ccols : cols, p ? 2 : 1, sigmas[p], opts, choice, pr, note, p ? pl.Luv : pl.Ly)) return rc;
        }
    }
    if (nframes == 0) return BLUR_OK;
    ChSigmasPart chroma;
    chroma.two_ok = true;
    return nv_run_parts(
        ctx, sigmas[0] > 0, sigmas[1] > 0 || sigmas[2] > 0, "luma on the plane path: ",
        [&] { return blur_ch_sigmas_batch_impl<T>(ctx, static_cast<const T*>(s.sy), static_cast<T*>(s.dy), nframes, rows, cols, 1, sigmas, opts, &pl.Ly); },
        [&] { return blur_ch_sigmas_batch_impl<T>(ctx, static_cast<const T*>(s.suv), static_cast<T*>(s.duv), nframes, pl.crows, pl.ccols, 2, sigmas + 1, opts, &pl.Luv, chroma); });
}

// blur_gaussian_{nv12,p016}_host: one packed surface (rows x cols luma samples, then rows / 2 rows of cols chroma samples) through the
// context's host staging buffer
template <typename T>
static int blur_nv_host(blur_ctx* ctx, const T* src, T* dst, int rows, int cols, const double* sigmas, const blur_opts* opts)
{
    const size_t pitch = cols > 0 ? static_cast<size_t>(cols) * sizeof(T) : 0, ybytes = rows > 0 ? pitch * rows : 0;
    NvSurface s{ src, reinterpret_cast<const char*>(src) + ybytes, dst, reinterpret_cast<char*>(dst) + ybytes, pitch, 0, 0, pitch, 0, 0 };
    if (!src || !dst) s.suv = s.duv = nullptr;
    const char* why = nullptr;
    if (int rc = nv_status(s, sizeof(T), 1, rows, cols, sigmas, &why)) return fail(ctx, rc, why);
    if (!ctx) return BLUR_ERR_INVALID;
    return blur_through_host_stage(ctx, src, dst, ybytes + ybytes / 2, [&](char* sd, char* dd) {
        return blur_nv_batch_impl<T>(ctx, NvSurface{ sd, sd + ybytes, dd, dd + ybytes, pitch, 0, 0, pitch, 0, 0 }, 1, rows, cols, sigmas, opts);
    });
}

// ======================================================================================
// One sigma per frame (blur_gaussian_{u8,f32,u16,f16,bf16}_frame_sigmas_*): frame f is what the scalar entry returns for it alone with
// sigmas[f]; sigma = 0 copies the frame
// ======================================================================================
// The frames of a call by sigma and by window class.  slot: the distinct positive sigmas in the order of their first frame (frames
// of equal sigma share their fragments and taps); group: the window classes in the order of their first frame (the frames of a
// class share a fused launch; class 0 = the pads without a fused kernel)
struct FrameSigmaPlan {
    struct Slot { double sigma; Sizing sz; int nkb; int group; };
    std::vector<Slot> slots;
    std::vector<int> slot_of;            // per frame; -1: sigma = 0
    std::vector<int> group_nkb;
};

// The arguments of every blur_gaussian_*_frame_sigmas_* entry, without a context or a device: the status and, where it is not
// BLUR_OK, its text in *why.  Every entry of sigmas is checked here, before anything is launched: a refused call has written nothing.
// two_ok: two channels are legal (the chroma plane of an NV12 / P016 surface: blur_nv_frame_sigmas_batch_impl only)
static int frame_sigmas_status(const void* src, const void* dst, int nframes, int rows, int cols, int channels, const double* sigmas, FrameSigmaPlan& pl, const char** why,
                               bool two_ok = false)
{
    auto no = [&](int rc, const char* text) { *why = text; return rc; };
    if (channels != 1 && channels != 3 && channels != 4 && !(two_ok && channels == 2)) return no(BLUR_ERR_INVALID, "channels must be 1, 3 or 4");
    if (!src || !dst || nframes < 0) return no(BLUR_ERR_INVALID, "null frame pointer or negative frame count");
    if (rows <= 0 || cols <= 0) return no(BLUR_ERR_INVALID, "rows and cols must be positive");
    if (!sigmas) return no(BLUR_ERR_INVALID, "sigmas must point to one sigma per frame");
    for (int f = 0; f < nframes; ++f)
        if (!(sigmas[f] >= 0) || !std::isfinite(sigmas[f])) return no(BLUR_ERR_INVALID, "every sigma must be finite and positive, or 0 for a frame that is copied");
    pl = FrameSigmaPlan{};
    pl.slot_of.assign(nframes, -1);
    std::map<double, int> seen;
    std::map<int, int> group_of_nkb;
    for (int f = 0; f < nframes; ++f) {
        if (sigmas[f] == 0) continue;
        auto it = seen.find(sigmas[f]);
        if (it == seen.end()) {
            FrameSigmaPlan::Slot sl{ sigmas[f], pffft_sizing(rows, cols, sigmas[f]), 0, 0 };
            if (sl.sz.pad > rows - 1 || sl.sz.pad > cols - 1)
                return no(BLUR_ERR_UNSUPPORTED, "pad > min(rows, cols) - 1 for one of the sigmas: reflect-101 would read outside the image (README.md:33-38)");
            const FxEntry* fe = find_entry_for_pad<FxEntry>(sl.sz.pad);
            sl.nkb = fe ? fe->nkb : 0;
            auto g = group_of_nkb.find(sl.nkb);
            if (g == group_of_nkb.end()) {
                g = group_of_nkb.emplace(sl.nkb, static_cast<int>(pl.group_nkb.size())).first;
                pl.group_nkb.push_back(sl.nkb);
            }
            sl.group = g->second;
            it = seen.emplace(sigmas[f], static_cast<int>(pl.slots.size())).first;
            pl.slots.push_back(sl);
        }
        pl.slot_of[f] = it->second;
    }
    return BLUR_OK;
}

// what a one-sigma-per-frame call reports of its frames on the plane path (blur_last_engine's note)
struct FramePlaneNote {
    int count = 0, first = -1;
    double sigma = 0;
    std::string why;
};

// The call's table -> the context's device workspace, in one upload on the call's stream.  The staging memory is pinned and
// reused from call to call; the upload that last read it may still be in flight (the call is asynchronous), so its event is
// waited for before the memory is rewritten -- the upload, not the kernels behind it.
static int fs_upload(blur_ctx* ctx, const std::vector<unsigned char>& host)
{
    if (int rc = ensure_buf(ctx, &ctx->fs_table, &ctx->fs_table_bytes, host.size())) return rc;
    if (ctx->fs_pending) {
        HIP_TRY(ctx, hipEventSynchronize(ctx->fs_uploaded));
        ctx->fs_pending = false;
    }
    if (ctx->fs_stage_bytes < host.size()) {
        if (ctx->fs_stage) { HIP_TRY(ctx, hipHostFree(ctx->fs_stage)); ctx->fs_stage = nullptr; ctx->fs_stage_bytes = 0; }
        const size_t bytes = host.size() + host.size() / 2;
        HIP_TRY(ctx, hipHostMalloc(&ctx->fs_stage, bytes, hipHostMallocDefault));
        ctx->fs_stage_bytes = bytes;
    }
    if (!ctx->fs_uploaded) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->fs_uploaded, hipEventDisableTiming));
    std::memcpy(ctx->fs_stage, host.data(), host.size());
    HIP_TRY(ctx, hipMemcpyAsync(ctx->fs_table, ctx->fs_stage, host.size(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->fs_uploaded, ctx->stream));
    ctx->fs_pending = true;
    return BLUR_OK;
}

// One driver over the five element types, next to blur_ch_sigmas_batch_impl (u16 and the half types take run_ff<T> as they do there).
// Every distinct sigma gets the engine blur_ch_batch_impl's rules give it (prepare's for the pad and the frame, then ch_fused_refusal;
// u8 with three channels: those of one and four channels, on fw_blur_u8<NKB, Q, 3> -- never the u8c3 entry, whatever the sigmas: a
// frame's bytes depend on its pixels, its sigma and opts alone) and its fragments, taps and gains from mx_host_tables, the code
// behind the scalar entries' cached tables; nothing goes into ctx->mx_tables.  All of that happens before the first launch.  Then, on
// the one stream: the copy of overlapping sources, the copies of the sigma = 0 frames (out of place only), the upload of the call's
// table, and per window class the pre-pass and ONE fused launch over the class's frames (their list: FwFrame); the frames without
// a fused kernel run one by one on the plane path.  The strips and sums workspaces are reused from class to class.
// note: null for the call itself; the parts of a large in-place batch add to their caller's, frame0 being their first frame in its batch
// two_ok (blur_nv_frame_sigmas_batch_impl: the interleaved Cb/Cr plane of an NV12 / P016 surface): channels = 2 is legal, u8 and u16 only.
// plan_only: return once every sigma has its engine, before anything is written (that caller's check of one part ahead of the other's
// launches)
struct ChFramePart { FramePlaneNote* note = nullptr; int frame0 = 0; bool two_ok = false, plan_only = false; };

template <typename T>
static int blur_ch_frame_sigmas_batch_impl(blur_ctx* ctx, const T* d_src, T* d_dst, int nframes, int rows, int cols, int channels, const double* sigmas, const blur_opts* opts,
                                           const ChLayout* lay = nullptr, const ChFramePart& part = {})
{
    FrameSigmaPlan pl;
    if (lay)
        if (int rc = check_ch_layout(ctx, nframes, rows, cols, channels, sizeof(T), *lay, true, part.two_ok)) return rc;
    const char* bad = nullptr;
    if (int rc = frame_sigmas_status(d_src, d_dst, nframes, rows, cols, channels, sigmas, pl, &bad, part.two_ok)) return fail(ctx, rc, bad);
    if (!ctx) return BLUR_ERR_INVALID;
    ChLayout L = lay ? *lay : ch_packed(rows, cols, channels, sizeof(T));
    if (nframes == 1) L.sframe = L.dframe = 0;
    const int choice = ch_engine_choice(ctx, opts, ch_type_name<T>(), " images, one sigma per frame");
    if (choice < 0) return BLUR_ERR_UNSUPPORTED;
    const bool quirk = opts ? opts->nyquist_quirk != 0 : true;
    const size_t rowbytes = static_cast<size_t>(cols) * channels * sizeof(T), fb = rowbytes * rows;
    // the engine and the tables of every distinct sigma
    const int nslots = static_cast<int>(pl.slots.size());
    std::vector<MxHostTables> tabs(nslots);
    std::vector<char> fused(nslots, 0);
    std::string plane_why;          // of the first sigma that stays on the plane path: the slots' order makes its first frame the first of those
    for (int s = 0; s < nslots && choice != BLUR_ENGINE_FFT; ++s) {
        const FrameSigmaPlan::Slot& sl = pl.slots[s];
        const char* w = sl.nkb ? fx_frame_limits(rows, cols, quirk) : "fused matrix-core engine: no kernel instantiated for this pad";
        if (!w) {
            std::vector<float> karr[2];
            if (mx_kernel_arrays(sl.sigma, sl.sz, nullptr, karr, &w) == BLUR_OK) (void)mx_host_tables(karr, sl.sz, sl.nkb, tabs[s], &w, false);
        }
        const std::string why = w ? std::string(w) : ch_fused_refusal<T>(sl.nkb, rows, cols, channels, choice, L, true);
        if (!why.empty() && choice == BLUR_ENGINE_FUSED) return fail(ctx, BLUR_ERR_UNSUPPORTED, why.c_str());
        fused[s] = why.empty();
        if (!fused[s] && plane_why.empty()) plane_why = why;
    }
    if (part.plan_only) return BLUR_OK;
    if (!part.note) ctx->engine_note.clear();
    if (nframes == 0) return BLUR_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool in_place = ch_in_place(d_src, d_dst, L);
    if (in_place && nslots == 0) return BLUR_OK;                  // every frame is left as it is
    FramePlaneNote mine;
    FramePlaneNote& pn = part.note ? *part.note : mine;
    int parts_rc;
    if (in_place && ch_in_place_parts(d_dst, nframes, fb, L.dframe, &parts_rc, [&](T* at, int nf, int f0) {
            ChFramePart sub = part;
            sub.note = &pn, sub.frame0 += f0;
            return blur_ch_frame_sigmas_batch_impl(ctx, at, at, nf, rows, cols, channels, sigmas + f0, opts, lay, sub);
        })) {
        if (parts_rc) return parts_rc;
        nframes = 0;                                               // (the note is written below)
    }
    // one gathered copy of an overlapping source; a broadcast source (frame stride 0) is one frame
    const bool broadcast = nframes > 1 && L.sframe == 0;
    if (nframes > 0) {
        if (int rc = ch_copy_source(ctx, &d_src, d_dst, nframes, broadcast ? 1 : nframes, rows, rowbytes, L)) return rc;
        if (broadcast || nframes == 1) L.sframe = 0;
    }
    auto src_of = [&](int f) { return reinterpret_cast<const T*>(reinterpret_cast<const char*>(d_src) + static_cast<size_t>(f) * L.sframe); };
    auto dst_of = [&](int f) { return reinterpret_cast<T*>(reinterpret_cast<char*>(d_dst) + static_cast<size_t>(f) * L.dframe); };
    // the sigma = 0 frames of an out-of-place call first
    if (!in_place)
        for (int f = 0; f < nframes; ++f)
            if (pl.slot_of[f] < 0) HIP_TRY(ctx, hipMemcpy2DAsync(dst_of(f), L.dpitch, src_of(f), L.spitch, rowbytes, rows, hipMemcpyDeviceToDevice, ctx->stream));
    // the call's table: [the frame lists of the classes, one behind the other][per fused sigma: its fragments, its taps]
    std::vector<std::vector<int>> members(pl.group_nkb.size());
    int nlisted = 0;
    for (int f = 0; f < nframes; ++f) {
        const int s = pl.slot_of[f];
        if (s >= 0 && fused[s]) { members[pl.slots[s].group].push_back(f); ++nlisted; }
    }
    if (nlisted > 0) {
        auto up16 = [](size_t v) { return (v + 15) & ~static_cast<size_t>(15); };
        size_t bytes = up16(static_cast<size_t>(nlisted) * sizeof(FwFrame));
        std::vector<size_t> frags_at(nslots, 0), taps_at(nslots, 0);
        std::vector<char> used(nslots, 0);
        for (int f = 0; f < nframes; ++f)
            if (pl.slot_of[f] >= 0 && fused[pl.slot_of[f]]) used[pl.slot_of[f]] = 1;
        for (int s = 0; s < nslots; ++s) {
            if (!used[s]) continue;
            frags_at[s] = bytes;
            bytes = up16(bytes + tabs[s].frags[0].size() * sizeof(uint16_t));
            taps_at[s] = bytes;
            bytes = up16(bytes + tabs[s].taps_row.size() * sizeof(float));
        }
        std::vector<unsigned char> host(bytes, 0);
        FwFrame* list = reinterpret_cast<FwFrame*>(host.data());
        int at = 0;
        for (const std::vector<int>& m : members)
            for (int f : m) {
                const int s = pl.slot_of[f];
                const MxHostTables& t = tabs[s];
                const int pad = pl.slots[s].sz.pad;
                // (bscale: B of ff_scale_exp, as run_ff makes it for a scalar call)
                list[at++] = FwFrame{ f, pad, static_cast<uint32_t>(frags_at[s] / 16), static_cast<uint32_t>(taps_at[s] / sizeof(float)), t.dr, t.dc,
                                      quirk ? 1.0 + std::fabs(static_cast<double>(t.dr)) * (static_cast<double>(cols) + 2.0 * pad) : 1.0 };
            }
        for (int s = 0; s < nslots; ++s) {
            if (!used[s]) continue;
            std::memcpy(host.data() + frags_at[s], tabs[s].frags[0].data(), tabs[s].frags[0].size() * sizeof(uint16_t));
            std::memcpy(host.data() + taps_at[s], tabs[s].taps_row.data(), tabs[s].taps_row.size() * sizeof(float));
        }
        if (int rc = fs_upload(ctx, host)) return rc;
        // per class: the pre-pass and one launch over its frames.  The runners take the class's kernel from p.fx, the table where a
        // scalar call has its fragments and taps, and everything that depends on sigma from the list
        MxTables table;
        table.frags_row = ctx->fs_table;
        table.taps_row = static_cast<float*>(ctx->fs_table);
        at = 0;
        for (size_t g = 0; g < members.size(); ++g) {
            const int n = static_cast<int>(members[g].size());
            if (n == 0) continue;
            Prepared p;
            p.sz = Sizing{};                                       // (the pads are the list's)
            p.fx = find_entry_for_pad<FxEntry>(8 * (pl.group_nkb[g] - 2));
            p.mxt = &table;
            p.mx_quirk = quirk;
            const FwFrame* ft = static_cast<const FwFrame*>(ctx->fs_table) + at;
            at += n;
            if (int rc = run_ch_fused<T>(ctx, d_src, d_dst, n, rows, cols, channels, p, fw_chsel_all(channels), L, ft)) return rc;
        }
    }
    // the frames without a fused kernel, one by one on the plane path
    const blur_opts fft_opts = with_engine(opts, BLUR_ENGINE_FFT);
    ChLayout L1 = L;
    L1.sframe = L1.dframe = 0;
    for (int f = 0; f < nframes; ++f) {
        const int s = pl.slot_of[f];
        if (s < 0 || fused[s]) continue;
        if (int rc = run_planes(ctx, src_of(f), dst_of(f), 1, rows, cols, channels, pl.slots[s].sigma, &fft_opts, L1)) return rc;
        if (pn.count++ == 0) { pn.first = part.frame0 + f; pn.sigma = pl.slots[s].sigma; pn.why = plane_why; }
    }
    if (!part.note) {
        // family 6: every blurred frame ran on the fused kernel; 0: frames took the plane path, and the note names the first
        ctx->last_family = pn.count ? 0 : 6;
        ctx->engine_note.clear();
        if (pn.count) {
            char head[128];
            std::snprintf(head, sizeof head, "%d frame%s on the plane path, the first frame %d (sigma %g)%s", pn.count, pn.count == 1 ? "" : "s", pn.first, pn.sigma,
                          pn.why.empty() ? "" : ": ");
            ctx->engine_note = head + pn.why;
        }
    }
    return BLUR_OK;
}

// ======================================================================================
// One luma and one chroma sigma per frame of a decoded clip (blur_gaussian_{nv12,p016}_frame_sigmas_batch_dev): sigmas[2 f] and
// sigmas[2 f + 1].  A call is a luma part (one channel) and a chroma part (two channels, two_ok) of blur_ch_frame_sigmas_batch_impl,
// as blur_nv_batch_impl is two parts of blur_ch_sigmas_batch_impl.
// ======================================================================================
static int nv_frame_sigmas_status(const NvSurface& s, size_t es, int nframes, int rows, int cols, const double* sigmas, const char** why)
{
    if (int rc = nv_layout_status(s, es, nframes, rows, cols, sigmas, why)) return rc;
    return nv_sigmas_status(sigmas, 2 * nframes, 2, rows, cols, "luma pad > min(rows, cols) - 1 for one of the frames: reflect-101 would read outside the plane",
                            "chroma pad > min(rows / 2, cols / 2) - 1 for one of the frames: reflect-101 would read outside the plane (chroma sigmas are in chroma pixels)", why);
}

template <typename T>
static int blur_nv_frame_sigmas_batch_impl(blur_ctx* ctx, NvSurface s, int nframes, int rows, int cols, const double* sigmas, const blur_opts* opts)
{
    const char* why = nullptr;
    if (int rc = nv_frame_sigmas_status(s, sizeof(T), nframes, rows, cols, sigmas, &why)) return fail(ctx, rc, why);
    if (!ctx) return BLUR_ERR_INVALID;
    const NvPlanes pl = nv_planes(s, nframes, rows, cols);
    const int choice = ch_engine_choice(ctx, opts, "NV12 / P016", " surfaces");
    if (choice < 0) return BLUR_ERR_UNSUPPORTED;
    std::vector<double> sy(nframes), sc(nframes);
    bool blur_y = false, blur_c = false;
    for (int f = 0; f < nframes; ++f) {
        sy[f] = sigmas[2 * f];
        sc[f] = sigmas[2 * f + 1];
        blur_y = blur_y || sy[f] > 0;
        blur_c = blur_c || sc[f] > 0;
    }
    const T* src_y = static_cast<const T*>(s.sy);
    const T* src_uv = static_cast<const T*>(s.suv);
    T* dst_y = static_cast<T*>(s.dy);
    T* dst_uv = static_cast<T*>(s.duv);
    // every chroma frame's engine before the luma part's first launch (the luma part chooses its own before it launches): a refused
    // call has written nothing.  Only FUSED refuses.
    ChFramePart chroma, chroma_plan;
    chroma.two_ok = chroma_plan.two_ok = true;
    chroma_plan.plan_only = true;
    if (choice == BLUR_ENGINE_FUSED)
        if (int rc = blur_ch_frame_sigmas_batch_impl<T>(ctx, src_uv, dst_uv, nframes, pl.crows, pl.ccols, 2, sc.data(), opts, &pl.Luv, chroma_plan)) return rc;
    if (nframes == 0) return BLUR_OK;
    return nv_run_parts(
        ctx, blur_y, blur_c, "luma: ", [&] { return blur_ch_frame_sigmas_batch_impl<T>(ctx, src_y, dst_y, nframes, rows, cols, 1, sy.data(), opts, &pl.Ly); },
        [&] { return blur_ch_frame_sigmas_batch_impl<T>(ctx, src_uv, dst_uv, nframes, pl.crows, pl.ccols, 2, sc.data(), opts, &pl.Luv, chroma); });
}

// ======================================================================================
// C ABI
// ======================================================================================
// ---- whole-image 2D path: helpers (the entry points are below, blur_pocketfft2d_*) ----
static int get_pos_of_freq(blur_ctx* ctx, DevicePlan* dp, const int** out)
{
    if (!dp->d_pos_of_freq) {
        const int n = dp->dev.n;
        std::vector<int> inv(n);
        for (int pos = 0; pos < n; ++pos) inv[dp->host.freq_of_pos[pos]] = pos;
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&dp->d_pos_of_freq), sizeof(int) * n));
        HIP_TRY(ctx, hipMemcpy(dp->d_pos_of_freq, inv.data(), sizeof(int) * n, hipMemcpyHostToDevice));
    }
    *out = dp->d_pos_of_freq;
    return BLUR_OK;
}

template <bool CONV>
static int launch_img2d_cols(blur_ctx* ctx, float2* z, int s0, int s1, const DevicePlan& plan, const float* mcol, const float* krow_pos)
{
    // widest strip of columns whose lines fit the LDS: 8 columns = one 64-byte segment of a spectrum row
    const size_t line = static_cast<size_t>(line_stride(s0)) * sizeof(float2);
    int G = 8;
    while (G > 1 && G * line > kLdsLimit) G >>= 1;
    if (G * line > kLdsLimit) return fail(ctx, BLUR_ERR_UNSUPPORTED, "2D path: column FFT length exceeds LDS capacity");
    const int grid = (s1 + G - 1) / G;
#define BLUR_IMG2D_COLS(G_)                                                                                                        \
    case G_:                                                                                                                        \
        if (int rc = set_lds(ctx, img2d_cols_kernel<G_, CONV>, G_ * line)) return rc;                                              \
        hipLaunchKernelGGL((img2d_cols_kernel<G_, CONV>), dim3(grid), dim3(kThreads), G_ * line, ctx->stream, z, s0, s1, plan.dev, \
                           plan.d_tw, mcol, krow_pos);                                                                             \
        break;
    switch (G) {
        BLUR_IMG2D_COLS(8)
        BLUR_IMG2D_COLS(4)
        BLUR_IMG2D_COLS(2)
        BLUR_IMG2D_COLS(1)
    }
#undef BLUR_IMG2D_COLS
    HIP_TRY(ctx, hipGetLastError());
    return BLUR_OK;
}

extern "C" {

void blur_opts_default(blur_opts* o)
{
    if (!o) return;
    std::memset(o, 0, sizeof *o);
    o->nyquist_quirk = 1;
}

int blur_gaussian_window(double sigma, int max_width) { return gaussian_window(sigma, max_width); }

int blur_get_gaussian(float* kernel, double sigma, int width, int fft_length)
{
    if (!kernel || !(sigma > 0) || width < 0 || fft_length < 0) return BLUR_ERR_INVALID;
    get_gaussian(kernel, sigma, width, fft_length);
    return BLUR_OK;
}

int blur_is_valid_size(int n) { return is_valid_size(n); }
int blur_nearest_transform_size(int n) { return nearest_transform_size(n); }

int blur_pffft_sizing(int rows, int cols, double sigma, int out[6])
{
    if (!out || rows <= 0 || cols <= 0 || !(sigma > 0)) return BLUR_ERR_INVALID;
    const Sizing s = pffft_sizing(rows, cols, sigma);
    out[0] = s.kSize; out[1] = s.pad; out[2] = s.n_col; out[3] = s.n_row; out[4] = s.tz_col; out[5] = s.tz_row;
    return BLUR_OK;
}

int blur_kernel_multipliers(double sigma, int ksize, int n, float* m)
{
    if (!m || !(sigma > 0) || ksize <= 0 || n < ksize) return BLUR_ERR_INVALID;
    kernel_multipliers(sigma, ksize, n, m);
    return BLUR_OK;
}

int blur_wr_kernel_multipliers(double sigma, int ksize, int n, int n_ref, int quirk, float* m)
{
    if (!m || !(sigma > 0) || ksize <= 0 || n < ksize || (n & 1) || n_ref <= 0) return BLUR_ERR_INVALID;
    std::vector<float> k(std::max(n, ksize));
    get_gaussian(k.data(), sigma, ksize, n);
    wr_multipliers(k.data(), n, n_ref, quirk != 0, m);
    return BLUR_OK;
}

int blur_fft_plan_radices(int n, int* radices)
{
    FftPlan p;
    if (!radices || !make_plan(n, p)) return 0;
    for (int i = 0; i < p.npass; ++i) radices[i] = p.radix[i];
    return p.npass;
}

int blur_ctx_create(blur_ctx** out, int device)
{
    if (!out) return BLUR_ERR_INVALID;
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        g_create_err = std::string("no HIP device available: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
        return BLUR_ERR_HIP;
    }
    if (device < 0 || device >= count) { g_create_err = "device ordinal out of range"; return BLUR_ERR_INVALID; }
    e = hipSetDevice(device);
    if (e != hipSuccess) { g_create_err = std::string("hipSetDevice: ") + hipGetErrorString(e); return BLUR_ERR_HIP; }
    blur_ctx* c = new blur_ctx();
    c->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) c->num_cus = prop.multiProcessorCount;
    int xccs = 0;   // the XCD-banded task maps of the matrix-core kernels (fx_kernels.hpp, mx_kernels.hpp) take the count from the device
    if (hipDeviceGetAttribute(&xccs, hipDeviceAttributeNumberOfXccs, device) == hipSuccess && xccs > 0) c->num_xcds = xccs;
    *out = c;
    return BLUR_OK;
}

int blur_ctx_destroy(blur_ctx* ctx)
{
    if (!ctx) return BLUR_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (auto& kv : ctx->plans) {
        if (kv.second->d_tw) (void)hipFree(kv.second->d_tw);
        if (kv.second->d_pos_of_freq) (void)hipFree(kv.second->d_pos_of_freq);
    }
    for (auto& kv : ctx->spectra) (void)hipFree(kv.second);
    if (ctx->d_w256) (void)hipFree(ctx->d_w256);
    for (auto& kv : ctx->wr_tw0) (void)hipFree(kv.second);
    for (auto& kv : ctx->wr_spectra) (void)hipFree(kv.second);
    for (auto& kv : ctx->mx_tables) {
        (void)hipFree(kv.second.frags_row); (void)hipFree(kv.second.frags_col);
        (void)hipFree(kv.second.taps_row);
    }
    for (auto& lt : ctx->lines_tables) (void)hipFree(lt.dev);
    if (ctx->fx_strips) (void)hipFree(ctx->fx_strips);
    if (ctx->fx_sums) (void)hipFree(ctx->fx_sums);
    if (ctx->tl_sums) (void)hipFree(ctx->tl_sums);
    if (ctx->tl_terms) (void)hipFree(ctx->tl_terms);
    if (ctx->tl_copy) (void)hipFree(ctx->tl_copy);
    for (auto& kv : ctx->tl_taps) (void)hipFree(kv.second);
    if (ctx->mx_sums) (void)hipFree(ctx->mx_sums);
    if (ctx->mx_terms) (void)hipFree(ctx->mx_terms);
    if (ctx->work) (void)hipFree(reinterpret_cast<char*>(ctx->work) - kWorkGuard);
    if (ctx->work2) (void)hipFree(ctx->work2);
    if (ctx->box_tmp) (void)hipFree(ctx->box_tmp);
    if (ctx->ch_planes) (void)hipFree(ctx->ch_planes);
    if (ctx->ch_copy) (void)hipFree(ctx->ch_copy);
    if (ctx->ff_sums) (void)hipFree(ctx->ff_sums);
    if (ctx->ff_strips) (void)hipFree(ctx->ff_strips);
    if (ctx->fs_table) (void)hipFree(ctx->fs_table);
    if (ctx->fs_stage) (void)hipHostFree(ctx->fs_stage);
    if (ctx->fs_uploaded) (void)hipEventDestroy(ctx->fs_uploaded);
    if (ctx->host_stage) (void)hipFree(ctx->host_stage);
    if (ctx->pipe.ready) {
        (void)hipStreamSynchronize(ctx->pipe.h2d);
        (void)hipStreamSynchronize(ctx->pipe.d2h);
        for (int k = 0; k < HostPipe::S; ++k) {
            if (ctx->pipe.buf[k]) (void)hipFree(ctx->pipe.buf[k]);
            (void)hipEventDestroy(ctx->pipe.in_done[k]);
            (void)hipEventDestroy(ctx->pipe.comp_done[k]);
            (void)hipEventDestroy(ctx->pipe.out_done[k]);
        }
        (void)hipStreamDestroy(ctx->pipe.h2d);
        (void)hipStreamDestroy(ctx->pipe.d2h);
    }
    for (auto& t : ctx->ev_busy) { (void)hipEventDestroy(std::get<0>(t)); (void)hipEventDestroy(std::get<1>(t)); }
    for (auto& t : ctx->ev_free) { (void)hipEventDestroy(t.first); (void)hipEventDestroy(t.second); }
    delete ctx;
    return BLUR_OK;
}

int blur_ctx_set_stream(blur_ctx* ctx, void* hip_stream)
{
    if (!ctx) return BLUR_ERR_INVALID;
    hipStream_t next = static_cast<hipStream_t>(hip_stream);
    if (next != ctx->stream) {
        // the workspace and the cached tables are shared: work queued on the old stream must be
        // finished before another stream may touch them
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        ctx->stream = next;
    }
    return BLUR_OK;
}

int blur_ctx_synchronize(blur_ctx* ctx)
{
    if (!ctx) return BLUR_ERR_INVALID;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return BLUR_OK;
}

const char* blur_last_error(const blur_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

int blur_ctx_timing_enable(blur_ctx* ctx, int on)
{
    if (!ctx) return BLUR_ERR_INVALID;
    ctx->timing = on == 2 ? 2 : on != 0 ? 1 : 0;
    return BLUR_OK;
}

int blur_ctx_timing(blur_ctx* ctx, double out_ms[2], int out_launches[2], int out_frames[2], int reset)
{
    if (!ctx) return BLUR_ERR_INVALID;
    if (int rc = timing_drain(ctx)) return rc;
    for (int i = 0; i < 2; ++i) {
        if (out_ms) out_ms[i] = ctx->ms[i];
        if (out_launches) out_launches[i] = ctx->launches[i];
        if (out_frames) out_frames[i] = ctx->frames[i];
        if (reset) { ctx->ms[i] = 0; ctx->launches[i] = 0; ctx->frames[i] = 0; }
    }
    return BLUR_OK;
}

// both passes on the matrix cores; V (24-bit fixed point, mx_kernels.hpp) lives in the float workspace
static int run_mx_u8c3(blur_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int nframes, int rows, int cols, int chunk, const Prepared& p)
{
    const size_t px = static_cast<size_t>(rows) * cols;
    MxGeom g{ rows, cols, p.sz.pad, p.mx_vpitch, 0, 0, mx_vrows(rows, p.mx->nkb), ctx->num_xcds };
    const int chunks = (cols + kMxRowChunk - 1) / kMxRowChunk, rblocks = g.vrows / 32, zblocks = (g.vrows + 255) / 256;
    // the quirk's scratch per frame: spart int [chunks][rows][3]; then floats: vpart [rblocks][vpitch], qrow [3][vrows], qcol [vpitch];
    // then doubles: zpart [zblocks][3]
    const size_t n_spart = static_cast<size_t>(chunks) * rows * 3, n_vpart = static_cast<size_t>(rblocks) * g.vpitch,
                 n_qrow = static_cast<size_t>(3) * g.vrows, n_qcol = g.vpitch, n_zpart = static_cast<size_t>(zblocks) * 3;
    const size_t sums_bytes = n_spart * sizeof(int) * chunk;
    const size_t terms_bytes = ((n_vpart + n_qrow + n_qcol) * sizeof(float) + n_zpart * sizeof(double)) * chunk + 64;
    if (p.mx_quirk) {
        if (ctx->mx_sums_bytes < sums_bytes) {
            if (ctx->mx_sums) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); HIP_TRY(ctx, hipFree(ctx->mx_sums)); ctx->mx_sums = nullptr; ctx->mx_sums_bytes = 0; }
            HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->mx_sums), sums_bytes));
            ctx->mx_sums_bytes = sums_bytes;
        }
        if (ctx->mx_terms_bytes < terms_bytes) {
            if (ctx->mx_terms) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); HIP_TRY(ctx, hipFree(ctx->mx_terms)); ctx->mx_terms = nullptr; ctx->mx_terms_bytes = 0; }
            HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->mx_terms), terms_bytes));
            ctx->mx_terms_bytes = terms_bytes;
        }
    }
    for (int f = 0; f < nframes; f += chunk) {
        const int nf = nframes - f < chunk ? nframes - f : chunk;
        const uint8_t* s = d_src + static_cast<size_t>(f) * px * 3;
        uint8_t* d = d_dst + static_cast<size_t>(f) * px * 3;
        g.nframes = nf;
        g.aligned = ((cols & 3) == 0 && (reinterpret_cast<uintptr_t>(s) & 3) == 0) ? 1 : 0;
        int* spart = nullptr;
        float *vpart = nullptr, *qrow = nullptr, *qcol = nullptr;
        double* zpart = nullptr;
        if (p.mx_quirk) {
            spart = ctx->mx_sums;
            zpart = reinterpret_cast<double*>(ctx->mx_terms);                      // doubles first: 8-byte aligned
            vpart = reinterpret_cast<float*>(zpart + n_zpart * nf);
            qrow = vpart + n_vpart * nf;
            qcol = qrow + n_qrow * nf;
        }
        { TimedLaunch t(ctx, 0, nf);
          HIP_TRY(ctx, p.mx->row_u8(ctx->stream, s, ctx->work, p.mxt->frags_row, g, ctx->num_cus, spart, vpart)); }
        if (p.mx_quirk) {
            // the Nyquist-slot terms from the row kernel's partial sums: two small launches between the passes
            hipLaunchKernelGGL(mx_quirk_rows, dim3(zblocks, nf), dim3(256), 0, ctx->stream, spart, qrow, zpart, g, chunks, 8 * (p.mx->nkb - 2), p.mxt->dr);
            HIP_TRY(ctx, hipGetLastError());
            hipLaunchKernelGGL(mx_quirk_cols, dim3((g.vpitch + 255) / 256, nf), dim3(256), 0, ctx->stream, vpart, zpart, qcol, g, rblocks, zblocks, p.mxt->dr, p.mxt->dc);
            HIP_TRY(ctx, hipGetLastError());
        }
        { TimedLaunch t(ctx, 1, nf);
          HIP_TRY(ctx, p.mx->col_u8(ctx->stream, ctx->work, d, p.mxt->frags_col, g, qcol, ctx->num_cus, qrow)); }
    }
    return BLUR_OK;
}

// both passes in one kernel on the matrix cores (fx_kernels.hpp): no intermediate in memory
// chsel != 0 (blur_ch_sigmas_batch_impl: one sigma per channel): only these channels, on the one-channel-per-workgroup kernel of
// the window class (Fw3Entry: whole-window strips)
// lay (with chsel only; null: packed frames): the caller's layout, source and destination already disjoint
// ft: the frame list of a launch over frames with their own sigmas (blur_ch_frame_sigmas_batch_impl; FwFrame), with chsel and a layout
static int run_fx_u8c3(blur_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int nframes, int rows, int cols, const Prepared& p, float* vdump = nullptr, FwChSel chsel = 0,
                       const ChLayout* lay = nullptr, const FwFrame* ft)
{
    const size_t px = static_cast<size_t>(rows) * cols;
    if (lay && !chsel) return fail(ctx, BLUR_ERR_INVALID, "run_fx_u8c3: a layout goes with a channel selection");
    if (ft && !lay) return fail(ctx, BLUR_ERR_INVALID, "run_fx_u8c3: a frame list goes with a layout");
    const FwPitch pt = lay ? fw_pitch_of(*lay) : fw_pitch_packed(rows, cols, 3, 1);
    // in place (the reference's own calling convention, Source.cpp:429,567): a strip reads its neighbours' columns and the rows
    // below while they are being written, so the frames are read from a copy in the workspace
    const uint8_t* lo = d_src < d_dst ? d_src : d_dst;
    const uint8_t* hi = d_src < d_dst ? d_dst : d_src;
    if (!lay && static_cast<size_t>(hi - lo) < px * 3 * nframes) {
        // (a large batch: in parts of at most 1 GiB, the cap of every engine's workspace -- frames are disjoint, so a part's result
        // never touches a later part's source)
        const size_t cap = std::max<size_t>(1, (static_cast<size_t>(1) << 30) / (px * 3));
        if (d_src == d_dst && static_cast<size_t>(nframes) > cap) {
            for (int f0 = 0; f0 < nframes; f0 += static_cast<int>(cap)) {
                const int nf = std::min<int>(static_cast<int>(cap), nframes - f0);
                if (int rc = run_fx_u8c3(ctx, d_src + static_cast<size_t>(f0) * px * 3, d_dst + static_cast<size_t>(f0) * px * 3, nf, rows, cols, p, vdump, chsel)) return rc;
            }
            return BLUR_OK;
        }
        if (int rc = ensure_work(ctx, px * 3 * nframes)) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(ctx->work, d_src, px * 3 * nframes, hipMemcpyDeviceToDevice, ctx->stream));
        d_src = reinterpret_cast<const uint8_t*>(ctx->work);
    }
    const int nkb = p.fx->nkb, pada = 8 * (nkb - 2);
    FxGeom g{ rows, cols, p.sz.pad, nframes, 0, (rows + 31) / 32, fx_right_strips(cols, pada), ctx->num_xcds };
    g.aligned = ((cols & 3) == 0 && (reinterpret_cast<uintptr_t>(d_src) & 3) == 0 && (reinterpret_cast<uintptr_t>(d_dst) & 3) == 0) ? 1 : 0;
    {   // the edge chunks' windows
        const int win = kFxChunk + 2 * pada, nstrips = fx_left_strips(pada) + g.nright;
        const size_t bytes = static_cast<size_t>(nframes) * nstrips * rows * win * 3 + 64;
        if (ctx->fx_strips_bytes < bytes) {
            if (ctx->fx_strips) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); HIP_TRY(ctx, hipFree(ctx->fx_strips)); ctx->fx_strips = nullptr; ctx->fx_strips_bytes = 0; }
            HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->fx_strips), bytes));
            ctx->fx_strips_bytes = bytes;
        }
    }
    // (the three-channel kernels read only the loads that touch a mirrored pixel from their strips: fx_strip_range)
    const int chunks_x = (cols + kFxChunk - 1) / kFxChunk, narrow =
#ifdef FX_FULL_STRIPS
        0;
#else
        p.fx->nkb <= 11 && !chsel ? 1 : 0;
#endif
    int strip_groups = (kFxChunk + 2 * pada) / 4;
    if (narrow) {
        const int gpr = strip_groups, per = (gpr + 7) / 8, nleft = fx_left_strips(pada);
        strip_groups = 0;
        for (int si = 0; si < nleft + g.nright; ++si) {
            int lo, hi;
            fx_strip_range(si < nleft ? si : chunks_x - g.nright + si - nleft, cols, pada, per, &lo, &hi);
            strip_groups = std::max(strip_groups, std::min(8 * hi, gpr) - 8 * lo);
        }
        if (strip_groups < 1) strip_groups = 1;
    }
    const int strip_blocks = (((rows + 3) / 4) * strip_groups + 255) / 256;
    const int n_strip = strip_blocks * (fx_left_strips(pada) + g.nright) * nframes;
    FxQuirk qk{};
    if (!p.mx_quirk) {
        TimedLaunch t(ctx, 1, nframes);
        if (ft)
            hipLaunchKernelGGL(fx_prepass_frames<1>, dim3(n_strip), dim3(256), 0, ctx->stream, d_src, nullptr, nullptr, nullptr, ctx->fx_strips, rows, cols, pada, 1, 1, 0,
                               chunks_x, g.nright, strip_blocks, kFxSumRows, narrow, pt.src_pitch, pt.src_frame, ft);
        else
            hipLaunchKernelGGL(fx_prepass<1>, dim3(n_strip), dim3(256), 0, ctx->stream, d_src, nullptr, nullptr, nullptr, ctx->fx_strips, rows, cols, p.sz.pad, pada, 1, 1, 0,
                               chunks_x, g.nright, strip_blocks, kFxSumRows, narrow, pt.src_pitch, pt.src_frame);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (p.mx_quirk) {
        // the quirk's partial sums (exact integers): srow_part [frame][batch][row][3], cpart [frame][band][3 cols], zpart (64-bit)
        // [frame][band][batch][3]; the fused kernel adds them up where it needs them (struct FxQuirk)
        const int gpt = fx_groups_per_thread(cols);
        const int groups = (cols + 3) / 4;
        const int band_rows = fx_band_rows(rows, cols, nframes, ctx->num_cus), nbands = (rows + band_rows - 1) / band_rows, nbatches = (groups + 256 * gpt - 1) / (256 * gpt);
        auto up4 = [](size_t v) { return (v + 3) & ~static_cast<size_t>(3); };
        const size_t n_srow = up4(static_cast<size_t>(nframes) * nbatches * rows * 3), n_cpart = up4(static_cast<size_t>(nframes) * nbands * 12 * groups);
        const size_t n_z = static_cast<size_t>(nframes) * nbands * nbatches * 3;
        const size_t bytes = (n_srow + n_cpart) * sizeof(int) + n_z * sizeof(long long) + 64;
        if (ctx->fx_sums_bytes < bytes) {
            if (ctx->fx_sums) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); HIP_TRY(ctx, hipFree(ctx->fx_sums)); ctx->fx_sums = nullptr; ctx->fx_sums_bytes = 0; }
            HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->fx_sums), bytes + bytes / 8));
            ctx->fx_sums_bytes = bytes + bytes / 8;
        }
        int* srow = ctx->fx_sums;
        int* cpart = srow + n_srow;                                                     // 16-byte aligned: int4 stores
        long long* zpart = reinterpret_cast<long long*>(cpart + n_cpart);
        { TimedLaunch t(ctx, 1, nframes);
          const int n_alt = nbands * nbatches * nframes;
          auto kern = gpt == 1 ? fx_prepass<1> : (gpt == 2 ? fx_prepass<2> : fx_prepass<4>);
          auto kern_frames = gpt == 1 ? fx_prepass_frames<1> : (gpt == 2 ? fx_prepass_frames<2> : fx_prepass_frames<4>);
          if (ft)
              hipLaunchKernelGGL(kern_frames, dim3(n_alt + n_strip), dim3(256), 0, ctx->stream, d_src, srow, cpart, zpart, ctx->fx_strips, rows, cols, pada, nbands, nbatches,
                                 n_alt, chunks_x, g.nright, strip_blocks, band_rows, narrow, pt.src_pitch, pt.src_frame, ft);
          else
              hipLaunchKernelGGL(kern, dim3(n_alt + n_strip), dim3(256), 0, ctx->stream, d_src, srow, cpart, zpart, ctx->fx_strips, rows, cols, p.sz.pad, pada, nbands,
                                 nbatches, n_alt, chunks_x, g.nright, strip_blocks, band_rows, narrow, pt.src_pitch, pt.src_frame);
          HIP_TRY(ctx, hipGetLastError()); }
        qk.srow_part = srow;
        qk.cpart = cpart;
        qk.zpart = zpart;
        qk.taps = p.mxt->taps_row;
        qk.nbatches = nbatches;
        qk.nbands = nbands;
        qk.cpitch = 12 * groups;
        qk.dr = p.mxt->dr;
        qk.dc = p.mxt->dc;
    }
    // diagnostic (timing-only -DFX_STAMPS builds of the kernel write here; see tools/fx_variants.sh): cycles per phase kind
    unsigned long long* stamps = nullptr;
    if (!p.mx_quirk && !vdump && std::getenv("BLUR_FX_STAMPS")) {
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&stamps), 64));
        HIP_TRY(ctx, hipMemset(stamps, 0, 64));
    }
    if (chsel) {
        const Fw3Entry* fe3 = find_entry<Fw3Entry>(nkb);
        if (!fe3 || vdump || stamps) return fail(ctx, BLUR_ERR_UNSUPPORTED, "fused kernel for a subset of three channels: no kernel instantiated for this pad");
        TimedLaunch t(ctx, 0, nframes);
        HIP_TRY(ctx, fe3->blur_u8(ctx->stream, d_src, d_dst, p.mxt->frags_row, g, ctx->num_cus, p.mx_quirk ? &qk : nullptr, ctx->fx_strips, chsel, pt, ft));
        return BLUR_OK;
    }
    { TimedLaunch t(ctx, 0, nframes);
      HIP_TRY(ctx, p.fx->blur_u8(ctx->stream, d_src, d_dst, p.mxt->frags_row, g, ctx->num_cus, p.mx_quirk ? &qk : nullptr, ctx->fx_strips, vdump, stamps)); }
    if (stamps) {
        unsigned long long h[8];
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipMemcpy(h, stamps, 64, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipFree(stamps));
        if (h[7]) {
            std::fprintf(stderr, "fx stamps: steps %llu, cycles per step: A0 %.0f B0 %.0f A1 %.0f B1 %.0f A2 %.0f B2 %.0f, whole task %.0f per step\n", h[7], h[0] / double(h[7]),
                         h[1] / double(h[7]), h[2] / double(h[7]), h[3] / double(h[7]), h[4] / double(h[7]), h[5] / double(h[7]), h[6] / double(h[7]));
        }
    }
    return BLUR_OK;
}

static bool bands_overlap(const uint8_t* lo, const uint8_t* hi, size_t bytes) { return static_cast<size_t>(hi - lo) < bytes; }

// Tiled wave-resident path (prepare(): plan_tiled): frame by frame, the quirk's sums (fx_prepass) and terms (tl_terms_kernel), then
// per band of rows the column kernel and per tile of columns the row kernel.  Intermediate: one band at a time in the workspace.
static int run_wr_tiled(blur_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int nframes, int rows, int cols, const Prepared& p)
{
    const size_t px = static_cast<size_t>(rows) * cols, fb = px * 3;
    const int pad = p.sz.pad;
    // (the pre-pass with one group of 4 pixels per thread: the term kernel adds up any number of batch parts, unlike the fused kernel)
    const int groups = (cols + 3) / 4, gpt = 1;
    if (p.tl_quirk && cols < 4) return fail(ctx, BLUR_ERR_UNSUPPORTED, "tiled wave-resident path: image narrower than 4 pixels (the quirk's pre-pass)");
    const int pitch = (cols + 7) & ~7;
    int *srow = nullptr, *cpart = nullptr;
    long long* zpart = nullptr;
    float *e = nullptr, *h = nullptr;
    int band_rows = 0, nbands = 0, nbatches = 0;
    if (p.tl_quirk) {
        // bands as tall as still give four workgroups per CU: the term kernel adds up the bands' parts per column
        band_rows = static_cast<long long>(rows) * cols < 4000000ll ? 16 : kFxSumRows;
        while (band_rows < 256 && static_cast<long long>((groups + 255) / 256) * ((rows + 2 * band_rows - 1) / (2 * band_rows)) >= 4ll * ctx->num_cus) band_rows *= 2;
        nbands = (rows + band_rows - 1) / band_rows;
        nbatches = (groups + 256 * gpt - 1) / (256 * gpt);
        auto up4 = [](size_t v) { return (v + 3) & ~static_cast<size_t>(3); };
        const size_t n_srow = up4(static_cast<size_t>(nbatches) * rows * 3), n_cpart = up4(static_cast<size_t>(nbands) * 12 * groups);
        const size_t n_z = static_cast<size_t>(nbands) * nbatches * 3;
        const size_t bytes = (n_srow + n_cpart) * sizeof(int) + n_z * sizeof(long long) + 64;
        if (ctx->tl_sums_bytes < bytes) {
            if (ctx->tl_sums) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); HIP_TRY(ctx, hipFree(ctx->tl_sums)); ctx->tl_sums = nullptr; ctx->tl_sums_bytes = 0; }
            HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->tl_sums), bytes));
            ctx->tl_sums_bytes = bytes;
        }
        srow = ctx->tl_sums;
        cpart = srow + n_srow;
        zpart = reinterpret_cast<long long*>(cpart + n_cpart);
        const size_t tbytes = (static_cast<size_t>(3) * pitch + static_cast<size_t>(3) * rows) * sizeof(float) + 64;
        if (ctx->tl_terms_bytes < tbytes) {
            if (ctx->tl_terms) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); HIP_TRY(ctx, hipFree(ctx->tl_terms)); ctx->tl_terms = nullptr; ctx->tl_terms_bytes = 0; }
            HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->tl_terms), tbytes));
            ctx->tl_terms_bytes = tbytes;
        }
        e = ctx->tl_terms;
        h = e + static_cast<size_t>(3) * pitch;
    }
    for (int f = 0; f < nframes; ++f) {
        const uint8_t* src = d_src + static_cast<size_t>(f) * fb;
        uint8_t* dst = d_dst + static_cast<size_t>(f) * fb;
        // in place (or overlapping): a band reads rows the band before it has already written
        const uint8_t* lo = src < dst ? src : dst;
        const uint8_t* hi = src < dst ? dst : src;
        if (bands_overlap(lo, hi, fb) && (p.bands.size() > 1 || p.tiles.size() > 1 || src == dst)) {
            if (ctx->tl_copy_bytes < fb) {
                if (ctx->tl_copy) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); HIP_TRY(ctx, hipFree(ctx->tl_copy)); ctx->tl_copy = nullptr; ctx->tl_copy_bytes = 0; }
                HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->tl_copy), fb));
                ctx->tl_copy_bytes = fb;
            }
            HIP_TRY(ctx, hipMemcpyAsync(ctx->tl_copy, src, fb, hipMemcpyDeviceToDevice, ctx->stream));
            src = ctx->tl_copy;
        }
        if (p.tl_quirk) {
            TimedLaunch t(ctx, 1, 1);
            const int n_alt = nbands * nbatches;
            hipLaunchKernelGGL(fx_prepass<1>, dim3(n_alt), dim3(256), 0, ctx->stream, src, srow, cpart, zpart, nullptr, rows, cols, pad, 0, nbands, nbatches, n_alt, 1, 0, 1, band_rows, 0,
                               static_cast<uint32_t>(cols) * 3u, static_cast<size_t>(rows) * cols * 3);
            HIP_TRY(ctx, hipGetLastError());
            const int ne = (pitch + 255) / 256, nh = (rows + 255) / 256;
            const size_t lds = (static_cast<size_t>(3) * (256 + 2 * pad) + (2 * pad + 1) + 3 + 3 * 256) * sizeof(double);
            if (lds > 64 * 1024) HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(tl_terms_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
            hipLaunchKernelGGL(tl_terms_kernel, dim3(ne + nh, 1), dim3(256), lds, ctx->stream, srow, cpart, zpart, p.tl_taps, e, h, rows, cols, pad, pitch, nbatches, nbands,
                               12 * groups, p.tl_dr, p.tl_dc, ne);
            HIP_TRY(ctx, hipGetLastError());
        }
        // consecutive middle bands of one shape, a constant (even) number of rows apart, are the "frames" of ONE launch per kernel
        auto group_of = [&](size_t bi, int& step) -> int {
            const Prepared::Span& b = p.bands[bi];
            const int brows = b.in1 - b.in0;
            int nb = 1;
            step = 0;
            if (b.padmode == 0) {
                while (bi + nb < p.bands.size()) {
                    const Prepared::Span& c = p.bands[bi + nb];
                    const int st = c.in0 - p.bands[bi + nb - 1].in0;
                    if (c.padmode != 0 || c.in1 - c.in0 != brows || c.v0 - c.in0 != b.v0 - b.in0 || c.v1 - c.v0 != b.v1 - b.v0 || (st & 1) || (nb > 1 && st != step)) break;
                    step = st;
                    ++nb;
                }
            }
            if (nb > 1 && wr_frame_floats(brows, cols, b.padmode, p.tl_col->g) * nb * sizeof(float) > (static_cast<size_t>(3) << 30)) { nb = 1; step = 0; }
            return nb;
        };
        {
            size_t need = 0;
            for (size_t bi = 0; bi < p.bands.size();) {
                int step;
                const int nb = group_of(bi, step);
                need = std::max(need, wr_frame_floats(p.bands[bi].in1 - p.bands[bi].in0, cols, p.bands[bi].padmode, p.tl_col->g) * nb * sizeof(float));
                bi += nb;
            }
            if (int rc = ensure_work(ctx, need)) return rc;
        }
        float* const inter = reinterpret_cast<float*>(ctx->work);
        for (size_t bi = 0; bi < p.bands.size();) {
            const Prepared::Span& b = p.bands[bi];
            const int brows = b.in1 - b.in0;
            int step = 0;
            const int nb = group_of(bi, step);
            const int vr_max = bi + nb < p.bands.size() ? p.bands[bi + nb].v0 : rows;       // rows from here on are the next band's
            WrColTerm term;
            if (p.tl_quirk) {
                term.e = e;
                term.pitch = pitch;
                term.sign = ((b.in0 + pad - b.padmode) & 1) ? -1.f : 1.f;       // (-1)^(image row + pad) of slot 0: slot = (band row + padmode) & 1
            }
            term.band_step = nb > 1 ? step : 0;
            { TimedLaunch t(ctx, 1, 1);
              HIP_TRY(ctx, p.tl_col->col_u8(ctx->stream, src + static_cast<size_t>(b.in0) * cols * 3, inter, brows, cols, b.padmode, nb, ctx->num_cus, ctx->d_w256, p.tl_tw0_col,
                                            p.tl_m_col, term)); }
            const int g = p.tl_col->g, npairs = wr_npairs(brows, b.padmode), strips_full = (cols + g - 1) / g;
            for (size_t ti = 0; ti < p.tiles.size(); ++ti) {
                const Prepared::Span& t = p.tiles[ti];
                WrRowTile tile;
                tile.h = p.tl_quirk ? h : nullptr;
                tile.rows_full = rows;
                tile.row_base = b.in0;
                tile.vr0 = b.v0;
                tile.vr1 = b.v1;
                tile.ypar = b.padmode & 1;
                tile.dst_pitch = cols * 3;
                tile.dst_x0 = t.in0;
                tile.vc0 = t.v0 - t.in0;
                tile.vc1 = t.v1 - t.in0;
                tile.xpar = (t.in0 + pad) & 1;                                   // (-1)^(image column + pad): the call's column 0 is image column in0
                tile.plane_strips = strips_full;
                tile.g = g;
                tile.t0 = (b.v0 - b.in0 + tile.ypar) >> 1;                        // the pairs that hold a kept row
                tile.tn = ((b.v1 - 1 - b.in0 + tile.ypar) >> 1) - tile.t0 + 1;
                tile.band_step = nb > 1 ? step : 0;
                tile.vr_max = vr_max;
                if (nb == 1 && tile.vr1 > vr_max) tile.vr1 = vr_max;
                TimedLaunch tl(ctx, 0, 1);
                HIP_TRY(ctx, p.tl_row[ti]->row_u8(ctx->stream, inter + static_cast<size_t>(t.in0 / g) * npairs * (2 * g), dst, brows, t.in1 - t.in0, t.padmode, nb, ctx->num_cus,
                                                  ctx->d_w256, p.tl_tw0_row[ti], p.tl_m_row[ti], tile));
            }
            bi += nb;
        }
    }
    return BLUR_OK;
}

static int blur_u8c3_batch_impl(blur_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int nframes,
                                int rows, int cols, double sigma, const blur_opts* opts, const CustomKernel* ck)
{
    if (!ctx) return BLUR_ERR_INVALID;
    if (!d_src || !d_dst || nframes < 0) return fail(ctx, BLUR_ERR_INVALID, "null frame pointer or negative frame count");
    Prepared p;
    const bool aligned = ((reinterpret_cast<uintptr_t>(d_src) | reinterpret_cast<uintptr_t>(d_dst)) & 3) == 0;
    if (int rc = prepare(ctx, rows, cols, sigma, opts, p, true, ck, true, aligned)) return rc;
    const size_t px = static_cast<size_t>(rows) * cols;
    // Frames per launch pair.  Measured on MI355X (4K, sigma 20): 1 frame 0.170 ms/frame, 2: 0.148, 4: 0.143,
    // 8: 0.140 -- the kernels are latency bound, not HBM bound, so filling every CU evenly and amortising
    // the per-workgroup table loads is worth more than keeping the float intermediate inside the 256 MiB
    // Infinity Cache.  The workspace is capped at 1 GiB.
    if (p.fx) {
        if (nframes == 0) return BLUR_OK;
        ctx->last_family = 6;
        return run_fx_u8c3(ctx, d_src, d_dst, nframes, rows, cols, p);
    }
    if (p.tiled) {
        if (nframes == 0) return BLUR_OK;
        ctx->last_family = 7;
        return run_wr_tiled(ctx, d_src, d_dst, nframes, rows, cols, p);
    }
    int chunk = opts && opts->frames_per_launch > 0 ? opts->frames_per_launch : static_cast<int>((1024u << 20) / (p.frame_elems * sizeof(float)));
    if (chunk < 1) chunk = 1;
    if (chunk > nframes) chunk = nframes;
    if (nframes == 0) return BLUR_OK;
    if (int rc = ensure_work(ctx, p.frame_elems * sizeof(float) * chunk)) return rc;
    ctx->last_family = p.mx ? 4 : p.wr_col ? 2 : ((p.row->fast && p.col->fast) ? 1 : 0);
    if (p.mx) return run_mx_u8c3(ctx, d_src, d_dst, nframes, rows, cols, chunk, p);
    for (int f = 0; f < nframes; f += chunk) {
        const int nf = nframes - f < chunk ? nframes - f : chunk;
        const uint8_t* s = d_src + static_cast<size_t>(f) * px * 3;
        uint8_t* d = d_dst + static_cast<size_t>(f) * px * 3;
        if (p.wr_col) {
            // columns first, then rows (wr_kernels.hpp); timing slot 1 = column kernel, 0 = row kernel as elsewhere
            { TimedLaunch t(ctx, 1, nf);
              HIP_TRY(ctx, p.wr_col->col_u8(ctx->stream, s, ctx->work, rows, cols, p.sz.pad, nf, ctx->num_cus, ctx->d_w256, p.wr_tw0_col, p.wr_m_col, WrColTerm{})); }
            { TimedLaunch t(ctx, 0, nf);
              WrRowTile whole;
              whole.g = p.wr_col->g;
              HIP_TRY(ctx, p.wr_row->row_u8(ctx->stream, ctx->work, d, rows, cols, p.sz.pad, nf, ctx->num_cus, ctx->d_w256, p.wr_tw0_row, p.wr_m_row, whole)); }
            continue;
        }
        if (int rc = run_rowpass_u8c3(ctx, s, ctx->work, rows, cols, nf, p, p.tile_w)) return rc;
        if (int rc = run_colpass_u8c3(ctx, ctx->work, d, rows, cols, nf, p)) return rc;
    }
    return BLUR_OK;
}

int blur_gaussian_u8c3_batch_dev(blur_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int nframes,
                                 int rows, int cols, double sigma, const blur_opts* opts)
{
    return blur_u8c3_batch_impl(ctx, d_src, d_dst, nframes, rows, cols, sigma, opts, nullptr);
}

int blur_separable_u8c3_dev(blur_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int rows, int cols,
                            const float* taps, int ksize, int pad, const blur_opts* opts)
{
    if (!ctx) return BLUR_ERR_INVALID;
    if (!taps || ksize <= 0 || (ksize & 1) == 0 || pad < 0) return fail(ctx, BLUR_ERR_INVALID, "separable kernel: odd tap count and pad >= 0 required");
    for (int t = 0; t < ksize / 2; ++t)
        if (taps[t] != taps[ksize - 1 - t]) return fail(ctx, BLUR_ERR_UNSUPPORTED, "separable kernel must be symmetric (real spectrum, Source.cpp:419)");
    CustomKernel ck;
    ck.taps = taps; ck.ksize = ksize; ck.pad = pad;
    return blur_u8c3_batch_impl(ctx, d_src, d_dst, 1, rows, cols, 0., opts, &ck);
}

int blur_boxfft_sizing(int rows, int cols, double nsmooth, int out[4])
{
    if (!out || rows <= 1 || cols <= 1 || !(nsmooth >= 1)) return BLUR_ERR_INVALID;
    int klen, pad;
    boxfft_sizing(rows, cols, nsmooth, klen, pad);
    const int n0 = rows + 2 * pad, n1 = cols + 2 * pad;
    out[0] = klen; out[1] = pad;
    out[2] = is_valid_size(n0) ? n0 : nearest_transform_size(n0);
    out[3] = is_valid_size(n1) ? n1 : nearest_transform_size(n1);
    return BLUR_OK;
}

int blur_box_kernel(float* kernel, int klen, int fft_length)
{
    if (!kernel || klen <= 0 || fft_length < 2 * klen + 2) return BLUR_ERR_INVALID;
    std::fill(kernel, kernel + fft_length, 0.f);
    box_kernel_1d(kernel, klen, fft_length);
    return BLUR_OK;
}

int blur_boxfft_u8c3_dev(blur_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int rows, int cols, double nsmooth, const blur_opts* opts)
{
    if (!ctx) return BLUR_ERR_INVALID;
    if (rows <= 1 || cols <= 1 || !(nsmooth >= 1)) return fail(ctx, BLUR_ERR_INVALID, "boxfft: rows, cols > 1 and nsmooth >= 1 required");
    CustomKernel ck;
    boxfft_sizing(rows, cols, nsmooth, ck.box_klen, ck.pad);
    if (ck.box_klen < 1) return fail(ctx, BLUR_ERR_INVALID, "boxfft: empty kernel");
    return blur_u8c3_batch_impl(ctx, d_src, d_dst, 1, rows, cols, 0., opts, &ck);
}

int blur_gaussian_u8c3_dev(blur_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int rows, int cols, double sigma, const blur_opts* opts)
{
    return blur_gaussian_u8c3_batch_dev(ctx, d_src, d_dst, 1, rows, cols, sigma, opts);
}

int blur_gaussian_f32c1_dev(blur_ctx* ctx, const float* d_src, float* d_dst, int rows, int cols, double sigma, const blur_opts* opts)
{
    if (!ctx) return BLUR_ERR_INVALID;
    if (!d_src || !d_dst) return fail(ctx, BLUR_ERR_INVALID, "null plane pointer");
    Prepared p;
    if (int rc = prepare(ctx, rows, cols, sigma, opts, p, false)) return rc;
    const size_t px = static_cast<size_t>(rows) * cols;
    if (int rc = ensure_work(ctx, px * sizeof(float))) return rc;
    if (int rc = launch_rowpass<float, 1>(ctx, d_src, ctx->work, rows, cols, p.sz.pad, *p.row, p.m_row)) return rc;
    return launch_colpass<float, 1>(ctx, ctx->work, d_dst, rows, cols, p.sz.pad, *p.col, p.m_col, p.col_group);
}

int blur_rowpass_u8c3_dev(blur_ctx* ctx, const uint8_t* d_src, float* d_planes, int rows, int cols, double sigma, const blur_opts* opts)
{
    if (!ctx) return BLUR_ERR_INVALID;
    if (!d_src || !d_planes) return fail(ctx, BLUR_ERR_INVALID, "null pointer");
    Prepared p;
    if (opts && opts->engine == BLUR_ENGINE_FUSED) {
        // the fused kernel's row-pass planes (tests): the whole blur runs, its bytes go to the workspace and are dropped
        const bool aligned = (reinterpret_cast<uintptr_t>(d_src) & 3) == 0;
        if (int rc = prepare(ctx, rows, cols, sigma, opts, p, true, nullptr, true, aligned)) return rc;
        if (!p.fx || p.fx->nkb > 11 || (cols & 3) != 0)
            return fail(ctx, BLUR_ERR_UNSUPPORTED, "row-pass planes of the fused engine: a test instantiation for pad <= 72 and widths that are multiples of 4");
        const size_t bytes = static_cast<size_t>(rows) * cols * 3;
        if (int rc = ensure_work(ctx, 2 * bytes + 64)) return rc;
        return run_fx_u8c3(ctx, d_src, reinterpret_cast<uint8_t*>(ctx->work) + ((bytes + 63) & ~static_cast<size_t>(63)), 1, rows, cols, p, d_planes);
    }
    if (int rc = prepare(ctx, rows, cols, sigma, opts, p, true, nullptr, false)) return rc;   // the rows-first kernels: row-major planes
    return run_rowpass_u8c3(ctx, d_src, d_planes, rows, cols, 1, p, -1);   // always row-major for the caller
}

int blur_gaussian_u8c3_host(blur_ctx* ctx, const uint8_t* src, uint8_t* dst, int rows, int cols, double sigma, const blur_opts* opts)
{
    if (!ctx) return BLUR_ERR_INVALID;
    if (!src || !dst || rows <= 0 || cols <= 0) return fail(ctx, BLUR_ERR_INVALID, "null image or non-positive size");
    return blur_through_host_stage(ctx, src, dst, static_cast<size_t>(rows) * cols * 3, [&](char* s, char* d) {
        return blur_gaussian_u8c3_dev(ctx, reinterpret_cast<const uint8_t*>(s), reinterpret_cast<uint8_t*>(d), rows, cols, sigma, opts);
    });
}

int blur_gaussian_u8c3_host_batch(blur_ctx* ctx, const uint8_t* src, uint8_t* dst, int nframes, int rows, int cols, double sigma,
                                  const blur_opts* opts)
{
    if (!ctx) return BLUR_ERR_INVALID;
    if (!src || !dst || nframes < 0 || rows <= 0 || cols <= 0) return fail(ctx, BLUR_ERR_INVALID, "null image, negative count or non-positive size");
    if (nframes == 0) return BLUR_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t fb = static_cast<size_t>(rows) * cols * 3;
    HostPipe& p = ctx->pipe;
    constexpr int S = HostPipe::S;
    if (!p.ready) {
        // non-blocking: the context's stream may be the null stream, which would otherwise serialise with these
        HIP_TRY(ctx, hipStreamCreateWithFlags(&p.h2d, hipStreamNonBlocking));
        HIP_TRY(ctx, hipStreamCreateWithFlags(&p.d2h, hipStreamNonBlocking));
        for (int k = 0; k < S; ++k) {
            HIP_TRY(ctx, hipEventCreateWithFlags(&p.in_done[k], hipEventDisableTiming));
            HIP_TRY(ctx, hipEventCreateWithFlags(&p.comp_done[k], hipEventDisableTiming));
            HIP_TRY(ctx, hipEventCreateWithFlags(&p.out_done[k], hipEventDisableTiming));
        }
        p.ready = true;
    }
    if (p.bytes < fb) {
        for (int k = 0; k < S; ++k) {
            if (p.buf[k]) { HIP_TRY(ctx, hipFree(p.buf[k])); p.buf[k] = nullptr; }
        }
        p.bytes = 0;
        for (int k = 0; k < S; ++k) HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&p.buf[k]), 2 * ((fb + 255) & ~static_cast<size_t>(255))));   // input | output
        p.bytes = fb;
    }
    int rc = BLUR_OK;
    hipError_t e = hipSuccess;
    auto step = [&](hipError_t r) { if (e == hipSuccess) e = r; return e == hipSuccess; };
    for (int i = 0; i < nframes && e == hipSuccess && rc == BLUR_OK; ++i) {
        const int k = i % S;
        if (i >= S && !step(hipStreamWaitEvent(p.h2d, p.out_done[k], 0))) break;   // the slot's previous frame has left
        if (!step(hipMemcpyAsync(p.buf[k], src + static_cast<size_t>(i) * fb, fb, hipMemcpyHostToDevice, p.h2d))) break;
        if (!step(hipEventRecord(p.in_done[k], p.h2d))) break;
        if (!step(hipStreamWaitEvent(ctx->stream, p.in_done[k], 0))) break;
        uint8_t* const obuf = p.buf[k] + ((fb + 255) & ~static_cast<size_t>(255));           // out of place: no copy into the workspace
        rc = blur_gaussian_u8c3_dev(ctx, p.buf[k], obuf, rows, cols, sigma, opts);
        if (rc != BLUR_OK) break;
        if (!step(hipEventRecord(p.comp_done[k], ctx->stream))) break;
        if (!step(hipStreamWaitEvent(p.d2h, p.comp_done[k], 0))) break;
        if (!step(hipMemcpyAsync(dst + static_cast<size_t>(i) * fb, obuf, fb, hipMemcpyDeviceToHost, p.d2h))) break;
        if (!step(hipEventRecord(p.out_done[k], p.d2h))) break;
    }
    // drain everything that was queued, whatever happened above
    const std::string first_err = ctx->err;
    const hipError_t s0 = hipStreamSynchronize(p.h2d), s1 = hipStreamSynchronize(ctx->stream), s2 = hipStreamSynchronize(p.d2h);
    if (rc != BLUR_OK) { ctx->err = first_err; return rc; }
    for (hipError_t r : { s0, s1, s2 }) step(r);
    if (e != hipSuccess) { ctx->err = std::string("host batch blur: ") + hipGetErrorString(e); return BLUR_ERR_HIP; }
    return BLUR_OK;
}

int blur_gaussian_u8c3_host_pitched(blur_ctx* ctx, const uint8_t* src, size_t src_pitch, uint8_t* dst, size_t dst_pitch,
                                    int rows, int cols, double sigma, const blur_opts* opts)
{
    if (!ctx) return BLUR_ERR_INVALID;
    const size_t row_bytes = static_cast<size_t>(cols) * 3;
    if (!src || !dst || rows <= 0 || cols <= 0 || src_pitch < row_bytes || dst_pitch < row_bytes)
        return fail(ctx, BLUR_ERR_INVALID, "null image, non-positive size or pitch shorter than a row");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    void* dv = nullptr;
    const size_t half = (row_bytes * rows + 255) & ~static_cast<size_t>(255);
    if (int rc0 = ensure_host_stage(ctx, 2 * half, &dv)) return rc0;
    uint8_t* d = static_cast<uint8_t*>(dv);
    int rc = BLUR_OK;
    // the rows are packed on the way in and unpacked on the way out (cv::Mat::step of a ROI or padded Mat); out of place on the device
    hipError_t e = hipMemcpy2DAsync(d, row_bytes, src, src_pitch, row_bytes, rows, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) rc = blur_gaussian_u8c3_dev(ctx, d, d + half, rows, cols, sigma, opts);
    if (e == hipSuccess && rc == BLUR_OK) e = hipMemcpy2DAsync(dst, dst_pitch, d + half, row_bytes, row_bytes, rows, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { ctx->err = std::string("host blur (pitched): ") + hipGetErrorString(e); return BLUR_ERR_HIP; }
    return rc;
}

int blur_gaussian_f32c1_host(blur_ctx* ctx, const float* src, float* dst, int rows, int cols, double sigma, const blur_opts* opts)
{
    if (!ctx) return BLUR_ERR_INVALID;
    if (!src || !dst || rows <= 0 || cols <= 0) return fail(ctx, BLUR_ERR_INVALID, "null plane or non-positive size");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t bytes = static_cast<size_t>(rows) * cols * sizeof(float);
    void* dv = nullptr;
    if (int rc0 = ensure_host_stage(ctx, 2 * bytes, &dv)) return rc0;
    float* d = static_cast<float*>(dv);
    int rc = BLUR_OK;
    hipError_t e = hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) rc = blur_gaussian_f32c1_dev(ctx, d, d + static_cast<size_t>(rows) * cols, rows, cols, sigma, opts);
    if (e == hipSuccess && rc == BLUR_OK) e = hipMemcpyAsync(dst, d + static_cast<size_t>(rows) * cols, bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { ctx->err = std::string("host blur: ") + hipGetErrorString(e); return BLUR_ERR_HIP; }
    return rc;
}

// ---- whole-image 2D transform path (pocketfft_2D, Source.cpp:143-277) -----------------------------------------
int blur_pocketfft2d_sizing(int rows, int cols, double sigma, int out[8])
{
    if (rows <= 0 || cols <= 0 || !(sigma > 0) || !out) return BLUR_ERR_INVALID;
    const Sizing2D s = pocketfft2d_sizing(rows, cols, sigma);
    const int v[8] = { s.kSize, s.pad, s.s0, s.s1, s.top, s.bottom, s.left, s.right };
    std::memcpy(out, v, sizeof v);
    return BLUR_OK;
}

int blur_pocketfft2d_u8c3_dev(blur_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int rows, int cols, double sigma, int dft_image, float* d_planes)
{
    if (!ctx) return BLUR_ERR_INVALID;
    if (!d_src || !d_dst) return fail(ctx, BLUR_ERR_INVALID, "null image pointer");
    if (rows <= 0 || cols <= 0 || !(sigma > 0)) return fail(ctx, BLUR_ERR_INVALID, "rows, cols and sigma must be positive");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const Sizing2D sz = pocketfft2d_sizing(rows, cols, sigma);
    // Reflect_101 clamps a border to dim - 1 (Utils.hpp:217-220) while pocketfft_2D keeps its own sizes[]: past that
    // point the reference's buffers no longer agree with each other
    if (std::max(sz.top, sz.bottom) > rows - 1 || std::max(sz.left, sz.right) > cols - 1)
        return fail(ctx, BLUR_ERR_UNSUPPORTED, "2D path: border > dim - 1 (Reflect_101 would clamp it, Utils.hpp:217-220)");
    if (static_cast<long long>(sz.s0) * sz.s1 > (1ll << 31) - 1) return fail(ctx, BLUR_ERR_UNSUPPORTED, "2D path: ndata exceeds int (Source.cpp:230)");
    DevicePlan *prow = nullptr, *pcol = nullptr;
    if (int rc = get_plan(ctx, sz.s1, false, false, &prow)) return rc;
    if (int rc = get_plan(ctx, sz.s0, false, true, &pcol)) return rc;
    const size_t row_lds = row_lds_bytes(sz.s1);
    if (row_lds > kLdsLimit) return fail(ctx, BLUR_ERR_UNSUPPORTED, "2D path: row FFT length exceeds LDS capacity");
    float *mrow = nullptr, *mcol = nullptr;
    const int *pofy = nullptr, *pofx = nullptr;
    if (dft_image) {
        if (int rc = get_pos_of_freq(ctx, pcol, &pofy)) return rc;
        if (int rc = get_pos_of_freq(ctx, prow, &pofx)) return rc;
    } else {
        // Re(kerf_1D_row[j]) * Re(kerf_1D_col[i]) * (1 / ndata) (:255-263) as two tables in position order, each
        // carrying the 1/n of its own axis; the mirrored upper half of kerf_1D_col (:207) is min(f, n - f) of the table
        if (int rc = get_spectrum(ctx, *prow, sigma, sz.kSize, false, &mrow)) return rc;
        if (int rc = get_spectrum(ctx, *pcol, sigma, sz.kSize, false, &mcol)) return rc;
    }
    if (int rc = ensure_work(ctx, static_cast<size_t>(sz.s0) * sz.s1 * sizeof(float2))) return rc;
    float2* z = reinterpret_cast<float2*>(ctx->work);
    if (int rc = set_lds(ctx, img2d_rows_fwd_kernel, row_lds)) return rc;
    if (int rc = set_lds(ctx, img2d_rows_inv_kernel, row_lds)) return rc;
    const Img2dGeom g{ rows, cols, sz.s0, sz.s1, sz.top, sz.left };
    ctx->last_family = 3;
    const int pairs[2][2] = { { 0, 1 }, { 2, -1 } };
    for (const auto& pr : pairs) {
        hipLaunchKernelGGL(img2d_rows_fwd_kernel, dim3(sz.s0), dim3(kThreads), row_lds, ctx->stream, d_src, z, g, pr[0], pr[1], prow->dev, prow->d_tw);
        HIP_TRY(ctx, hipGetLastError());
        if (dft_image) {
            if (int rc = launch_img2d_cols<false>(ctx, z, sz.s0, sz.s1, *pcol, nullptr, nullptr)) return rc;
            const size_t px = static_cast<size_t>(rows) * cols;
            const int grid = static_cast<int>(std::min<size_t>((px + 255) / 256, static_cast<size_t>(ctx->num_cus) * 16));
            hipLaunchKernelGGL(img2d_logspec_kernel, dim3(grid), dim3(256), 0, ctx->stream, z, d_dst, d_planes, g, pr[0], pr[1], pofy, pofx);
        } else {
            if (int rc = launch_img2d_cols<true>(ctx, z, sz.s0, sz.s1, *pcol, mcol, mrow)) return rc;
            hipLaunchKernelGGL(img2d_rows_inv_kernel, dim3(rows), dim3(kThreads), row_lds, ctx->stream, z, d_dst, d_planes, g, pr[0], pr[1], prow->dev, prow->d_tw);
        }
        HIP_TRY(ctx, hipGetLastError());
    }
    return BLUR_OK;
}

int blur_pocketfft2d_u8c3_host(blur_ctx* ctx, const uint8_t* src, uint8_t* dst, int rows, int cols, double sigma, int dft_image)
{
    if (!ctx) return BLUR_ERR_INVALID;
    if (!src || !dst || rows <= 0 || cols <= 0) return fail(ctx, BLUR_ERR_INVALID, "null image or non-positive size");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t bytes = static_cast<size_t>(rows) * cols * 3;
    void* dv = nullptr;
    if (int rc0 = ensure_host_stage(ctx, bytes, &dv)) return rc0;
    uint8_t* d = static_cast<uint8_t*>(dv);
    int rc = BLUR_OK;
    hipError_t e = hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, ctx->stream);
    // in place on the device, like the reference (image.data is source and destination): the pass over planes 0 and 1
    // writes only their bytes, and the later pass over plane 2 reads only plane 2
    if (e == hipSuccess) rc = blur_pocketfft2d_u8c3_dev(ctx, d, d, rows, cols, sigma, dft_image, nullptr);
    if (e == hipSuccess && rc == BLUR_OK) e = hipMemcpyAsync(dst, d, bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { ctx->err = std::string("host 2D path: ") + hipGetErrorString(e); return BLUR_ERR_HIP; }
    return rc;
}

int blur_reflect101_u8_dev(blur_ctx* ctx, const uint8_t* d_in, uint8_t* d_out, int rows, int cols, int channels, int top, int bottom, int left, int right,
                           int out_size[2])
{
    if (!ctx) return BLUR_ERR_INVALID;
    if (rows <= 0 || cols <= 0 || channels <= 0 || top < 0 || bottom < 0 || left < 0 || right < 0)
        return fail(ctx, BLUR_ERR_INVALID, "Reflect_101: bad arguments");
    // the reference's only difference to cv::copyMakeBorder: borders are clamped to dim - 1 (Utils.hpp:217-220)
    top = std::min(top, rows - 1);
    bottom = std::min(bottom, rows - 1);
    left = std::min(left, cols - 1);
    right = std::min(right, cols - 1);
    const int orows = rows + top + bottom, ocols = cols + left + right;
    if (out_size) { out_size[0] = orows; out_size[1] = ocols; }
    if (!d_out) return BLUR_OK;                                  // size query
    if (!d_in || d_in == d_out) return fail(ctx, BLUR_ERR_INVALID, "Reflect_101: null input or in place");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t px = static_cast<size_t>(orows) * ocols;
    const int grid = static_cast<int>(std::min<size_t>((px + 255) / 256, static_cast<size_t>(ctx->num_cus) * 16));
    hipLaunchKernelGGL(reflect101_u8_kernel, dim3(grid), dim3(256), 0, ctx->stream, d_in, d_out, rows, cols, channels, top, left, orows, ocols);
    HIP_TRY(ctx, hipGetLastError());
    return BLUR_OK;
}

int blur_flip_block_f32_dev(blur_ctx* ctx, const float* d_in, float* d_out, int w, int h)
{
    if (!ctx) return BLUR_ERR_INVALID;
    if (!d_in || !d_out || w <= 0 || h <= 0 || d_in == d_out) return fail(ctx, BLUR_ERR_INVALID, "flip_block: bad arguments (out of place only)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int tiles = ((w + 63) / 64) * ((h + 63) / 64);
    hipLaunchKernelGGL(flip_block_kernel, dim3(tiles), dim3(256), 0, ctx->stream, d_in, d_out, w, h);
    HIP_TRY(ctx, hipGetLastError());
    return BLUR_OK;
}

int blur_deinterleave_bgr_u8_f32_dev(blur_ctx* ctx, const uint8_t* d_in, float* d_planes, uint32_t total)
{
    if (!ctx) return BLUR_ERR_INVALID;
    if (!d_in || !d_planes) return fail(ctx, BLUR_ERR_INVALID, "null pointer");
    if (!total) return BLUR_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const unsigned grid = std::min<uint32_t>((total + 255) / 256, 2048u * 8);
    hipLaunchKernelGGL(deinterleave_kernel, dim3(grid), dim3(256), 0, ctx->stream, d_in, d_planes, total);
    HIP_TRY(ctx, hipGetLastError());
    return BLUR_OK;
}

int blur_interleave_bgr_f32_u8_dev(blur_ctx* ctx, const float* d_planes, uint8_t* d_out, uint32_t total)
{
    if (!ctx) return BLUR_ERR_INVALID;
    if (!d_planes || !d_out) return fail(ctx, BLUR_ERR_INVALID, "null pointer");
    if (!total) return BLUR_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const unsigned grid = std::min<uint32_t>((total + 255) / 256, 2048u * 8);
    hipLaunchKernelGGL(interleave_kernel, dim3(grid), dim3(256), 0, ctx->stream, d_planes, d_out, total);
    HIP_TRY(ctx, hipGetLastError());
    return BLUR_OK;
}

// BLUR_BOX_NO_MFMA=1 (developer switch): the accumulator kernels only
static bool box_no_mfma()
{
    static const bool off = [] { const char* e = getenv("BLUR_BOX_NO_MFMA"); return e && *e && *e != '0'; }();
    return off;
}

// ---- fastboxblur: one chunk of whole frames, and the plan that cuts a batch into chunks ----------------------------------
// The horizontal sweeps see a chunk of nframes frames of h rows as one image of nframes h rows (rows are independent); the
// vertical ones walk frame by frame (bx_vertical's frame dimension; the accumulator fallbacks loop over the frames on the host).
// A chunk of one frame is exactly the single-image call.
static int box_run_chunk(blur_ctx* ctx, uint8_t* d_inout, int nframes, int w, int h, int channels, int ksize, int passes)
{
    const size_t fbytes = static_cast<size_t>(w) * h * channels;
    const size_t bytes = fbytes * nframes;
    const int rows = nframes * h;         // (a chunk's bytes are below 2^31: box_batch_plan)
    // the second image, and behind it the mirrored row margins of the matrix-core horizontal kernel (bx_box.hip)
    const size_t margins_at = (bytes + 255) & ~static_cast<size_t>(255);
    const size_t margins_bytes = bx_horizontal_scratch(rows, w, channels, std::min((ksize - 1) / 2, w - 1), std::min(passes, 3));
    if (ctx->box_bytes < margins_at + margins_bytes) {
        if (ctx->box_tmp) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); HIP_TRY(ctx, hipFree(ctx->box_tmp)); ctx->box_tmp = nullptr; ctx->box_bytes = 0; }
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->box_tmp), margins_at + margins_bytes));
        ctx->box_bytes = margins_at + margins_bytes;
    }
    uint8_t *a = d_inout, *b = ctx->box_tmp;
    uint8_t* margins = margins_bytes ? ctx->box_tmp + margins_at : nullptr;
    // one sweep of the accumulator kernel over `frames` frames of `fstride` bytes each (one launch per frame)
    auto sweep = [&](int nlines, int n, size_t lstride, size_t xstride, int frames, size_t fstride) {
        int r = (ksize - 1) / 2;
        if (r > n - 1) r = n - 1;
        const int seg_len = std::max(64, (n + 31) / 32);
        const int nseg = (n + seg_len - 1) / seg_len;
        const long long items = static_cast<long long>(nlines) * channels * nseg;
        const unsigned grid = static_cast<unsigned>((items + 255) / 256);
        for (int f = 0; f < frames; ++f)
            hipLaunchKernelGGL(boxsweep_kernel, dim3(grid), dim3(256), 0, ctx->stream, a + fstride * f, b + fstride * f, nlines, n, lstride, xstride, channels, r, seg_len);
        std::swap(a, b);
    };
    // horizontal sweeps: all passes of a row inside LDS when two copies of the row fit
    const size_t row_lds = 2 * ((static_cast<size_t>(w) * channels + 3) & ~static_cast<size_t>(3));
    // four-pixel-per-step kernel: row + physical reflect borders (r + 1 pixels) + slack for whole groups, twice
    int r_row = (ksize - 1) / 2;
    if (r_row > w - 1) r_row = w - 1;
    const int off0 = ((r_row + 2) * channels + 4 + 15) & ~15;                       // whole aligned dwords left of pixel -(r+1)
    const int buf_bytes = (off0 + (w + r_row + 8) * channels + 16 + 15) & ~15;       // ... and right of pixel w+r+3
    // horizontal sweeps: up to three at a time in one launch on the integer matrix cores where that kernel applies
    int hdone = 0;
    if (!box_no_mfma() && r_row > 0) {
        while (hdone < passes) {
            const int now = std::min(3, passes - hdone);
            bool ran = false;
            HIP_TRY(ctx, bx_horizontal(ctx->stream, a, b, margins, rows, w, channels, r_row, now, ctx->num_cus, &ran));
            if (!ran) break;
            std::swap(a, b);
            hdone += now;
        }
    }
    if (r_row == 0) hdone = passes;               // a box of one pixel
    const int hleft = passes - hdone;
    if (hleft == 0) {
    } else if ((channels == 1 || channels == 3 || channels == 4) && 2 * static_cast<size_t>(buf_bytes) <= kLdsLimit) {
        const int gpt = ((w + 3) / 4 + 255) / 256;
        const size_t lds = 2 * static_cast<size_t>(buf_bytes);
        auto launch = [&](auto kern) -> int {
            if (int rc = set_lds(ctx, kern, lds)) return rc;
            hipLaunchKernelGGL(kern, dim3(rows), dim3(256), lds, ctx->stream, a, b, w, r_row, hleft, gpt, off0, buf_bytes);
            return BLUR_OK;
        };
        int rc = channels == 1 ? launch(boxrow4_kernel<1>) : channels == 3 ? launch(boxrow4_kernel<3>) : launch(boxrow4_kernel<4>);
        if (rc) return rc;
        std::swap(a, b);
    } else if (row_lds <= kLdsLimit) {
        if (int rc = set_lds(ctx, boxrow_kernel, row_lds)) return rc;
        int r = (ksize - 1) / 2;
        if (r > w - 1) r = w - 1;
        const int nseg = std::max(1, 256 / channels);
        const int seg_len = (w + nseg - 1) / nseg;
        hipLaunchKernelGGL(boxrow_kernel, dim3(rows), dim3(256), row_lds, ctx->stream, a, b, w, channels, r, hleft, seg_len, nseg);
        std::swap(a, b);
    } else {
        for (int p = 0; p < hleft; ++p) sweep(rows, w, static_cast<size_t>(w) * channels, static_cast<size_t>(channels), 1, 0);
    }
    // vertical sweeps: up to three at a time in one launch on the integer matrix cores (bx_box.hip) where that kernel applies
    int vdone = 0;
    if (!box_no_mfma()) {
        int r = (ksize - 1) / 2;
        if (r > h - 1) r = h - 1;
        while (vdone < passes && r > 0) {
            const int now = std::min(3, passes - vdone);
            bool ran = false;
            HIP_TRY(ctx, bx_vertical(ctx->stream, a, b, nframes, h, static_cast<int>(static_cast<size_t>(w) * channels), r, now, ctx->num_cus, &ran));
            if (!ran) break;
            std::swap(a, b);
            vdone += now;
        }
        if (r == 0) vdone = passes;            // a box of one row
    }
    if (vdone == passes) {
    } else if ((static_cast<size_t>(w) * channels) % 4 == 0) {
        const int pitch4 = static_cast<int>(static_cast<size_t>(w) * channels / 4);
        int r = (ksize - 1) / 2;
        if (r > h - 1) r = h - 1;
        // enough (dword column, segment) items to fill the chip a few times over
        int nseg = std::max(1, std::min(h / std::max(2 * r + 1, 64), (256 * 2048) / std::max(1, pitch4) + 1));
        const int seg_len = (h + nseg - 1) / nseg;
        nseg = (h + seg_len - 1) / seg_len;
        const long long items = static_cast<long long>(pitch4) * nseg;
        for (int p = vdone; p < passes; ++p) {
            for (int f = 0; f < nframes; ++f)
                hipLaunchKernelGGL(boxcol4_kernel, dim3(static_cast<unsigned>((items + 255) / 256)), dim3(256), 0, ctx->stream, a + fbytes * f, b + fbytes * f, h, pitch4, r, seg_len, nseg);
            std::swap(a, b);
        }
    } else {
        for (int p = vdone; p < passes; ++p) sweep(w, h, static_cast<size_t>(channels), static_cast<size_t>(w) * channels, nframes, fbytes);
    }
    HIP_TRY(ctx, hipGetLastError());
    if (a != d_inout) HIP_TRY(ctx, hipMemcpyAsync(d_inout, a, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return BLUR_OK;
}

// Chunk cap: a chunk's intermediate image (between the horizontal and the vertical kernel) should stay in the 256 MB Infinity
// Cache.  BLUR_BOX_CHUNK_MIB (developer knob, tools/bx_batch.py sweeps it) overrides it.
constexpr size_t kBoxChunkCap = 128ull << 20;
// the rows of one launch of bx_margins_kernel: its grid has one row of blocks per 8 image rows (gridDim.y < 65536)
constexpr long long kBoxChunkRows = 65535ll * 8;

struct BoxBatchPlan {
    int frames_per_chunk = 0, chunks = 0;
    bool vert_mfma = false, horz_mfma = false;    // every sweep of that direction on the integer matrix cores (bx_box.hip)
};

// argument checks and chunking of a batch (no GPU): false = bad arguments.  Chunks are as many whole frames as fit under the cap
// and under 2^31 bytes (the 32-bit offsets of the matrix-core kernels) and kBoxChunkRows rows; a frame larger than that is a
// chunk of its own (the single-image call).
static bool box_batch_plan(int nframes, int w, int h, int channels, int ksize, int passes, BoxBatchPlan* plan)
{
    if (nframes < 0 || w <= 0 || h <= 0 || channels <= 0 || ksize <= 0 || passes < 0) return false;
    long long pitch = 0, fbytes = 0, total = 0;
    if (__builtin_mul_overflow(static_cast<long long>(w), channels, &pitch) || pitch > INT32_MAX || __builtin_mul_overflow(pitch, h, &fbytes) ||
        __builtin_mul_overflow(fbytes, nframes, &total))
        return false;
    const char* e = getenv("BLUR_BOX_CHUNK_MIB");
    const long long cap = e && atoi(e) > 0 ? static_cast<long long>(atoi(e)) << 20 : static_cast<long long>(kBoxChunkCap);
    long long fpc = std::min({ cap / fbytes, ((1ll << 31) - 1) / fbytes, kBoxChunkRows / h });
    fpc = std::max(1ll, std::min(fpc, std::max(1ll, static_cast<long long>(nframes))));
    plan->frames_per_chunk = static_cast<int>(fpc);
    plan->chunks = static_cast<int>((nframes + fpc - 1) / fpc);
    // the matrix-core flags: the decline rules of bx_box.hip on the rows of a (full) chunk.  The sweeps go in groups of up to three
    // and a rule that admits three sweeps admits fewer, so the first group decides
    const int rows = static_cast<int>(fpc * h), now = std::min(passes, 3);
    const int rh = std::min((ksize - 1) / 2, w - 1), rv = std::min((ksize - 1) / 2, h - 1);
    plan->horz_mfma = !box_no_mfma() && passes > 0 && rh > 0 && bx_horizontal_applies(rows, w, channels, rh, now);
    plan->vert_mfma = !box_no_mfma() && passes > 0 && rv > 0 && bx_vertical_applies(h, static_cast<int>(pitch), rv, now);
    return true;
}

int blur_fastboxblur_u8_dev(blur_ctx* ctx, uint8_t* d_inout, int w, int h, int channels, int ksize, int passes)
{
    if (!ctx) return BLUR_ERR_INVALID;
    if (!d_inout || w <= 0 || h <= 0 || channels <= 0 || ksize <= 0 || passes < 0)
        return fail(ctx, BLUR_ERR_INVALID, "fastboxblur: bad arguments");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return box_run_chunk(ctx, d_inout, 1, w, h, channels, ksize, passes);
}

int blur_fastboxblur_batch_plan(int nframes, int w, int h, int channels, int ksize, int passes, int out[4])
{
    BoxBatchPlan p;
    if (!out || !box_batch_plan(nframes, w, h, channels, ksize, passes, &p)) return BLUR_ERR_INVALID;
    out[0] = p.frames_per_chunk;
    out[1] = p.chunks;
    out[2] = p.vert_mfma ? 1 : 0;
    out[3] = p.horz_mfma ? 1 : 0;
    return BLUR_OK;
}

int blur_fastboxblur_u8_batch_dev(blur_ctx* ctx, uint8_t* d_inout, int nframes, int w, int h, int channels, int ksize, int passes)
{
    if (!ctx) return BLUR_ERR_INVALID;
    BoxBatchPlan p;
    if (!box_batch_plan(nframes, w, h, channels, ksize, passes, &p) || (nframes > 0 && !d_inout))
        return fail(ctx, BLUR_ERR_INVALID, "fastboxblur batch: bad arguments");
    if (nframes == 0) return BLUR_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t fbytes = static_cast<size_t>(w) * h * channels;
    for (int f = 0; f < nframes; f += p.frames_per_chunk)
        if (int rc = box_run_chunk(ctx, d_inout + fbytes * f, std::min(p.frames_per_chunk, nframes - f), w, h, channels, ksize, passes)) return rc;
    return BLUR_OK;
}

int blur_fastboxblur_u8_host_batch(blur_ctx* ctx, uint8_t* inout, int nframes, int w, int h, int channels, int ksize, int passes)
{
    if (!ctx) return BLUR_ERR_INVALID;
    BoxBatchPlan p;
    if (!box_batch_plan(nframes, w, h, channels, ksize, passes, &p) || (nframes > 0 && !inout))
        return fail(ctx, BLUR_ERR_INVALID, "fastboxblur batch: bad arguments");
    if (nframes == 0) return BLUR_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t fbytes = static_cast<size_t>(w) * h * channels;
    void* dv = nullptr;
    if (int rc0 = ensure_host_stage(ctx, fbytes * p.frames_per_chunk, &dv)) return rc0;
    uint8_t* d = static_cast<uint8_t*>(dv);
    // chunk by chunk through the stage: copy in, blur, copy out (stream order keeps the stage's reuse safe)
    int rc = BLUR_OK;
    hipError_t e = hipSuccess;
    for (int f = 0; f < nframes && e == hipSuccess && rc == BLUR_OK; f += p.frames_per_chunk) {
        const int n = std::min(p.frames_per_chunk, nframes - f);
        e = hipMemcpyAsync(d, inout + fbytes * f, fbytes * n, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) rc = box_run_chunk(ctx, d, n, w, h, channels, ksize, passes);
        if (e == hipSuccess && rc == BLUR_OK) e = hipMemcpyAsync(inout + fbytes * f, d, fbytes * n, hipMemcpyDeviceToHost, ctx->stream);
    }
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) { ctx->err = std::string("host fastboxblur batch: ") + hipGetErrorString(e); return BLUR_ERR_HIP; }
    return rc;
}

int blur_fastboxblur_u8_host(blur_ctx* ctx, uint8_t* inout, int w, int h, int channels, int ksize, int passes)
{
    if (!ctx) return BLUR_ERR_INVALID;
    if (!inout || w <= 0 || h <= 0 || channels <= 0) return fail(ctx, BLUR_ERR_INVALID, "fastboxblur: bad arguments");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t bytes = static_cast<size_t>(w) * h * channels;
    void* dv = nullptr;
    if (int rc0 = ensure_host_stage(ctx, bytes, &dv)) return rc0;
    uint8_t* d = static_cast<uint8_t*>(dv);
    int rc = BLUR_OK;
    hipError_t e = hipMemcpyAsync(d, inout, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) rc = blur_fastboxblur_u8_dev(ctx, d, w, h, channels, ksize, passes);
    if (e == hipSuccess && rc == BLUR_OK) e = hipMemcpyAsync(inout, d, bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { ctx->err = std::string("host fastboxblur: ") + hipGetErrorString(e); return BLUR_ERR_HIP; }
    return rc;
}

/* diagnostic builds (-DFK_STAMPS): copy the stamp tail behind the multiplier table of FFT length n
   (role 1 = specialised row plan, 2 = specialised column plan) */
// ---- several GPUs from one host thread ------------------------------------------------------------
// Frames are independent (Source.cpp:510 even runs channels serially), so a batch shards by frame with no exchange
// between the shards: shard r gets frames [n r / S, n (r + 1) / S) and its own context and stream.  `devices` may
// repeat an ordinal: several logical shards on one GPU (that is also how the path is tested on a one-GPU box).
struct blur_multi {
    std::vector<int> devices;
    std::vector<blur_ctx*> ctxs;
    std::vector<hipStream_t> streams;
    std::vector<uint8_t*> stage;        // per shard: frames of this shard on its device (shards away from the frames' device)
    std::vector<size_t> stage_bytes;
    std::string err;
};

int blur_multi_create(blur_multi** out, const int* devices, int ndevices)
{
    if (!out || !devices || ndevices <= 0) return BLUR_ERR_INVALID;
    *out = nullptr;
    auto m = std::make_unique<blur_multi>();
    for (int r = 0; r < ndevices; ++r) {
        blur_ctx* c = nullptr;
        int rc = blur_ctx_create(&c, devices[r]);
        hipStream_t st = nullptr;
        if (rc == BLUR_OK && (hipSetDevice(devices[r]) != hipSuccess || hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess)) rc = BLUR_ERR_HIP;
        if (rc == BLUR_OK) rc = blur_ctx_set_stream(c, st);
        if (rc != BLUR_OK) {
            if (c) blur_ctx_destroy(c);
            if (st) (void)hipStreamDestroy(st);
            for (size_t i = 0; i < m->ctxs.size(); ++i) { blur_ctx_destroy(m->ctxs[i]); (void)hipStreamDestroy(m->streams[i]); }
            return rc;
        }
        m->devices.push_back(devices[r]);
        m->ctxs.push_back(c);
        m->streams.push_back(st);
        m->stage.push_back(nullptr);
        m->stage_bytes.push_back(0);
    }
    *out = m.release();
    return BLUR_OK;
}

int blur_multi_destroy(blur_multi* m)
{
    if (!m) return BLUR_ERR_INVALID;
    for (size_t r = 0; r < m->ctxs.size(); ++r) {
        (void)hipSetDevice(m->devices[r]);
        (void)hipStreamSynchronize(m->streams[r]);
        if (m->stage[r]) (void)hipFree(m->stage[r]);
        blur_ctx_destroy(m->ctxs[r]);          // synchronises its stream before freeing
        (void)hipStreamDestroy(m->streams[r]);
    }
    delete m;
    return BLUR_OK;
}

int blur_multi_shards(const blur_multi* m) { return m ? static_cast<int>(m->ctxs.size()) : 0; }
const char* blur_multi_last_error(const blur_multi* m) { return m ? m->err.c_str() : "null blur_multi"; }

// location: 0 = src/dst are host pointers (pinned memory overlaps the copies of different shards), 1 = device pointers
// on devices[0].  Synchronous: returns when every shard is done.  `fb`: bytes per frame (0: a non-positive size);
// `body(ctx, in, out, n)` queues the work of one shard's n frames on its context's stream.
using ShardBody = std::function<int(blur_ctx*, const uint8_t*, uint8_t*, int)>;
static int blur_multi_run(blur_multi* m, const uint8_t* src, uint8_t* dst, int nframes, size_t fb, int location, const ShardBody& body)
{
    if (!m) return BLUR_ERR_INVALID;
    if (!src || !dst || nframes < 0 || fb == 0) { m->err = "null frame pointer, negative frame count or non-positive size"; return BLUR_ERR_INVALID; }
    const int S = static_cast<int>(m->ctxs.size());
    int rc_all = BLUR_OK;
    for (int r = 0; r < S && rc_all == BLUR_OK; ++r) {
        const int b = static_cast<int>(static_cast<long long>(nframes) * r / S), e = static_cast<int>(static_cast<long long>(nframes) * (r + 1) / S);
        if (e <= b) continue;
        const size_t bytes = fb * (e - b);
        blur_ctx* c = m->ctxs[r];
        hipStream_t st = m->streams[r];
        auto hip_fail = [&](hipError_t er, const char* what) { m->err = std::string(what) + ": " + hipGetErrorString(er); rc_all = BLUR_ERR_HIP; };
        if (hipError_t er = hipSetDevice(m->devices[r]); er != hipSuccess) { hip_fail(er, "hipSetDevice"); break; }
        const bool local = location == 1 && m->devices[r] == m->devices[0];
        const uint8_t* in = src + fb * b;
        uint8_t* outp = dst + fb * b;
        uint8_t* work_in = const_cast<uint8_t*>(in);
        uint8_t* work_out = outp;
        if (!local) {
            if (m->stage_bytes[r] < bytes) {
                if (m->stage[r]) { (void)hipStreamSynchronize(st); (void)hipFree(m->stage[r]); m->stage[r] = nullptr; m->stage_bytes[r] = 0; }
                if (hipError_t er = hipMalloc(reinterpret_cast<void**>(&m->stage[r]), bytes); er != hipSuccess) { hip_fail(er, "hipMalloc (shard staging)"); break; }
                m->stage_bytes[r] = bytes;
            }
            work_in = work_out = m->stage[r];
            const hipError_t er = location == 0 ? hipMemcpyAsync(work_in, in, bytes, hipMemcpyHostToDevice, st)
                                                : hipMemcpyPeerAsync(work_in, m->devices[r], in, m->devices[0], bytes, st);
            if (er != hipSuccess) { hip_fail(er, "fan-out copy"); break; }
        }
        const int rc = body(c, work_in, work_out, e - b);
        if (rc != BLUR_OK) { m->err = std::string("shard ") + std::to_string(r) + ": " + blur_last_error(c); rc_all = rc; break; }
        if (!local) {
            const hipError_t er = location == 0 ? hipMemcpyAsync(outp, work_out, bytes, hipMemcpyDeviceToHost, st)
                                                : hipMemcpyPeerAsync(outp, m->devices[0], work_out, m->devices[r], bytes, st);
            if (er != hipSuccess) { hip_fail(er, "fan-in copy"); break; }
        }
    }
    for (int r = 0; r < S; ++r) {
        (void)hipSetDevice(m->devices[r]);
        const hipError_t er = hipStreamSynchronize(m->streams[r]);
        if (er != hipSuccess && rc_all == BLUR_OK) { m->err = std::string("hipStreamSynchronize: ") + hipGetErrorString(er); rc_all = BLUR_ERR_HIP; }
    }
    return rc_all;
}

static size_t gaussian_frame_bytes(int rows, int cols) { return rows > 0 && cols > 0 ? static_cast<size_t>(rows) * cols * 3 : 0; }
static ShardBody gaussian_shard(int rows, int cols, double sigma, const blur_opts* opts)
{
    return [=](blur_ctx* c, const uint8_t* in, uint8_t* out, int n) { return blur_gaussian_u8c3_batch_dev(c, in, out, n, rows, cols, sigma, opts); };
}

int blur_gaussian_u8c3_batch_multi_dev(blur_multi* m, const uint8_t* d_src, uint8_t* d_dst, int nframes, int rows, int cols, double sigma, const blur_opts* opts)
{
    if (m) {
        // frames queued by the caller on devices[0] must be complete before other devices (and other streams) read them
        if (hipSetDevice(m->devices[0]) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { m->err = "hipDeviceSynchronize on the frames' device failed"; return BLUR_ERR_HIP; }
    }
    return blur_multi_run(m, d_src, d_dst, nframes, gaussian_frame_bytes(rows, cols), 1, gaussian_shard(rows, cols, sigma, opts));
}

int blur_gaussian_u8c3_batch_multi_host(blur_multi* m, const uint8_t* src, uint8_t* dst, int nframes, int rows, int cols, double sigma, const blur_opts* opts)
{
    return blur_multi_run(m, src, dst, nframes, gaussian_frame_bytes(rows, cols), 0, gaussian_shard(rows, cols, sigma, opts));
}

// fastboxblur: in place, so every shard's input is its output
static int box_multi(blur_multi* m, uint8_t* inout, int nframes, int w, int h, int channels, int ksize, int passes, int location)
{
    if (!m) return BLUR_ERR_INVALID;
    BoxBatchPlan p;
    if (!box_batch_plan(nframes, w, h, channels, ksize, passes, &p) || (nframes > 0 && !inout)) { m->err = "fastboxblur batch: bad arguments"; return BLUR_ERR_INVALID; }
    if (nframes == 0) return BLUR_OK;
    if (location == 1 && (hipSetDevice(m->devices[0]) != hipSuccess || hipDeviceSynchronize() != hipSuccess)) { m->err = "hipDeviceSynchronize on the frames' device failed"; return BLUR_ERR_HIP; }
    const size_t fb = static_cast<size_t>(w) * h * channels;
    return blur_multi_run(m, inout, inout, nframes, fb, location, [=](blur_ctx* c, const uint8_t*, uint8_t* out, int n) {
        return blur_fastboxblur_u8_batch_dev(c, out, n, w, h, channels, ksize, passes);
    });
}

int blur_fastboxblur_u8_batch_multi_dev(blur_multi* m, uint8_t* d_inout, int nframes, int w, int h, int channels, int ksize, int passes)
{
    return box_multi(m, d_inout, nframes, w, h, channels, ksize, passes, 1);
}

int blur_fastboxblur_u8_batch_multi_host(blur_multi* m, uint8_t* inout, int nframes, int w, int h, int channels, int ksize, int passes)
{
    return box_multi(m, inout, nframes, w, h, channels, ksize, passes, 0);
}

// blur_gaussian_{u8,f32,u16,f16,bf16}_batch_multi_*: the frames of a batch sharded over the devices (a template: C++ linkage)
extern "C++" {
// the shards of a per-channel batch whose arguments have been checked: body(ctx, in, out, n) queues one shard's n frames
template <typename T, typename Body>
static int blur_ch_multi_run(blur_multi* m, const T* src, T* dst, int nframes, int rows, int cols, int channels, int location, Body body)
{
    if (!m) return BLUR_ERR_INVALID;
    if (nframes == 0) return BLUR_OK;
    // frames queued by the caller on devices[0] must be complete before other devices (and other streams) read them
    if (location == 1 && (hipSetDevice(m->devices[0]) != hipSuccess || hipDeviceSynchronize() != hipSuccess)) { m->err = "hipDeviceSynchronize on the frames' device failed"; return BLUR_ERR_HIP; }
    const size_t fb = rows > 0 && cols > 0 ? static_cast<size_t>(rows) * cols * channels * sizeof(T) : 0;
    return blur_multi_run(m, reinterpret_cast<const uint8_t*>(src), reinterpret_cast<uint8_t*>(dst), nframes, fb, location,
                          [=](blur_ctx* c, const uint8_t* in, uint8_t* out, int n) { return body(c, reinterpret_cast<const T*>(in), reinterpret_cast<T*>(out), n); });
}

template <typename T>
static int blur_ch_multi(blur_multi* m, const T* src, T* dst, int nframes, int rows, int cols, int channels, double sigma, const blur_opts* opts, int location)
{
    if (!m) return BLUR_ERR_INVALID;
    if (channels != 1 && channels != 3 && channels != 4) { m->err = "channels must be 1, 3 or 4"; return BLUR_ERR_INVALID; }
    if (!src || !dst || nframes < 0) { m->err = "null frame pointer or negative frame count"; return BLUR_ERR_INVALID; }
    return blur_ch_multi_run(m, src, dst, nframes, rows, cols, channels, location,
                             [=](blur_ctx* c, const T* in, T* out, int n) { return blur_ch_batch_impl(c, in, out, n, rows, cols, channels, sigma, opts); });
}
}  // extern "C++"

// 1-, 3- and 4-channel u8 images (channels == 3: the u8c3 entry points)
int blur_gaussian_u8_batch_dev(blur_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int nframes, int rows, int cols, int channels, double sigma,
                               const blur_opts* opts)
{
    return blur_ch_batch_impl(ctx, d_src, d_dst, nframes, rows, cols, channels, sigma, opts);
}

int blur_gaussian_u8_dev(blur_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int rows, int cols, int channels, double sigma, const blur_opts* opts)
{
    return blur_ch_batch_impl(ctx, d_src, d_dst, 1, rows, cols, channels, sigma, opts);
}

int blur_gaussian_u8_host(blur_ctx* ctx, const uint8_t* src, uint8_t* dst, int rows, int cols, int channels, double sigma, const blur_opts* opts)
{
    return blur_ch_host(ctx, src, dst, rows, cols, channels, sigma, opts);
}

int blur_gaussian_u8_batch_multi_dev(blur_multi* m, const uint8_t* d_src, uint8_t* d_dst, int nframes, int rows, int cols, int channels, double sigma,
                                     const blur_opts* opts)
{
    return blur_ch_multi(m, d_src, d_dst, nframes, rows, cols, channels, sigma, opts, 1);
}

int blur_gaussian_u8_batch_multi_host(blur_multi* m, const uint8_t* src, uint8_t* dst, int nframes, int rows, int cols, int channels, double sigma,
                                      const blur_opts* opts)
{
    return blur_ch_multi(m, src, dst, nframes, rows, cols, channels, sigma, opts, 0);
}

// float32 images of 1, 3 or 4 channels
int blur_gaussian_f32_batch_dev(blur_ctx* ctx, const float* d_src, float* d_dst, int nframes, int rows, int cols, int channels, double sigma,
                                const blur_opts* opts)
{
    return blur_ch_batch_impl(ctx, d_src, d_dst, nframes, rows, cols, channels, sigma, opts);
}

int blur_gaussian_f32_dev(blur_ctx* ctx, const float* d_src, float* d_dst, int rows, int cols, int channels, double sigma, const blur_opts* opts)
{
    return blur_ch_batch_impl(ctx, d_src, d_dst, 1, rows, cols, channels, sigma, opts);
}

int blur_gaussian_f32_host(blur_ctx* ctx, const float* src, float* dst, int rows, int cols, int channels, double sigma, const blur_opts* opts)
{
    return blur_ch_host(ctx, src, dst, rows, cols, channels, sigma, opts);
}

int blur_gaussian_f32_batch_multi_dev(blur_multi* m, const float* d_src, float* d_dst, int nframes, int rows, int cols, int channels, double sigma,
                                      const blur_opts* opts)
{
    return blur_ch_multi(m, d_src, d_dst, nframes, rows, cols, channels, sigma, opts, 1);
}

int blur_gaussian_f32_batch_multi_host(blur_multi* m, const float* src, float* dst, int nframes, int rows, int cols, int channels, double sigma,
                                       const blur_opts* opts)
{
    return blur_ch_multi(m, src, dst, nframes, rows, cols, channels, sigma, opts, 0);
}

// u16 images of 1, 3 or 4 channels
int blur_gaussian_u16_batch_dev(blur_ctx* ctx, const uint16_t* d_src, uint16_t* d_dst, int nframes, int rows, int cols, int channels, double sigma,
                                const blur_opts* opts)
{
    return blur_ch_batch_impl(ctx, d_src, d_dst, nframes, rows, cols, channels, sigma, opts);
}

int blur_gaussian_u16_dev(blur_ctx* ctx, const uint16_t* d_src, uint16_t* d_dst, int rows, int cols, int channels, double sigma, const blur_opts* opts)
{
    return blur_ch_batch_impl(ctx, d_src, d_dst, 1, rows, cols, channels, sigma, opts);
}

int blur_gaussian_u16_host(blur_ctx* ctx, const uint16_t* src, uint16_t* dst, int rows, int cols, int channels, double sigma, const blur_opts* opts)
{
    return blur_ch_host(ctx, src, dst, rows, cols, channels, sigma, opts);
}

int blur_gaussian_u16_batch_multi_dev(blur_multi* m, const uint16_t* d_src, uint16_t* d_dst, int nframes, int rows, int cols, int channels, double sigma,
                                      const blur_opts* opts)
{
    return blur_ch_multi(m, d_src, d_dst, nframes, rows, cols, channels, sigma, opts, 1);
}

int blur_gaussian_u16_batch_multi_host(blur_multi* m, const uint16_t* src, uint16_t* dst, int nframes, int rows, int cols, int channels, double sigma,
                                       const blur_opts* opts)
{
    return blur_ch_multi(m, src, dst, nframes, rows, cols, channels, sigma, opts, 0);
}

// float16 images of 1, 3 or 4 channels: the bit patterns in uint16_t (the C header has no 16-bit floating type)
int blur_gaussian_f16_batch_dev(blur_ctx* ctx, const uint16_t* d_src, uint16_t* d_dst, int nframes, int rows, int cols, int channels, double sigma,
                                const blur_opts* opts)
{
    return blur_ch_batch_impl(ctx, reinterpret_cast<const ff_f16*>(d_src), reinterpret_cast<ff_f16*>(d_dst), nframes, rows, cols, channels, sigma, opts);
}

int blur_gaussian_f16_dev(blur_ctx* ctx, const uint16_t* d_src, uint16_t* d_dst, int rows, int cols, int channels, double sigma, const blur_opts* opts)
{
    return blur_ch_batch_impl(ctx, reinterpret_cast<const ff_f16*>(d_src), reinterpret_cast<ff_f16*>(d_dst), 1, rows, cols, channels, sigma, opts);
}

int blur_gaussian_f16_host(blur_ctx* ctx, const uint16_t* src, uint16_t* dst, int rows, int cols, int channels, double sigma, const blur_opts* opts)
{
    return blur_ch_host(ctx, reinterpret_cast<const ff_f16*>(src), reinterpret_cast<ff_f16*>(dst), rows, cols, channels, sigma, opts);
}

int blur_gaussian_f16_batch_multi_dev(blur_multi* m, const uint16_t* d_src, uint16_t* d_dst, int nframes, int rows, int cols, int channels, double sigma,
                                      const blur_opts* opts)
{
    return blur_ch_multi(m, reinterpret_cast<const ff_f16*>(d_src), reinterpret_cast<ff_f16*>(d_dst), nframes, rows, cols, channels, sigma, opts, 1);
}

int blur_gaussian_f16_batch_multi_host(blur_multi* m, const uint16_t* src, uint16_t* dst, int nframes, int rows, int cols, int channels, double sigma,
                                       const blur_opts* opts)
{
    return blur_ch_multi(m, reinterpret_cast<const ff_f16*>(src), reinterpret_cast<ff_f16*>(dst), nframes, rows, cols, channels, sigma, opts, 0);
}

// bfloat16 images of 1, 3 or 4 channels: the bit patterns in uint16_t (the C header has no 16-bit floating type)
int blur_gaussian_bf16_batch_dev(blur_ctx* ctx, const uint16_t* d_src, uint16_t* d_dst, int nframes, int rows, int cols, int channels, double sigma,
                                const blur_opts* opts)
{
    return blur_ch_batch_impl(ctx, reinterpret_cast<const ff_bf16*>(d_src), reinterpret_cast<ff_bf16*>(d_dst), nframes, rows, cols, channels, sigma, opts);
}

int blur_gaussian_bf16_dev(blur_ctx* ctx, const uint16_t* d_src, uint16_t* d_dst, int rows, int cols, int channels, double sigma, const blur_opts* opts)
{
    return blur_ch_batch_impl(ctx, reinterpret_cast<const ff_bf16*>(d_src), reinterpret_cast<ff_bf16*>(d_dst), 1, rows, cols, channels, sigma, opts);
}

int blur_gaussian_bf16_host(blur_ctx* ctx, const uint16_t* src, uint16_t* dst, int rows, int cols, int channels, double sigma, const blur_opts* opts)
{
    return blur_ch_host(ctx, reinterpret_cast<const ff_bf16*>(src), reinterpret_cast<ff_bf16*>(dst), rows, cols, channels, sigma, opts);
}

int blur_gaussian_bf16_batch_multi_dev(blur_multi* m, const uint16_t* d_src, uint16_t* d_dst, int nframes, int rows, int cols, int channels, double sigma,
                                      const blur_opts* opts)
{
    return blur_ch_multi(m, reinterpret_cast<const ff_bf16*>(d_src), reinterpret_cast<ff_bf16*>(d_dst), nframes, rows, cols, channels, sigma, opts, 1);
}

int blur_gaussian_bf16_batch_multi_host(blur_multi* m, const uint16_t* src, uint16_t* dst, int nframes, int rows, int cols, int channels, double sigma,
                                       const blur_opts* opts)
{
    return blur_ch_multi(m, reinterpret_cast<const ff_bf16*>(src), reinterpret_cast<ff_bf16*>(dst), nframes, rows, cols, channels, sigma, opts, 0);
}

// blur_gaussian_*_sigmas_batch_multi_*: as blur_ch_multi with one sigma per channel (each shard gets its own copy of the sigmas)
extern "C++" {
template <typename T>
static int blur_ch_sigmas_multi(blur_multi* m, const T* src, T* dst, int nframes, int rows, int cols, int channels, const double* sigmas, const blur_opts* opts, int location)
{
    SigmaGroups sg;
    const char* why = nullptr;
    if (int rc = ch_sigmas_status(src, dst, nframes, rows, cols, channels, sigmas, sg, &why)) { if (m) m->err = why; return rc; }
    const std::array<double, 4> sv = { sigmas[0], channels > 1 ? sigmas[1] : 0.0, channels > 2 ? sigmas[2] : 0.0, channels > 3 ? sigmas[3] : 0.0 };
    return blur_ch_multi_run(m, src, dst, nframes, rows, cols, channels, location,
                             [=](blur_ctx* c, const T* in, T* out, int n) { return blur_ch_sigmas_batch_impl(c, in, out, n, rows, cols, channels, sv.data(), opts); });
}
}  // extern "C++"

// host-only: how a call with these sigmas groups its channels
int blur_gaussian_sigmas_plan(int rows, int cols, int channels, const double* sigmas, int* out)
{
    SigmaGroups sg;
    int dummy = 0;
    const char* why = nullptr;
    if (!out) return BLUR_ERR_INVALID;
    if (int rc = ch_sigmas_status(&dummy, &dummy, 0, rows, cols, channels, sigmas, sg, &why)) return rc;
    for (int c = 0; c < channels; ++c) {
        const int g = sg.group_of[c];
        out[3 * c] = g;
        out[3 * c + 1] = out[3 * c + 2] = 0;
        if (g < 0) continue;
        const int pad = pffft_sizing(rows, cols, sg.sigma[g]).pad;
        const FxEntry* fe = find_entry_for_pad<FxEntry>(pad);
        out[3 * c + 1] = pad;
        out[3 * c + 2] = fe ? fe->nkb : 0;
    }
    return BLUR_OK;
}

// pitched frames and regions of interest (blur_amd.h: blur_gaussian_*_pitched_batch_dev): pitches and frame strides in bytes
int blur_gaussian_u8_pitched_batch_dev(blur_ctx* ctx, const uint8_t* d_src, size_t src_pitch, size_t src_frame_stride, uint8_t* d_dst, size_t dst_pitch,
                                       size_t dst_frame_stride, int nframes, int rows, int cols, int channels, double sigma, const blur_opts* opts)
{
    const ChLayout L{ src_pitch, src_frame_stride, dst_pitch, dst_frame_stride };
    return blur_ch_batch_impl(ctx, d_src, d_dst, nframes, rows, cols, channels, sigma, opts, &L);
}

int blur_gaussian_u8_sigmas_pitched_batch_dev(blur_ctx* ctx, const uint8_t* d_src, size_t src_pitch, size_t src_frame_stride, uint8_t* d_dst, size_t dst_pitch,
                                              size_t dst_frame_stride, int nframes, int rows, int cols, int channels, const double* sigmas, const blur_opts* opts)
{
    const ChLayout L{ src_pitch, src_frame_stride, dst_pitch, dst_frame_stride };
    return blur_ch_sigmas_batch_impl(ctx, d_src, d_dst, nframes, rows, cols, channels, sigmas, opts, &L);
}

int blur_gaussian_f32_pitched_batch_dev(blur_ctx* ctx, const float* d_src, size_t src_pitch, size_t src_frame_stride, float* d_dst, size_t dst_pitch,
                                        size_t dst_frame_stride, int nframes, int rows, int cols, int channels, double sigma, const blur_opts* opts)
{
    const ChLayout L{ src_pitch, src_frame_stride, dst_pitch, dst_frame_stride };
    return blur_ch_batch_impl(ctx, d_src, d_dst, nframes, rows, cols, channels, sigma, opts, &L);
}

int blur_gaussian_f32_sigmas_pitched_batch_dev(blur_ctx* ctx, const float* d_src, size_t src_pitch, size_t src_frame_stride, float* d_dst, size_t dst_pitch,
                                               size_t dst_frame_stride, int nframes, int rows, int cols, int channels, const double* sigmas, const blur_opts* opts)
{
    const ChLayout L{ src_pitch, src_frame_stride, dst_pitch, dst_frame_stride };
    return blur_ch_sigmas_batch_impl(ctx, d_src, d_dst, nframes, rows, cols, channels, sigmas, opts, &L);
}

int blur_gaussian_u16_pitched_batch_dev(blur_ctx* ctx, const uint16_t* d_src, size_t src_pitch, size_t src_frame_stride, uint16_t* d_dst, size_t dst_pitch,
                                        size_t dst_frame_stride, int nframes, int rows, int cols, int channels, double sigma, const blur_opts* opts)
{
    const ChLayout L{ src_pitch, src_frame_stride, dst_pitch, dst_frame_stride };
    return blur_ch_batch_impl(ctx, d_src, d_dst, nframes, rows, cols, channels, sigma, opts, &L);
}

int blur_gaussian_u16_sigmas_pitched_batch_dev(blur_ctx* ctx, const uint16_t* d_src, size_t src_pitch, size_t src_frame_stride, uint16_t* d_dst, size_t dst_pitch,
                                               size_t dst_frame_stride, int nframes, int rows, int cols, int channels, const double* sigmas, const blur_opts* opts)
{
    const ChLayout L{ src_pitch, src_frame_stride, dst_pitch, dst_frame_stride };
    return blur_ch_sigmas_batch_impl(ctx, d_src, d_dst, nframes, rows, cols, channels, sigmas, opts, &L);
}

int blur_gaussian_f16_pitched_batch_dev(blur_ctx* ctx, const uint16_t* d_src, size_t src_pitch, size_t src_frame_stride, uint16_t* d_dst, size_t dst_pitch,
                                        size_t dst_frame_stride, int nframes, int rows, int cols, int channels, double sigma, const blur_opts* opts)
{
    const ChLayout L{ src_pitch, src_frame_stride, dst_pitch, dst_frame_stride };
    return blur_ch_batch_impl(ctx, reinterpret_cast<const ff_f16*>(d_src), reinterpret_cast<ff_f16*>(d_dst), nframes, rows, cols, channels, sigma, opts, &L);
}

int blur_gaussian_f16_sigmas_pitched_batch_dev(blur_ctx* ctx, const uint16_t* d_src, size_t src_pitch, size_t src_frame_stride, uint16_t* d_dst, size_t dst_pitch,
                                               size_t dst_frame_stride, int nframes, int rows, int cols, int channels, const double* sigmas, const blur_opts* opts)
{
    const ChLayout L{ src_pitch, src_frame_stride, dst_pitch, dst_frame_stride };
    return blur_ch_sigmas_batch_impl(ctx, reinterpret_cast<const ff_f16*>(d_src), reinterpret_cast<ff_f16*>(d_dst), nframes, rows, cols, channels, sigmas, opts, &L);
}

int blur_gaussian_bf16_pitched_batch_dev(blur_ctx* ctx, const uint16_t* d_src, size_t src_pitch, size_t src_frame_stride, uint16_t* d_dst, size_t dst_pitch,
                                         size_t dst_frame_stride, int nframes, int rows, int cols, int channels, double sigma, const blur_opts* opts)
{
    const ChLayout L{ src_pitch, src_frame_stride, dst_pitch, dst_frame_stride };
    return blur_ch_batch_impl(ctx, reinterpret_cast<const ff_bf16*>(d_src), reinterpret_cast<ff_bf16*>(d_dst), nframes, rows, cols, channels, sigma, opts, &L);
}

int blur_gaussian_bf16_sigmas_pitched_batch_dev(blur_ctx* ctx, const uint16_t* d_src, size_t src_pitch, size_t src_frame_stride, uint16_t* d_dst, size_t dst_pitch,
                                                size_t dst_frame_stride, int nframes, int rows, int cols, int channels, const double* sigmas, const blur_opts* opts)
{
    const ChLayout L{ src_pitch, src_frame_stride, dst_pitch, dst_frame_stride };
    return blur_ch_sigmas_batch_impl(ctx, reinterpret_cast<const ff_bf16*>(d_src), reinterpret_cast<ff_bf16*>(d_dst), nframes, rows, cols, channels, sigmas, opts, &L);
}

// decoded video surfaces (blur_amd.h: blur_gaussian_nv12_*, blur_gaussian_p016_*): pitches and frame strides in bytes
int blur_gaussian_nv12_batch_dev(blur_ctx* ctx, const uint8_t* d_src_y, const uint8_t* d_src_uv, size_t src_pitch, size_t src_y_frame_stride, size_t src_uv_frame_stride,
                                 uint8_t* d_dst_y, uint8_t* d_dst_uv, size_t dst_pitch, size_t dst_y_frame_stride, size_t dst_uv_frame_stride, int nframes, int rows,
                                 int cols, const double* sigmas, const blur_opts* opts)
{
    return blur_nv_batch_impl<uint8_t>(ctx, NvSurface{ d_src_y, d_src_uv, d_dst_y, d_dst_uv, src_pitch, src_y_frame_stride, src_uv_frame_stride, dst_pitch,
                                                       dst_y_frame_stride, dst_uv_frame_stride }, nframes, rows, cols, sigmas, opts);
}

int blur_gaussian_nv12_dev(blur_ctx* ctx, const uint8_t* d_src_y, const uint8_t* d_src_uv, size_t src_pitch, uint8_t* d_dst_y, uint8_t* d_dst_uv, size_t dst_pitch, int rows,
                           int cols, const double* sigmas, const blur_opts* opts)
{
    return blur_nv_batch_impl<uint8_t>(ctx, NvSurface{ d_src_y, d_src_uv, d_dst_y, d_dst_uv, src_pitch, 0, 0, dst_pitch, 0, 0 }, 1, rows, cols, sigmas, opts);
}

int blur_gaussian_nv12_host(blur_ctx* ctx, const uint8_t* src, uint8_t* dst, int rows, int cols, const double* sigmas, const blur_opts* opts)
{
    return blur_nv_host(ctx, src, dst, rows, cols, sigmas, opts);
}

int blur_gaussian_p016_batch_dev(blur_ctx* ctx, const uint16_t* d_src_y, const uint16_t* d_src_uv, size_t src_pitch, size_t src_y_frame_stride, size_t src_uv_frame_stride,
                                 uint16_t* d_dst_y, uint16_t* d_dst_uv, size_t dst_pitch, size_t dst_y_frame_stride, size_t dst_uv_frame_stride, int nframes, int rows,
                                 int cols, const double* sigmas, const blur_opts* opts)
{
    return blur_nv_batch_impl<uint16_t>(ctx, NvSurface{ d_src_y, d_src_uv, d_dst_y, d_dst_uv, src_pitch, src_y_frame_stride, src_uv_frame_stride, dst_pitch,
                                                        dst_y_frame_stride, dst_uv_frame_stride }, nframes, rows, cols, sigmas, opts);
}

int blur_gaussian_p016_dev(blur_ctx* ctx, const uint16_t* d_src_y, const uint16_t* d_src_uv, size_t src_pitch, uint16_t* d_dst_y, uint16_t* d_dst_uv, size_t dst_pitch,
                           int rows, int cols, const double* sigmas, const blur_opts* opts)
{
    return blur_nv_batch_impl<uint16_t>(ctx, NvSurface{ d_src_y, d_src_uv, d_dst_y, d_dst_uv, src_pitch, 0, 0, dst_pitch, 0, 0 }, 1, rows, cols, sigmas, opts);
}

int blur_gaussian_p016_host(blur_ctx* ctx, const uint16_t* src, uint16_t* dst, int rows, int cols, const double* sigmas, const blur_opts* opts)
{
    return blur_nv_host(ctx, src, dst, rows, cols, sigmas, opts);
}

// one sigma per frame (blur_amd.h)
int blur_gaussian_u8_frame_sigmas_batch_dev(blur_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int nframes, int rows, int cols, int channels, const double* sigmas,
                                            const blur_opts* opts)
{
    return blur_ch_frame_sigmas_batch_impl(ctx, d_src, d_dst, nframes, rows, cols, channels, sigmas, opts);
}

int blur_gaussian_f32_frame_sigmas_batch_dev(blur_ctx* ctx, const float* d_src, float* d_dst, int nframes, int rows, int cols, int channels, const double* sigmas,
                                             const blur_opts* opts)
{
    return blur_ch_frame_sigmas_batch_impl(ctx, d_src, d_dst, nframes, rows, cols, channels, sigmas, opts);
}

int blur_gaussian_u8_frame_sigmas_pitched_batch_dev(blur_ctx* ctx, const uint8_t* d_src, size_t src_pitch, size_t src_frame_stride, uint8_t* d_dst, size_t dst_pitch,
                                                    size_t dst_frame_stride, int nframes, int rows, int cols, int channels, const double* sigmas, const blur_opts* opts)
{
    const ChLayout L{ src_pitch, src_frame_stride, dst_pitch, dst_frame_stride };
    return blur_ch_frame_sigmas_batch_impl(ctx, d_src, d_dst, nframes, rows, cols, channels, sigmas, opts, &L);
}

int blur_gaussian_f32_frame_sigmas_pitched_batch_dev(blur_ctx* ctx, const float* d_src, size_t src_pitch, size_t src_frame_stride, float* d_dst, size_t dst_pitch,
                                                     size_t dst_frame_stride, int nframes, int rows, int cols, int channels, const double* sigmas, const blur_opts* opts)
{
    const ChLayout L{ src_pitch, src_frame_stride, dst_pitch, dst_frame_stride };
    return blur_ch_frame_sigmas_batch_impl(ctx, d_src, d_dst, nframes, rows, cols, channels, sigmas, opts, &L);
}

int blur_gaussian_u16_frame_sigmas_batch_dev(blur_ctx* ctx, const uint16_t* d_src, uint16_t* d_dst, int nframes, int rows, int cols, int channels, const double* sigmas,
                    const blur_opts* opts)
{
    return blur_ch_frame_sigmas_batch_impl(ctx, d_src, d_dst, nframes, rows, cols, channels, sigmas, opts);
}

int blur_gaussian_u16_frame_sigmas_pitched_batch_dev(blur_ctx* ctx, const uint16_t* d_src, size_t src_pitch, size_t src_frame_stride, uint16_t* d_dst, size_t dst_pitch,
                    size_t dst_frame_stride, int nframes, int rows, int cols, int channels, const double* sigmas, const blur_opts* opts)
{
    const ChLayout L{ src_pitch, src_frame_stride, dst_pitch, dst_frame_stride };
    return blur_ch_frame_sigmas_batch_impl(ctx, d_src, d_dst, nframes, rows, cols, channels, sigmas, opts, &L);
}

int blur_gaussian_f16_frame_sigmas_batch_dev(blur_ctx* ctx, const uint16_t* d_src, uint16_t* d_dst, int nframes, int rows, int cols, int channels, const double* sigmas,
                    const blur_opts* opts)
{
    return blur_ch_frame_sigmas_batch_impl(ctx, reinterpret_cast<const ff_f16*>(d_src), reinterpret_cast<ff_f16*>(d_dst), nframes, rows, cols, channels, sigmas, opts);
}

int blur_gaussian_f16_frame_sigmas_pitched_batch_dev(blur_ctx* ctx, const uint16_t* d_src, size_t src_pitch, size_t src_frame_stride, uint16_t* d_dst, size_t dst_pitch,
                    size_t dst_frame_stride, int nframes, int rows, int cols, int channels, const double* sigmas, const blur_opts* opts)
{
    const ChLayout L{ src_pitch, src_frame_stride, dst_pitch, dst_frame_stride };
    return blur_ch_frame_sigmas_batch_impl(ctx, reinterpret_cast<const ff_f16*>(d_src), reinterpret_cast<ff_f16*>(d_dst), nframes, rows, cols, channels, sigmas, opts, &L);
}

int blur_gaussian_bf16_frame_sigmas_batch_dev(blur_ctx* ctx, const uint16_t* d_src, uint16_t* d_dst, int nframes, int rows, int cols, int channels, const double* sigmas,
                    const blur_opts* opts)
{
    return blur_ch_frame_sigmas_batch_impl(ctx, reinterpret_cast<const ff_bf16*>(d_src), reinterpret_cast<ff_bf16*>(d_dst), nframes, rows, cols, channels, sigmas, opts);
}

int blur_gaussian_bf16_frame_sigmas_pitched_batch_dev(blur_ctx* ctx, const uint16_t* d_src, size_t src_pitch, size_t src_frame_stride, uint16_t* d_dst, size_t dst_pitch,
                    size_t dst_frame_stride, int nframes, int rows, int cols, int channels, const double* sigmas, const blur_opts* opts)
{
    const ChLayout L{ src_pitch, src_frame_stride, dst_pitch, dst_frame_stride };
    return blur_ch_frame_sigmas_batch_impl(ctx, reinterpret_cast<const ff_bf16*>(d_src), reinterpret_cast<ff_bf16*>(d_dst), nframes, rows, cols, channels, sigmas, opts, &L);
}

int blur_gaussian_nv12_frame_sigmas_batch_dev(blur_ctx* ctx, const uint8_t* d_src_y, const uint8_t* d_src_uv, size_t src_pitch, size_t src_y_frame_stride,
                                              size_t src_uv_frame_stride, uint8_t* d_dst_y, uint8_t* d_dst_uv, size_t dst_pitch, size_t dst_y_frame_stride,
                                              size_t dst_uv_frame_stride, int nframes, int rows, int cols, const double* sigmas, const blur_opts* opts)
{
    return blur_nv_frame_sigmas_batch_impl<uint8_t>(ctx, NvSurface{ d_src_y, d_src_uv, d_dst_y, d_dst_uv, src_pitch, src_y_frame_stride, src_uv_frame_stride, dst_pitch,
                                                    dst_y_frame_stride, dst_uv_frame_stride }, nframes, rows, cols, sigmas, opts);
}

int blur_gaussian_p016_frame_sigmas_batch_dev(blur_ctx* ctx, const uint16_t* d_src_y, const uint16_t* d_src_uv, size_t src_pitch, size_t src_y_frame_stride,
                                              size_t src_uv_frame_stride, uint16_t* d_dst_y, uint16_t* d_dst_uv, size_t dst_pitch, size_t dst_y_frame_stride,
                                              size_t dst_uv_frame_stride, int nframes, int rows, int cols, const double* sigmas, const blur_opts* opts)
{
    return blur_nv_frame_sigmas_batch_impl<uint16_t>(ctx, NvSurface{ d_src_y, d_src_uv, d_dst_y, d_dst_uv, src_pitch, src_y_frame_stride, src_uv_frame_stride, dst_pitch,
                                                    dst_y_frame_stride, dst_uv_frame_stride }, nframes, rows, cols, sigmas, opts);
}

// host-only: how a call with these sigmas groups its frames
int blur_gaussian_frame_sigmas_plan(int rows, int cols, int nframes, const double* sigmas, int* out)
{
    FrameSigmaPlan pl;
    int dummy = 0;
    const char* why = nullptr;
    if (!out) return BLUR_ERR_INVALID;
    if (int rc = frame_sigmas_status(&dummy, &dummy, nframes, rows, cols, 1, sigmas, pl, &why)) return rc;
    for (int f = 0; f < nframes; ++f) {
        const int s = pl.slot_of[f];
        out[4 * f] = s < 0 ? -1 : pl.slots[s].group;
        out[4 * f + 1] = s < 0 ? 0 : pl.slots[s].sz.pad;
        out[4 * f + 2] = s < 0 ? 0 : pl.slots[s].nkb;
        out[4 * f + 3] = s;
    }
    return BLUR_OK;
}

// u8 images, one sigma per channel
int blur_gaussian_u8_sigmas_batch_dev(blur_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int nframes, int rows, int cols, int channels, const double* sigmas,
                                      const blur_opts* opts)
{
    return blur_ch_sigmas_batch_impl(ctx, d_src, d_dst, nframes, rows, cols, channels, sigmas, opts);
}

int blur_gaussian_u8_sigmas_dev(blur_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int rows, int cols, int channels, const double* sigmas, const blur_opts* opts)
{
    return blur_ch_sigmas_batch_impl(ctx, d_src, d_dst, 1, rows, cols, channels, sigmas, opts);
}

int blur_gaussian_u8_sigmas_host(blur_ctx* ctx, const uint8_t* src, uint8_t* dst, int rows, int cols, int channels, const double* sigmas, const blur_opts* opts)
{
    return blur_ch_sigmas_host(ctx, src, dst, rows, cols, channels, sigmas, opts);
}

int blur_gaussian_u8_sigmas_batch_multi_dev(blur_multi* m, const uint8_t* d_src, uint8_t* d_dst, int nframes, int rows, int cols, int channels, const double* sigmas,
                                            const blur_opts* opts)
{
    return blur_ch_sigmas_multi(m, d_src, d_dst, nframes, rows, cols, channels, sigmas, opts, 1);
}

int blur_gaussian_u8_sigmas_batch_multi_host(blur_multi* m, const uint8_t* src, uint8_t* dst, int nframes, int rows, int cols, int channels, const double* sigmas,
                                             const blur_opts* opts)
{
    return blur_ch_sigmas_multi(m, src, dst, nframes, rows, cols, channels, sigmas, opts, 0);
}

// float32 images, one sigma per channel
int blur_gaussian_f32_sigmas_batch_dev(blur_ctx* ctx, const float* d_src, float* d_dst, int nframes, int rows, int cols, int channels, const double* sigmas,
                                       const blur_opts* opts)
{
    return blur_ch_sigmas_batch_impl(ctx, d_src, d_dst, nframes, rows, cols, channels, sigmas, opts);
}

int blur_gaussian_f32_sigmas_dev(blur_ctx* ctx, const float* d_src, float* d_dst, int rows, int cols, int channels, const double* sigmas, const blur_opts* opts)
{
    return blur_ch_sigmas_batch_impl(ctx, d_src, d_dst, 1, rows, cols, channels, sigmas, opts);
}

int blur_gaussian_f32_sigmas_host(blur_ctx* ctx, const float* src, float* dst, int rows, int cols, int channels, const double* sigmas, const blur_opts* opts)
{
    return blur_ch_sigmas_host(ctx, src, dst, rows, cols, channels, sigmas, opts);
}

int blur_gaussian_f32_sigmas_batch_multi_dev(blur_multi* m, const float* d_src, float* d_dst, int nframes, int rows, int cols, int channels, const double* sigmas,
                                             const blur_opts* opts)
{
    return blur_ch_sigmas_multi(m, d_src, d_dst, nframes, rows, cols, channels, sigmas, opts, 1);
}

int blur_gaussian_f32_sigmas_batch_multi_host(blur_multi* m, const float* src, float* dst, int nframes, int rows, int cols, int channels, const double* sigmas,
                                              const blur_opts* opts)
{
    return blur_ch_sigmas_multi(m, src, dst, nframes, rows, cols, channels, sigmas, opts, 0);
}

// u16 images, one sigma per channel
int blur_gaussian_u16_sigmas_batch_dev(blur_ctx* ctx, const uint16_t* d_src, uint16_t* d_dst, int nframes, int rows, int cols, int channels, const double* sigmas,
                                       const blur_opts* opts)
{
    return blur_ch_sigmas_batch_impl(ctx, d_src, d_dst, nframes, rows, cols, channels, sigmas, opts);
}

int blur_gaussian_u16_sigmas_dev(blur_ctx* ctx, const uint16_t* d_src, uint16_t* d_dst, int rows, int cols, int channels, const double* sigmas, const blur_opts* opts)
{
    return blur_ch_sigmas_batch_impl(ctx, d_src, d_dst, 1, rows, cols, channels, sigmas, opts);
}

int blur_gaussian_u16_sigmas_host(blur_ctx* ctx, const uint16_t* src, uint16_t* dst, int rows, int cols, int channels, const double* sigmas, const blur_opts* opts)
{
    return blur_ch_sigmas_host(ctx, src, dst, rows, cols, channels, sigmas, opts);
}

int blur_gaussian_u16_sigmas_batch_multi_dev(blur_multi* m, const uint16_t* d_src, uint16_t* d_dst, int nframes, int rows, int cols, int channels, const double* sigmas,
                                             const blur_opts* opts)
{
    return blur_ch_sigmas_multi(m, d_src, d_dst, nframes, rows, cols, channels, sigmas, opts, 1);
}

int blur_gaussian_u16_sigmas_batch_multi_host(blur_multi* m, const uint16_t* src, uint16_t* dst, int nframes, int rows, int cols, int channels, const double* sigmas,
                                              const blur_opts* opts)
{
    return blur_ch_sigmas_multi(m, src, dst, nframes, rows, cols, channels, sigmas, opts, 0);
}

// float16 (bit patterns) images, one sigma per channel
int blur_gaussian_f16_sigmas_batch_dev(blur_ctx* ctx, const uint16_t* d_src, uint16_t* d_dst, int nframes, int rows, int cols, int channels, const double* sigmas,
                                       const blur_opts* opts)
{
    return blur_ch_sigmas_batch_impl(ctx, reinterpret_cast<const ff_f16*>(d_src), reinterpret_cast<ff_f16*>(d_dst), nframes, rows, cols, channels, sigmas, opts);
}

int blur_gaussian_f16_sigmas_dev(blur_ctx* ctx, const uint16_t* d_src, uint16_t* d_dst, int rows, int cols, int channels, const double* sigmas, const blur_opts* opts)
{
    return blur_ch_sigmas_batch_impl(ctx, reinterpret_cast<const ff_f16*>(d_src), reinterpret_cast<ff_f16*>(d_dst), 1, rows, cols, channels, sigmas, opts);
}

int blur_gaussian_f16_sigmas_host(blur_ctx* ctx, const uint16_t* src, uint16_t* dst, int rows, int cols, int channels, const double* sigmas, const blur_opts* opts)
{
    return blur_ch_sigmas_host(ctx, reinterpret_cast<const ff_f16*>(src), reinterpret_cast<ff_f16*>(dst), rows, cols, channels, sigmas, opts);
}

int blur_gaussian_f16_sigmas_batch_multi_dev(blur_multi* m, const uint16_t* d_src, uint16_t* d_dst, int nframes, int rows, int cols, int channels, const double* sigmas,
                                             const blur_opts* opts)
{
    return blur_ch_sigmas_multi(m, reinterpret_cast<const ff_f16*>(d_src), reinterpret_cast<ff_f16*>(d_dst), nframes, rows, cols, channels, sigmas, opts, 1);
}

int blur_gaussian_f16_sigmas_batch_multi_host(blur_multi* m, const uint16_t* src, uint16_t* dst, int nframes, int rows, int cols, int channels, const double* sigmas,
                                              const blur_opts* opts)
{
    return blur_ch_sigmas_multi(m, reinterpret_cast<const ff_f16*>(src), reinterpret_cast<ff_f16*>(dst), nframes, rows, cols, channels, sigmas, opts, 0);
}

// bfloat16 (bit patterns) images, one sigma per channel
int blur_gaussian_bf16_sigmas_batch_dev(blur_ctx* ctx, const uint16_t* d_src, uint16_t* d_dst, int nframes, int rows, int cols, int channels, const double* sigmas,
                                        const blur_opts* opts)
{
    return blur_ch_sigmas_batch_impl(ctx, reinterpret_cast<const ff_bf16*>(d_src), reinterpret_cast<ff_bf16*>(d_dst), nframes, rows, cols, channels, sigmas, opts);
}

int blur_gaussian_bf16_sigmas_dev(blur_ctx* ctx, const uint16_t* d_src, uint16_t* d_dst, int rows, int cols, int channels, const double* sigmas, const blur_opts* opts)
{
    return blur_ch_sigmas_batch_impl(ctx, reinterpret_cast<const ff_bf16*>(d_src), reinterpret_cast<ff_bf16*>(d_dst), 1, rows, cols, channels, sigmas, opts);
}

int blur_gaussian_bf16_sigmas_host(blur_ctx* ctx, const uint16_t* src, uint16_t* dst, int rows, int cols, int channels, const double* sigmas, const blur_opts* opts)
{
    return blur_ch_sigmas_host(ctx, reinterpret_cast<const ff_bf16*>(src), reinterpret_cast<ff_bf16*>(dst), rows, cols, channels, sigmas, opts);
}

int blur_gaussian_bf16_sigmas_batch_multi_dev(blur_multi* m, const uint16_t* d_src, uint16_t* d_dst, int nframes, int rows, int cols, int channels, const double* sigmas,
                                              const blur_opts* opts)
{
    return blur_ch_sigmas_multi(m, reinterpret_cast<const ff_bf16*>(d_src), reinterpret_cast<ff_bf16*>(d_dst), nframes, rows, cols, channels, sigmas, opts, 1);
}

int blur_gaussian_bf16_sigmas_batch_multi_host(blur_multi* m, const uint16_t* src, uint16_t* dst, int nframes, int rows, int cols, int channels, const double* sigmas,
                                               const blur_opts* opts)
{
    return blur_ch_sigmas_multi(m, reinterpret_cast<const ff_bf16*>(src), reinterpret_cast<ff_bf16*>(dst), nframes, rows, cols, channels, sigmas, opts, 0);
}

int blur_convolve_lines_c32_dev(blur_ctx* ctx, const float* d_in, float* d_out, int nlines, int n, const float* multipliers)
{
    if (!ctx) return BLUR_ERR_INVALID;
    if (!d_in || !d_out || !multipliers || nlines < 0 || n <= 0) return fail(ctx, BLUR_ERR_INVALID, "null pointer or non-positive size");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const WrEntry* e = nullptr;
    for (int role = 0; role < 2 && !e; ++role) {
        const WrEntry* c = find_wr_entry(n, role != 0);
        if (c && c->r0 * kWrS == n) e = c;
    }
    if (!e) return fail(ctx, BLUR_ERR_UNSUPPORTED, "no wave-resident kernel for this length (blur_wr_length)");
    float2* tw0 = nullptr;
    if (int rc = wr_get_tables(ctx, e, &tw0)) return rc;
    // the caller's multiplier tables, cached by content (hash AND a full comparison: a colliding table would give a wrong image
    // silently); at most kLinesCacheMax tables are kept, the least recently used one goes first
    constexpr size_t kLinesCacheMax = 16;
    float* d_m = nullptr;
    const uint64_t h = fnv1a(multipliers, sizeof(float) * n);
    for (auto it = ctx->lines_tables.begin(); it != ctx->lines_tables.end(); ++it) {
        if (it->hash == h && static_cast<int>(it->host.size()) == n && std::memcmp(it->host.data(), multipliers, sizeof(float) * n) == 0) {
            d_m = it->dev;
            ctx->lines_tables.splice(ctx->lines_tables.begin(), ctx->lines_tables, it);      // most recently used first
            break;
        }
    }
    if (!d_m) {
        if (ctx->lines_tables.size() >= kLinesCacheMax) {
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                                   // a launch may still read the table
            (void)hipFree(ctx->lines_tables.back().dev);
            ctx->lines_tables.pop_back();
        }
        // (the tail behind the table is only written by -DWR_STAMPS diagnostic builds, as in wr_get_spectrum)
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&d_m), sizeof(float) * (n + kWrStampTailFloats)));
        if (hipMemset(d_m, 0, sizeof(float) * (n + kWrStampTailFloats)) != hipSuccess ||
            hipMemcpy(d_m, multipliers, sizeof(float) * n, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(d_m);
            return fail(ctx, BLUR_ERR_HIP, "blur_convolve_lines_c32_dev: table upload failed");
        }
        ctx->lines_tables.push_front({ h, std::vector<float>(multipliers, multipliers + n), d_m });
    }
    HIP_TRY(ctx, e->lines(ctx->stream, reinterpret_cast<const float2*>(d_in), reinterpret_cast<float2*>(d_out), nlines, ctx->num_cus, ctx->d_w256, tw0, d_m));
    return BLUR_OK;
}

int blur_mx_fragments(const float* taps, int pad, int nkb, uint16_t* out)
{
    if (!taps || !out || pad < 0 || nkb < mx_nkb(pad)) return BLUR_ERR_INVALID;
    mx_fragments(taps, pad, nkb, out);
    return BLUR_OK;
}

int blur_mx_window_blocks(int pad)
{
    const MxEntry* e = pad >= 0 ? find_entry_for_pad<MxEntry>(pad) : nullptr;
    return e ? e->nkb : 0;
}

int blur_wr_length(int need, int column_role)
{
    const WrEntry* e = find_wr_entry(need, column_role != 0);
    return e ? e->r0 * kWrS : 0;
}

// which kernels the last 8-bit 3-channel blur of this context ran: 0 run-time-planned, 1 specialised rows-first (both passes),
// 2 wave-resident, 3 whole-image 2D transform, 4 two-kernel matrix-core engine, 6 fused matrix-core kernel; -1 none yet
// (bench.py --preset reference-sweep reports it per size)
int blur_debug_last_family(const blur_ctx* ctx) { return ctx ? ctx->last_family : -1; }

int blur_last_engine(const blur_ctx* ctx, char* note, size_t n)
{
    if (!ctx) return -1;
    static const char* const names[] = { "run-time-planned FFT kernels", "specialised rows-first FFT kernels", "wave-resident FFT kernels", "whole-image 2D FFT",
                                         "two-kernel matrix-core engine", "?", "fused matrix-core kernel", "tiled wave-resident FFT kernels" };
    if (note && n > 0) {
        std::string t = ctx->last_family >= 0 && ctx->last_family <= 7 ? names[ctx->last_family] : "none yet";
        if (!ctx->engine_note.empty()) t += " (not taken: " + ctx->engine_note + ")";
        std::snprintf(note, n, "%s", t.c_str());
    }
    return ctx->last_family;
}

// redzone tests: number of bytes of the workspace's two guard bands that were overwritten (0 = intact; -1 = no workspace yet)
int blur_debug_check_workspace_guards(blur_ctx* ctx)
{
    if (!ctx) return -1;
    if (!ctx->work) return -1;
    if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) return -1;
    std::vector<unsigned char> g(2 * kWorkGuard);
    const char* base = reinterpret_cast<const char*>(ctx->work) - kWorkGuard;
    if (hipMemcpy(g.data(), base, kWorkGuard, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (hipMemcpy(g.data() + kWorkGuard, base + kWorkGuard + ctx->work_bytes, kWorkGuard, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    int bad = 0;
    for (unsigned char c : g) bad += c != 0xA5;
    return bad;
}

int blur_debug_read_stamps(blur_ctx* ctx, int n, int role, unsigned long long* out, int count)
{
    if (!ctx || !out) return BLUR_ERR_INVALID;
    auto it = ctx->last_spectrum.find(role < 0 ? -n : 4 * n + role);      // role < 0: the wave-resident kernel of length n
    if (it == ctx->last_spectrum.end() || count * sizeof(unsigned long long) > kStampTailFloats * sizeof(float)) return BLUR_ERR_INVALID;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out, it->second + n, count * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return BLUR_OK;
}

int blur_malloc(blur_ctx* ctx, void** d_ptr, size_t bytes)
{
    if (!ctx || !d_ptr) return BLUR_ERR_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMalloc(d_ptr, bytes ? bytes : 1));
    return BLUR_OK;
}

int blur_host_alloc(blur_ctx* ctx, void** h_ptr, size_t bytes)
{
    if (!ctx || !h_ptr) return BLUR_ERR_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipHostMalloc(h_ptr, bytes ? bytes : 1, hipHostMallocDefault));
    return BLUR_OK;
}

int blur_host_free(blur_ctx* ctx, void* h_ptr)
{
    if (!ctx) return BLUR_ERR_INVALID;
    HIP_TRY(ctx, hipHostFree(h_ptr));
    return BLUR_OK;
}

int blur_free(blur_ctx* ctx, void* d_ptr)
{
    if (!ctx) return BLUR_ERR_INVALID;
    HIP_TRY(ctx, hipFree(d_ptr));
    return BLUR_OK;
}

int blur_memcpy_h2d(blur_ctx* ctx, void* d_dst, const void* src, size_t bytes)
{
    if (!ctx) return BLUR_ERR_INVALID;
    HIP_TRY(ctx, hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return BLUR_OK;
}

int blur_memcpy_d2h(blur_ctx* ctx, void* dst, const void* d_src, size_t bytes)
{
    if (!ctx) return BLUR_ERR_INVALID;
    HIP_TRY(ctx, hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return BLUR_OK;
}

int blur_copy_bandwidth(blur_ctx* ctx, size_t bytes, int reps, double* gbs)
{
    if (!ctx || !gbs || reps <= 0 || bytes < 4096) return BLUR_ERR_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n16 = bytes / 16;
    uint4 *a = nullptr, *b = nullptr;
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&a), n16 * 16));
    if (hipMalloc(reinterpret_cast<void**>(&b), n16 * 16) != hipSuccess) { (void)hipFree(a); return fail(ctx, BLUR_ERR_NOMEM, "blur_copy_bandwidth: out of device memory"); }
    (void)hipMemsetAsync(a, 0x5a, n16 * 16, ctx->stream);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    const int grid = ctx->num_cus * 8;
    hipLaunchKernelGGL(copy16_kernel, dim3(grid), dim3(256), 0, ctx->stream, a, b, n16);
    (void)hipEventRecord(e0, ctx->stream);
    for (int i = 0; i < reps; ++i) hipLaunchKernelGGL(copy16_kernel, dim3(grid), dim3(256), 0, ctx->stream, a, b, n16);
    (void)hipEventRecord(e1, ctx->stream);
    hipError_t err = hipEventSynchronize(e1);
    float ms = 0.f;
    if (err == hipSuccess) err = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipFree(a);
    (void)hipFree(b);
    if (err != hipSuccess || !(ms > 0.f)) return fail(ctx, BLUR_ERR_HIP, "blur_copy_bandwidth: timing failed");
    *gbs = 2.0 * static_cast<double>(n16) * 16.0 * reps / (ms * 1e-3) / 1e9;
    return BLUR_OK;
}

}  // extern "C"
