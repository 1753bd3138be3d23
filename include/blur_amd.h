/*
 * blur_amd.h -- C ABI of the MI355X (gfx950) FFT Gaussian-blur engine.
 *
 * This is the drop-in boundary for ONE hot path of michelerenzullo/Blur_algorithms:
 * the 1D-tiled FFT convolution `pffft_(cv::Mat&, double)` (Source.cpp:429-570) and,
 * for BASELINE config 5, `fastboxblur` (call site Source.cpp:587).  The reference has
 * no FFI of its own (README.md:151-152 "Usage and APIs coming soon"); the entry points
 * below are what a binding for that path would bind: plain pointers and sizes, no C++
 * or torch types.  Each one cites the reference interface it replaces.
 *
 * All device work is hand-written HIP for gfx950 inside libblur_amd.so; there is no
 * CPU fallback: a call that cannot run on the GPU returns an error code.
 *
 * Threading: a blur_ctx is thread-compatible (one call at a time per ctx).  Calls on
 * device pointers are ASYNCHRONOUS on the ctx's stream unless stated otherwise.
 */
#ifndef BLUR_AMD_H
#define BLUR_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BLUR_AMD_VERSION 100

/* status codes (the reference returns void and checks nothing: Utils.hpp:59-65,
   Source.cpp:477-478,612-621) */
enum {
    BLUR_OK = 0,
    BLUR_ERR_INVALID = 1,      /* bad argument (null pointer, non-positive size, sigma <= 0) */
    BLUR_ERR_UNSUPPORTED = 2,  /* pad > min(rows,cols)-1 (UB in the reference, README.md:33-38) or FFT length too long for LDS */
    BLUR_ERR_HIP = 3,          /* a HIP runtime call failed; see blur_last_error() */
    BLUR_ERR_NOMEM = 4
};

typedef struct blur_ctx blur_ctx;

/* blur_opts.engine.  Every engine computes the same blur under the same parity contract (Parity); the choice is
   about speed and about what each engine can hold.  engine.hip: prepare() holds the policy table of BLUR_ENGINE_AUTO. */
enum blur_engine {
    BLUR_ENGINE_AUTO = 0,            /* fused matrix-core kernel where it exists for the kernel's half width (pad <= 72; pad <= 168
                                        on frames of 1 MP and more; any image width, any pointer alignment); else the two-kernel
                                        matrix-core engine (pad <= 168, non-negative taps) except where the FFT engine has a faster
                                        compile-time family (small frames, the widest kernels on 4K frames); else FFT.  The choice
                                        depends on rows, cols and the kernel only: never on the number of frames, on where the
                                        frames lie in memory or on the environment (blur_last_engine() names it) */
    BLUR_ENGINE_FFT_ROWS_FIRST = 1,  /* FFT kernels, never the wave-resident family */
    BLUR_ENGINE_FFT_WAVE_RESIDENT = 2, /* FFT kernels, wave-resident (transform length 256 R0, columns first) wherever the image fits */
    BLUR_ENGINE_MATRIX = 3,          /* two-kernel matrix-core engine (mx_kernels.hpp); BLUR_ERR_UNSUPPORTED if it cannot hold the kernel */
    BLUR_ENGINE_FFT = 5,             /* FFT kernels with their own measured choice of family */
    BLUR_ENGINE_FUSED = 6            /* fused matrix-core kernels (fx_kernels.hpp, pad <= 72; fw_kernels.hpp, pad <= 168); BLUR_ERR_UNSUPPORTED
                                        where they do not apply */
};

/* Options of the whole-image blur.  Zero-initialise, then blur_opts_default(). */
typedef struct blur_opts {
    /* 1 (default): reproduce pffft_sorted_optimized_convolution exactly
       (Source.cpp:420-425): the Nyquist bin, packed in slot 1 of pffft's ordered
       layout, is scaled with the kernel's DC gain.  0: scale it with the kernel's
       Nyquist gain (what pocketfft_1D does, Source.cpp:362,378). */
    int nyquist_quirk;
    /* columns per workgroup of the column pass (0 = auto: 8 or less as LDS allows) */
    int col_group;
    /* 1: use the run-time-planned FFT kernels even where a compile-time specialised one exists (tests) */
    int force_generic;
    /* > 0: frames per launch pair of the batch entry point (0 = auto: as many as fit a 1 GiB float workspace;
       the fused matrix-core engine has no workspace and takes the whole batch in one launch) */
    int frames_per_launch;
    /* 1: keep the FFT engine's float intermediate in row-major planes even when both passes are specialised
       (default: strips of 8 columns stored contiguously) */
    int row_major_planes;
    /* which kernels run the u8c3 blur: one of enum blur_engine; 0 = the library's choice */
    int engine;
    /* tests: > 0 forces the tiled wave-resident path (bands of rows / tiles of columns through the wave-resident kernels, the quirk
       as rank-one terms) with no transform longer than this many points; 0 = the library decides (lines too long for one transform) */
    int tile_points;
    int reserved[1];   /* must be zero */
} blur_opts;

void blur_opts_default(blur_opts* o);

/* ---- host-side sizing: bit-identical replacements, no GPU needed ------------------ */

/* gaussian_window(sigma, max_width)                      Source.cpp:60-73 */
int blur_gaussian_window(double sigma, int max_width);

/* getGaussian(kernel, sigma, width, FFT_length)          Source.cpp:75-102
   kernel must hold max(width, fft_length) floats (width==0 -> gaussian_window(sigma)). */
int blur_get_gaussian(float* kernel, double sigma, int width, int fft_length);

/* isValidSize / nearestTransformSize                     Utils.hpp:141-157 */
int blur_is_valid_size(int n);
int blur_nearest_transform_size(int n);

/* the sizing block of pffft_()                           Source.cpp:434-457
   out = { kSize, pad, sizes[0] (column FFT length), sizes[1] (row FFT length),
           trailing_zeros[0], trailing_zeros[1] } */
int blur_pffft_sizing(int rows, int cols, double sigma, int out[6]);

/* per-bin multiplier kerf[2i]*scaler of Source.cpp:423 for bins 0..n/2 (n/2+1 floats);
   the kernel spectrum is computed on the host in float64 and rounded to float once */
int blur_kernel_multipliers(double sigma, int ksize, int n, float* m);

/* radix sequence the engine uses for a complex FFT of length n (returns the number of
   passes, 0 if n is unsupported); radices[] must hold 16 ints */
int blur_fft_plan_radices(int n, int* radices);

/* ---- context ---------------------------------------------------------------------- */

/* device: HIP device ordinal.  Owns plan/twiddle caches, kernel-spectrum caches and the
   float32 intermediate workspace.  (Role of pffft_new_setup/pffft_destroy_setup,
   Source.cpp:477-478,565-566, which the reference rebuilds on every call.) */
int blur_ctx_create(blur_ctx** out, int device);
int blur_ctx_destroy(blur_ctx* ctx);
/* hipStream_t to launch on (NULL = the default stream).  Switching to a different stream first
   waits for the work queued on the previous one (the workspace is shared). */
int blur_ctx_set_stream(blur_ctx* ctx, void* hip_stream);
int blur_ctx_synchronize(blur_ctx* ctx);
/* message of the last failing call on this ctx ("" if none); ctx may be NULL for
   failures of blur_ctx_create */
const char* blur_last_error(const blur_ctx* ctx);
/* which kernels the last u8c3 blur (or blur_gaussian_u8_*) on this ctx ran on: returns 0 run-time-planned FFT, 1 specialised rows-first
   FFT, 2 wave-resident FFT, 3 whole-image 2D FFT, 4 two-kernel matrix-core engine, 6 fused matrix-core kernel, 7 tiled wave-resident
   FFT (-1: none yet); 1- and 4-channel u8 images and float32 images report 6 (their fused kernel) or 0 (the plane fallback), and it
   writes into note (n bytes, may be NULL) the engine's name and, under BLUR_ENGINE_AUTO, why a faster engine was passed over -- e.g.
   "two-kernel matrix-core engine (not taken: wide fused kernel (pad 73 .. 168): frames below 1 MP run on two kernels or the FFT kernels)" */
int blur_last_engine(const blur_ctx* ctx, char* note, size_t n);

/* Per-kernel timing with HIP events on the ctx's stream.  While enabled, every launch
   of the row-pass and column-pass kernels is bracketed by events; blur_ctx_timing()
   synchronises, then returns the summed milliseconds, the launch counts and the number of
   frames those launches covered (a batch launch processes several frames) since the last
   reset:  out_ms[0]=row pass, out_ms[1]=column pass; the others likewise.  (The fused engine: [0] = the fused kernel,
   [1] = its side kernels per call.)  on = 2 brackets slot 0 only: an event between two kernels keeps the second from
   starting while the first drains, about 3.5 us each on MI355X, and a measurement run may want to pay that once per call. */
int blur_ctx_timing_enable(blur_ctx* ctx, int on);
int blur_ctx_timing(blur_ctx* ctx, double out_ms[2], int out_launches[2], int out_frames[2], int reset);

/* ---- the hot path: pffft_(image, sigma)             Source.cpp:429-570 ------------- */

/* One BGR/RGB u8 frame, interleaved, rows*cols*3 bytes contiguous (cv::Mat::data of
   Source.cpp:459-461,567), DEVICE pointers.  dst may equal src (the reference works in
   place).  Asynchronous on the ctx's stream. */
int blur_gaussian_u8c3_dev(blur_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst,
                           int rows, int cols, double sigma, const blur_opts* opts);

/* nframes frames of identical shape stored back to back (frame stride rows*cols*3). */
int blur_gaussian_u8c3_batch_dev(blur_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int nframes,
                                 int rows, int cols, double sigma, const blur_opts* opts);

/* One float32 plane (the per-channel body Source.cpp:510-564; BASELINE config 1). */
int blur_gaussian_f32c1_dev(blur_ctx* ctx, const float* d_src, float* d_dst,
                            int rows, int cols, double sigma, const blur_opts* opts);

/* 1-, 3- or 4-channel u8 frames (grayscale, BGR, BGRA / RGBA), interleaved, rows*cols*channels bytes per frame, nframes back to
   back, DEVICE pointers.  Every channel is blurred on its own exactly as pffft_() blurs one of its three (Source.cpp:510-564: sizing
   and kernel from (rows, cols, sigma), reflect-101, the Nyquist-slot quirk per channel plane, + 0.5f truncation); the alpha channel
   is blurred like the others.  channels == 3 is blur_gaussian_u8c3_batch_dev.  channels 1 and 4: opts->engine AUTO takes the
   fused matrix-core kernel wherever it applies (pad <= 168 and the fused engine's frame limits: everywhere the u8c3 call on the
   same frame and sigma takes it, and also where that call prefers an FFT family), the f32 plane path per channel elsewhere;
   FUSED fails with BLUR_ERR_UNSUPPORTED where the fused kernel does not apply; FFT always takes the plane path; other engines
   are BLUR_ERR_UNSUPPORTED.  d_dst may equal d_src; other overlaps are detected over the whole batch and read from a copy.
   BLUR_ERR_INVALID: channels not in {1, 3, 4}, a NULL pointer, nframes < 0, rows, cols or sigma <= 0; BLUR_ERR_UNSUPPORTED: pad >
   min(rows, cols) - 1.  These are checked before the device is touched (ctx may then be NULL); nframes == 0 is a no-op. */
int blur_gaussian_u8_batch_dev(blur_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int nframes, int rows, int cols, int channels,
                               double sigma, const blur_opts* opts);
int blur_gaussian_u8_dev(blur_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int rows, int cols, int channels, double sigma,
                         const blur_opts* opts);
/* the same for one frame in HOST memory: copy in, blur, copy out, synchronise */
int blur_gaussian_u8_host(blur_ctx* ctx, const uint8_t* src, uint8_t* dst, int rows, int cols, int channels, double sigma,
                          const blur_opts* opts);

/* float32 frames of 1, 3 or 4 channels, interleaved, rows*cols*channels floats per frame, nframes back to back, DEVICE pointers
   (4-byte aligned; any float offset).  Every channel is blurred on its own exactly as pffft_() blurs one of its planes (sizing and
   kernel from (rows, cols, sigma), reflect-101, the Nyquist-slot quirk per channel plane unless opts->nyquist_quirk = 0) and the
   result is the float plane as blur_gaussian_f32c1_dev returns it: no + 0.5f truncation, no clamping.  Parity: |got - float64
   reference| <= 1e-6 max|x| of the frame, per pixel and channel, under AUTO and FFT.  opts->engine AUTO takes the fused matrix-core
   kernel for pad <= 104 (frames of at most 4 GiB - 4 KiB), the f32 plane path per channel elsewhere; FUSED runs the fused kernel
   wherever one exists (pad <= 168; pad 153 .. 168 for 1 channel only) and fails with BLUR_ERR_UNSUPPORTED elsewhere: for pad
   105 .. 168 it is outside the parity bound where the output is as large as max|x| over an area (measured 1.19e-6 max|x| on step
   images; within the bound on noise), which is why AUTO does not take it there; FFT always takes the plane path, which scales each frame by a power of two as the fused
   kernel does (measured within the bound from max|x| = 0.7e-37 to 0.7e37); other
   engines are BLUR_ERR_UNSUPPORTED.  blur_last_engine reports 6 (fused) or 0 (plane path).  The call is asynchronous on the
   context's stream.  Results are bit-reproducible: a frame gives the same bits alone and inside a batch.  d_dst may equal d_src;
   other overlaps are detected over the whole batch and read from a copy.  Inputs holding NaN or +-Inf give unspecified output
   values (no kernel reads or writes outside its buffers).  BLUR_ERR_INVALID: channels not in {1, 3, 4}, a NULL pointer,
   nframes < 0, rows, cols or sigma <= 0; BLUR_ERR_UNSUPPORTED: pad > min(rows, cols) - 1.  These are checked before the device is
   touched (ctx may then be NULL); nframes == 0 is a no-op. */
int blur_gaussian_f32_batch_dev(blur_ctx* ctx, const float* d_src, float* d_dst, int nframes, int rows, int cols, int channels,
                                double sigma, const blur_opts* opts);
int blur_gaussian_f32_dev(blur_ctx* ctx, const float* d_src, float* d_dst, int rows, int cols, int channels, double sigma,
                          const blur_opts* opts);
/* the same for one frame in HOST memory: copy in, blur, copy out, synchronise */
int blur_gaussian_f32_host(blur_ctx* ctx, const float* src, float* dst, int rows, int cols, int channels, double sigma,
                           const blur_opts* opts);

/* u16 frames (16-bit PNG / TIFF, camera RAW, depth maps: CV_16U) of 1, 3 or 4 channels, interleaved, rows*cols*channels samples
   per frame, nframes back to back, DEVICE pointers (2-byte aligned; any element offset, so a pointer need not be 4-byte aligned).
   Every channel is blurred on its own exactly as pffft_() blurs one of its planes (sizing and kernel from (rows, cols, sigma),
   reflect-101, the Nyquist-slot quirk per channel plane unless opts->nyquist_quirk = 0).  With v the float plane (what
   blur_gaussian_f32_* returns for the same frame widened to float) the output sample is
       (uint16_t)((uint32_t)(int32_t)(v + 0.5f) & 0xffff)
   the reference's interleave_BGR<T, U> rule (Utils.hpp:186-210) with T = uint16_t: add 0.5, truncate towards zero, keep the low 16
   bits.  NO clamping: with the quirk on, full-scale content leaves the range on both sides and wraps (a constant 65535 frame can
   come out as 250, a 0 / 65533 step as 65363), as u8 output wraps at 255.5.  The alpha channel is blurred like the others;
   channels == 3 has no shortcut to a u8c3 path.  Parity: the sample equals the rule applied to the float64 reference plane,
   except where that plane + 0.5 lies within 1e-6 * 65535 + 2^-9 = 0.0675 of an integer (the float entry's bound at full scale,
   plus half a float32 ulp at 65535); there it may be one level off (modulo 65536).  opts->engine as for blur_gaussian_f32_*: AUTO
   takes the fused matrix-core kernel for pad <= 104 (frames of at most 4 GiB - 4 KiB), the f32 plane path per channel
   elsewhere; FUSED runs the fused kernel wherever one exists (pad <= 168, every channel count) and fails with
   BLUR_ERR_UNSUPPORTED elsewhere: for pad 105 .. 168 it shares the float kernel's f32-accumulator rounding, outside the parity bound
   where the output is near full scale over an area (steps, constants), which is why AUTO does not take it there; FFT always
   takes the plane path; other engines are BLUR_ERR_UNSUPPORTED.  blur_last_engine reports 6 (fused) or 0 (plane path).  The call
   is asynchronous on the context's stream.  Results are bit-reproducible: a frame gives the same bits alone and inside a batch
   (the scale is a constant of the call, 2^e with 65535 B 2^e in [2^13, 2^14), not the frame's maximum; the quirk's sums are
   integers held in doubles, exact in any order).  d_dst may equal d_src; other overlaps are detected over the whole batch and
   read from a copy.  BLUR_ERR_INVALID: channels not in {1, 3, 4}, a NULL pointer, nframes < 0, rows, cols or sigma <= 0;
   BLUR_ERR_UNSUPPORTED: pad > min(rows, cols) - 1.  These are checked before the device is touched (ctx may then be NULL);
   nframes == 0 is a no-op. */
int blur_gaussian_u16_batch_dev(blur_ctx* ctx, const uint16_t* d_src, uint16_t* d_dst, int nframes, int rows, int cols, int channels,
                                double sigma, const blur_opts* opts);
int blur_gaussian_u16_dev(blur_ctx* ctx, const uint16_t* d_src, uint16_t* d_dst, int rows, int cols, int channels, double sigma,
                          const blur_opts* opts);
/* the same for one frame in HOST memory: copy in, blur, copy out, synchronise */
int blur_gaussian_u16_host(blur_ctx* ctx, const uint16_t* src, uint16_t* dst, int rows, int cols, int channels, double sigma,
                           const blur_opts* opts);

/* float16 (IEEE binary16: blur_gaussian_f16_*) and bfloat16 (blur_gaussian_bf16_*) frames of 1, 3 or 4 channels, interleaved,
   rows*cols*channels samples per frame, nframes back to back, DEVICE pointers to the samples' BIT PATTERNS (this header is C and
   has no 16-bit floating type: pass a torch.float16 / torch.bfloat16 tensor's data pointer, an _Float16 or __bf16 array; 2-byte
   aligned, any element offset).  Every channel is blurred on its own exactly as pffft_() blurs one of its planes (sizing and
   kernel from (rows, cols, sigma), reflect-101, the Nyquist-slot quirk per channel plane unless opts->nyquist_quirk = 0).  With v
   the float plane (what blur_gaussian_f32_* computes for the same frame widened to float, which is exact for both types) the
   output sample is v rounded ONCE to the sample type, to nearest even: binary16 as the float -> half conversion defines it
   (subnormals kept, |v| past 65504 becomes +-Inf: with the quirk on, a frame near the type's largest value can overflow);
   bfloat16 likewise (8 significant bits, float32's range).  No clamping and no + 0.5.  Parity: with ref the float64 reference plane,
   m = max|x| of the frame and tol = 1e-6 m (the float entry's bound), the sample lies in [RN(ref - tol), RN(ref + tol)], RN the
   rounding to the sample type; where the two ends are equal the sample is exactly the correctly rounded reference.  The frame is
   scaled by a power of two taken from its own max|x| (found on the device, nothing waits for the host), as a float frame is.
   opts->engine as for blur_gaussian_f32_*: AUTO takes the fused matrix-core kernel for pad <= 104 (frames of at most 4 GiB - 4 KiB)
   and the f32 plane path per channel elsewhere; FUSED runs the fused kernel wherever one exists (pad <= 168, every channel count)
   and fails with BLUR_ERR_UNSUPPORTED elsewhere; FFT always takes the plane path; other engines are BLUR_ERR_UNSUPPORTED.
   blur_last_engine reports 6 (fused) or 0 (plane path).  The call is asynchronous on the context's stream.  Results are
   bit-reproducible: a frame gives the same bits alone and inside a batch.  d_dst may equal d_src; other overlaps are detected
   over the whole batch and read from a copy.  NaN or +-Inf in the input: unspecified values in that frame, no fault.
   BLUR_ERR_INVALID: channels not in {1, 3, 4}, a NULL pointer, nframes < 0, rows, cols or sigma <= 0; BLUR_ERR_UNSUPPORTED:
   pad > min(rows, cols) - 1.  These are checked before the device is touched (ctx may then be NULL); nframes == 0 is a no-op. */
int blur_gaussian_f16_batch_dev(blur_ctx* ctx, const uint16_t* d_src, uint16_t* d_dst, int nframes, int rows, int cols, int channels,
                                double sigma, const blur_opts* opts);
int blur_gaussian_f16_dev(blur_ctx* ctx, const uint16_t* d_src, uint16_t* d_dst, int rows, int cols, int channels, double sigma,
                          const blur_opts* opts);
/* the same for one frame in HOST memory: copy in, blur, copy out, synchronise */
int blur_gaussian_f16_host(blur_ctx* ctx, const uint16_t* src, uint16_t* dst, int rows, int cols, int channels, double sigma,
                           const blur_opts* opts);
int blur_gaussian_bf16_batch_dev(blur_ctx* ctx, const uint16_t* d_src, uint16_t* d_dst, int nframes, int rows, int cols, int channels,
                                 double sigma, const blur_opts* opts);
int blur_gaussian_bf16_dev(blur_ctx* ctx, const uint16_t* d_src, uint16_t* d_dst, int rows, int cols, int channels, double sigma,
                           const blur_opts* opts);
int blur_gaussian_bf16_host(blur_ctx* ctx, const uint16_t* src, uint16_t* dst, int rows, int cols, int channels, double sigma,
                            const blur_opts* opts);

/* HOST pointers: copy in, blur, copy out, synchronise (what a cv::Mat caller needs). */
int blur_gaussian_u8c3_host(blur_ctx* ctx, const uint8_t* src, uint8_t* dst,
                            int rows, int cols, double sigma, const blur_opts* opts);
int blur_gaussian_f32c1_host(blur_ctx* ctx, const float* src, float* dst,
                             int rows, int cols, double sigma, const blur_opts* opts);
/* nframes frames back to back in host memory (a video-style caller: the loop around pffft_() in Test(),
   Source.cpp:627-635, with the frames of a clip instead of sigmas).  Frame i+1 is copied to the device and frame i-1
   back while frame i is in the kernels; with pinned host memory (blur_host_alloc) the copies run at PCIe rate in both
   directions at once, with pageable memory the call is still correct but the copies serialise.  src == dst allowed.
   Synchronous. */
int blur_gaussian_u8c3_host_batch(blur_ctx* ctx, const uint8_t* src, uint8_t* dst, int nframes,
                                  int rows, int cols, double sigma, const blur_opts* opts);
/* the same for images whose rows are src_pitch / dst_pitch BYTES apart (cv::Mat::step of a ROI or
   of a padded Mat; pffft_() itself assumes image.data is continuous, Source.cpp:459-461) */
int blur_gaussian_u8c3_host_pitched(blur_ctx* ctx, const uint8_t* src, size_t src_pitch, uint8_t* dst, size_t dst_pitch,
                                    int rows, int cols, double sigma, const blur_opts* opts);

/* Row pass only (Source.cpp:520-537): u8c3 frame -> three float planes, row-major
   (what `resf` holds at Source.cpp:536).  d_planes: 3*rows*cols floats.  For tests. */
int blur_rowpass_u8c3_dev(blur_ctx* ctx, const uint8_t* d_src, float* d_planes,
                          int rows, int cols, double sigma, const blur_opts* opts);

/* ---- other separable kernels on the same engine ------------------ */

/* Any symmetric separable kernel instead of getGaussian(): taps[ksize] (HOST pointer, odd ksize,
   centre tap in the middle, taps[i] == taps[ksize-1-i] so the spectrum is real, Source.cpp:419),
   reflect-101 padding of `pad` pixels (>= ksize/2 for a linear convolution); the FFT lengths
   follow Source.cpp:445-457 from pad.  Device frame pointers, asynchronous. */
int blur_separable_u8c3_dev(blur_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int rows, int cols,
                            const float* taps, int ksize, int pad, const blur_opts* opts);

/* The `#define boxblur` mode of pffft_() (Source.cpp:437-442,468-472): FFT-domain tent kernel
   box_kernel(nsmooth^2) with passes = 2 padding. */
int blur_boxfft_u8c3_dev(blur_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int rows, int cols,
                         double nsmooth, const blur_opts* opts);
/* its sizing: out = { kLen, pad, sizes[0], sizes[1] }                     Source.cpp:437-457 */
int blur_boxfft_sizing(int rows, int cols, double nsmooth, int out[4]);
/* box_kernel(kernel, kLen, FFT_length), 1D form: fft_length floats (host)  Source.cpp:129-140 */
int blur_box_kernel(float* kernel, int klen, int fft_length);

/* ---- pocketfft_2D: the whole padded image as ONE 2D transform      Source.cpp:143-277 ---- */

/* its sizing: out = { kSize, pad, sizes[0], sizes[1], border top, bottom, left, right }   Source.cpp:149-176
   (extra padding for a 2^a 3^b 5^c side goes into the reflect-101 borders of that axis: floor before, ceil after) */
int blur_pocketfft2d_sizing(int rows, int cols, double sigma, int out[8]);
/* pocketfft_2D(image, sigma): Reflect_101 on four sides, deinterleave, r2c over both axes, multiply by
   Re(kerf_1D_row[j]) Re(kerf_1D_col[i]), c2r with 1/ndata, interleave ("+0.5f, truncate"), crop   (:178-276).
   dft_image != 0 builds the `#define DFT_image` variant instead (:235-252): every plane of the result is the
   fft-shifted log spectrum 20 log10(|Re F| + 1e-5) of the padded plane, read with the reference's index arithmetic,
   then interleaved and cropped like the blur.  d_planes (optional, may be NULL): the cropped float planes
   [3][rows][cols] before the "+0.5f, truncate".  d_dst may equal d_src.  Asynchronous on the context's stream.
   In exact arithmetic the blur equals blur_gaussian_u8c3_dev with nyquist_quirk = 0, which is several times faster
   (two fused kernels instead of six); this entry point exists for the spectrum image and for callers who want the
   reference's 2D structure (its sizes and borders) reproduced step by step.
   BLUR_ERR_UNSUPPORTED when a border exceeds dim - 1 (Reflect_101 clamps there, Utils.hpp:217-220, and the
   reference's own buffers stop agreeing) or a side does not fit the LDS (about 19000). */
int blur_pocketfft2d_u8c3_dev(blur_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int rows, int cols, double sigma,
                              int dft_image, float* d_planes);
int blur_pocketfft2d_u8c3_host(blur_ctx* ctx, const uint8_t* src, uint8_t* dst, int rows, int cols, double sigma, int dft_image);

/* ---- the pieces either side of it -------------------------------------------------- */

/* Reflect_101<uint8_t, C>(input, output, top, bottom, left, right, original_size)       Utils.hpp:212-243
   borders are clamped to dim - 1 like the reference; out_size = { rows + top + bottom, cols + left + right } after the
   clamp (d_out == NULL: size query only).  Out of place. */
int blur_reflect101_u8_dev(blur_ctx* ctx, const uint8_t* d_in, uint8_t* d_out, int rows, int cols, int channels,
                           int top, int bottom, int left, int right, int out_size[2]);

/* flip_block<float,1>(in, out, w, h): out[x*h+y] = in[y*w+x]     call sites Source.cpp:540,562 */
int blur_flip_block_f32_dev(blur_ctx* ctx, const float* d_in, float* d_out, int w, int h);

/* deinterleave_BGR<uint8_t,float> / interleave_BGR<uint8_t,float>   Utils.hpp:159-210
   d_planes: 3 planes of `total` floats, back to back. */
int blur_deinterleave_bgr_u8_f32_dev(blur_ctx* ctx, const uint8_t* d_in, float* d_planes, uint32_t total);
int blur_interleave_bgr_f32_u8_dev(blur_ctx* ctx, const float* d_planes, uint8_t* d_out, uint32_t total);

/* fastboxblur(in, w, h, channels, ksize, passes), in place     call site Source.cpp:587 */
int blur_fastboxblur_u8_dev(blur_ctx* ctx, uint8_t* d_inout, int w, int h, int channels,
                            int ksize, int passes);
int blur_fastboxblur_u8_host(blur_ctx* ctx, uint8_t* inout, int w, int h, int channels,
                             int ksize, int passes);

/* fastboxblur over a batch of nframes frames stored back to back (stride w*h*channels bytes), in place; every frame is
   blurred on its own (reflect-101 at its own borders), byte for byte what nframes single calls give.  The batch runs in
   chunks of whole frames: as many as fit under 2^31 bytes (the kernels' 32-bit offsets), under 65535*8 rows and under a cap
   of 128 MiB that keeps the intermediate image between the horizontal and the vertical sweeps in the Infinity Cache (DESIGN.md
   section 5); a frame larger than that is a chunk of its own.  Per chunk, with passes <= 3 on the integer matrix cores, two
   launches: horizontal in -> scratch, vertical scratch -> in.  The ctx's scratch is sized per chunk, not per batch.
   BLUR_ERR_INVALID: nframes < 0, a non-positive w / h / channels / ksize, passes < 0, nframes*w*h*channels overflowing,
   w*channels above INT_MAX, or a null pointer with nframes > 0.  nframes == 0 is a no-op.
     ..._batch_dev : DEVICE memory, asynchronous on the ctx's stream;
     ..._host_batch: HOST memory, synchronous: each chunk is copied in, blurred and copied out through the ctx's staging buffer. */
int blur_fastboxblur_u8_batch_dev(blur_ctx* ctx, uint8_t* d_inout, int nframes, int w, int h, int channels,
                                  int ksize, int passes);
int blur_fastboxblur_u8_host_batch(blur_ctx* ctx, uint8_t* inout, int nframes, int w, int h, int channels,
                                   int ksize, int passes);
/* host-only plan of the call above (no GPU needed; the same host code the batch entries use):
   out = { frames_per_chunk, chunks, vertical_on_matrix_cores (0/1), horizontal_on_matrix_cores (0/1) }.  A flag is 1 when that
   direction has sweeps to do (passes > 0, a box wider than one pixel after clamping r to w-1 / h-1) and they all run on the
   matrix cores; 0 means the accumulator kernels.  The vertical kernel declines (per frame) r > 56, w*channels not a multiple of
   4, h < passes*delta + 32 (delta = 24 for r <= 24, 56 for r <= 56; passes counted up to 3) and frames of 2^31 bytes or more;
   the horizontal ones decline r > 56 for three channels and channels*r > 120 otherwise, rows under 128 bytes,
   rows not a multiple of 4 bytes (other than three channels), channel counts other than 1/3/4.  4-byte aligned pointers assumed.
   BLUR_ERR_INVALID on the arguments the batch entries refuse (or a null `out`). */
int blur_fastboxblur_batch_plan(int nframes, int w, int h, int channels, int ksize, int passes, int out[4]);

/* ---- several GPUs behind one handle (SURVEY.md 8(b) S1 "ctx owning a device list", 8(e)) -------------------------------
   Frames are independent (Source.cpp:510 runs even the channels serially; the reference's only parallelism is
   hybrid_loop over tiles, Utils.hpp:16-55), so a batch shards by frame with no exchange: shard r of S takes frames
   [n r / S, n (r + 1) / S), has its own context (plans and kernel spectra are deterministic host code: nothing to
   broadcast) and its own stream; one host thread drives all of them.  `devices` may repeat an ordinal (several logical
   shards on one GPU).  Both calls are SYNCHRONOUS.
     ..._multi_dev : frames in the memory of devices[0]; shards on other GPUs receive and return their frames by peer
                     copies over xGMI (point to point: no ring, nothing to reduce), shards on devices[0] work in place;
     ..._multi_host: frames in host memory (blur_host_alloc for DMA without staging); every shard copies its own slice. */
typedef struct blur_multi blur_multi;
int blur_multi_create(blur_multi** out, const int* devices, int ndevices);
int blur_multi_destroy(blur_multi* m);
int blur_multi_shards(const blur_multi* m);
const char* blur_multi_last_error(const blur_multi* m);
int blur_gaussian_u8c3_batch_multi_dev(blur_multi* m, const uint8_t* d_src, uint8_t* d_dst, int nframes, int rows, int cols,
                                       double sigma, const blur_opts* opts);
int blur_gaussian_u8c3_batch_multi_host(blur_multi* m, const uint8_t* src, uint8_t* dst, int nframes, int rows, int cols,
                                        double sigma, const blur_opts* opts);
/* blur_gaussian_u8_batch_dev over a batch, sharded by frame exactly like the two calls above */
int blur_gaussian_u8_batch_multi_dev(blur_multi* m, const uint8_t* d_src, uint8_t* d_dst, int nframes, int rows, int cols, int channels,
                                     double sigma, const blur_opts* opts);
int blur_gaussian_u8_batch_multi_host(blur_multi* m, const uint8_t* src, uint8_t* dst, int nframes, int rows, int cols, int channels,
                                      double sigma, const blur_opts* opts);
/* blur_gaussian_f32_batch_dev over a batch, sharded by frame exactly like the calls above */
int blur_gaussian_f32_batch_multi_dev(blur_multi* m, const float* d_src, float* d_dst, int nframes, int rows, int cols, int channels,
                                      double sigma, const blur_opts* opts);
int blur_gaussian_f32_batch_multi_host(blur_multi* m, const float* src, float* dst, int nframes, int rows, int cols, int channels,
                                       double sigma, const blur_opts* opts);
/* blur_gaussian_u16_batch_dev over a batch, sharded by frame exactly like the calls above */
int blur_gaussian_u16_batch_multi_dev(blur_multi* m, const uint16_t* d_src, uint16_t* d_dst, int nframes, int rows, int cols, int channels,
                                      double sigma, const blur_opts* opts);
int blur_gaussian_u16_batch_multi_host(blur_multi* m, const uint16_t* src, uint16_t* dst, int nframes, int rows, int cols, int channels,
                                       double sigma, const blur_opts* opts);
/* blur_gaussian_f16_batch_dev / blur_gaussian_bf16_batch_dev over a batch, sharded by frame exactly like the calls above */
int blur_gaussian_f16_batch_multi_dev(blur_multi* m, const uint16_t* d_src, uint16_t* d_dst, int nframes, int rows, int cols, int channels,
                                      double sigma, const blur_opts* opts);
int blur_gaussian_f16_batch_multi_host(blur_multi* m, const uint16_t* src, uint16_t* dst, int nframes, int rows, int cols, int channels,
                                       double sigma, const blur_opts* opts);
int blur_gaussian_bf16_batch_multi_dev(blur_multi* m, const uint16_t* d_src, uint16_t* d_dst, int nframes, int rows, int cols, int channels,
                                       double sigma, const blur_opts* opts);
int blur_gaussian_bf16_batch_multi_host(blur_multi* m, const uint16_t* src, uint16_t* dst, int nframes, int rows, int cols, int channels,
                                        double sigma, const blur_opts* opts);
/* ---- one sigma per channel ---------------------------------------------------------------------------------------------
   The _sigmas_ entries take `const double sigmas[channels]` where the entries above take `double sigma` (a Lab or YCrCb image whose
   luminance and colour channels want different blurs; BGRA whose alpha is to stay as it is).
     sigmas[c] > 0   channel c of the result is, bit for bit, channel c of what the scalar entry of the same type returns for sigma =
                     sigmas[c] with the same opts (for float32, float16 and bfloat16 the frame's power-of-two scale still comes from
                     max|x| over the whole frame).  The one exception is u8 with three channels, where the scalar call runs other
                     kernels (the u8c3 policy): there the channel meets the same float64 oracle under the same tie rule.
     sigmas[c] == 0  channel c is copied bit for bit; an in-place call does not touch it.  All zeros: a copy of the batch.
   All positive entries equal and no zero: the call IS the scalar entry (u8 with three channels: blur_gaussian_u8c3_batch_dev).
   Otherwise the channels are grouped by sigma and opts->engine applies per group: AUTO gives a group the fused kernel wherever
   the scalar entry's rules give it to that sigma (u8 with three channels: wherever the 1- and 4-channel rules do) and the f32
   plane path elsewhere; FUSED fails with BLUR_ERR_UNSUPPORTED if any group has no fused kernel; FFT takes the plane path for every
   group.  After the call blur_last_engine returns family 6 if every blurred group ran on the fused kernel and 0 otherwise, the note
   naming the groups on the plane path.  Any overlap of source and destination, in place included, is read from one copy.
   BLUR_ERR_INVALID: channels not in {1, 3, 4}, a NULL pointer (sigmas included), nframes < 0, rows or cols <= 0, a negative, NaN or
   infinite sigma; BLUR_ERR_UNSUPPORTED: an entry whose pad exceeds min(rows, cols) - 1.  Every entry is checked before the device
   is touched (ctx may then be NULL) and before anything is written; nframes == 0 is a no-op.  The f16 / bf16 entries take the
   samples' bit patterns, as the scalar ones.  _batch_multi_: sharded by frame like the scalar calls.
   Cost (DESIGN.md 2.5 has the measurements): the call is cheaper than what it replaces, one scalar call per distinct sigma into a
   temporary and a gather of one channel from each, and with two or more distinct sigmas cheaper than those scalar calls alone.
   It is NOT cheaper than one scalar call: with one distinct sigma beside zeros it costs about one scalar call (4 channels), and
   for u8 with three channels more than one -- (0, s, s) with a narrow window (pad <= 72) takes about 1.4 times the u8c3 call
   with s, whose kernel blurs three channels per workgroup where this path blurs one. */
int blur_gaussian_u8_sigmas_batch_dev(blur_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int nframes, int rows, int cols, int channels,
                                      const double* sigmas, const blur_opts* opts);
int blur_gaussian_u8_sigmas_dev(blur_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int rows, int cols, int channels,
                                const double* sigmas, const blur_opts* opts);
int blur_gaussian_u8_sigmas_host(blur_ctx* ctx, const uint8_t* src, uint8_t* dst, int rows, int cols, int channels,
                                 const double* sigmas, const blur_opts* opts);
int blur_gaussian_u8_sigmas_batch_multi_dev(blur_multi* m, const uint8_t* d_src, uint8_t* d_dst, int nframes, int rows, int cols, int channels,
                                            const double* sigmas, const blur_opts* opts);
int blur_gaussian_u8_sigmas_batch_multi_host(blur_multi* m, const uint8_t* src, uint8_t* dst, int nframes, int rows, int cols, int channels,
                                             const double* sigmas, const blur_opts* opts);
int blur_gaussian_f32_sigmas_batch_dev(blur_ctx* ctx, const float* d_src, float* d_dst, int nframes, int rows, int cols, int channels,
                                       const double* sigmas, const blur_opts* opts);
int blur_gaussian_f32_sigmas_dev(blur_ctx* ctx, const float* d_src, float* d_dst, int rows, int cols, int channels,
                                 const double* sigmas, const blur_opts* opts);
int blur_gaussian_f32_sigmas_host(blur_ctx* ctx, const float* src, float* dst, int rows, int cols, int channels,
                                  const double* sigmas, const blur_opts* opts);
int blur_gaussian_f32_sigmas_batch_multi_dev(blur_multi* m, const float* d_src, float* d_dst, int nframes, int rows, int cols, int channels,
                                             const double* sigmas, const blur_opts* opts);
int blur_gaussian_f32_sigmas_batch_multi_host(blur_multi* m, const float* src, float* dst, int nframes, int rows, int cols, int channels,
                                              const double* sigmas, const blur_opts* opts);
int blur_gaussian_u16_sigmas_batch_dev(blur_ctx* ctx, const uint16_t* d_src, uint16_t* d_dst, int nframes, int rows, int cols, int channels,
                                       const double* sigmas, const blur_opts* opts);
int blur_gaussian_u16_sigmas_dev(blur_ctx* ctx, const uint16_t* d_src, uint16_t* d_dst, int rows, int cols, int channels,
                                 const double* sigmas, const blur_opts* opts);
int blur_gaussian_u16_sigmas_host(blur_ctx* ctx, const uint16_t* src, uint16_t* dst, int rows, int cols, int channels,
                                  const double* sigmas, const blur_opts* opts);
int blur_gaussian_u16_sigmas_batch_multi_dev(blur_multi* m, const uint16_t* d_src, uint16_t* d_dst, int nframes, int rows, int cols, int channels,
                                             const double* sigmas, const blur_opts* opts);
int blur_gaussian_u16_sigmas_batch_multi_host(blur_multi* m, const uint16_t* src, uint16_t* dst, int nframes, int rows, int cols, int channels,
                                              const double* sigmas, const blur_opts* opts);
int blur_gaussian_f16_sigmas_batch_dev(blur_ctx* ctx, const uint16_t* d_src, uint16_t* d_dst, int nframes, int rows, int cols, int channels,
                                       const double* sigmas, const blur_opts* opts);
int blur_gaussian_f16_sigmas_dev(blur_ctx* ctx, const uint16_t* d_src, uint16_t* d_dst, int rows, int cols, int channels,
                                 const double* sigmas, const blur_opts* opts);
int blur_gaussian_f16_sigmas_host(blur_ctx* ctx, const uint16_t* src, uint16_t* dst, int rows, int cols, int channels,
                                  const double* sigmas, const blur_opts* opts);
int blur_gaussian_f16_sigmas_batch_multi_dev(blur_multi* m, const uint16_t* d_src, uint16_t* d_dst, int nframes, int rows, int cols, int channels,
                                             const double* sigmas, const blur_opts* opts);
int blur_gaussian_f16_sigmas_batch_multi_host(blur_multi* m, const uint16_t* src, uint16_t* dst, int nframes, int rows, int cols, int channels,
                                              const double* sigmas, const blur_opts* opts);
int blur_gaussian_bf16_sigmas_batch_dev(blur_ctx* ctx, const uint16_t* d_src, uint16_t* d_dst, int nframes, int rows, int cols, int channels,
                                        const double* sigmas, const blur_opts* opts);
int blur_gaussian_bf16_sigmas_dev(blur_ctx* ctx, const uint16_t* d_src, uint16_t* d_dst, int rows, int cols, int channels,
                                  const double* sigmas, const blur_opts* opts);
int blur_gaussian_bf16_sigmas_host(blur_ctx* ctx, const uint16_t* src, uint16_t* dst, int rows, int cols, int channels,
                                   const double* sigmas, const blur_opts* opts);
int blur_gaussian_bf16_sigmas_batch_multi_dev(blur_multi* m, const uint16_t* d_src, uint16_t* d_dst, int nframes, int rows, int cols, int channels,
                                              const double* sigmas, const blur_opts* opts);
int blur_gaussian_bf16_sigmas_batch_multi_host(blur_multi* m, const uint16_t* src, uint16_t* dst, int nframes, int rows, int cols, int channels,
                                               const double* sigmas, const blur_opts* opts);
/* ---- pitched frames and regions of interest, DEVICE pointers ---------------------------------------------------------------
   The entries above take densely packed frames.  These take frames whose rows lie src_pitch / dst_pitch BYTES apart and whose
   frames lie src_frame_stride / dst_frame_stride BYTES apart, for the source and the destination independently: a
   hipMallocPitch or decoder surface (1920 pixels in a 2048-pixel pitch), or a region of interest inside a larger image (a
   cv::Mat ROI: data pointer of the ROI's first pixel, pitch = Mat::step; the frames of a batch of such views lie one parent frame
   apart).  Nothing is repacked: the kernels address the rows through the pitches, and no byte of the destination outside the
   rows x cols rectangles is written (every store is masked by x < cols).  The result in the rectangle is, bit for bit, what the
   packed entry of the same type returns for the packed copy of the source -- with one exception: three-channel u8 frames with
   one sigma run on the one-channel-per-workgroup kernel here (the route of the _sigmas_ entries) where the packed entry has its
   three-channel kernel; both meet the u8 parity contract, a rounding tie may fall differently.
   Overlap: the byte spans [base, base + (nframes - 1) frame_stride + (rows - 1) pitch + cols channels sizeof(element)) of the
   source and the destination are compared.  Where they intersect -- an in-place call, two rectangles of one parent image -- the
   source rectangles are first gathered into the context's workspace (one launch on the call's stream), so the result is always
   what reading the whole source before the first write gives.
   Arguments: the rules of the packed entry of the type (sigma, sizes, engine), and BLUR_ERR_INVALID for a pitch below
   cols * channels * sizeof(element), a pitch or frame stride that is no multiple of sizeof(element), and, with nframes > 1, a
   frame stride below (rows - 1) * pitch + cols * channels * sizeof(element); checked before the device is touched (ctx may then
   be NULL).  A frame stride of 0 with nframes == 1 is accepted.  A frame whose span (rows - 1) * pitch + cols * channels *
   sizeof(element) exceeds 4 GiB - 4 KiB takes the plane path, or fails with BLUR_ERR_UNSUPPORTED under engine = FUSED, as a packed
   frame of that size does.  pitch = cols * channels * sizeof(element) and frame_stride = rows * pitch is the packed entry. */
int blur_gaussian_u8_pitched_batch_dev(blur_ctx* ctx, const uint8_t* d_src, size_t src_pitch, size_t src_frame_stride, uint8_t* d_dst,
                                       size_t dst_pitch, size_t dst_frame_stride, int nframes, int rows, int cols, int channels,
                                       double sigma, const blur_opts* opts);
int blur_gaussian_f32_pitched_batch_dev(blur_ctx* ctx, const float* d_src, size_t src_pitch, size_t src_frame_stride, float* d_dst,
                                        size_t dst_pitch, size_t dst_frame_stride, int nframes, int rows, int cols, int channels,
                                        double sigma, const blur_opts* opts);
int blur_gaussian_u16_pitched_batch_dev(blur_ctx* ctx, const uint16_t* d_src, size_t src_pitch, size_t src_frame_stride, uint16_t* d_dst,
                                        size_t dst_pitch, size_t dst_frame_stride, int nframes, int rows, int cols, int channels,
                                        double sigma, const blur_opts* opts);
int blur_gaussian_f16_pitched_batch_dev(blur_ctx* ctx, const uint16_t* d_src, size_t src_pitch, size_t src_frame_stride, uint16_t* d_dst,
                                        size_t dst_pitch, size_t dst_frame_stride, int nframes, int rows, int cols, int channels,
                                        double sigma, const blur_opts* opts);
int blur_gaussian_bf16_pitched_batch_dev(blur_ctx* ctx, const uint16_t* d_src, size_t src_pitch, size_t src_frame_stride, uint16_t* d_dst,
                                         size_t dst_pitch, size_t dst_frame_stride, int nframes, int rows, int cols, int channels,
                                         double sigma, const blur_opts* opts);
/* one sigma per channel (the _sigmas_ entries' rules: 0 leaves the channel as it is; its samples in the rectangle are copied) */
int blur_gaussian_u8_sigmas_pitched_batch_dev(blur_ctx* ctx, const uint8_t* d_src, size_t src_pitch, size_t src_frame_stride, uint8_t* d_dst,
                                              size_t dst_pitch, size_t dst_frame_stride, int nframes, int rows, int cols, int channels,
                                              const double* sigmas, const blur_opts* opts);
int blur_gaussian_f32_sigmas_pitched_batch_dev(blur_ctx* ctx, const float* d_src, size_t src_pitch, size_t src_frame_stride, float* d_dst,
                                               size_t dst_pitch, size_t dst_frame_stride, int nframes, int rows, int cols, int channels,
                                               const double* sigmas, const blur_opts* opts);
int blur_gaussian_u16_sigmas_pitched_batch_dev(blur_ctx* ctx, const uint16_t* d_src, size_t src_pitch, size_t src_frame_stride, uint16_t* d_dst,
                                               size_t dst_pitch, size_t dst_frame_stride, int nframes, int rows, int cols, int channels,
                                               const double* sigmas, const blur_opts* opts);
int blur_gaussian_f16_sigmas_pitched_batch_dev(blur_ctx* ctx, const uint16_t* d_src, size_t src_pitch, size_t src_frame_stride, uint16_t* d_dst,
                                               size_t dst_pitch, size_t dst_frame_stride, int nframes, int rows, int cols, int channels,
                                               const double* sigmas, const blur_opts* opts);
int blur_gaussian_bf16_sigmas_pitched_batch_dev(blur_ctx* ctx, const uint16_t* d_src, size_t src_pitch, size_t src_frame_stride, uint16_t* d_dst,
                                                size_t dst_pitch, size_t dst_frame_stride, int nframes, int rows, int cols, int channels,
                                                const double* sigmas, const blur_opts* opts);

/* ---- decoded video surfaces: NV12 (8-bit) and P010 / P016 (16-bit), DEVICE pointers -------------------------------------------
   What rocDecode, VA-API and the other decoders produce: a rows x cols luma plane and a rows / 2 x cols / 2 plane of interleaved
   Cb/Cr pairs (cols samples per chroma row), both with the same row pitch.  The planes are passed separately (in a decoder
   surface d_src_uv = d_src_y + surface_height * pitch), so the entries do not care how many rows of padding lie between them.
   A call blurs the luma plane with sigmas[0], Cb with sigmas[1] and Cr with sigmas[2], each sigma in pixels OF THE PLANE IT
   APPLIES TO (the same blur in luma pixels on all three is (s, s / 2, s / 2)); nothing is split, converted or repacked: the
   chroma plane runs on the two-channel instantiation of the fused kernel.
     result   the luma plane is, bit for bit, what blur_gaussian_u8_pitched_batch_dev (p016: ..._u16_...) returns for that plane
              with channels = 1 and sigmas[0]; Cb (Cr) is, bit for bit, what that entry returns for the de-interleaved rows / 2 x
              cols / 2 Cb (Cr) plane with sigmas[1] (sigmas[2]).
     zero     sigmas[p] == 0 leaves the plane or channel as it is: copied out of place, untouched in place.
     p016     samples are uint16_t, pitches and strides in BYTES; the output follows the u16 rule (uint16_t)((uint32_t)(int32_t)(v +
              0.5f) & 0xffff).  The low bits of P010 data (10 significant bits in the HIGH bits of the word, the low 6 zero) are NOT
              masked: a blurred P010 surface has non-zero low bits, which a P010 consumer ignores and a P016 consumer uses.
     writes   no byte outside the rows x cols and rows / 2 x cols rectangles is written (padding between rows and planes stays).
     overlap  per plane as for the pitched entries: an in-place call (d_dst_y == d_src_y, d_dst_uv == d_src_uv, equal pitches) and
              overlapping spans read from one gathered copy.  The destination of one plane must not overlap the source of the other.
     engine   per plane, the one-channel entries' rules: AUTO takes the fused kernel wherever they give one to that pad (nv12: pad
              <= 168; p016: pad <= 104), FUSED fails with BLUR_ERR_UNSUPPORTED, before anything is written, where a blurred plane has
              no fused kernel, FFT takes the plane path.  blur_last_engine reports 6 if every blurred plane ran fused, else 0 with a
              note naming the planes on the plane path.
   BLUR_ERR_INVALID: a NULL pointer (sigmas included), nframes < 0, rows or cols <= 0 or odd, a pitch below cols * sizeof(sample)
   or no multiple of sizeof(sample), with nframes > 1 a frame stride below its plane's span ((plane rows - 1) * pitch + cols *
   sizeof(sample)) or no multiple of sizeof(sample), a negative, NaN or infinite sigma.  BLUR_ERR_UNSUPPORTED: the luma pad exceeds
   min(rows, cols) - 1 or a chroma pad exceeds min(rows / 2, cols / 2) - 1.  Checked in this order before the device is touched (ctx
   may then be NULL); nframes == 0 is a no-op.  The _host entries take one PACKED surface in host memory: rows * cols luma samples,
   then rows / 2 rows of cols chroma samples (src and dst apart or equal). */
int blur_gaussian_nv12_batch_dev(blur_ctx* ctx, const uint8_t* d_src_y, const uint8_t* d_src_uv, size_t src_pitch, size_t src_y_frame_stride,
                                 size_t src_uv_frame_stride, uint8_t* d_dst_y, uint8_t* d_dst_uv, size_t dst_pitch, size_t dst_y_frame_stride,
                                 size_t dst_uv_frame_stride, int nframes, int rows, int cols, const double* sigmas, const blur_opts* opts);
int blur_gaussian_nv12_dev(blur_ctx* ctx, const uint8_t* d_src_y, const uint8_t* d_src_uv, size_t src_pitch, uint8_t* d_dst_y, uint8_t* d_dst_uv,
                           size_t dst_pitch, int rows, int cols, const double* sigmas, const blur_opts* opts);
int blur_gaussian_nv12_host(blur_ctx* ctx, const uint8_t* src, uint8_t* dst, int rows, int cols, const double* sigmas, const blur_opts* opts);
int blur_gaussian_p016_batch_dev(blur_ctx* ctx, const uint16_t* d_src_y, const uint16_t* d_src_uv, size_t src_pitch, size_t src_y_frame_stride,
                                 size_t src_uv_frame_stride, uint16_t* d_dst_y, uint16_t* d_dst_uv, size_t dst_pitch, size_t dst_y_frame_stride,
                                 size_t dst_uv_frame_stride, int nframes, int rows, int cols, const double* sigmas, const blur_opts* opts);
int blur_gaussian_p016_dev(blur_ctx* ctx, const uint16_t* d_src_y, const uint16_t* d_src_uv, size_t src_pitch, uint16_t* d_dst_y, uint16_t* d_dst_uv,
                           size_t dst_pitch, int rows, int cols, const double* sigmas, const blur_opts* opts);
int blur_gaussian_p016_host(blur_ctx* ctx, const uint16_t* src, uint16_t* dst, int rows, int cols, const double* sigmas, const blur_opts* opts);

/* host-only plan of the _sigmas_ entries (no GPU needed; the same host code the entries use): for channel c, out[3 c] = its group (the
   channels of equal sigma share an index, counted in the order of their first channel; -1 for sigma = 0), out[3 c + 1] = the pad
   of its sigma on this frame, out[3 c + 2] = the fused kernel's window class NKB, 8 (NKB - 4) < pad <= 8 (NKB - 2), or 0 where the
   pad has no fused kernel (pad > 168).  Status as the entries above; BLUR_ERR_INVALID also for a null `out`. */
int blur_gaussian_sigmas_plan(int rows, int cols, int channels, const double* sigmas, int* out);

/* ---- one sigma per frame, DEVICE pointers -------------------------------------------------------------------------------------
   The _frame_sigmas_ entries take `const double sigmas[nframes]` (HOST memory) where the batch entries take `double sigma`: an
   augmentation that draws a sigma per image of a training batch, a clip whose blur changes from frame to frame, or (pitched entry,
   src_frame_stride = 0) one frame blurred with K sigmas into K outputs.  u8, float32, u16, float16 and bfloat16 (the 16-bit types as
   uint16_t samples, as in their scalar entries), channels in {1, 3, 4}; decoded NV12 / P016 clips have entries of their own below.
     sigmas[f] > 0   frame f of the result is, bit for bit, what the scalar entry of the same type returns for that frame alone with
                     sigma = sigmas[f] and the same opts (a float32, float16 or bfloat16 frame's power-of-two scale comes from its own
                     max|x|).  The one
                     exception is u8 with three channels, where the scalar call runs its own three-channel kernels: such a frame
                     runs on the one-channel-per-workgroup kernel (the route of the _sigmas_ and pitched entries) and meets the same
                     float64 oracle under the same tie rule.  Three-channel u8 frames are NEVER forwarded to the u8c3 entry, not even
                     when every sigma is equal: a frame's bytes depend on its pixels, its sigma and opts only -- not on its position
                     in the batch, on the other frames, or on whether it is blurred alone.  (A caller with ONE sigma for all of its
                     BGR frames should call the scalar entry: its kernel is faster for narrow windows, pad <= 72.)
     sigmas[f] == 0  frame f is copied bit for bit; an in-place call does not touch it.
   Cost: the frames are grouped by the fused kernel's window class (NKB = 3, 5 .. 23: pad <= 8 (NKB - 2)) and every class is ONE
   pre-pass and ONE fused launch over its frames, whatever their sigmas: at most 11 fused launches per call where the loop over the
   scalar entry has one per frame.  The fragments and taps of the call's sigmas are built on the host and uploaded once per call
   into a workspace of the context; nothing is cached per sigma, so a stream of never-repeating sigmas costs no device memory.
   opts->engine applies per frame: AUTO gives a frame the fused kernel wherever the scalar entry's rules give it to that sigma (u8
   with three channels: wherever the 1- and 4-channel rules do; float32, u16 and the half types: pad <= 104) and the f32 plane path
   elsewhere, one frame at a time; FUSED fails
   with BLUR_ERR_UNSUPPORTED, before anything is written, if any frame has no fused kernel; FFT takes the plane path for every
   frame.  After the call blur_last_engine returns family 6 if every blurred frame ran on the fused kernel and 0 otherwise; the note
   then says how many frames took the plane path and names the first of them, its sigma and the reason.
   BLUR_ERR_INVALID: channels not in {1, 3, 4}, a NULL pointer (sigmas included), nframes < 0, rows or cols <= 0, a negative, NaN or
   infinite sigma; BLUR_ERR_UNSUPPORTED: a frame whose pad exceeds min(rows, cols) - 1.  Every entry of sigmas is checked before the
   device is touched (ctx may then be NULL) and before anything is written; nframes == 0 is a no-op.
   Pitched entries: the rules of blur_gaussian_*_pitched_batch_dev, and src_frame_stride == 0 is accepted for any nframes: every
   frame of the result is blurred from the same source frame (scale space, difference of Gaussians).  A dst_frame_stride of 0 with
   nframes > 1 stays BLUR_ERR_INVALID.  Stores are masked by x < cols; overlapping source and destination spans, in place
   included, are read from one gathered copy (a large in-place batch in parts of 1 GiB).
   Asynchronous on the context's stream as far as the kernels go; the call keeps the host busy while it builds and uploads its
   tables.  sigmas is read before the call returns. */
int blur_gaussian_u8_frame_sigmas_batch_dev(blur_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int nframes, int rows, int cols, int channels,
                                            const double* sigmas, const blur_opts* opts);
int blur_gaussian_f32_frame_sigmas_batch_dev(blur_ctx* ctx, const float* d_src, float* d_dst, int nframes, int rows, int cols, int channels,
                                             const double* sigmas, const blur_opts* opts);
int blur_gaussian_u8_frame_sigmas_pitched_batch_dev(blur_ctx* ctx, const uint8_t* d_src, size_t src_pitch, size_t src_frame_stride, uint8_t* d_dst,
                                                    size_t dst_pitch, size_t dst_frame_stride, int nframes, int rows, int cols, int channels,
                                                    const double* sigmas, const blur_opts* opts);
int blur_gaussian_f32_frame_sigmas_pitched_batch_dev(blur_ctx* ctx, const float* d_src, size_t src_pitch, size_t src_frame_stride, float* d_dst,
                                                     size_t dst_pitch, size_t dst_frame_stride, int nframes, int rows, int cols, int channels,
                                                     const double* sigmas, const blur_opts* opts);
int blur_gaussian_u16_frame_sigmas_batch_dev(blur_ctx* ctx, const uint16_t* d_src, uint16_t* d_dst, int nframes, int rows, int cols, int channels,
                                             const double* sigmas, const blur_opts* opts);
int blur_gaussian_f16_frame_sigmas_batch_dev(blur_ctx* ctx, const uint16_t* d_src, uint16_t* d_dst, int nframes, int rows, int cols, int channels,
                                             const double* sigmas, const blur_opts* opts);
int blur_gaussian_bf16_frame_sigmas_batch_dev(blur_ctx* ctx, const uint16_t* d_src, uint16_t* d_dst, int nframes, int rows, int cols, int channels,
                                              const double* sigmas, const blur_opts* opts);
int blur_gaussian_u16_frame_sigmas_pitched_batch_dev(blur_ctx* ctx, const uint16_t* d_src, size_t src_pitch, size_t src_frame_stride, uint16_t* d_dst,
                                                     size_t dst_pitch, size_t dst_frame_stride, int nframes, int rows, int cols, int channels,
                                                     const double* sigmas, const blur_opts* opts);
int blur_gaussian_f16_frame_sigmas_pitched_batch_dev(blur_ctx* ctx, const uint16_t* d_src, size_t src_pitch, size_t src_frame_stride, uint16_t* d_dst,
                                                     size_t dst_pitch, size_t dst_frame_stride, int nframes, int rows, int cols, int channels,
                                                     const double* sigmas, const blur_opts* opts);
int blur_gaussian_bf16_frame_sigmas_pitched_batch_dev(blur_ctx* ctx, const uint16_t* d_src, size_t src_pitch, size_t src_frame_stride, uint16_t* d_dst,
                                                      size_t dst_pitch, size_t dst_frame_stride, int nframes, int rows, int cols, int channels,
                                                      const double* sigmas, const blur_opts* opts);
/* A decoded clip whose blur changes from frame to frame (a focus pull, a blur ramp): the arguments of blur_gaussian_{nv12,p016}_batch_dev
   with `const double sigmas[2 * nframes]` (HOST memory): sigmas[2 f] is frame f's luma sigma, sigmas[2 f + 1] the sigma of both of
   its chroma channels, each in pixels of its own plane (separate Cb and Cr sigmas per frame: the scalar entry, frame by frame).
     result   the planes of frame f are, bit for bit, what blur_gaussian_{nv12,p016}_dev returns for that frame alone with
              (sigmas[2 f], sigmas[2 f + 1], sigmas[2 f + 1]) and the same opts.
     zero     a sigma of 0 leaves that plane of that frame as it is: copied out of place, untouched in place.
     writes, overlap   as the scalar surface entries, per plane.
     cost     the luma planes and the chroma planes are each one call of the driver behind the entries above: per window class one
              pre-pass and one fused launch over the class's frames (the chroma plane on the two-channel kernels).
     engine   per plane and per frame, the scalar surface entry's rules; the engine of every plane of every frame is chosen before
              the first launch, so a FUSED refusal has written nothing.  blur_last_engine: 6 if every blurred plane of every frame
              ran fused, else 0 with a note that names the luma and / or chroma frames on the plane path.
   Status: the scalar surface entries' checks in their order, with both sigmas of every frame checked (finite, >= 0), then
   BLUR_ERR_UNSUPPORTED where any frame's luma pad exceeds min(rows, cols) - 1 or its chroma pad min(rows / 2, cols / 2) - 1; all
   before the device is touched (ctx may then be NULL). */
int blur_gaussian_nv12_frame_sigmas_batch_dev(blur_ctx* ctx, const uint8_t* d_src_y, const uint8_t* d_src_uv, size_t src_pitch, size_t src_y_frame_stride,
                                              size_t src_uv_frame_stride, uint8_t* d_dst_y, uint8_t* d_dst_uv, size_t dst_pitch,
                                              size_t dst_y_frame_stride, size_t dst_uv_frame_stride, int nframes, int rows, int cols,
                                              const double* sigmas, const blur_opts* opts);
int blur_gaussian_p016_frame_sigmas_batch_dev(blur_ctx* ctx, const uint16_t* d_src_y, const uint16_t* d_src_uv, size_t src_pitch, size_t src_y_frame_stride,
                                              size_t src_uv_frame_stride, uint16_t* d_dst_y, uint16_t* d_dst_uv, size_t dst_pitch,
                                              size_t dst_y_frame_stride, size_t dst_uv_frame_stride, int nframes, int rows, int cols,
                                              const double* sigmas, const blur_opts* opts);
/* host-only plan of the _frame_sigmas_ entries of one pixel type (no GPU needed; the same host code the entries use): for frame f, out[4 f] = its launch group
   (the frames of one window class share an index, counted in the order of their first frame; -1 for sigma = 0), out[4 f + 1] = the
   pad of its sigma, out[4 f + 2] = the fused kernel's window class NKB, 8 (NKB - 4) < pad <= 8 (NKB - 2), or 0 where the pad has no
   fused kernel (pad > 168; these frames form a group of their own), out[4 f + 3] = its table slot (frames of equal sigma share
   one, counted in the order of their first frame; -1 for sigma = 0).  Status as the entries above; BLUR_ERR_INVALID also for a null
   `out`. */
int blur_gaussian_frame_sigmas_plan(int rows, int cols, int nframes, const double* sigmas, int* out);

/* fastboxblur over a batch, sharded by frame exactly like the two calls above, in place (blur_fastboxblur_u8_batch_dev on
   each shard); arguments and errors as blur_fastboxblur_u8_batch_dev, nframes == 0 is a no-op, shards without frames idle. */
int blur_fastboxblur_u8_batch_multi_dev(blur_multi* m, uint8_t* d_inout, int nframes, int w, int h, int channels,
                                        int ksize, int passes);
int blur_fastboxblur_u8_batch_multi_host(blur_multi* m, uint8_t* inout, int nframes, int w, int h, int channels,
                                         int ksize, int passes);

/* ---- batched line convolution: what pffft_transform_ordered(FORWARD) -> pffft_sorted_optimized_convolution ->
   pffft_transform_ordered(BACKWARD) (Source.cpp:531-533,553-555) is per tile, for MANY lines at once --------------
   d_in / d_out: nlines complex lines of n points each (interleaved re, im floats; in == out allowed),
   out = IDFT_n(multipliers .* DFT_n(in)), UNNORMALISED like pffft (fold 1/n into the multipliers, Source.cpp:423);
   multipliers: n real factors in natural frequency order (host pointer; cached on the device by content).
   Two real lines ride in one complex line when the multipliers are even (m[f] = m[n-f]): re and im are then
   convolved independently.  n must be a length the wave-resident kernels support: blur_wr_length(). */
int blur_convolve_lines_c32_dev(blur_ctx* ctx, const float* d_in, float* d_out, int nlines, int n, const float* multipliers);
/* ---- matrix-core engine (mx_kernels.hpp): both passes as banded Toeplitz products on v_mfma_f32_32x32x16_f16 ----
   blur_opts.engine = BLUR_ENGINE_MATRIX selects it for the u8c3 entry points (BLUR_ENGINE_FUSED: the one-kernel form of the same
   products, fx_kernels.hpp, which is the library's own choice where it applies).  Same linear map as the FFT product inside the
   crop (Source.cpp:536,558), Nyquist-slot quirk (Source.cpp:420-425) included as a rank-one term per line.
   blur_mx_window_blocks(pad): window blocks (of 16 positions) of the kernel instantiated for this pad, 0 = none.
   blur_mx_fragments: the Toeplitz operand fragments the kernels load, [2][nkb][64][8] binary16 (hi, lo halves of
   taps * 2^14); taps: 2 pad + 1 floats, centre at index pad (host only; tests). */
int blur_mx_window_blocks(int pad);
int blur_mx_fragments(const float* taps, int pad, int nkb, uint16_t* out);

/* smallest supported transform length >= need for the column (1) or row (0) role; 0 if there is none.
   (The engine's transform length need not be nearestTransformSize(): only the Nyquist-slot term of Source.cpp:420-425
   depends on the reference's length, and the multiplier of bin n/2 reproduces it.) */
int blur_wr_length(int need, int column_role);
/* the multipliers those kernels use for the Gaussian, all n bins in natural order: m[f] = Re DFT_n(kernel)[f] / n, and with
   quirk != 0 bin n/2 carries the reference's Nyquist-slot term for ITS transform length n_ref (Source.cpp:420-425).  Host only. */
int blur_wr_kernel_multipliers(double sigma, int ksize, int n, int n_ref, int quirk, float* m);

/* ---- plain device-memory plumbing for callers without a HIP runtime of their own --- */
int blur_malloc(blur_ctx* ctx, void** d_ptr, size_t bytes);
int blur_free(blur_ctx* ctx, void* d_ptr);
int blur_memcpy_h2d(blur_ctx* ctx, void* d_dst, const void* src, size_t bytes);   /* synchronous */
int blur_memcpy_d2h(blur_ctx* ctx, void* dst, const void* d_src, size_t bytes);   /* synchronous */
/* page-locked host memory (the role PFAlloc plays for pffft's aligned buffers, Utils.hpp:57-138: memory the
   transport wants): host images that live here are copied by DMA without a staging pass */
int blur_host_alloc(blur_ctx* ctx, void** h_ptr, size_t bytes);
int blur_host_free(blur_ctx* ctx, void* h_ptr);

/* ---- measurement: the box's streaming rate as THIS library's kernels would see it: a 16-byte-per-lane copy of `bytes` bytes
   (device to device, `reps` launches between two events on the context's stream); *gbs = (bytes read + bytes written) / s / 1e9.
   bench.py prints it beside the 8 TB/s spec figure (MI355X_MICROARCH.md gives 6.29 TB/s for this access shape). */
int blur_copy_bandwidth(blur_ctx* ctx, size_t bytes, int reps, double* gbs);

#ifdef __cplusplus
}
#endif
#endif /* BLUR_AMD_H */
