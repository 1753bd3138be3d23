"""Host-side mirror of the reference's call surface for the FFT-blur hot path.

Names and argument meaning follow michelerenzullo/Blur_algorithms (Source.cpp / Utils.hpp);
the work happens in libblur_amd.so (hand-written HIP for gfx950) through the C ABI of
include/blur_amd.h.  torch is used only to hold device memory and the stream.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import BlurError, BlurOpts


def _L():
    return _lib.load()


# ---- sizing (host, bit-identical to the reference) -------------------------------------
def gaussian_window(sigma, max_width=0):
    """gaussian_window(sigma, max_width) -- Source.cpp:60-73"""
    return _L().blur_gaussian_window(float(sigma), int(max_width))


def getGaussian(sigma, width=0, FFT_length=0):
    """getGaussian(kernel, sigma, width, FFT_length) -- Source.cpp:75-102; returns the kernel"""
    w = width or gaussian_window(sigma)
    k = np.zeros(max(w, FFT_length), np.float32)
    rc = _L().blur_get_gaussian(k.ctypes.data, float(sigma), int(width), int(FFT_length))
    if rc:
        raise BlurError(rc, "getGaussian: bad arguments")
    return k


def isValidSize(N):
    """isValidSize -- Utils.hpp:141-148"""
    return _L().blur_is_valid_size(int(N))


def nearestTransformSize(N):
    """nearestTransformSize -- Utils.hpp:150-157"""
    return _L().blur_nearest_transform_size(int(N))


def pffft_sizing(rows, cols, sigma):
    """the sizing block of pffft_() -- Source.cpp:434-457"""
    out = (C.c_int * 6)()
    rc = _L().blur_pffft_sizing(int(rows), int(cols), float(sigma), out)
    if rc:
        raise BlurError(rc, "pffft_sizing: bad arguments")
    return dict(kSize=out[0], pad=out[1], N0=out[2], N1=out[3], tz0=out[4], tz1=out[5])


def kernel_multipliers(sigma, ksize, n):
    m = np.empty(n // 2 + 1, np.float32)
    rc = _L().blur_kernel_multipliers(float(sigma), int(ksize), int(n), m.ctypes.data)
    if rc:
        raise BlurError(rc, "kernel_multipliers: bad arguments")
    return m


def box_kernel(kLen, FFT_length):
    """box_kernel(kernel, kLen, FFT_length), 1D form -- Source.cpp:129-140; returns the kernel"""
    k = np.zeros(int(FFT_length), np.float32)
    rc = _L().blur_box_kernel(k.ctypes.data, int(kLen), int(FFT_length))
    if rc:
        raise BlurError(rc, "box_kernel: bad arguments")
    return k


def pocketfft2d_sizing(rows, cols, sigma):
    """the sizing block of pocketfft_2D -- Source.cpp:149-176"""
    out = (C.c_int * 8)()
    rc = _L().blur_pocketfft2d_sizing(int(rows), int(cols), float(sigma), out)
    if rc:
        raise BlurError(rc, "pocketfft2d_sizing: bad arguments")
    return dict(kSize=out[0], pad=out[1], sizes=(out[2], out[3]), border=(out[4], out[5], out[6], out[7]))


def boxfft_sizing(rows, cols, nsmooth):
    """sizing of the `#define boxblur` mode of pffft_() -- Source.cpp:437-457"""
    out = (C.c_int * 4)()
    rc = _L().blur_boxfft_sizing(int(rows), int(cols), float(nsmooth), out)
    if rc:
        raise BlurError(rc, "boxfft_sizing: bad arguments")
    return dict(kLen=out[0], pad=out[1], N0=out[2], N1=out[3])


def fastboxblur_batch_plan(nframes, w, h, channels, ksize, passes):
    """how blur_fastboxblur_u8_batch_dev runs a batch (host only, no GPU):
    (frames_per_chunk, chunks, vertical_on_matrix_cores, horizontal_on_matrix_cores)"""
    out = (C.c_int * 4)()
    rc = _L().blur_fastboxblur_batch_plan(int(nframes), int(w), int(h), int(channels), int(ksize), int(passes), out)
    if rc:
        raise BlurError(rc, "fastboxblur_batch_plan: bad arguments")
    return tuple(out)


def _box_frames_shape(shape):
    """[n, h, w] or [n, h, w, C] -> (n, w, h, C)"""
    if len(shape) not in (3, 4):
        raise ValueError("expected uint8 frames [n, h, w] or [n, h, w, C]")
    return shape[0], shape[2], shape[1], 1 if len(shape) == 3 else shape[3]


def _gauss_frames_shape(shape):
    """[rows, cols], [rows, cols, C] or [n, rows, cols, C] with C in {1, 3, 4} and rows, cols > 0 -> (n, rows, cols, C)"""
    if len(shape) == 2:
        n, rows, cols, ch = 1, shape[0], shape[1], 1
    elif len(shape) == 3:
        n, (rows, cols, ch) = 1, shape
    elif len(shape) == 4:
        n, rows, cols, ch = shape
    else:
        n = rows = cols = ch = 0
    if ch not in (1, 3, 4) or rows <= 0 or cols <= 0:
        raise ValueError("expected [rows, cols], [rows, cols, C] or [n, rows, cols, C] with C in {1, 3, 4}")
    return n, rows, cols, ch


_gauss_f32_frames_shape = _gauss_frames_shape      # (the float32 entry points' name for the same helper)


BF16 = "bfloat16"      # the dtype key of the bfloat16 entries (numpy has no bfloat16: host frames are CPU torch.bfloat16 tensors)


def _dtype_name(dtype):
    return dtype if isinstance(dtype, str) else np.dtype(dtype).name


def _is_host_frames(image, dtype):
    """whether a per-channel Gaussian call takes the host route: a numpy array, or for bfloat16 a CPU torch tensor"""
    if isinstance(image, np.ndarray):
        return True
    return dtype == BF16 and not getattr(image, "is_cuda", True)


def _bf16_bits(t, what):
    """a contiguous CPU torch.bfloat16 tensor as a numpy uint16 array over the same memory"""
    import torch
    if not isinstance(t, torch.Tensor) or t.dtype != torch.bfloat16 or t.is_cuda:
        raise ValueError("%s: expected a torch.bfloat16 tensor" % what)
    return t.contiguous().view(torch.uint16).numpy()


def _gauss_result(res, out, dtype):
    """what a host-route call returns: the result array; bfloat16: a CPU torch.bfloat16 tensor over it (or `out`)"""
    if dtype != BF16:
        return res
    import torch
    return out if out is not None else torch.from_numpy(res).view(torch.bfloat16)


def _gauss_array(image, out, dtype, batch=False):
    """the host arrays of a per-channel Gaussian call: (source, result, (n, rows, cols, C)).  uint8 input of another dtype is
    converted, as pffft_ does; float32 input must be float32, uint16 input uint16 and float16 input float16; bfloat16 input is a
    CPU torch.bfloat16 tensor, passed as its 16-bit patterns.  batch: frames [n, rows, cols, C] only"""
    if dtype == BF16:
        if isinstance(image, np.ndarray):
            raise ValueError("expected a torch.bfloat16 tensor (numpy has no bfloat16; a uint16 array is a u16 image)")
        image = _bf16_bits(image, "image")
        if out is not None:
            bits = _bf16_bits(out, "out")
            if not out.is_contiguous() or bits.shape != image.shape:
                raise ValueError("out must match the input")
            out = bits
        dtype = np.uint16
    if dtype != np.uint8 and image.dtype != dtype:
        raise ValueError("expected a %s array" % np.dtype(dtype).name)
    a = np.ascontiguousarray(image, dtype)
    if batch and a.ndim != 4:
        raise ValueError("expected %s frames [n, rows, cols, C]" % np.dtype(dtype).name)
    shape = _gauss_frames_shape(a.shape)
    res = np.empty_like(a) if out is None else out
    if not isinstance(res, np.ndarray) or res.shape != a.shape or res.dtype != a.dtype or not res.flags["C_CONTIGUOUS"]:
        raise ValueError("out must match the input")
    return a, res, shape


def _gauss_strided_layout(shape, strides):
    """The pitched layout of a frame tensor [rows, cols], [rows, cols, C] or [n, rows, cols, C] with these strides (in elements):
    (row pitch, frame stride) in elements, or None where the pitched entries cannot address it.  Accepted: contiguous tensors, and
    views with strides (frame_stride, pitch, C, 1), (pitch, C, 1) or (pitch, 1) with pitch >= cols * C and positive strides -- a
    region of interest `frames[:, y0:y1, x0:x1, :]`, a surface with padded rows.  A slice along the channel axis, a stepped
    slice, a flipped or permuted view is None.  (The stride of a dimension of size 1 addresses nothing and is not looked at; a
    single frame's stride is rows * pitch then.)"""
    shape, strides = tuple(shape), tuple(strides)
    if len(shape) != len(strides) or len(shape) not in (2, 3, 4):
        return None
    if len(shape) == 2:
        (rows, cols), ch, (pitch, sx), sc, n, fs = shape, 1, strides, 1, 1, None
    elif len(shape) == 3:
        (rows, cols, ch), (pitch, sx, sc), n, fs = shape, strides, 1, None
    else:
        (n, rows, cols, ch), (fs, pitch, sx, sc) = shape, strides
    if (ch > 1 and sc != 1) or (cols > 1 and sx != ch):
        return None
    if rows > 1:
        if pitch < cols * ch:
            return None
    else:
        pitch = cols * ch
    if n > 1:
        if fs < (rows - 1) * pitch + cols * ch:
            return None
    else:
        fs = rows * pitch
    return pitch, fs


def _gauss_tensor(image, out, dtype, device=None):
    """the CUDA tensors of a per-channel Gaussian call: (source, result (default: the source), (n, rows, cols, C), layout).
    device (BlurMulti): contiguous frames [n, rows, cols, C] on that device only, layout None.  Otherwise the source and the result
    may each be contiguous or a pitched view (_gauss_strided_layout); layout is None when both are contiguous, else (source
    pitch, source frame stride, result pitch, result frame stride) in BYTES"""
    import torch
    want = {np.uint8: torch.uint8, np.uint16: torch.uint16, np.float32: torch.float32, np.float16: torch.float16, BF16: torch.bfloat16}[dtype]
    t = image
    sl = None
    if isinstance(t, torch.Tensor) and device is None:
        sl = _gauss_strided_layout(t.shape, t.stride())
    if (not isinstance(t, torch.Tensor) or t.dtype != want or not t.is_cuda or not (t.is_contiguous() or sl is not None)
            or (device is not None and (t.dim() != 4 or t.device.index != device))):
        layout = "[rows, cols], [rows, cols, C] or [n, rows, cols, C]" if device is None else "[n, rows, cols, C] on devices[0]"
        raise ValueError("expected a contiguous CUDA %s tensor %s%s" % (_dtype_name(dtype), layout, ", or a view of one with whole pixels in rows "
                                                                         "a pitch apart (a region of interest, padded rows)" if device is None else ""))
    shape = _gauss_frames_shape(tuple(t.shape))
    dst = t if out is None else out
    dl = None
    if isinstance(dst, torch.Tensor) and device is None:
        dl = _gauss_strided_layout(dst.shape, dst.stride())
    if (not isinstance(dst, torch.Tensor) or dst.shape != t.shape or dst.dtype != t.dtype or not dst.is_cuda
            or not (dst.is_contiguous() or dl is not None)):
        raise ValueError("out must match the input")
    if device is not None or (t.is_contiguous() and dst.is_contiguous()):
        return t, dst, shape, None
    es = t.element_size()
    return t, dst, shape, (sl[0] * es, sl[1] * es, dl[0] * es, dl[1] * es)


def _nv12_layout(y_shape, y_strides, uv_shape, uv_strides):
    """The layout of an NV12 / P016 surface given as two tensors, from their shapes and strides (in elements): y is [rows, cols] or
    [n, rows, cols], uv is [rows / 2, cols / 2, 2] or [n, rows / 2, cols / 2, 2] (interleaved Cb/Cr pairs).  Returns (n, rows, cols,
    pitch, y frame stride, uv frame stride) in elements.  Both planes must be row-pitched views with the SAME pitch >= cols: luma
    strides ([fs_y,] pitch, 1), chroma strides ([fs_uv,] pitch, 2, 1) -- the two planes of one decoder surface, regions of them, or
    contiguous tensors (pitch = cols).  ValueError for mismatched shapes, odd sizes, unequal pitches and every other view.  (The
    stride of a dimension of size 1 addresses nothing and is not looked at.)"""
    y_shape, y_strides, uv_shape, uv_strides = tuple(y_shape), tuple(y_strides), tuple(uv_shape), tuple(uv_strides)
    if len(y_shape) != len(y_strides) or len(uv_shape) != len(uv_strides) or len(y_shape) not in (2, 3) or len(uv_shape) != len(y_shape) + 1:
        raise ValueError("expected y [rows, cols] with uv [rows / 2, cols / 2, 2], or y [n, rows, cols] with uv [n, rows / 2, cols / 2, 2]")
    if len(y_shape) == 3:
        (n, rows, cols), (fs_y, pitch, sx) = y_shape, y_strides
        (n_uv, crows, ccols, two), (fs_uv, cpitch, cx, cc) = uv_shape, uv_strides
    else:
        n = n_uv = 1
        fs_y = fs_uv = None
        (rows, cols), (pitch, sx) = y_shape, y_strides
        (crows, ccols, two), (cpitch, cx, cc) = uv_shape, uv_strides
    if rows <= 0 or cols <= 0 or rows % 2 or cols % 2:
        raise ValueError("rows and cols of the luma plane must be positive and even, got %d x %d" % (rows, cols))
    if (n_uv, crows, ccols, two) != (n, rows // 2, cols // 2, 2):
        raise ValueError("uv must be %s for y %s" % ((([n] if len(y_shape) == 3 else []) + [rows // 2, cols // 2, 2]), list(y_shape)))
    if sx != 1 or cc != 1 or (ccols > 1 and cx != 2):
        raise ValueError("y and uv must be row-pitched views: samples of a row (Cb/Cr pairs of a chroma row) next to each other")
    if pitch < cols:
        raise ValueError("the rows of y overlap or run backwards (pitch %d < cols %d)" % (pitch, cols))
    if crows > 1 and cpitch != pitch:
        raise ValueError("y and uv must have the same row pitch (got %d and %d elements)" % (pitch, cpitch))
    if n > 1:
        if fs_y < (rows - 1) * pitch + cols or fs_uv < (crows - 1) * pitch + cols:
            raise ValueError("the frames of y or of uv overlap or run backwards")
    else:
        fs_y, fs_uv = rows * pitch, crows * pitch
    return n, rows, cols, pitch, fs_y, fs_uv


def _nv12_sigmas(sigma):
    """the three sigmas (Y, Cb, Cr) of an NV12 / P016 call, each in pixels of its own plane: a scalar s means (s, s / 2, s / 2), the
    same blur in luma pixels on all three; a sequence of three is taken as given"""
    if not _is_sigma_sequence(sigma):
        s = float(sigma)
        return (s, s / 2, s / 2)
    vals = tuple(float(v) for v in sigma)
    if len(vals) != 3:
        raise ValueError("sigma: expected a number or a sequence of 3 (Y, Cb, Cr), got %d" % len(vals))
    return vals


def _nv12_frame_sigmas(sigmas, y):
    """the (luma, chroma) sigmas of every frame of a gaussian_nv12_per_frame call on the clip y [n, rows, cols], each in pixels of its
    own plane: an entry that is a number s means (s, s / 2), a pair is taken as given"""
    if len(y.shape) != 3:
        raise ValueError("expected a clip: y [n, rows, cols] with uv [n, rows / 2, cols / 2, 2]")
    if not _is_sigma_sequence(sigmas):
        raise ValueError("sigmas: expected a sequence with one entry per frame")
    pairs = []
    for f, e in enumerate(sigmas):
        if not _is_sigma_sequence(e):
            s = float(e)
            pairs.append((s, s / 2))
            continue
        vals = tuple(float(v) for v in e)
        if len(vals) != 2:
            raise ValueError("sigmas[%d]: expected a number or a pair (sigma_y, sigma_c), got %d values" % (f, len(vals)))
        pairs.append(vals)
    if len(pairs) != y.shape[0]:
        raise ValueError("sigmas: expected one entry per frame (%d), got %d" % (y.shape[0], len(pairs)))
    return pairs


def _nv12_tensors(y, uv, out, require_cuda=True):
    """the checks of BlurContext.gaussian_nv12 on its tensors, before the library is called: (y, uv, y_out, uv_out, source layout,
    result layout), the layouts as _nv12_layout returns them.  uint8 is NV12, uint16 P016"""
    import torch
    for t in (y, uv):
        if not isinstance(t, torch.Tensor) or t.dtype not in (torch.uint8, torch.uint16) or (require_cuda and not t.is_cuda):
            raise ValueError("expected CUDA uint8 (NV12) or uint16 (P016) tensors y and uv")
    if y.dtype != uv.dtype or y.device != uv.device:
        raise ValueError("y and uv must have the same dtype and device")
    sl = _nv12_layout(y.shape, y.stride(), uv.shape, uv.stride())
    if out is None:
        return y, uv, y, uv, sl, sl
    if not isinstance(out, (tuple, list)) or len(out) != 2:
        raise ValueError("out: expected (y_out, uv_out)")
    yo, uvo = out
    for t, s in ((yo, y), (uvo, uv)):
        if not isinstance(t, torch.Tensor) or t.dtype != s.dtype or t.device != s.device or tuple(t.shape) != tuple(s.shape):
            raise ValueError("out must match the input: (y_out, uv_out) with the shapes, dtype and device of (y, uv)")
    dl = _nv12_layout(yo.shape, yo.stride(), uvo.shape, uvo.stride())
    return y, uv, yo, uvo, sl, dl


def _nv12_per_frame_tensors(y, uv, sigmas, out, require_cuda=True):
    """the checks of BlurContext.gaussian_nv12_per_frame on its tensors and sigmas, before the library is called: what _nv12_tensors
    returns, and the (luma, chroma) sigmas per frame"""
    r = _nv12_tensors(y, uv, out, require_cuda)
    return r + (_nv12_frame_sigmas(sigmas, y),)


def _is_sigma_sequence(sigma):
    """whether `sigma` is one value per channel (a list, tuple, numpy array or tensor of numbers) rather than a scalar.  A 0-d
    numpy array or tensor is a scalar, as it was before sequences were accepted"""
    if getattr(sigma, "ndim", 1) == 0:
        return False
    return hasattr(sigma, "__len__") and not isinstance(sigma, (str, bytes))


def _sigma_arg(sigma, ch, two_d=False):
    """the `sigma` argument of a per-channel Gaussian entry: a float, or for a sequence a double[ch] for the _sigmas_ entries (0 = the
    channel is left as it is).  The sequence has one entry per channel; two_d: a [rows, cols] image takes a sequence of one"""
    if not _is_sigma_sequence(sigma):
        return float(sigma)
    vals = [float(v) for v in sigma]
    if len(vals) != ch:
        raise ValueError("sigma: expected a number or a sequence of %d (one per channel%s), got %d"
                         % (ch, " of the [rows, cols] image" if two_d else "", len(vals)))
    return (C.c_double * ch)(*vals)


def gaussian_sigmas_plan(rows, cols, sigmas):
    """how a per-channel-sigma Gaussian call groups its channels (host only, no GPU): a list with one (group, pad, nkb) per channel.
    group: channels of equal sigma share an index, -1 for sigma = 0 (the channel is copied); pad: pffft_sizing's; nkb: the fused
    kernel's window class, 0 where the pad has none (pad > 168: the plane path)"""
    vals = [float(v) for v in sigmas]
    out = (C.c_int * (3 * len(vals)))()
    rc = _L().blur_gaussian_sigmas_plan(int(rows), int(cols), len(vals), (C.c_double * max(1, len(vals)))(*vals), out)
    if rc:
        raise BlurError(rc, "gaussian_sigmas_plan: bad arguments")
    return [(out[3 * c], out[3 * c + 1], out[3 * c + 2]) for c in range(len(vals))]


def gaussian_frame_sigmas_plan(rows, cols, sigmas):
    """how a one-sigma-per-frame Gaussian call groups its frames (host only, no GPU): a list with one (group, pad, nkb, slot) per
    frame.  group: the frames of one window class share a launch and an index, counted by first frame, -1 for sigma = 0 (the frame
    is copied); pad: pffft_sizing's; nkb: the fused kernel's window class, 0 where the pad has none (pad > 168: the plane path);
    slot: frames of equal sigma share their tables and an index, -1 for sigma = 0"""
    vals = [float(v) for v in sigmas]
    out = (C.c_int * max(1, 4 * len(vals)))()
    rc = _L().blur_gaussian_frame_sigmas_plan(int(rows), int(cols), len(vals), (C.c_double * max(1, len(vals)))(*vals), out)
    if rc:
        raise BlurError(rc, "gaussian_frame_sigmas_plan: bad arguments")
    return [(out[4 * f], out[4 * f + 1], out[4 * f + 2], out[4 * f + 3]) for f in range(len(vals))]


def _broadcast_frames_layout(t):
    """(pitch, 0) in elements for frames [n, rows, cols, C] that all are one frame (`img.expand(n, -1, -1, -1)`: frame stride 0), None
    for any other tensor"""
    if t.dim() != 4 or t.shape[0] < 2 or t.stride(0) != 0:
        return None
    one = _gauss_strided_layout(tuple(t.shape[1:]), tuple(t.stride()[1:]))
    return None if one is None else (one[0], 0)


def fft_plan_radices(n):
    r = (C.c_int * 16)()
    k = _L().blur_fft_plan_radices(int(n), r)
    return [r[i] for i in range(k)]


# ---- the GPU context ------------------------------------------------------------------
# enum blur_engine (include/blur_amd.h)
ENGINES = {"auto": 0, "rows-first": 1, "wave-resident": 2, "matrix": 3, "fft": 5, "fused": 6}


class BlurContext:
    """Owns the plan / kernel-spectrum caches and the float32 workspace on one GPU
    (role of the PFFFT_Setup pair the reference rebuilds per call, Source.cpp:477-478)."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        self._lib = _L()
        rc = self._lib.blur_ctx_create(C.byref(self._h), int(device))
        if rc:
            raise BlurError(rc, self._lib.blur_last_error(None).decode())
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.blur_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise BlurError(rc, self._lib.blur_last_error(self._h).decode())

    def _opts(self, nyquist_quirk=True, col_group=0, force_generic=False, frames_per_launch=0, row_major_planes=False,
              wave_resident=None, engine=None, tile_points=0):
        # one blur_opts per distinct argument tuple, built once (a call on a small image is tens of microseconds of GPU time: the
        # wrapper must not cost more than the kernels)
        key = (bool(nyquist_quirk), int(col_group), bool(force_generic), int(frames_per_launch), bool(row_major_planes), wave_resident, engine, int(tile_points))
        cache = self.__dict__.setdefault("_opts_cache", {})
        o = cache.get(key)
        if o is not None:
            return o
        o = cache[key] = self._build_opts(*key)
        return o

    def _build_opts(self, nyquist_quirk, col_group, force_generic, frames_per_launch, row_major_planes, wave_resident, engine, tile_points=0):
        o = BlurOpts()
        self._lib.blur_opts_default(C.byref(o))
        o.nyquist_quirk = 1 if nyquist_quirk else 0
        o.col_group = int(col_group)
        o.force_generic = 1 if force_generic else 0   # tests: run the run-time-planned kernels even where a specialised one exists
        o.frames_per_launch = int(frames_per_launch)
        o.row_major_planes = 1 if row_major_planes else 0
        # wave-resident kernels (transform length 256 * R0, columns first): None = where they pay (the image fills most
        # of the transform), False = never, True = wherever the image fits one
        o.engine = 0 if wave_resident is None else (2 if wave_resident else 1)
        # engine (enum blur_engine): None = the library's choice (the fused matrix-core kernel where it applies, else the two-kernel
        # matrix-core engine, else the FFT kernels); "fused" / "matrix" = Toeplitz products on the f16 matrix cores in one kernel
        # (fx_kernels.hpp) / two (mx_kernels.hpp); "fft" = the FFT kernels with their own measured choice of family;
        # "wave-resident" / "rows-first" = one FFT family
        if engine is not None:
            o.engine = ENGINES[engine]
        o.tile_points = int(tile_points)      # tests: force the tiled wave-resident path with transforms of at most this many points
        return o

    def use_torch_stream(self):
        """launch on torch's current stream of this device (the raw handle: torch.cuda.current_stream() builds a Stream object per
        call, several microseconds; the context is only told when the handle changed)"""
        import torch
        try:
            h = torch._C._cuda_getCurrentRawStream(self.device)
        except AttributeError:  # pragma: no cover - older / newer torch without the private accessor
            h = torch.cuda.current_stream(self.device).cuda_stream
        if h != self.__dict__.get("_stream_handle", -1):
            self._check(self._lib.blur_ctx_set_stream(self._h, C.c_void_p(h)))
            self._stream_handle = h

    def set_stream(self, handle):
        self._check(self._lib.blur_ctx_set_stream(self._h, C.c_void_p(handle)))
        self._stream_handle = handle

    def synchronize(self):
        self._check(self._lib.blur_ctx_synchronize(self._h))

    def last_family(self):
        """kernels the last u8c3 blur ran on: 0 run-time plans, 1 rows-first, 2 wave-resident, 3 whole-image 2D, 4 matrix-core
        (two kernels), 6 fused matrix-core (debug query, not declared in the public header)"""
        fn = self._lib.blur_debug_last_family
        fn.argtypes = [C.c_void_p]
        fn.restype = C.c_int
        return int(fn(self._h))

    def last_engine(self):
        """(family code, note): the kernels the last u8c3 blur ran on and, under the library's own choice, why a faster engine was
        passed over (blur_last_engine)"""
        buf = C.create_string_buffer(512)
        fam = int(self._lib.blur_last_engine(self._h, buf, 512))
        return fam, buf.value.decode()

    def copy_bandwidth(self, mib=1024, reps=5):
        """GB/s (read + written) of a 16-byte-per-lane device copy of `mib` MiB: the box's streaming rate for the kernels' access shape"""
        g = C.c_double(0)
        self._check(self._lib.blur_copy_bandwidth(self._h, int(mib) << 20, int(reps), C.byref(g)))
        return g.value

    def timing_enable(self, on=True):
        """per-kernel HIP events on the launch stream: True / 1 = every timed launch, 2 = slot 0 only (the dominant kernel), False = off"""
        self._check(self._lib.blur_ctx_timing_enable(self._h, 2 if on == 2 and on is not True else (1 if on else 0)))

    def timing(self, reset=True):
        ms = (C.c_double * 2)()
        n = (C.c_int * 2)()
        fr = (C.c_int * 2)()
        self._check(self._lib.blur_ctx_timing(self._h, ms, n, fr, 1 if reset else 0))
        return dict(row_ms=ms[0], col_ms=ms[1], row_launches=n[0], col_launches=n[1], row_frames=fr[0], col_frames=fr[1])

    # -- pffft_(image, sigma): Source.cpp:429-570 -----------------------------------------
    def pffft_(self, image, sigma, out=None, nyquist_quirk=True, col_group=0, force_generic=False, frames_per_launch=0,
               row_major_planes=False, wave_resident=None, engine=None, tile_points=0):
        """Gaussian blur of a BGR/RGB uint8 image [rows, cols, 3] or a batch [n, rows, cols, 3].

        torch CUDA tensor: asynchronous on torch's current stream, returns `out`
        (default: in place, like the reference).  numpy array: host round trip, returns a new array.
        """
        o = self._opts(nyquist_quirk, col_group, force_generic, frames_per_launch, row_major_planes, wave_resident, engine, tile_points)
        if isinstance(image, np.ndarray):
            if (image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3 and not image.flags["C_CONTIGUOUS"]
                    and image.strides[2] == 1 and image.strides[1] == 3 and image.strides[0] >= 3 * image.shape[1]):
                # a view with padded rows (a cv::Mat ROI): pitched entry point, no host-side repacking
                res = np.empty(image.shape, np.uint8)
                self._check(self._lib.blur_gaussian_u8c3_host_pitched(self._h, image.ctypes.data, image.strides[0], res.ctypes.data,
                                                                      res.strides[0], image.shape[0], image.shape[1], float(sigma), C.byref(o)))
                return res
            a = np.ascontiguousarray(image, np.uint8)
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError("expected a uint8 image of shape [rows, cols, 3]")
            res = np.empty_like(a)
            self._check(self._lib.blur_gaussian_u8c3_host(self._h, a.ctypes.data, res.ctypes.data, a.shape[0], a.shape[1],
                                                          float(sigma), C.byref(o)))
            return res
        import torch
        t = image
        if t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous() or t.shape[-1] != 3 or t.dim() not in (3, 4):
            raise ValueError("expected a contiguous CUDA uint8 tensor [rows, cols, 3] or [n, rows, cols, 3]")
        dst = t if out is None else out
        if dst.shape != t.shape or dst.dtype != t.dtype or not dst.is_cuda or not dst.is_contiguous():
            raise ValueError("out must match the input")
        self.use_torch_stream()
        n = 1 if t.dim() == 3 else t.shape[0]
        rows, cols = t.shape[-3], t.shape[-2]
        self._check(self._lib.blur_gaussian_u8c3_batch_dev(self._h, t.data_ptr(), dst.data_ptr(), n, rows, cols, float(sigma), C.byref(o)))
        return dst

    def convolve_lines(self, lines, multipliers, out=None):
        """lines: CUDA complex64 tensor [nlines, n]; multipliers: n real factors (numpy float32, natural frequency order).
        Returns IDFT(multipliers * DFT(line)) per line, unnormalised (blur_convolve_lines_c32_dev): the batched form of
        pffft_transform_ordered / pffft_sorted_optimized_convolution / pffft_transform_ordered (Source.cpp:531-533)."""
        import torch
        t = lines
        if t.dtype != torch.complex64 or not t.is_cuda or not t.is_contiguous() or t.dim() != 2:
            raise ValueError("expected a contiguous CUDA complex64 tensor [nlines, n]")
        dst = torch.empty_like(t) if out is None else out
        m = np.ascontiguousarray(multipliers, np.float32)
        if m.shape != (t.shape[1],):
            raise ValueError("one multiplier per frequency")
        self.use_torch_stream()
        self._check(self._lib.blur_convolve_lines_c32_dev(self._h, t.data_ptr(), dst.data_ptr(), t.shape[0], t.shape[1], m.ctypes.data))
        return dst

    def pinned_empty(self, shape, dtype=np.uint8):
        """numpy array in page-locked host memory (blur_host_alloc); freed when the array and its views are gone"""
        import weakref
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        self._check(self._lib.blur_host_alloc(self._h, C.byref(p), n))
        raw = (C.c_uint8 * max(n, 1)).from_address(p.value)
        lib, h, addr = self._lib, self._h, p.value
        weakref.finalize(raw, lambda: lib.blur_host_free(h, addr))
        return np.frombuffer(raw, np.uint8, n).view(dtype).reshape(shape)

    def pffft_host_batch(self, frames, sigma, out=None, nyquist_quirk=True):
        """frames: numpy uint8 [n, rows, cols, 3] in host memory (pinned_empty() for full PCIe overlap);
        copies in, kernels and copies out are pipelined over three device slots.  Returns `out` (default: a new array)."""
        a = frames
        if not (isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.ndim == 4 and a.shape[3] == 3 and a.flags["C_CONTIGUOUS"]):
            raise ValueError("expected a contiguous uint8 array [n, rows, cols, 3]")
        res = np.empty_like(a) if out is None else out
        if res.shape != a.shape or res.dtype != np.uint8 or not res.flags["C_CONTIGUOUS"]:
            raise ValueError("out must match the input")
        o = self._opts(nyquist_quirk)
        self._check(self._lib.blur_gaussian_u8c3_host_batch(self._h, a.ctypes.data, res.ctypes.data, a.shape[0], a.shape[1], a.shape[2],
                                                            float(sigma), C.byref(o)))
        return res

    def pocketfft_1D(self, image, sigma, out=None, **kw):
        """pocketfft_1D(image, sigma) (Source.cpp:280-392): the same 1D tiles as pffft_() with N/2+1 bins and the
        true Nyquist multiplier (:362,:378) -- this engine's `nyquist_quirk = 0` mode."""
        return self.pffft_(image, sigma, out=out, nyquist_quirk=False, **kw)

    def pocketfft_2D(self, image, sigma, out=None, **kw):
        """pocketfft_2D(image, sigma) (Source.cpp:143-277): Reflect_101 of the whole image, 2D r2c, separable
        multiply, c2r, crop.  Inside the crop that is the linear convolution of the reflect-101 extended image with
        the same taps (every border is >= the kernel half width, so neither the wrap-around nor the extra
        transform-size padding reaches a kept pixel): the 1D-tiled engine computes it without materialising the
        padded image.  tests/ compare with the scipy.fft (pocketfft) restatement of the 2D path.

        whole_image=True runs the reference's own structure instead (blur_pocketfft2d_u8c3_dev: the padded image as
        ONE 2D transform with pocketfft_2D's sizes and borders); want_planes=True then also returns the float planes
        [3, rows, cols] before the "+0.5f, truncate"."""
        if kw.pop("whole_image", False):
            return self._pocketfft2d(image, sigma, out, 0, kw.pop("want_planes", False))
        return self.pffft_(image, sigma, out=out, nyquist_quirk=False, **kw)

    def DFT_image(self, image, sigma, out=None, want_planes=False):
        """pocketfft_2D compiled with `#define DFT_image` (Source.cpp:235-252): every plane becomes the fft-shifted
        log spectrum 20 log10(|Re F| + 1e-5) of the reflect-101 padded plane (sigma only sets the padding), read with
        the reference's index arithmetic, interleaved ("+0.5f, truncate") and cropped like the blur."""
        return self._pocketfft2d(image, sigma, out, 1, want_planes)

    def _pocketfft2d(self, image, sigma, out, dft_image, want_planes):
        if isinstance(image, np.ndarray):                       # host round trip, returns a new array
            a = np.ascontiguousarray(image, np.uint8)
            if a.ndim != 3 or a.shape[2] != 3 or want_planes:
                raise ValueError("expected a uint8 image [rows, cols, 3] (float planes: device tensors only)")
            res = np.empty_like(a)
            self._check(self._lib.blur_pocketfft2d_u8c3_host(self._h, a.ctypes.data, res.ctypes.data, a.shape[0], a.shape[1], float(sigma), int(dft_image)))
            return res
        import torch
        if image.dtype != torch.uint8 or not image.is_cuda or not image.is_contiguous() or image.dim() != 3 or image.shape[-1] != 3:
            raise ValueError("expected a contiguous CUDA uint8 tensor [rows, cols, 3]")
        dst = image if out is None else out
        planes = torch.empty((3, image.shape[0], image.shape[1]), dtype=torch.float32, device=image.device) if want_planes else None
        self.use_torch_stream()
        self._check(self._lib.blur_pocketfft2d_u8c3_dev(self._h, image.data_ptr(), dst.data_ptr(), image.shape[0], image.shape[1], float(sigma),
                                                        int(dft_image), planes.data_ptr() if want_planes else None))
        return (dst, planes) if want_planes else dst

    def Reflect_101(self, image, top, bottom, left, right):
        """Reflect_101<uint8_t, C> (Utils.hpp:212-243): uint8 CUDA tensor [rows, cols, C] -> padded tensor; borders are
        clamped to dim - 1 like the reference"""
        import torch
        rows, cols, ch = image.shape
        size = (C.c_int * 2)()
        self._check(self._lib.blur_reflect101_u8_dev(self._h, None, None, rows, cols, ch, int(top), int(bottom), int(left), int(right), size))
        out = torch.empty((size[0], size[1], ch), dtype=torch.uint8, device=image.device)
        self.use_torch_stream()
        self._check(self._lib.blur_reflect101_u8_dev(self._h, image.data_ptr(), out.data_ptr(), rows, cols, ch, int(top), int(bottom), int(left), int(right), size))
        return out

    def pffft_boxblur(self, image, nsmooth, out=None, nyquist_quirk=True):
        """pffft_() compiled with `#define boxblur`: FFT-domain tent kernel (Source.cpp:437-442,468-472);
        uint8 CUDA tensor [rows, cols, 3]"""
        o = self._opts(nyquist_quirk)
        dst = image if out is None else out
        self.use_torch_stream()
        self._check(self._lib.blur_boxfft_u8c3_dev(self._h, image.data_ptr(), dst.data_ptr(), image.shape[0], image.shape[1],
                                                   float(nsmooth), C.byref(o)))
        return dst

    def separable(self, image, taps, pad=None, out=None, nyquist_quirk=True, engine=None):
        """any symmetric separable kernel (odd tap count) through the same engines; pad defaults to len(taps)//2"""
        o = self._opts(nyquist_quirk, engine=engine)
        t = np.ascontiguousarray(taps, np.float32)
        dst = image if out is None else out
        self.use_torch_stream()
        self._check(self._lib.blur_separable_u8c3_dev(self._h, image.data_ptr(), dst.data_ptr(), image.shape[0], image.shape[1],
                                                      t.ctypes.data, t.size, t.size // 2 if pad is None else int(pad), C.byref(o)))
        return dst

    def pffft_plane(self, plane, sigma, out=None, nyquist_quirk=True, col_group=0):
        """the per-channel body of pffft_() on one float32 plane (Source.cpp:510-564)"""
        o = self._opts(nyquist_quirk, col_group)
        if isinstance(plane, np.ndarray):
            a = np.ascontiguousarray(plane, np.float32)
            res = np.empty_like(a)
            self._check(self._lib.blur_gaussian_f32c1_host(self._h, a.ctypes.data, res.ctypes.data, a.shape[0], a.shape[1],
                                                           float(sigma), C.byref(o)))
            return res
        import torch
        t = plane
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.dim() != 2:
            raise ValueError("expected a contiguous CUDA float32 tensor [rows, cols]")
        dst = torch.empty_like(t) if out is None else out
        self.use_torch_stream()
        self._check(self._lib.blur_gaussian_f32c1_dev(self._h, t.data_ptr(), dst.data_ptr(), t.shape[0], t.shape[1], float(sigma), C.byref(o)))
        return dst

    def rowpass(self, image, sigma, nyquist_quirk=True, force_generic=False, engine=None):
        """row pass only: uint8 [rows, cols, 3] CUDA tensor -> float32 [3, rows, cols] (Source.cpp:520-537); engine="fused": the planes the
        fused matrix-core kernel hands from its row pass to its column pass (a test build of the kernel writes them out)"""
        import torch
        o = self._opts(nyquist_quirk, 0, force_generic, engine=engine)
        rows, cols = image.shape[0], image.shape[1]
        planes = torch.empty((3, rows, cols), dtype=torch.float32, device=image.device)
        self.use_torch_stream()
        self._check(self._lib.blur_rowpass_u8c3_dev(self._h, image.data_ptr(), planes.data_ptr(), rows, cols, float(sigma), C.byref(o)))
        return planes

    # -- the pieces either side ----------------------------------------------------------------
    def flip_block(self, plane, w, h):
        """flip_block<float,1>(in, out, w, h) -- call sites Source.cpp:540,562"""
        import torch
        out = torch.empty_like(plane)
        self.use_torch_stream()
        self._check(self._lib.blur_flip_block_f32_dev(self._h, plane.data_ptr(), out.data_ptr(), int(w), int(h)))
        return out

    def deinterleave_BGR(self, image):
        """deinterleave_BGR<uint8_t,float> -- Utils.hpp:159-184; returns float32 [3, total]"""
        import torch
        total = image.numel() // 3
        planes = torch.empty((3, total), dtype=torch.float32, device=image.device)
        self.use_torch_stream()
        self._check(self._lib.blur_deinterleave_bgr_u8_f32_dev(self._h, image.data_ptr(), planes.data_ptr(), total))
        return planes

    def interleave_BGR(self, planes):
        """interleave_BGR<uint8_t,float> -- Utils.hpp:186-210; planes float32 [3, total]"""
        import torch
        total = planes.shape[1]
        out = torch.empty(total * 3, dtype=torch.uint8, device=planes.device)
        self.use_torch_stream()
        self._check(self._lib.blur_interleave_bgr_f32_u8_dev(self._h, planes.data_ptr(), out.data_ptr(), total))
        return out

    def gaussian(self, image, sigma, out=None, nyquist_quirk=True, engine=None):
        """Gaussian blur of a 1-, 3- or 4-channel uint8 image (grayscale, BGR, BGRA / RGBA): [rows, cols], [rows, cols, C] or a batch
        [n, rows, cols, C], C in {1, 3, 4}.  Every channel, alpha included, is blurred on its own exactly as pffft_ blurs one of
        its three (blur_gaussian_u8_batch_dev).  engine: None (the library's choice), "fused" or "fft".
        sigma: a number, or a sequence of C numbers, one per channel (blur_gaussian_u8_sigmas_batch_dev): channel c is blurred as the
        scalar call with sigma[c] blurs it, and 0 leaves the channel as it is (BGRA with (s, s, s, 0): the alpha is untouched).  The
        same holds for gaussian_f32, gaussian_u16, gaussian_f16 and gaussian_bf16.

        torch CUDA tensor: asynchronous on torch's current stream, returns `out` (default: in place, like pffft_).  numpy array:
        host round trip, returns a new array.

        The CUDA tensor, and `out` independently, may be a pitched view instead of a contiguous tensor: a region of interest
        `frames[:, y0:y1, x0:x1, :]`, a surface whose rows are padded (strides (frame_stride, pitch, C, 1), (pitch, C, 1) or
        (pitch, 1), pitch >= cols * C).  Nothing is repacked and nothing outside the view is written; `out=None` blurs the view in
        place.  Channel slices, stepped, flipped or permuted views raise ValueError.  The same holds for gaussian_f32, gaussian_u16,
        gaussian_f16 and gaussian_bf16; BlurMulti takes contiguous frames only.
        """
        return self._gaussian(image, sigma, out, nyquist_quirk, engine, np.uint8, "u8")

    def gaussian_f32(self, image, sigma, out=None, nyquist_quirk=True, engine=None):
        """Gaussian blur of a float32 image of 1, 3 or 4 channels: [rows, cols], [rows, cols, C] or a batch [n, rows, cols, C].  Every
        channel is blurred on its own as pffft_ blurs one of its planes, without the + 0.5f truncation (blur_gaussian_f32_batch_dev).
        engine: None (the library's choice), "fused" or "fft".

        torch CUDA tensor: asynchronous on torch's current stream, returns `out` (default: in place).  numpy array: host round trip,
        returns a new array.
        """
        return self._gaussian(image, sigma, out, nyquist_quirk, engine, np.float32, "f32")

    def gaussian_u16(self, image, sigma, out=None, nyquist_quirk=True, engine=None):
        """Gaussian blur of a uint16 image of 1, 3 or 4 channels: [rows, cols], [rows, cols, C] or a batch [n, rows, cols, C].  Every
        channel is blurred on its own as pffft_ blurs one of its planes; the float result v leaves as (v + 0.5) truncated, low 16
        bits kept: no clamping (blur_gaussian_u16_batch_dev).  engine: None (the library's choice), "fused" or "fft".

        torch CUDA tensor (torch.uint16): asynchronous on torch's current stream, returns `out` (default: in place).  numpy array:
        host round trip, returns a new array.
        """
        return self._gaussian(image, sigma, out, nyquist_quirk, engine, np.uint16, "u16")

    def gaussian_f16(self, image, sigma, out=None, nyquist_quirk=True, engine=None):
        """Gaussian blur of a float16 (IEEE binary16) image of 1, 3 or 4 channels: [rows, cols], [rows, cols, C] or a batch [n, rows,
        cols, C].  Every channel is blurred on its own as pffft_ blurs one of its planes; the float result is rounded once to
        float16, to nearest even, values past 65504 to +-Inf (blur_gaussian_f16_batch_dev).  engine: None (the library's choice),
        "fused" or "fft".

        torch CUDA tensor (torch.float16): asynchronous on torch's current stream, returns `out` (default: in place).  numpy float16
        array: host round trip, returns a new array.  A uint16 array is refused: it is a u16 image (gaussian_u16).
        """
        return self._gaussian(image, sigma, out, nyquist_quirk, engine, np.float16, "f16")

    def gaussian_bf16(self, image, sigma, out=None, nyquist_quirk=True, engine=None):
        """Gaussian blur of a bfloat16 image of 1, 3 or 4 channels: [rows, cols], [rows, cols, C] or a batch [n, rows, cols, C].  Every
        channel is blurred on its own as pffft_ blurs one of its planes; the float result is rounded once to bfloat16, to nearest
        even (blur_gaussian_bf16_batch_dev).  engine: None (the library's choice), "fused" or "fft".

        torch CUDA tensor (torch.bfloat16): asynchronous on torch's current stream, returns `out` (default: in place).  CPU
        torch.bfloat16 tensor: host round trip, returns a new CPU tensor (numpy has no bfloat16; a numpy array is refused).
        """
        return self._gaussian(image, sigma, out, nyquist_quirk, engine, BF16, "bf16")

    def gaussian_nv12(self, y, uv, sigma, out=None, nyquist_quirk=True, engine=None):
        """Gaussian blur of a decoded video surface where it lies: NV12 (uint8) or P010 / P016 (uint16).  y is the luma plane [rows,
        cols] or [n, rows, cols]; uv the plane of interleaved Cb/Cr pairs [rows / 2, cols / 2, 2] or [n, rows / 2, cols / 2, 2]; both
        row-pitched views with the same pitch (the two planes of one surface: `surf[:rows, :cols]` and `surf[h:h + rows // 2,
        :cols].view(rows // 2, cols // 2, 2)`), or contiguous tensors.  The strides supply the pitch and the two frame strides.
        sigma: a number s blurs all three planes alike in luma pixels -- (s, s / 2, s / 2), each sigma being in pixels of its own
        plane; a sequence (Y, Cb, Cr) is taken as given, and 0 leaves that plane or channel as it is (`(0, 5, 5)`: the chroma
        smoothing of a YCrCb image).  Each plane is, bit for bit, what gaussian() / gaussian_u16() returns for it as a one-channel
        image (blur_gaussian_nv12_batch_dev, blur_gaussian_p016_batch_dev).  P016 results keep all 16 bits: the low bits of P010
        data are not masked.  engine: None (the library's choice), "fused" or "fft", per plane.

        torch CUDA tensors: asynchronous on torch's current stream; out=(y_out, uv_out) or, by default, in place; returns (y_out,
        uv_out).  numpy arrays (contiguous): host round trip, returns new arrays (or `out`).  ValueError, before the library is
        called: mismatched shapes or dtypes, odd sizes, unequal row pitches of y and uv, anything that is not a row-pitched view.
        """
        sg = (C.c_double * 3)(*_nv12_sigmas(sigma))
        o = self._opts(nyquist_quirk, engine=engine)
        if isinstance(y, np.ndarray) or isinstance(uv, np.ndarray):
            if not (isinstance(y, np.ndarray) and isinstance(uv, np.ndarray)) or y.dtype != uv.dtype or y.dtype not in (np.uint8, np.uint16):
                raise ValueError("expected uint8 (NV12) or uint16 (P016) arrays y and uv")
            ya, uva = np.ascontiguousarray(y), np.ascontiguousarray(uv)
            n, rows, cols, _, _, _ = _nv12_layout(ya.shape, [s // ya.itemsize for s in ya.strides], uva.shape, [s // uva.itemsize for s in uva.strides])
            yo, uvo = (np.empty_like(ya), np.empty_like(uva)) if out is None else out
            for t, s in ((yo, ya), (uvo, uva)):
                if not isinstance(t, np.ndarray) or t.shape != s.shape or t.dtype != s.dtype or not t.flags["C_CONTIGUOUS"]:
                    raise ValueError("out must match the input: contiguous (y_out, uv_out)")
            host_entry = self._lib.blur_gaussian_nv12_host if ya.dtype == np.uint8 else self._lib.blur_gaussian_p016_host
            ny = rows * cols
            for f in range(n):
                src = np.concatenate([ya.reshape(n, -1)[f], uva.reshape(n, -1)[f]])
                res = np.empty_like(src)
                self._check(host_entry(self._h, src.ctypes.data, res.ctypes.data, rows, cols, sg, C.byref(o)))
                yo.reshape(n, -1)[f] = res[:ny]
                uvo.reshape(n, -1)[f] = res[ny:]
            return yo, uvo
        y, uv, yo, uvo, sl, dl = _nv12_tensors(y, uv, out)
        n, rows, cols = sl[:3]
        es = y.element_size()
        self.use_torch_stream()
        entry = self._lib.blur_gaussian_nv12_batch_dev if es == 1 else self._lib.blur_gaussian_p016_batch_dev
        self._check(entry(self._h, y.data_ptr(), uv.data_ptr(), sl[3] * es, sl[4] * es, sl[5] * es, yo.data_ptr(), uvo.data_ptr(), dl[3] * es, dl[4] * es, dl[5] * es,
                          n, rows, cols, sg, C.byref(o)))
        return yo, uvo

    def gaussian_per_frame(self, frames, sigmas, out=None, nyquist_quirk=True, engine=None):
        """Gaussian blur of uint8 frames [n, rows, cols, C] or [n, rows, cols] (C in {1, 3, 4}) with one sigma per FRAME: `sigmas` is a
        sequence of n numbers, frame f is what gaussian() returns for it alone with sigmas[f], and 0 copies the frame
        (blur_gaussian_u8_frame_sigmas_batch_dev: the frames of one window class share one launch, whatever their sigmas).  The
        one exception to "what gaussian() returns": three-channel frames run on the one-channel-per-workgroup kernel, never on
        gaussian()'s three-channel kernels, and meet the same oracle; with ONE sigma for all BGR frames call gaussian().
        engine: None (the library's choice), "fused" or "fft", frame by frame.

        torch CUDA tensor: asynchronous on torch's current stream, returns `out` (default: in place).  The tensor, and `out`
        independently, may be the pitched views gaussian() accepts.  A source whose frame stride is 0 -- `img.expand(k, -1, -1,
        -1)`: one frame, k sigmas, k results (scale space, difference of Gaussians) -- is accepted too and needs `out`.
        numpy array: host round trip frame by frame through the scalar entry, returns a new array.
        """
        return self._gaussian_per_frame(frames, sigmas, out, nyquist_quirk, engine, np.uint8, "u8")

    def gaussian_f32_per_frame(self, frames, sigmas, out=None, nyquist_quirk=True, engine=None):
        """gaussian_per_frame for float32 frames: frame f is, bit for bit, what gaussian_f32() returns for it alone with sigmas[f] (its
        power-of-two scale comes from its own max|x|), for 1, 3 and 4 channels (blur_gaussian_f32_frame_sigmas_batch_dev)."""
        return self._gaussian_per_frame(frames, sigmas, out, nyquist_quirk, engine, np.float32, "f32")

    def gaussian_u16_per_frame(self, frames, sigmas, out=None, nyquist_quirk=True, engine=None):
        """gaussian_per_frame for uint16 frames (torch.uint16 or numpy uint16): frame f is, bit for bit, what gaussian_u16() returns for
        it alone with sigmas[f], for 1, 3 and 4 channels (blur_gaussian_u16_frame_sigmas_batch_dev)."""
        return self._gaussian_per_frame(frames, sigmas, out, nyquist_quirk, engine, np.uint16, "u16")

    def gaussian_f16_per_frame(self, frames, sigmas, out=None, nyquist_quirk=True, engine=None):
        """gaussian_per_frame for float16 frames (torch.float16 or numpy float16): frame f is, bit for bit, what gaussian_f16() returns
        for it alone with sigmas[f] (its power-of-two scale comes from its own max|x|), for 1, 3 and 4 channels
        (blur_gaussian_f16_frame_sigmas_batch_dev)."""
        return self._gaussian_per_frame(frames, sigmas, out, nyquist_quirk, engine, np.float16, "f16")

    def gaussian_bf16_per_frame(self, frames, sigmas, out=None, nyquist_quirk=True, engine=None):
        """gaussian_per_frame for bfloat16 frames (torch.bfloat16; a CPU tensor takes the host route): frame f is, bit for bit, what
        gaussian_bf16() returns for it alone with sigmas[f] (its power-of-two scale comes from its own max|x|), for 1, 3 and 4
        channels (blur_gaussian_bf16_frame_sigmas_batch_dev)."""
        return self._gaussian_per_frame(frames, sigmas, out, nyquist_quirk, engine, BF16, "bf16")

    def gaussian_nv12_per_frame(self, y, uv, sigmas, out=None, nyquist_quirk=True, engine=None):
        """Gaussian blur of a decoded clip with its own sigmas per FRAME (a focus pull, a blur ramp): NV12 (uint8) or P010 / P016
        (uint16).  y is [n, rows, cols], uv [n, rows / 2, cols / 2, 2], with the views and layout rules of gaussian_nv12.  `sigmas`
        is a sequence of n entries, each a number s -- (s, s / 2): the same blur in luma pixels on luma and chroma -- or a pair
        (sigma_y, sigma_c), each in pixels of its own plane; sigma_c blurs Cb and Cr alike, and a 0 leaves that plane of that frame
        as it is.  The planes of frame f are, bit for bit, what gaussian_nv12() returns for that frame alone with (sigma_y, sigma_c,
        sigma_c) (blur_gaussian_nv12_frame_sigmas_batch_dev, blur_gaussian_p016_frame_sigmas_batch_dev: per plane, the frames of one
        window class share one launch).  engine: None (the library's choice), "fused" or "fft", per plane and frame.

        torch CUDA tensors: asynchronous on torch's current stream; out=(y_out, uv_out) or, by default, in place; returns (y_out,
        uv_out).  numpy arrays (contiguous): host round trip frame by frame through the scalar entry, returns new arrays (or
        `out`).  ValueError, before the library is called: what gaussian_nv12 refuses, y that is not [n, rows, cols], sigmas of
        another length than n, an entry that is neither a number nor a pair.
        """
        if isinstance(y, np.ndarray) or isinstance(uv, np.ndarray):
            if not (isinstance(y, np.ndarray) and isinstance(uv, np.ndarray)):
                raise ValueError("expected uint8 (NV12) or uint16 (P016) arrays y and uv")
            pairs = _nv12_frame_sigmas(sigmas, y)
            n = y.shape[0]
            if len(uv.shape) != 4 or uv.shape[0] != n:
                raise ValueError("uv must be [n, rows / 2, cols / 2, 2] for y [n, rows, cols]")
            yo, uvo = (np.empty_like(np.ascontiguousarray(y)), np.empty_like(np.ascontiguousarray(uv))) if out is None else out
            for f in range(n):
                sy, sc = pairs[f]
                self.gaussian_nv12(y[f:f + 1], uv[f:f + 1], (sy, sc, sc), out=(yo[f:f + 1], uvo[f:f + 1]), nyquist_quirk=nyquist_quirk, engine=engine)
            return yo, uvo
        y, uv, yo, uvo, sl, dl, pairs = _nv12_per_frame_tensors(y, uv, sigmas, out)
        n, rows, cols = sl[:3]
        sg = (C.c_double * max(1, 2 * n))(*[v for p in pairs for v in p])
        o = self._opts(nyquist_quirk, engine=engine)
        es = y.element_size()
        self.use_torch_stream()
        entry = self._lib.blur_gaussian_nv12_frame_sigmas_batch_dev if es == 1 else self._lib.blur_gaussian_p016_frame_sigmas_batch_dev
        self._check(entry(self._h, y.data_ptr(), uv.data_ptr(), sl[3] * es, sl[4] * es, sl[5] * es, yo.data_ptr(), uvo.data_ptr(), dl[3] * es, dl[4] * es, dl[5] * es,
                          n, rows, cols, sg, C.byref(o)))
        return yo, uvo

    def _gaussian_per_frame(self, frames, sigmas, out, nyquist_quirk, engine, dtype, tname):
        o = self._opts(nyquist_quirk, engine=engine)
        vals = [float(v) for v in sigmas]
        if len(frames.shape) not in (3, 4):
            raise ValueError("expected frames [n, rows, cols, C] or [n, rows, cols]")
        if len(vals) != frames.shape[0]:
            raise ValueError("sigmas: expected one per frame (%d), got %d" % (frames.shape[0], len(vals)))
        sg = (C.c_double * max(1, len(vals)))(*vals)
        if _is_host_frames(frames, dtype):
            a, res, _ = _gauss_array(frames if frames.ndim == 4 else frames[..., None], out if out is None or out.ndim == 4 else out[..., None], dtype, batch=True)
            n, rows, cols, ch = a.shape
            host_entry = getattr(self._lib, "blur_gaussian_%s_host" % tname)
            for f in range(n):
                if vals[f] == 0:
                    res[f] = a[f]
                else:
                    self._check(host_entry(self._h, a[f].ctypes.data, res[f].ctypes.data, rows, cols, ch, vals[f], C.byref(o)))
            res = _gauss_result(res, out, dtype)
            return res if frames.ndim == 4 or out is not None else res[..., 0]
        import torch
        t4 = frames.unsqueeze(-1) if isinstance(frames, torch.Tensor) and frames.dim() == 3 else frames
        o4 = out.unsqueeze(-1) if isinstance(out, torch.Tensor) and out.dim() == 3 else out
        bl = _broadcast_frames_layout(t4) if isinstance(t4, torch.Tensor) else None
        if bl is not None:
            if o4 is None:
                raise ValueError("frames with a frame stride of 0 (one frame, several sigmas) need `out`: there is no in-place result")
            # (the checks of _gauss_tensor on one frame of the source and on the whole result)
            _gauss_tensor(t4[0], None, dtype)
            _, dst, (n, rows, cols, ch), _ = _gauss_tensor(o4, None, dtype)
            if tuple(o4.shape) != tuple(t4.shape):
                raise ValueError("out must match the input")
            es = t4.element_size()
            dl = _gauss_strided_layout(dst.shape, dst.stride())
            lay = (bl[0] * es, 0, dl[0] * es, dl[1] * es)
            t = t4
        else:
            t, dst, (n, rows, cols, ch), lay = _gauss_tensor(t4, o4, dtype)
            if t.dim() != 4:
                raise ValueError("expected frames [n, rows, cols, C] or [n, rows, cols]")
        self.use_torch_stream()
        if lay is not None:
            pitched_entry = getattr(self._lib, "blur_gaussian_%s_frame_sigmas_pitched_batch_dev" % tname)
            self._check(pitched_entry(self._h, t.data_ptr(), lay[0], lay[1], dst.data_ptr(), lay[2], lay[3], n, rows, cols, ch, sg, C.byref(o)))
        else:
            batch_entry = getattr(self._lib, "blur_gaussian_%s_frame_sigmas_batch_dev" % tname)
            self._check(batch_entry(self._h, t.data_ptr(), dst.data_ptr(), n, rows, cols, ch, sg, C.byref(o)))
        return frames if out is None else out

    def _gaussian(self, image, sigma, out, nyquist_quirk, engine, dtype, tname):
        """tname: the entry points' type name (blur_gaussian_<tname>_host, _batch_dev; a sequence `sigma`: _sigmas_host, _sigmas_batch_dev)"""
        o = self._opts(nyquist_quirk, engine=engine)
        per_channel = _is_sigma_sequence(sigma)
        mid = "_sigmas" if per_channel else ""
        if _is_host_frames(image, dtype):
            a, res, (n, rows, cols, ch) = _gauss_array(image, out, dtype)
            sg = _sigma_arg(sigma, ch, a.ndim == 2)
            host_entry = getattr(self._lib, "blur_gaussian_%s%s_host" % (tname, mid))
            fb = rows * cols * ch * a.itemsize
            for f in range(n):
                self._check(host_entry(self._h, a.ctypes.data + f * fb, res.ctypes.data + f * fb, rows, cols, ch, sg, C.byref(o)))
            return _gauss_result(res, out, dtype)
        t, dst, (n, rows, cols, ch), lay = _gauss_tensor(image, out, dtype)
        sg = _sigma_arg(sigma, ch, t.dim() == 2)
        self.use_torch_stream()
        if lay is not None:           # a pitched view on either side (blur_gaussian_<tname>[_sigmas]_pitched_batch_dev): nothing is repacked
            pitched_entry = getattr(self._lib, "blur_gaussian_%s%s_pitched_batch_dev" % (tname, mid))
            self._check(pitched_entry(self._h, t.data_ptr(), lay[0], lay[1], dst.data_ptr(), lay[2], lay[3], n, rows, cols, ch, sg, C.byref(o)))
            return dst
        batch_dev_entry = getattr(self._lib, "blur_gaussian_%s%s_batch_dev" % (tname, mid))
        self._check(batch_dev_entry(self._h, t.data_ptr(), dst.data_ptr(), n, rows, cols, ch, sg, C.byref(o)))
        return dst

    def fastboxblur(self, image, ksize, passes):
        """fastboxblur(in, w, h, channels, ksize, passes), in place -- call site Source.cpp:587"""
        if isinstance(image, np.ndarray):
            a = np.array(image, np.uint8, order="C")
            h, w = a.shape[:2]
            ch = 1 if a.ndim == 2 else a.shape[2]
            self._check(self._lib.blur_fastboxblur_u8_host(self._h, a.ctypes.data, w, h, ch, int(ksize), int(passes)))
            return a
        h, w = image.shape[0], image.shape[1]
        ch = 1 if image.dim() == 2 else image.shape[2]
        self.use_torch_stream()
        self._check(self._lib.blur_fastboxblur_u8_dev(self._h, image.data_ptr(), w, h, ch, int(ksize), int(passes)))
        return image

    def fastboxblur_batch(self, frames, ksize, passes):
        """fastboxblur of every frame of a batch: frames uint8 [n, h, w] or [n, h, w, C].  A contiguous torch CUDA tensor is blurred
        in place on torch's current stream (blur_fastboxblur_u8_batch_dev) and returned; a numpy array goes through the host
        batch entry and the blurred copy is returned."""
        if isinstance(frames, np.ndarray):
            a = np.array(frames, np.uint8, order="C")
            n, w, h, ch = _box_frames_shape(a.shape)
            self._check(self._lib.blur_fastboxblur_u8_host_batch(self._h, a.ctypes.data, n, w, h, ch, int(ksize), int(passes)))
            return a
        import torch
        t = frames
        if t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous():
            raise ValueError("expected a contiguous CUDA uint8 tensor [n, h, w] or [n, h, w, C]")
        n, w, h, ch = _box_frames_shape(tuple(t.shape))
        self.use_torch_stream()
        self._check(self._lib.blur_fastboxblur_u8_batch_dev(self._h, t.data_ptr(), n, w, h, ch, int(ksize), int(passes)))
        return t


class BlurMulti:
    """Several GPUs (or several logical shards on one GPU) behind one handle: blur_multi_* of include/blur_amd.h.
    Frames of a batch are sharded by frame, one context and stream per shard, driven from this one host thread."""

    def __init__(self, devices):
        self._lib = _L()
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        self._h = C.c_void_p()
        rc = self._lib.blur_multi_create(C.byref(self._h), devs, len(devices))
        if rc:
            raise BlurError(rc, "blur_multi_create failed")
        self.devices = list(devices)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.blur_multi_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise BlurError(rc, self._lib.blur_multi_last_error(self._h).decode())

    def pffft_(self, frames, sigma, out=None, nyquist_quirk=True, wave_resident=None):
        """frames: uint8 [n, rows, cols, 3]; a torch CUDA tensor on devices[0] or a numpy array in host memory.  Synchronous."""
        o = BlurOpts()
        self._lib.blur_opts_default(C.byref(o))
        o.nyquist_quirk = 1 if nyquist_quirk else 0
        o.engine = 0 if wave_resident is None else (2 if wave_resident else 1)
        if isinstance(frames, np.ndarray):
            a = np.ascontiguousarray(frames, np.uint8)
            if a.ndim != 4 or a.shape[3] != 3:
                raise ValueError("expected uint8 frames [n, rows, cols, 3]")
            res = np.empty_like(a) if out is None else out
            self._check(self._lib.blur_gaussian_u8c3_batch_multi_host(self._h, a.ctypes.data, res.ctypes.data, a.shape[0], a.shape[1], a.shape[2],
                                                                      float(sigma), C.byref(o)))
            return res
        import torch
        t = frames
        if t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous() or t.dim() != 4 or t.shape[-1] != 3 or t.device.index != self.devices[0]:
            raise ValueError("expected a contiguous CUDA uint8 tensor [n, rows, cols, 3] on devices[0]")
        dst = t if out is None else out
        torch.cuda.synchronize(t.device)
        self._check(self._lib.blur_gaussian_u8c3_batch_multi_dev(self._h, t.data_ptr(), dst.data_ptr(), t.shape[0], t.shape[1], t.shape[2],
                                                                 float(sigma), C.byref(o)))
        return dst

    def gaussian(self, frames, sigma, out=None, nyquist_quirk=True, engine=None):
        """BlurContext.gaussian over a batch sharded by frame: frames uint8 [n, rows, cols, C], C in {1, 3, 4}; a torch CUDA
        tensor on devices[0] (default: in place) or a numpy array in host memory (a new array).  Synchronous."""
        return self._gaussian(frames, sigma, out, nyquist_quirk, engine, np.uint8, "u8")

    def gaussian_f32(self, frames, sigma, out=None, nyquist_quirk=True, engine=None):
        """BlurContext.gaussian_f32 over a batch sharded by frame: frames float32 [n, rows, cols, C], C in {1, 3, 4}; a torch CUDA
        tensor on devices[0] (default: in place) or a numpy array in host memory (a new array).  Synchronous."""
        return self._gaussian(frames, sigma, out, nyquist_quirk, engine, np.float32, "f32")

    def gaussian_u16(self, frames, sigma, out=None, nyquist_quirk=True, engine=None):
        """BlurContext.gaussian_u16 over a batch sharded by frame: frames uint16 [n, rows, cols, C], C in {1, 3, 4}; a torch CUDA
        tensor on devices[0] (default: in place) or a numpy array in host memory (a new array).  Synchronous."""
        return self._gaussian(frames, sigma, out, nyquist_quirk, engine, np.uint16, "u16")

    def gaussian_f16(self, frames, sigma, out=None, nyquist_quirk=True, engine=None):
        """BlurContext.gaussian_f16 over a batch sharded by frame: frames float16 [n, rows, cols, C], C in {1, 3, 4}; a torch CUDA
        tensor on devices[0] (default: in place) or a numpy array in host memory (a new array).  Synchronous."""
        return self._gaussian(frames, sigma, out, nyquist_quirk, engine, np.float16, "f16")

    def gaussian_bf16(self, frames, sigma, out=None, nyquist_quirk=True, engine=None):
        """BlurContext.gaussian_bf16 over a batch sharded by frame: frames torch.bfloat16 [n, rows, cols, C], C in {1, 3, 4}; a CUDA
        tensor on devices[0] (default: in place) or a CPU tensor (a new CPU tensor).  Synchronous."""
        return self._gaussian(frames, sigma, out, nyquist_quirk, engine, BF16, "bf16")

    def _gaussian(self, frames, sigma, out, nyquist_quirk, engine, dtype, tname):
        o = BlurOpts()
        self._lib.blur_opts_default(C.byref(o))
        o.nyquist_quirk = 1 if nyquist_quirk else 0
        if engine is not None:
            o.engine = ENGINES[engine]
        mid = "_sigmas" if _is_sigma_sequence(sigma) else ""
        if _is_host_frames(frames, dtype):
            a, res, (n, rows, cols, ch) = _gauss_array(frames, out, dtype, batch=True)
            multi_host_entry = getattr(self._lib, "blur_gaussian_%s%s_batch_multi_host" % (tname, mid))
            self._check(multi_host_entry(self._h, a.ctypes.data, res.ctypes.data, n, rows, cols, ch, _sigma_arg(sigma, ch), C.byref(o)))
            return _gauss_result(res, out, dtype)
        import torch
        t, dst, (n, rows, cols, ch), _ = _gauss_tensor(frames, out, dtype, device=self.devices[0])
        torch.cuda.synchronize(t.device)
        multi_dev_entry = getattr(self._lib, "blur_gaussian_%s%s_batch_multi_dev" % (tname, mid))
        self._check(multi_dev_entry(self._h, t.data_ptr(), dst.data_ptr(), n, rows, cols, ch, _sigma_arg(sigma, ch), C.byref(o)))
        return dst

    def fastboxblur(self, frames, ksize, passes):
        """fastboxblur of every frame: frames uint8 [n, h, w] or [n, h, w, C]; a torch CUDA tensor on devices[0] (blurred in place
        and returned) or a numpy array in host memory (the blurred copy is returned).  Synchronous."""
        if isinstance(frames, np.ndarray):
            a = np.array(frames, np.uint8, order="C")
            n, w, h, ch = _box_frames_shape(a.shape)
            self._check(self._lib.blur_fastboxblur_u8_batch_multi_host(self._h, a.ctypes.data, n, w, h, ch, int(ksize), int(passes)))
            return a
        import torch
        t = frames
        if t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous() or t.device.index != self.devices[0]:
            raise ValueError("expected a contiguous CUDA uint8 tensor [n, h, w] or [n, h, w, C] on devices[0]")
        n, w, h, ch = _box_frames_shape(tuple(t.shape))
        torch.cuda.synchronize(t.device)
        self._check(self._lib.blur_fastboxblur_u8_batch_multi_dev(self._h, t.data_ptr(), n, w, h, ch, int(ksize), int(passes)))
        return t
