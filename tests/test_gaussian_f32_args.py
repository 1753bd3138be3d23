"""blur_gaussian_f32_*: argument validation that needs no device (the checks run before the context is touched, so ctx may be
NULL), the bindings of the new entry points, the Python shape and dtype checks, and the per-frame scale rule of the fused float
kernel (ff_kernels.hpp: ff_scale_exp) mirrored in Python."""
import ctypes as C
import math

import numpy as np
import pytest

INVALID, UNSUPPORTED = 1, 2


def lib():
    from blur_algorithms_amd import _lib
    return _lib.load()


def opts():
    from blur_algorithms_amd._lib import BlurOpts
    o = BlurOpts()
    lib().blur_opts_default(C.byref(o))
    return o


BUF = (C.c_float * 64)()
P = C.addressof(BUF)


def entries(L):
    """(name, call(src, dst, nframes, rows, cols, channels, sigma)) for every float entry point"""
    o = opts()
    return [
        ("batch_dev", lambda s, d, n, r, c, ch, sg: L.blur_gaussian_f32_batch_dev(None, s, d, n, r, c, ch, sg, C.byref(o))),
        ("dev", lambda s, d, n, r, c, ch, sg: L.blur_gaussian_f32_dev(None, s, d, r, c, ch, sg, C.byref(o))),
        ("host", lambda s, d, n, r, c, ch, sg: L.blur_gaussian_f32_host(None, s, d, r, c, ch, sg, C.byref(o))),
    ]


def test_symbols_bound():
    L = lib()
    for name in ("blur_gaussian_f32_batch_dev", "blur_gaussian_f32_dev", "blur_gaussian_f32_host",
                 "blur_gaussian_f32_batch_multi_dev", "blur_gaussian_f32_batch_multi_host"):
        assert getattr(L, name) is not None


@pytest.mark.parametrize("channels", [0, 2, 5, -1, 3 * 256])
def test_bad_channel_count(channels):
    L = lib()
    for _, call in entries(L):
        assert call(P, P, 1, 4, 4, channels, 1.0) == INVALID
    o = opts()
    assert L.blur_gaussian_f32_batch_multi_dev(None, P, P, 1, 4, 4, channels, 1.0, C.byref(o)) == INVALID
    assert L.blur_gaussian_f32_batch_multi_host(None, P, P, 1, 4, 4, channels, 1.0, C.byref(o)) == INVALID


@pytest.mark.parametrize("channels", [1, 3, 4])
def test_null_pointers_counts_and_sizes(channels):
    L = lib()
    for _, call in entries(L):
        for src, dst in ((None, P), (P, None), (None, None)):
            assert call(src, dst, 1, 4, 4, channels, 1.0) == INVALID
        for rows, cols, sigma in ((0, 4, 1.0), (4, -1, 1.0), (4, 4, 0.0), (4, 4, -2.0)):
            assert call(P, P, 1, rows, cols, channels, sigma) == INVALID
    o = opts()
    assert L.blur_gaussian_f32_batch_dev(None, P, P, -1, 4, 4, channels, 1.0, C.byref(o)) == INVALID


@pytest.mark.parametrize("channels", [1, 3, 4])
def test_pad_too_large_and_zero_frames(channels):
    """pad > min(rows, cols) - 1 -> BLUR_ERR_UNSUPPORTED before the device; nframes == 0 and every argument valid: the only thing
    left is the missing context (BLUR_ERR_INVALID), so the shape checks passed"""
    import blur_algorithms_amd as B
    L = lib()
    rows, cols, big = 40, 90, 30.0
    assert B.pffft_sizing(rows, cols, big)["pad"] > rows - 1
    for _, call in entries(L):
        assert call(P, P, 1, rows, cols, channels, big) == UNSUPPORTED
        assert call(P, P, 1, rows, cols, channels, 2.0) == INVALID          # valid: no context
    o = opts()
    assert L.blur_gaussian_f32_batch_dev(None, P, P, 0, rows, cols, channels, big, C.byref(o)) == UNSUPPORTED
    assert L.blur_gaussian_f32_batch_dev(None, P, P, 0, rows, cols, channels, 2.0, C.byref(o)) == INVALID


def test_python_shapes_and_dtypes():
    from blur_algorithms_amd import api
    for shape in ((4, 5, 2), (2, 4, 5, 5), (4,), (1, 2, 3, 4, 1), (0, 5), (4, 0, 1)):
        with pytest.raises(ValueError):
            api._gauss_f32_frames_shape(shape)
    assert api._gauss_f32_frames_shape((4, 5)) == (1, 4, 5, 1)
    assert api._gauss_f32_frames_shape((4, 5, 3)) == (1, 4, 5, 3)
    assert api._gauss_f32_frames_shape((2, 4, 5, 4)) == (2, 4, 5, 4)
    assert api._gauss_f32_frames_shape is api._gauss_frames_shape          # one helper for both dtypes
    # dtype and layout are refused before the context is used
    ctx = object.__new__(api.BlurContext)
    ctx._lib = lib()
    ctx._h = None
    for bad in (np.zeros((8, 8), np.float64), np.zeros((8, 8), np.uint8), np.zeros((8, 8, 2), np.float32)):
        with pytest.raises(ValueError):
            api.BlurContext.gaussian_f32(ctx, bad, 2.0)


def scale_exp(maxabs, bscale):
    """ff_kernels.hpp: ff_scale_exp"""
    maxabs = float(np.float32(maxabs))
    if not maxabs > 0:
        return 0
    _, k = math.frexp(maxabs * bscale)
    return min(max(14 - k, -125), 125)


@pytest.mark.parametrize("maxabs", [1e-30, 1e-6, 0.37, 1.0, 255.0, 1e3, 65504.0, 1e6, 3e38])
@pytest.mark.parametrize("bscale", [1.0, 1.37, 9.5])
def test_scale_rule(maxabs, bscale):
    """s = 2^e: a power of two (exact scaling) with max|x| s B in [2^13, 2^14): every V stays below binary16's largest value 65504
    with about 4x headroom, and the largest input keeps 13 bits above 1 (its lo part well inside the normal range)"""
    e = scale_exp(maxabs, bscale)
    v = float(np.float32(maxabs)) * bscale * 2.0 ** e
    assert 2.0 ** 13 <= v < 2.0 ** 14
    assert v * 3 < 65504.0 and v < 2.0 ** 14
    assert np.isfinite(np.float32(2.0 ** e)) and np.float32(2.0 ** -e) > 0


def test_scale_rule_zero_and_nan():
    assert scale_exp(0.0, 1.0) == 0
    assert scale_exp(float("nan"), 1.0) == 0
