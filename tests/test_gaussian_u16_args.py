"""blur_gaussian_u16_*: argument validation that needs no device (the checks run before the context is touched, so ctx may be
NULL), the bindings of the five entry points, the Python shape and dtype checks, the constant scale of the fused kernel's u16
instantiation (ff_kernels.hpp: ff_scale_exp(65535, B)) mirrored in Python, and the parity helper's own arithmetic on hand values."""
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


BUF = (C.c_uint16 * 64)()
P = C.addressof(BUF)


def entries(L):
    """(name, call(src, dst, nframes, rows, cols, channels, sigma)) for every u16 entry point"""
    o = opts()
    return [
        ("batch_dev", lambda s, d, n, r, c, ch, sg: L.blur_gaussian_u16_batch_dev(None, s, d, n, r, c, ch, sg, C.byref(o))),
        ("dev", lambda s, d, n, r, c, ch, sg: L.blur_gaussian_u16_dev(None, s, d, r, c, ch, sg, C.byref(o))),
        ("host", lambda s, d, n, r, c, ch, sg: L.blur_gaussian_u16_host(None, s, d, r, c, ch, sg, C.byref(o))),
    ]


def test_symbols_bound():
    L = lib()
    for name in ("blur_gaussian_u16_batch_dev", "blur_gaussian_u16_dev", "blur_gaussian_u16_host",
                 "blur_gaussian_u16_batch_multi_dev", "blur_gaussian_u16_batch_multi_host"):
        assert getattr(L, name) is not None


@pytest.mark.parametrize("channels", [0, 2, 5, -1, 3 * 256])
def test_bad_channel_count(channels):
    L = lib()
    for _, call in entries(L):
        assert call(P, P, 1, 4, 4, channels, 1.0) == INVALID
    o = opts()
    assert L.blur_gaussian_u16_batch_multi_dev(None, P, P, 1, 4, 4, channels, 1.0, C.byref(o)) == INVALID
    assert L.blur_gaussian_u16_batch_multi_host(None, P, P, 1, 4, 4, channels, 1.0, C.byref(o)) == INVALID


@pytest.mark.parametrize("channels", [1, 3, 4])
def test_null_pointers_counts_and_sizes(channels):
    L = lib()
    for _, call in entries(L):
        for src, dst in ((None, P), (P, None), (None, None)):
            assert call(src, dst, 1, 4, 4, channels, 1.0) == INVALID
        for rows, cols, sigma in ((0, 4, 1.0), (4, -1, 1.0), (4, 4, 0.0), (4, 4, -2.0)):
            assert call(P, P, 1, rows, cols, channels, sigma) == INVALID
    o = opts()
    assert L.blur_gaussian_u16_batch_dev(None, P, P, -1, 4, 4, channels, 1.0, C.byref(o)) == INVALID


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
    assert L.blur_gaussian_u16_batch_dev(None, P, P, 0, rows, cols, channels, big, C.byref(o)) == UNSUPPORTED
    assert L.blur_gaussian_u16_batch_dev(None, P, P, 0, rows, cols, channels, 2.0, C.byref(o)) == INVALID


def test_python_shapes_and_dtypes():
    from blur_algorithms_amd import api
    # dtype and layout are refused before the context is used
    ctx = object.__new__(api.BlurContext)
    ctx._lib = lib()
    ctx._h = None
    for bad in (np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.float32), np.zeros((8, 8), np.int16), np.zeros((8, 8, 2), np.uint16),
                np.zeros((2, 8, 8, 5), np.uint16), np.zeros((8,), np.uint16)):
        with pytest.raises(ValueError):
            api.BlurContext.gaussian_u16(ctx, bad, 2.0)
    m = object.__new__(api.BlurMulti)
    m._lib = lib()
    m._h = None
    for bad in (np.zeros((2, 8, 8, 1), np.uint8), np.zeros((2, 8, 8, 1), np.float32), np.zeros((2, 8, 8, 1), np.int16), np.zeros((8, 8, 1), np.uint16)):
        with pytest.raises(ValueError):
            api.BlurMulti.gaussian_u16(m, bad, 2.0)


def scale_exp(maxabs, bscale):
    """ff_kernels.hpp: ff_scale_exp"""
    maxabs = float(np.float32(maxabs))
    if not maxabs > 0:
        return 0
    _, k = math.frexp(maxabs * bscale)
    return min(max(14 - k, -125), 125)


@pytest.mark.parametrize("bscale", [1.0, 1.0 + 1e-4 * (517 + 2 * 40), 1.37, 2.0, 9.5, 1.0 + 0.02 * (3840 + 336), 1000.0])
def test_constant_scale_rule(bscale):
    """u16: s = 2^e with e = ff_scale_exp(65535, B), a constant of the call: 65535 s B in [2^13, 2^14), so every V of the hand-off
    stays below binary16's largest value with about 4x headroom, whatever the frame holds"""
    e = scale_exp(65535.0, bscale)
    v = 65535.0 * bscale * 2.0 ** e
    assert 2.0 ** 13 <= v < 2.0 ** 14
    assert v * 3 < 65504.0
    # a u16 sample times a power of two splits exactly into two binary16 values: hi = f16(x s), lo = f16(x s - hi)
    x = np.arange(0, 65536, dtype=np.float64) * 2.0 ** e
    hi = x.astype(np.float16).astype(np.float64)
    lo = (x - hi).astype(np.float16).astype(np.float64)
    assert np.all(hi + lo == x)


def test_parity_helper_hand_values():
    import u16_parity as U
    w = np.array([-113.6, 65785.7, 0.49, -0.6, 65535.49, 65535.5])
    assert U.round_u16(w).tolist() == [65423, 250, 0, 0, 65535, 0]
    assert abs(U.TIE_TOL_U16 - (0.065535 + 1.0 / 512)) < 1e-12
    # exact match required away from a tie; one level (modulo 65536) allowed at one
    planes = np.array([[100.2, 65535.49, 7.3]])
    assert U.assert_u16_parity(np.array([[100, 0, 7]], np.uint16), planes) == 1          # 65535.99: a tie; 0 is one level from 65535
    with pytest.raises(AssertionError):
        U.assert_u16_parity(np.array([[101, 65535, 7]], np.uint16), planes)              # 100.7 is no tie
    with pytest.raises(AssertionError):
        U.assert_u16_parity(np.array([[100, 1, 7]], np.uint16), planes)                  # two levels off at a tie
    with pytest.raises(AssertionError):
        U.assert_u16_parity(np.array([[100, 65535]], np.uint16), np.array([[99.51, 65535.49]]))      # every sample excused: over the cap
