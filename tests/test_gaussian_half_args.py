"""blur_gaussian_f16_* / blur_gaussian_bf16_*: argument validation that needs no device (the checks run before the context is
touched, so ctx may be NULL), the bindings of the ten entry points, the Python shape and dtype checks, and the exactness of the fused
kernel's staging for the half types (ff_kernels.hpp: x 2^e is a binary16 value) mirrored in numpy over every finite bit pattern."""
import ctypes as C

import numpy as np
import pytest

import half_parity as H

INVALID, UNSUPPORTED = 1, 2
KINDS = ("f16", "bf16")
NAMES = [n % k for k in KINDS for n in ("blur_gaussian_%s_batch_dev", "blur_gaussian_%s_dev", "blur_gaussian_%s_host",
                                        "blur_gaussian_%s_batch_multi_dev", "blur_gaussian_%s_batch_multi_host")]


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


def entries(L, kind):
    """(name, call(src, dst, nframes, rows, cols, channels, sigma)) for the three single-context entry points of a type"""
    o = opts()
    batch, dev, host = (getattr(L, "blur_gaussian_%s_%s" % (kind, n)) for n in ("batch_dev", "dev", "host"))
    return [
        ("batch_dev", lambda s, d, n, r, c, ch, sg: batch(None, s, d, n, r, c, ch, sg, C.byref(o))),
        ("dev", lambda s, d, n, r, c, ch, sg: dev(None, s, d, r, c, ch, sg, C.byref(o))),
        ("host", lambda s, d, n, r, c, ch, sg: host(None, s, d, r, c, ch, sg, C.byref(o))),
    ]


def multi(L, kind):
    return [getattr(L, "blur_gaussian_%s_batch_multi_%s" % (kind, n)) for n in ("dev", "host")]


def test_symbols_bound():
    from blur_algorithms_amd import _lib
    L = lib()
    assert len(NAMES) == 10
    for name in NAMES:
        assert name in _lib.SYMBOLS
        assert getattr(L, name) is not None


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("channels", [0, 2, 5, -1, 3 * 256])
def test_bad_channel_count(kind, channels):
    L = lib()
    for _, call in entries(L, kind):
        assert call(P, P, 1, 4, 4, channels, 1.0) == INVALID
    o = opts()
    for f in multi(L, kind):
        assert f(None, P, P, 1, 4, 4, channels, 1.0, C.byref(o)) == INVALID


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("channels", [1, 3, 4])
def test_null_pointers_counts_and_sizes(kind, channels):
    L = lib()
    for _, call in entries(L, kind):
        for src, dst in ((None, P), (P, None), (None, None)):
            assert call(src, dst, 1, 4, 4, channels, 1.0) == INVALID
        for rows, cols, sigma in ((0, 4, 1.0), (4, -1, 1.0), (4, 4, 0.0), (4, 4, -2.0)):
            assert call(P, P, 1, rows, cols, channels, sigma) == INVALID
    o = opts()
    assert getattr(L, "blur_gaussian_%s_batch_dev" % kind)(None, P, P, -1, 4, 4, channels, 1.0, C.byref(o)) == INVALID
    for f in multi(L, kind):                          # no handle: BLUR_ERR_INVALID whatever else is passed
        assert f(None, None, P, 1, 4, 4, channels, 1.0, C.byref(o)) == INVALID
        assert f(None, P, P, -1, 4, 4, channels, 1.0, C.byref(o)) == INVALID


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("channels", [1, 3, 4])
def test_pad_too_large_and_zero_frames(kind, channels):
    """pad > min(rows, cols) - 1 -> BLUR_ERR_UNSUPPORTED before the device; nframes == 0 and every argument valid: the only thing
    left is the missing context (BLUR_ERR_INVALID), so the shape checks passed"""
    import blur_algorithms_amd as B
    L = lib()
    rows, cols, big = 40, 90, 30.0
    assert B.pffft_sizing(rows, cols, big)["pad"] > rows - 1
    for _, call in entries(L, kind):
        assert call(P, P, 1, rows, cols, channels, big) == UNSUPPORTED
        assert call(P, P, 1, rows, cols, channels, 2.0) == INVALID          # valid: no context
    o = opts()
    batch = getattr(L, "blur_gaussian_%s_batch_dev" % kind)
    assert batch(None, P, P, 0, rows, cols, channels, big, C.byref(o)) == UNSUPPORTED
    assert batch(None, P, P, 0, rows, cols, channels, 2.0, C.byref(o)) == INVALID
    for f in multi(L, kind):
        assert f(None, P, P, 0, rows, cols, channels, 2.0, C.byref(o)) == INVALID


def bare():
    from blur_algorithms_amd import api
    ctx = object.__new__(api.BlurContext)
    ctx._lib = lib()
    ctx._h = None
    m = object.__new__(api.BlurMulti)
    m._lib = lib()
    m._h = None
    m.devices = [0]
    return api, ctx, m


def test_python_shapes_and_dtypes_f16():
    """dtype and layout are refused before the context is used; a uint16 array is a u16 image, not float16 bit patterns"""
    import torch
    api, ctx, m = bare()
    for bad in (np.zeros((8, 8), np.uint16), np.zeros((8, 8), np.float32), np.zeros((8, 8), np.float64), np.zeros((8, 8), np.uint8),
                np.zeros((8, 8, 2), np.float16), np.zeros((2, 8, 8, 5), np.float16), np.zeros((8,), np.float16),
                torch.zeros((8, 8), dtype=torch.bfloat16), torch.zeros((8, 8), dtype=torch.float16), torch.zeros((8, 8), dtype=torch.float32)):
        with pytest.raises(ValueError):
            api.BlurContext.gaussian_f16(ctx, bad, 2.0)           # (a CPU torch.float16 tensor is no CUDA tensor: numpy is the host route)
    for bad in (np.zeros((2, 8, 8, 1), np.uint16), np.zeros((2, 8, 8, 1), np.float32), np.zeros((2, 8, 8, 1), np.float64),
                np.zeros((8, 8, 1), np.float16), torch.zeros((2, 8, 8, 1), dtype=torch.bfloat16)):
        with pytest.raises(ValueError):
            api.BlurMulti.gaussian_f16(m, bad, 2.0)


def test_python_shapes_and_dtypes_bf16():
    import torch
    api, ctx, m = bare()
    bf = torch.bfloat16
    for bad in (np.zeros((8, 8), np.uint16), np.zeros((8, 8), np.float16), np.zeros((8, 8), np.float32), np.zeros((8, 8), np.float64),
                torch.zeros((8, 8), dtype=torch.float16), torch.zeros((8, 8), dtype=torch.float32), torch.zeros((8, 8), dtype=torch.uint16),
                torch.zeros((8, 8, 2), dtype=bf), torch.zeros((2, 8, 8, 5), dtype=bf), torch.zeros((8,), dtype=bf)):
        with pytest.raises(ValueError):
            api.BlurContext.gaussian_bf16(ctx, bad, 2.0)
    with pytest.raises(ValueError):                               # out of another type or shape
        api.BlurContext.gaussian_bf16(ctx, torch.zeros((8, 8), dtype=bf), 2.0, out=torch.zeros((8, 8), dtype=torch.float16))
    with pytest.raises(ValueError):
        api.BlurContext.gaussian_bf16(ctx, torch.zeros((8, 8), dtype=bf), 2.0, out=torch.zeros((8, 9), dtype=bf))
    for bad in (np.zeros((2, 8, 8, 1), np.uint16), torch.zeros((2, 8, 8, 1), dtype=torch.float16), torch.zeros((8, 8, 1), dtype=bf),
                torch.zeros((2, 8, 8, 2), dtype=bf)):
        with pytest.raises(ValueError):
            api.BlurMulti.gaussian_bf16(m, bad, 2.0)


def test_bf16_host_view_round_trip():
    """the host route passes a CPU bfloat16 tensor as its 16-bit patterns, over the same memory"""
    import torch
    from blur_algorithms_amd import api
    t = torch.tensor([[1.0, -0.0], [3.140625, 1e-37]], dtype=torch.bfloat16)
    a, res, shape = api._gauss_array(t, None, api.BF16)
    assert a.dtype == np.uint16 and res.dtype == np.uint16 and shape == (1, 2, 2, 1)
    assert a.tolist() == H.to_bits("bf16", t.float().numpy()).tolist()
    assert a[0, 0] == 0x3f80 and a[0, 1] == 0x8000
    back = api._gauss_result(a.copy(), None, api.BF16)
    assert back.dtype == torch.bfloat16 and torch.equal(back, t)


# ---- the staging: x 2^e is a binary16 value ----------------------------------------------------------------------------------------
def finite_patterns(kind):
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    with np.errstate(invalid="ignore"):
        x = H.from_bits(kind, bits).astype(np.float64)
    return x[np.isfinite(x)]


@pytest.mark.parametrize("bscale", [1.0, 1.37, 2.0])
@pytest.mark.parametrize("kind", KINDS)
def test_staging_is_exact(kind, bscale):
    """for every finite bit pattern x, with e = ff_scale_exp(M, B) for M = |x| and for M = the type's largest finite value:
    f16(x 2^e) equals x 2^e unless |x 2^e| < 2^-14, and then differs by at most 2^-25 (half a binary16 subnormal step).  The kernel
    multiplies in f32: x 2^e is exact there too (a power of two, |e| <= 125, results inside f32's normal range or zero)"""
    x = finite_patterns(kind)
    assert len(x) == (63488 if kind == "f16" else 65280)
    top = H.F16_MAX if kind == "f16" else H.BF16_MAX
    e_own = np.array([H.scale_exp(abs(v), bscale) for v in x])
    e_top = H.scale_exp(top, bscale)
    assert np.all(np.abs(e_own) <= 125) and abs(e_top) <= 125
    if kind == "bf16":                          # magnitudes whose exponent would pass a float32-normal 2^e: the clamp holds e at 125
        assert H.scale_exp(1e-38, bscale) == 125 and H.scale_exp(2.0 ** -133, bscale) == 125
        assert 14 - 125 > e_top >= 14 - 130      # the top of the range needs no clamp
    for e in (e_own, np.full(len(x), e_top)):
        xs32 = (x.astype(np.float32) * np.exp2(e.astype(np.float64)).astype(np.float32)).astype(np.float64)
        xs = x * np.exp2(e.astype(np.float64))
        big = np.abs(xs) >= 2.0 ** -126
        assert np.array_equal(xs32[big], xs[big])                                        # the f32 product is exact
        h = H.rn_f16(xs)
        normal = np.abs(xs) >= 2.0 ** -14
        assert np.array_equal(h[normal | (xs == 0)], xs[normal | (xs == 0)])
        assert np.all(np.abs(h - xs)[~normal] <= 2.0 ** -25)
    # with its own maximum as the scale a sample lands in [2^13, 2^14) / B: always normal, always exact
    own = np.abs(x) > 0
    clamped = np.abs(e_own) == 125
    v = np.abs(x * np.exp2(e_own.astype(np.float64))) * bscale
    assert np.all((v[own & ~clamped] >= 2.0 ** 13) & (v[own & ~clamped] < 2.0 ** 14))
