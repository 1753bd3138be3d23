"""blur_gaussian_{u16,f16,bf16}_frame_sigmas_* and blur_gaussian_{nv12,p016}_frame_sigmas_batch_dev: what needs no device.  The
argument checks run before the context is touched, so ctx is NULL here: a call whose arguments pass ends in BLUR_ERR_INVALID for the
missing context, and layouts are told apart by whether a call with an unsupported pad reaches BLUR_ERR_UNSUPPORTED."""
import ctypes as C
import math

import numpy as np
import pytest

from test_gaussian_frame_sigmas_args import BUF, P, both_entries, dbl, lib, opts

INVALID, UNSUPPORTED, OK = 1, 2, 0
TYPES = (("u16", 2), ("f16", 2), ("bf16", 2))          # entry name, bytes per sample
KINDS = (("nv12", 1), ("p016", 2))


# ---- u16, f16, bf16: the status table of the u8 and f32 entries ---------------------------------------------------------------------
@pytest.mark.parametrize("t,es", TYPES)
def test_invalid_arguments(t, es):
    ok3 = dbl(1.0, 2.0, 0.0)
    assert both_entries(t, es, P, P, 3, 8, 8, 3, None) == [INVALID] * 2
    assert both_entries(t, es, P, P, 3, 8, 8, 3, dbl(1.0, -0.5, 1.0)) == [INVALID] * 2
    assert both_entries(t, es, P, P, 3, 8, 8, 3, dbl(1.0, math.nan, 1.0)) == [INVALID] * 2
    assert both_entries(t, es, P, P, 3, 8, 8, 3, dbl(math.inf, 1.0, 1.0)) == [INVALID] * 2
    assert both_entries(t, es, P, P, 4, 8, 8, 1, dbl(0.0, 0.0, 0.0, -math.inf)) == [INVALID] * 2
    for channels in (0, 2, 5, -1):
        assert both_entries(t, es, P, P, 3, 8, 8, channels, ok3) == [INVALID] * 2
    for src, dst in ((None, P), (P, None)):
        assert both_entries(t, es, src, dst, 3, 8, 8, 3, ok3) == [INVALID] * 2
    assert both_entries(t, es, P, P, 3, 0, 8, 3, ok3) == [INVALID] * 2
    assert both_entries(t, es, P, P, 3, 8, -3, 3, ok3) == [INVALID] * 2
    assert both_entries(t, es, P, P, -1, 8, 8, 3, ok3) == [INVALID] * 2
    assert both_entries(t, es, P, P, 3, 8, 8, 3, ok3) == [INVALID] * 2               # valid arguments, no context
    assert both_entries(t, es, P, P, 3, 8, 8, 3, dbl(0.0, 0.0, 0.0)) == [INVALID] * 2


@pytest.mark.parametrize("t,es", TYPES)
@pytest.mark.parametrize("channels", [1, 3, 4])
def test_a_pad_past_the_frame_refuses_the_call(t, es, channels):
    import blur_algorithms_amd as B
    rows, cols, big, small = 40, 90, 30.0, 2.0
    assert B.pffft_sizing(rows, cols, big)["pad"] > rows - 1 >= B.pffft_sizing(rows, cols, small)["pad"]
    n = 6
    for at in (0, 3, n - 1):
        s = [small, 0.0, small, 1.0, small, small]
        s[at] = big
        assert both_entries(t, es, P, P, n, rows, cols, channels, dbl(*s)) == [UNSUPPORTED] * 2
    for bad in (-1.0, math.nan, math.inf):
        assert both_entries(t, es, P, P, n, rows, cols, channels, dbl(*([small] * (n - 1) + [bad]))) == [INVALID] * 2
    # an invalid entry behind an unsupported one: the call is invalid
    assert both_entries(t, es, P, P, n, rows, cols, channels, dbl(*([big] + [small] * (n - 2) + [-1.0]))) == [INVALID] * 2
    # two channels with an unsupported pad: still invalid, not unsupported (no public entry takes channels = 2)
    assert both_entries(t, es, P, P, n, rows, cols, 2, dbl(*([big] + [small] * (n - 1)))) == [INVALID] * 2


@pytest.mark.parametrize("t,es", TYPES)
def test_pitched_argument_rules(t, es):
    entry = getattr(lib(), "blur_gaussian_%s_frame_sigmas_pitched_batch_dev" % t)
    o = opts()
    rows, cols, ch, n = 40, 90, 3, 3
    row = cols * ch * es
    wide = dbl(1.0, 2.0, 30.0)

    def reaches_the_sigmas(sp, sf, dp, df, nframes=n):
        return entry(None, P, sp, sf, P, dp, df, nframes, rows, cols, ch, wide, C.byref(o)) == UNSUPPORTED

    fs = rows * (row + 8 * es)
    assert reaches_the_sigmas(row, rows * row, row, rows * row)
    assert reaches_the_sigmas(row + 8 * es, fs, row + 4 * es, fs)
    assert reaches_the_sigmas(row, 0, row, rows * row)                                 # source frame stride 0: scale space
    assert not reaches_the_sigmas(row, rows * row, row, 0)
    assert entry(None, P, row, rows * row, P, row, 0, n, rows, cols, ch, wide, C.byref(o)) == INVALID
    assert not reaches_the_sigmas(row - es, rows * row, row, rows * row)
    assert not reaches_the_sigmas(row, rows * row - es, row, rows * row)
    assert not reaches_the_sigmas(row + 1, fs, row, rows * row)                        # no multiple of the sample size
    assert not reaches_the_sigmas(row, rows * row + 1, row, rows * row)


# ---- NV12 / P016 ---------------------------------------------------------------------------------------------------------------------
ROWS, COLS = 40, 92


def nv(kind, es, sigmas, nframes=3, rows=ROWS, cols=COLS, sy=P, suv=P, dy=P, duv=P, spitch=None, dpitch=None, strides=None):
    entry = getattr(lib(), "blur_gaussian_%s_frame_sigmas_batch_dev" % kind)
    o = opts()
    spitch = max(cols, 1) * es if spitch is None else spitch
    dpitch = max(cols, 1) * es if dpitch is None else dpitch
    r = max(rows, 2)
    sys_, suvs, dys, duvs = strides if strides else (r * spitch, r // 2 * spitch, r * dpitch, r // 2 * dpitch)
    return entry(None, sy, suv, spitch, sys_, suvs, dy, duv, dpitch, dys, duvs, nframes, rows, cols, sigmas, C.byref(o))


@pytest.mark.parametrize("kind,es", KINDS)
def test_nv_pointers_sizes_and_sigmas(kind, es):
    ok = dbl(2.0, 1.0, 0.0, 0.0, 3.0, 1.5)
    assert nv(kind, es, ok) == INVALID                                                   # valid arguments, no context
    assert nv(kind, es, None) == INVALID
    for null in ("sy", "suv", "dy", "duv"):
        assert nv(kind, es, ok, **{null: None}) == INVALID
    assert nv(kind, es, ok, nframes=-1) == INVALID
    for rows, cols in ((ROWS + 1, COLS), (ROWS, COLS + 1), (0, COLS), (ROWS, -2)):       # odd or empty
        assert nv(kind, es, ok, rows=rows, cols=cols) == INVALID
    for at in range(6):                                                                  # both sigmas of every frame are checked
        for bad in (-1.0, math.nan, math.inf):
            s = [2.0, 1.0, 0.0, 0.0, 3.0, 1.5]
            s[at] = bad
            assert nv(kind, es, dbl(*s)) == INVALID
    assert nv(kind, es, dbl(1.0), nframes=0) == INVALID                                  # a no-op with a context; here the context is missing


@pytest.mark.parametrize("kind,es", KINDS)
def test_nv_pad_limits_per_plane_and_frame(kind, es):
    import blur_algorithms_amd as B
    pad = lambda r, c, s: B.pffft_sizing(r, c, s)["pad"]
    luma_big, chroma_big, small = 30.0, 12.0, 1.0
    assert pad(ROWS, COLS, luma_big) > ROWS - 1
    # a chroma sigma that the luma plane would take and the chroma plane does not
    assert ROWS // 2 - 1 < pad(ROWS // 2, COLS // 2, chroma_big) and pad(ROWS, COLS, chroma_big) <= ROWS - 1
    assert pad(ROWS // 2, COLS // 2, small) <= ROWS // 2 - 1
    base = [small, small, 0.0, small, small, 0.0]
    assert nv(kind, es, dbl(*base)) == INVALID                                           # passes every check
    for f in range(3):
        s = list(base)
        s[2 * f + 1] = chroma_big                                                        # the chroma pad of one frame only
        assert nv(kind, es, dbl(*s)) == UNSUPPORTED
        s = list(base)
        s[2 * f] = luma_big
        assert nv(kind, es, dbl(*s)) == UNSUPPORTED
        s = list(base)
        s[2 * f] = chroma_big                                                            # fine on the luma plane
        assert nv(kind, es, dbl(*s)) == INVALID


@pytest.mark.parametrize("kind,es", KINDS)
def test_nv_error_order(kind, es):
    """nv_status's order: pointers, sizes, pitches, strides, the sigmas' values, then the pads"""
    unsup = dbl(1.0, 1.0, 1.0, 12.0, 1.0, 1.0)
    row = COLS * es
    assert nv(kind, es, unsup) == UNSUPPORTED
    assert nv(kind, es, unsup, spitch=row - es) == INVALID                               # pitch below the row
    assert nv(kind, es, unsup, dpitch=row - es) == INVALID
    assert nv(kind, es, unsup, spitch=row + 16) == UNSUPPORTED                           # a padded pitch passes
    if es > 1:
        assert nv(kind, es, unsup, spitch=row + 1) == INVALID
    packed = (ROWS * row, ROWS // 2 * row, ROWS * row, ROWS // 2 * row)
    for i in range(4):                                                                   # a frame stride below its plane's span
        st = list(packed)
        st[i] -= es
        assert nv(kind, es, unsup, strides=tuple(st)) == INVALID
        st[i] = 0
        assert nv(kind, es, unsup, strides=tuple(st)) == INVALID                         # no broadcast source here
    assert nv(kind, es, unsup, nframes=1, strides=(0, 0, 0, 0)) == INVALID               # one frame: only its two sigmas are read
    assert nv(kind, es, dbl(1.0, 12.0), nframes=1, strides=(0, 0, 0, 0)) == UNSUPPORTED
    assert nv(kind, es, dbl(1.0, 1.0, 1.0, 12.0, 1.0, -1.0)) == INVALID                  # an invalid sigma behind an unsupported one
    assert nv(kind, es, unsup, rows=ROWS + 1) == INVALID                                 # odd size before the pads
    assert nv(kind, es, unsup, sy=None) == INVALID


# ---- the bindings ----------------------------------------------------------------------------------------------------------------------
NEW = (["blur_gaussian_%s_frame_sigmas_%sbatch_dev" % (t, p) for t, _ in TYPES for p in ("", "pitched_")]
       + ["blur_gaussian_%s_frame_sigmas_batch_dev" % k for k, _ in KINDS])


def test_symbols_header_and_library_in_step():
    import os
    from blur_algorithms_amd import _lib
    L = lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "blur_amd.h")).read()
    assert len(NEW) == 8
    for name in NEW:
        assert name in _lib.SYMBOLS, name
        assert hasattr(L, name), name
        assert ("int %s(" % name) in header, name
        assert len(getattr(L, name).argtypes) == len(_lib.SYMBOLS[name][1])


# ---- the Python wrappers, before the library is called -----------------------------------------------------------------------------------
def no_device_ctx():
    import blur_algorithms_amd as B
    ctx = B.BlurContext.__new__(B.BlurContext)          # no device: every case stops in the wrapper
    ctx._lib, ctx._h = lib(), C.c_void_p()
    return ctx


def test_per_frame_methods_check_before_the_library():
    import torch
    ctx = no_device_ctx()
    frames = np.zeros((3, 16, 16, 3), np.uint16)
    for sig in ((1.0, 2.0), (1.0, 2.0, 3.0, 4.0), ()):
        with pytest.raises(ValueError):
            ctx.gaussian_u16_per_frame(frames, sig)
        with pytest.raises(ValueError):
            ctx.gaussian_f16_per_frame(frames.astype(np.float16), sig)
        with pytest.raises(ValueError):
            ctx.gaussian_bf16_per_frame(torch.zeros((3, 16, 16, 3), dtype=torch.bfloat16), sig)
    with pytest.raises(ValueError):
        ctx.gaussian_u16_per_frame(np.zeros((16, 16), np.uint16), (1.0,) * 16)
    with pytest.raises(ValueError):
        ctx.gaussian_f16_per_frame(frames, (1.0, 2.0, 3.0))                              # a uint16 array is a u16 image
    with pytest.raises(ValueError):
        ctx.gaussian_bf16_per_frame(frames, (1.0, 2.0, 3.0))                             # numpy has no bfloat16
    with pytest.raises(ValueError):
        ctx.gaussian_u16_per_frame(torch.zeros((3, 16, 16, 3), dtype=torch.uint16), (1.0, 2.0, 3.0))      # a CPU tensor


def test_nv12_per_frame_sigmas_and_shapes():
    import torch
    from blur_algorithms_amd import api
    y, uv = torch.zeros((3, 40, 92), dtype=torch.uint8), torch.zeros((3, 20, 46, 2), dtype=torch.uint8)
    r = api._nv12_per_frame_tensors(y, uv, (4.0, (3.0, 0.0), (0, 2)), None, require_cuda=False)
    assert r[6] == [(4.0, 2.0), (3.0, 0.0), (0.0, 2.0)]                                  # a number s: (s, s / 2); a pair as given
    assert r[2] is y and r[3] is uv and r[4][:3] == (3, 40, 92)
    surf = torch.zeros((3, 64, 100), dtype=torch.uint16)
    r = api._nv12_per_frame_tensors(surf[:, :40, :92], surf[:, 42:62, :92].unflatten(-1, (46, 2)), [1.0] * 3, None, require_cuda=False)
    assert r[4] == (3, 40, 92, 100, 6400, 6400)
    for sig in ((1.0, 2.0), (1.0,) * 4, (), 2.0, (1.0, 2.0, (1.0, 2.0, 3.0)), (1.0, 2.0, (1.0,)), ((1.0, 2.0, 3.0),) * 3):
        with pytest.raises((ValueError, TypeError)):
            api._nv12_per_frame_tensors(y, uv, sig, None, require_cuda=False)
    with pytest.raises(ValueError):                                                      # a single surface is not a clip
        api._nv12_per_frame_tensors(y[0], uv[0], (1.0,), None, require_cuda=False)
    with pytest.raises(ValueError):
        api._nv12_per_frame_tensors(y, uv[:2], (1.0,) * 3, None, require_cuda=False)
    with pytest.raises(ValueError):
        api._nv12_per_frame_tensors(y, uv.to(torch.uint16), (1.0,) * 3, None, require_cuda=False)
    with pytest.raises(ValueError):
        api._nv12_per_frame_tensors(y, uv, (1.0,) * 3, (y.clone(),), require_cuda=False)
    ctx = no_device_ctx()
    with pytest.raises(ValueError):
        ctx.gaussian_nv12_per_frame(y, uv, (1.0,) * 3)                                   # CPU tensors
    with pytest.raises(ValueError):
        ctx.gaussian_nv12_per_frame(y.numpy(), uv.numpy(), (1.0,) * 2)
    with pytest.raises(ValueError):
        ctx.gaussian_nv12_per_frame(y.numpy(), uv.numpy()[:2], (1.0,) * 3)
    import inspect
    import blur_algorithms_amd as B
    assert list(inspect.signature(B.BlurContext.gaussian_nv12_per_frame).parameters) == ["self", "y", "uv", "sigmas", "out", "nyquist_quirk", "engine"]
