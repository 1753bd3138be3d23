"""blur_gaussian_*_sigmas_*: one sigma per channel.  What needs no device: the argument checks (they run before the context is touched,
so ctx may be NULL), the host-only plan of the grouping, and the Python wrappers' handling of a scalar against a sequence."""
import ctypes as C
import math

import numpy as np
import pytest

INVALID, UNSUPPORTED = 1, 2
TYPES = ("u8", "u16", "f32", "f16", "bf16")

BUF = (C.c_uint8 * 256)()
P = C.addressof(BUF)


def lib():
    from blur_algorithms_amd import _lib
    return _lib.load()


def opts():
    from blur_algorithms_amd._lib import BlurOpts
    o = BlurOpts()
    lib().blur_opts_default(C.byref(o))
    return o


def dbl(*v):
    return (C.c_double * max(1, len(v)))(*v)


def every_entry(t, src, dst, nframes, rows, cols, channels, sigmas):
    """the status of the five entries of type t for the same arguments, without a context"""
    L, o = lib(), opts()
    return [
        getattr(L, "blur_gaussian_%s_sigmas_batch_dev" % t)(None, src, dst, nframes, rows, cols, channels, sigmas, C.byref(o)),
        getattr(L, "blur_gaussian_%s_sigmas_dev" % t)(None, src, dst, rows, cols, channels, sigmas, C.byref(o)),
        getattr(L, "blur_gaussian_%s_sigmas_host" % t)(None, src, dst, rows, cols, channels, sigmas, C.byref(o)),
        getattr(L, "blur_gaussian_%s_sigmas_batch_multi_dev" % t)(None, src, dst, nframes, rows, cols, channels, sigmas, C.byref(o)),
        getattr(L, "blur_gaussian_%s_sigmas_batch_multi_host" % t)(None, src, dst, nframes, rows, cols, channels, sigmas, C.byref(o)),
    ]


@pytest.mark.parametrize("t", TYPES)
def test_invalid_arguments(t):
    ok3 = dbl(1.0, 2.0, 0.0)
    assert every_entry(t, P, P, 1, 8, 8, 3, None) == [INVALID] * 5                          # sigmas == NULL
    assert every_entry(t, P, P, 1, 8, 8, 3, dbl(1.0, -0.5, 1.0)) == [INVALID] * 5           # a negative entry
    assert every_entry(t, P, P, 1, 8, 8, 3, dbl(1.0, math.nan, 1.0)) == [INVALID] * 5
    assert every_entry(t, P, P, 1, 8, 8, 3, dbl(math.inf, 1.0, 1.0)) == [INVALID] * 5
    assert every_entry(t, P, P, 1, 8, 8, 4, dbl(0.0, 0.0, 0.0, -math.inf)) == [INVALID] * 5
    for channels in (0, 2, 5, -1):
        assert every_entry(t, P, P, 1, 8, 8, channels, dbl(1.0, 1.0, 1.0, 1.0, 1.0)) == [INVALID] * 5
    for src, dst in ((None, P), (P, None)):
        assert every_entry(t, src, dst, 1, 8, 8, 3, ok3) == [INVALID] * 5
    assert every_entry(t, P, P, 1, 0, 8, 3, ok3) == [INVALID] * 5
    assert every_entry(t, P, P, 1, 8, -3, 3, ok3) == [INVALID] * 5
    L, o = lib(), opts()
    assert getattr(L, "blur_gaussian_%s_sigmas_batch_dev" % t)(None, P, P, -1, 8, 8, 3, ok3, C.byref(o)) == INVALID
    # valid arguments without a context: BLUR_ERR_INVALID, as the scalar entries
    assert every_entry(t, P, P, 1, 8, 8, 3, ok3) == [INVALID] * 5
    assert every_entry(t, P, P, 1, 8, 8, 3, dbl(0.0, 0.0, 0.0)) == [INVALID] * 5


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("channels", [1, 3, 4])
def test_pad_too_large_for_one_entry_only(t, channels):
    import blur_algorithms_amd as B
    rows, cols, big, small = 40, 90, 30.0, 2.0
    assert B.pffft_sizing(rows, cols, big)["pad"] > rows - 1 >= B.pffft_sizing(rows, cols, small)["pad"]
    for at in range(channels):
        s = [small] * channels
        s[at] = big
        if channels > 1:
            s[(at + 1) % channels] = 0.0
        assert every_entry(t, P, P, 1, rows, cols, channels, dbl(*s)) == [UNSUPPORTED] * 5
    # an invalid entry beside it: the call is invalid
    if channels > 1:
        assert every_entry(t, P, P, 1, rows, cols, channels, dbl(*([big] + [-1.0] * (channels - 1)))) == [INVALID] * 5


def expected_nkb(pad):
    """the class rule 8 (NKB - 4) < pad <= 8 (NKB - 2) over the odd NKB 3 .. 23; 0 past pad 168"""
    for nkb in range(3, 25, 2):
        if pad <= 8 * (nkb - 2):
            assert nkb == 3 or pad > 8 * (nkb - 4)
            return nkb
    return 0


def test_plan_groups_pads_and_classes():
    import blur_algorithms_amd as B
    from blur_algorithms_amd.api import gaussian_sigmas_plan
    rows, cols = 2160, 3840
    pad = lambda s: B.pffft_sizing(rows, cols, s)["pad"]
    assert gaussian_sigmas_plan(rows, cols, (1.0, 11.0, 11.0)) == [(0, pad(1.0), expected_nkb(pad(1.0))), (1, pad(11.0), expected_nkb(pad(11.0))),
                                                                   (1, pad(11.0), expected_nkb(pad(11.0)))]
    assert [g for g, _, _ in gaussian_sigmas_plan(rows, cols, (5.0, 5.0, 7.0))] == [0, 0, 1]
    assert [g for g, _, _ in gaussian_sigmas_plan(rows, cols, (7.0, 5.0, 7.0, 5.0))] == [0, 1, 0, 1]
    assert gaussian_sigmas_plan(rows, cols, (20.0, 20.0, 20.0, 0.0))[3] == (-1, 0, 0)
    assert [g for g, _, _ in gaussian_sigmas_plan(rows, cols, (0.0, 11.0, 11.0))] == [-1, 0, 0]
    assert gaussian_sigmas_plan(rows, cols, (0.0, 0.0, 0.0)) == [(-1, 0, 0)] * 3
    assert gaussian_sigmas_plan(rows, cols, (3.0,)) == [(0, pad(3.0), expected_nkb(pad(3.0)))]
    # every class, and past the widest one
    seen = set()
    for sigma in (0.5, 1.0, 2.0, 3.0, 5.0, 7.0, 9.0, 12.0, 15.0, 18.0, 20.0, 24.0, 27.0, 30.0, 33.0, 36.0, 40.0, 44.0, 48.0, 51.0, 54.0, 60.0, 80.0):
        (g, p, nkb), = gaussian_sigmas_plan(rows, cols, (sigma,))
        assert (g, p, nkb) == (0, pad(sigma), expected_nkb(pad(sigma)))
        assert (nkb == 0) == (p > 168)
        seen.add(nkb)
    assert seen == {0, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23}


def test_plan_status_codes():
    from blur_algorithms_amd import BlurError
    from blur_algorithms_amd.api import gaussian_sigmas_plan
    L = lib()
    out = (C.c_int * 12)()
    assert L.blur_gaussian_sigmas_plan(100, 100, 3, None, out) == INVALID
    assert L.blur_gaussian_sigmas_plan(100, 100, 3, dbl(1.0, 1.0, 1.0), None) == INVALID
    assert L.blur_gaussian_sigmas_plan(100, 100, 2, dbl(1.0, 1.0), out) == INVALID
    assert L.blur_gaussian_sigmas_plan(100, 100, 3, dbl(1.0, -1.0, 1.0), out) == INVALID
    assert L.blur_gaussian_sigmas_plan(100, 100, 3, dbl(1.0, math.nan, 1.0), out) == INVALID
    assert L.blur_gaussian_sigmas_plan(0, 100, 3, dbl(1.0, 1.0, 1.0), out) == INVALID
    assert L.blur_gaussian_sigmas_plan(40, 90, 3, dbl(1.0, 30.0, 0.0), out) == UNSUPPORTED
    with pytest.raises(BlurError):
        gaussian_sigmas_plan(40, 90, (1.0, 30.0, 0.0))


class SpyLib:
    """stands in for the loaded library inside a wrapper object: records the entry a call reaches, and stops there"""

    class Reached(Exception):
        pass

    def __init__(self, real):
        self._real = real
        self.calls = []

    def __getattr__(self, name):
        real = getattr(self._real, name)
        if not name.startswith("blur_gaussian_"):
            return real

        def entry(*args):
            self.calls.append((name, args))
            raise SpyLib.Reached(name)
        return entry


def spy_context():
    import blur_algorithms_amd as B
    ctx = B.BlurContext.__new__(B.BlurContext)          # no device: the wrappers are stopped at the entry
    ctx._lib = SpyLib(lib())
    ctx._h = C.c_void_p()
    return ctx


def spy_multi():
    import blur_algorithms_amd as B
    m = B.BlurMulti.__new__(B.BlurMulti)
    m._lib = SpyLib(lib())
    m._h = C.c_void_p()
    m.devices = [0]
    return m


WRAPPERS = (("gaussian", "u8", np.uint8), ("gaussian_f32", "f32", np.float32), ("gaussian_u16", "u16", np.uint16), ("gaussian_f16", "f16", np.float16))


@pytest.mark.parametrize("method,t,dtype", WRAPPERS)
def test_scalar_reaches_the_scalar_symbol_and_a_sequence_the_new_one(method, t, dtype):
    ctx = spy_context()
    img = np.zeros((16, 16, 3), dtype)
    with pytest.raises(SpyLib.Reached):
        getattr(ctx, method)(img, 2.0)
    name, args = ctx._lib.calls[-1]
    assert name == "blur_gaussian_%s_host" % t and args[6] == 2.0 and isinstance(args[6], float)
    with pytest.raises(SpyLib.Reached):
        getattr(ctx, method)(img, np.float64(2.0))                 # a numpy scalar is a scalar
    assert ctx._lib.calls[-1][0] == "blur_gaussian_%s_host" % t
    with pytest.raises(SpyLib.Reached):
        getattr(ctx, method)(img, (1.0, 0, 11))
    name, args = ctx._lib.calls[-1]
    assert name == "blur_gaussian_%s_sigmas_host" % t and list(args[6]) == [1.0, 0.0, 11.0] and args[5] == 3
    with pytest.raises(SpyLib.Reached):
        getattr(ctx, method)(np.zeros((16, 16), dtype), [3.0])     # [rows, cols]: a sequence of one
    name, args = ctx._lib.calls[-1]
    assert name == "blur_gaussian_%s_sigmas_host" % t and list(args[6]) == [3.0] and args[5] == 1
    with pytest.raises(SpyLib.Reached):
        getattr(ctx, method)(img, np.array([2.0, 2.0, 5.0]))
    assert ctx._lib.calls[-1][0] == "blur_gaussian_%s_sigmas_host" % t

    m = spy_multi()
    frames = np.zeros((2, 16, 16, 4), dtype)
    with pytest.raises(SpyLib.Reached):
        getattr(m, method)(frames, 2.0)
    assert m._lib.calls[-1][0] == "blur_gaussian_%s_batch_multi_host" % t
    with pytest.raises(SpyLib.Reached):
        getattr(m, method)(frames, (2.0, 2.0, 2.0, 0.0))
    name, args = m._lib.calls[-1]
    assert name == "blur_gaussian_%s_sigmas_batch_multi_host" % t and list(args[7]) == [2.0, 2.0, 2.0, 0.0]


def test_bf16_wrappers_route_the_same_way():
    import torch
    ctx, m = spy_context(), spy_multi()
    img = torch.zeros((16, 16, 3), dtype=torch.bfloat16)
    with pytest.raises(SpyLib.Reached):
        ctx.gaussian_bf16(img, 2.0)
    assert ctx._lib.calls[-1][0] == "blur_gaussian_bf16_host"
    with pytest.raises(SpyLib.Reached):
        ctx.gaussian_bf16(img, (2.0, 0.0, 3.0))
    assert ctx._lib.calls[-1][0] == "blur_gaussian_bf16_sigmas_host"
    with pytest.raises(SpyLib.Reached):
        m.gaussian_bf16(img[None], (2.0, 0.0, 3.0))
    assert m._lib.calls[-1][0] == "blur_gaussian_bf16_sigmas_batch_multi_host"
    with pytest.raises(ValueError):
        ctx.gaussian_bf16(img, (2.0, 3.0))


@pytest.mark.parametrize("method,t,dtype", WRAPPERS)
def test_wrong_length_sequence_raises(method, t, dtype):
    ctx, m = spy_context(), spy_multi()
    for shape, sig in (((16, 16, 3), (1.0, 2.0)), ((16, 16, 3), (1.0, 2.0, 3.0, 4.0)), ((16, 16, 4), (1.0, 2.0, 3.0)), ((16, 16), (1.0, 2.0)),
                       ((16, 16, 1), ()), ((2, 16, 16, 3), (1.0,))):
        with pytest.raises(ValueError):
            getattr(ctx, method)(np.zeros(shape, dtype), sig)
    with pytest.raises(ValueError):
        getattr(m, method)(np.zeros((2, 16, 16, 3), dtype), (1.0, 2.0))
    assert ctx._lib.calls == [] and m._lib.calls == []


def test_zero_dimensional_values_stay_scalars():
    """a 0-d numpy array (and a 0-d tensor) was a scalar sigma before sequences were accepted, through float(); it still is"""
    import torch
    from blur_algorithms_amd import api
    for v in (np.float64(6.0), np.array(6.0), np.array(6, dtype=np.int32), torch.tensor(6.0)):
        assert not api._is_sigma_sequence(v)
        assert api._sigma_arg(v, 3) == 6.0 and isinstance(api._sigma_arg(v, 3), float)
    for v in ([6.0], (1, 2, 3), np.array([6.0]), torch.tensor([1.0, 2.0, 3.0])):
        assert api._is_sigma_sequence(v)
