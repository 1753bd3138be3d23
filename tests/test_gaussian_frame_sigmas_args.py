"""blur_gaussian_*_frame_sigmas_*: one sigma per frame of a batch.  What needs no device: the argument checks (they run before the
context is touched, so ctx is NULL here), the pitched entries' layout rules, and the host-only plan of the grouping."""
import ctypes as C
import math

import numpy as np
import pytest

INVALID, UNSUPPORTED, OK = 1, 2, 0
TYPES = (("u8", 1), ("f32", 4))          # entry name, bytes per sample

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


def both_entries(t, es, src, dst, nframes, rows, cols, channels, sigmas):
    """the status of the packed and the pitched entry of type t for the same (packed) frames, without a context"""
    L, o = lib(), opts()
    pitch = max(cols, 1) * max(channels, 1) * es
    return [
        getattr(L, "blur_gaussian_%s_frame_sigmas_batch_dev" % t)(None, src, dst, nframes, rows, cols, channels, sigmas, C.byref(o)),
        getattr(L, "blur_gaussian_%s_frame_sigmas_pitched_batch_dev" % t)(None, src, pitch, max(rows, 1) * pitch, dst, pitch, max(rows, 1) * pitch, nframes, rows, cols,
                                                                          channels, sigmas, C.byref(o)),
    ]


@pytest.mark.parametrize("t,es", TYPES)
def test_invalid_arguments(t, es):
    ok3 = dbl(1.0, 2.0, 0.0)
    assert both_entries(t, es, P, P, 3, 8, 8, 3, None) == [INVALID] * 2                          # sigmas == NULL
    assert both_entries(t, es, P, P, 3, 8, 8, 3, dbl(1.0, -0.5, 1.0)) == [INVALID] * 2           # a negative entry
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
    # valid arguments without a context: BLUR_ERR_INVALID, as the scalar entries
    assert both_entries(t, es, P, P, 3, 8, 8, 3, ok3) == [INVALID] * 2
    assert both_entries(t, es, P, P, 3, 8, 8, 3, dbl(0.0, 0.0, 0.0)) == [INVALID] * 2


@pytest.mark.parametrize("t,es", TYPES)
@pytest.mark.parametrize("channels", [1, 3, 4])
def test_one_bad_sigma_in_the_last_frame_refuses_the_call(t, es, channels):
    import blur_algorithms_amd as B
    rows, cols, big, small = 40, 90, 30.0, 2.0
    assert B.pffft_sizing(rows, cols, big)["pad"] > rows - 1 >= B.pffft_sizing(rows, cols, small)["pad"]
    n = 6
    for at in (0, 3, n - 1):                                # the pad of one frame exceeds min(rows, cols) - 1
        s = [small, 0.0, small, 1.0, small, small]
        s[at] = big
        assert both_entries(t, es, P, P, n, rows, cols, channels, dbl(*s)) == [UNSUPPORTED] * 2
    for bad in (-1.0, math.nan, math.inf):                  # the last frame's sigma is invalid
        assert both_entries(t, es, P, P, n, rows, cols, channels, dbl(*([small] * (n - 1) + [bad]))) == [INVALID] * 2
    # an invalid entry behind an unsupported one: the call is invalid
    assert both_entries(t, es, P, P, n, rows, cols, channels, dbl(*([big] + [small] * (n - 2) + [-1.0]))) == [INVALID] * 2


@pytest.mark.parametrize("t,es", TYPES)
def test_pitched_argument_rules(t, es):
    L, o = lib(), opts()
    entry = getattr(L, "blur_gaussian_%s_frame_sigmas_pitched_batch_dev" % t)
    rows, cols, ch, n = 8, 8, 3, 3
    row = cols * ch * es
    sig = dbl(1.0, 2.0, 0.0)
    bad = dbl(1.0, 2.0, -1.0)

    def status(sp, sf, dp, df, nframes=n, sigmas=sig):
        return entry(None, P, sp, sf, P, dp, df, nframes, rows, cols, ch, sigmas, C.byref(o))

    span = (rows - 1) * (row + 4 * es) + row
    # With valid sigmas and no context every accepted layout ends in INVALID (the missing context) too, so the layouts are told apart
    # by what they do to a call whose LAST sigma is bad in another way: an unsupported pad.  40 x 90, sigma 30: BLUR_ERR_UNSUPPORTED
    # is reached only if the layout passed.
    rows2, cols2 = 40, 90
    row2 = cols2 * ch * es
    wide = dbl(1.0, 2.0, 30.0)

    def reaches_the_sigmas(sp, sf, dp, df, nframes=n):
        return entry(None, P, sp, sf, P, dp, df, nframes, rows2, cols2, ch, wide, C.byref(o)) == UNSUPPORTED

    fs2 = rows2 * (row2 + 8 * es)
    assert reaches_the_sigmas(row2, rows2 * row2, row2, rows2 * row2)                    # packed
    assert reaches_the_sigmas(row2 + 8 * es, fs2, row2 + 4 * es, fs2)                    # padded rows
    assert reaches_the_sigmas(row2, 0, row2, rows2 * row2)                               # source frame stride 0: accepted for any nframes
    assert reaches_the_sigmas(row2 + 8 * es, 0, row2, rows2 * row2)
    assert not reaches_the_sigmas(row2, rows2 * row2, row2, 0)                           # destination frame stride 0 with nframes > 1
    assert entry(None, P, row2, rows2 * row2, P, row2, 0, n, rows2, cols2, ch, wide, C.byref(o)) == INVALID
    assert entry(None, P, row2, 0, P, row2, 0, 1, rows2, cols2, ch, dbl(30.0), C.byref(o)) == UNSUPPORTED      # one frame: strides not looked at
    assert not reaches_the_sigmas(row2 - es, rows2 * row2, row2, rows2 * row2)           # pitch below a row
    assert not reaches_the_sigmas(row2, rows2 * row2, row2 - es, rows2 * row2)
    assert not reaches_the_sigmas(row2, rows2 * row2 - es, row2, rows2 * row2)           # frames would overlap (and not 0)
    assert not reaches_the_sigmas(row2, rows2 * row2, row2, rows2 * row2 - es)
    if es > 1:
        assert not reaches_the_sigmas(row2 + 1, fs2, row2, rows2 * row2)                 # no multiple of the element size
        assert not reaches_the_sigmas(row2, rows2 * row2 + 2, row2, rows2 * row2)
    # and the plain statuses
    assert status(row + 4 * es, span, row, rows * row) == INVALID
    assert status(row, rows * row, row, rows * row, sigmas=bad) == INVALID
    assert status(row, 0, row, 0) == INVALID


def expected_nkb(pad):
    """the class rule 8 (NKB - 4) < pad <= 8 (NKB - 2) over the odd NKB 3 .. 23; 0 past pad 168"""
    for nkb in range(3, 25, 2):
        if pad <= 8 * (nkb - 2):
            assert nkb == 3 or pad > 8 * (nkb - 4)
            return nkb
    return 0


def test_plan_pads_and_classes():
    import blur_algorithms_amd as B
    from blur_algorithms_amd.api import gaussian_frame_sigmas_plan
    rows, cols = 2160, 3840
    pad = lambda s: B.pffft_sizing(rows, cols, s)["pad"]
    sigmas = (0.5, 1.0, 2.0, 3.0, 5.0, 7.0, 9.0, 12.0, 15.0, 18.0, 20.0, 24.0, 27.0, 30.0, 33.0, 36.0, 40.0, 44.0, 48.0, 51.0, 54.0, 60.0, 80.0)
    plan = gaussian_frame_sigmas_plan(rows, cols, sigmas)
    assert len(plan) == len(sigmas)
    seen = []
    for f, (s, (group, p, nkb, slot)) in enumerate(zip(sigmas, plan)):
        assert p == pad(s) and nkb == expected_nkb(p)
        assert (nkb == 0) == (p > 168)
        assert slot == f                                           # all distinct: one slot each, in order
        if nkb not in seen:
            seen.append(nkb)
        assert group == seen.index(nkb)                            # groups are numbered by their first frame
    assert set(seen) == {0, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23}
    # the same on the suites' ragged default frame
    rows, cols = 397, 517
    for s, (group, p, nkb, slot) in zip((1.0, 6.0, 20.0, 50.0), gaussian_frame_sigmas_plan(rows, cols, (1.0, 6.0, 20.0, 50.0))):
        assert p == B.pffft_sizing(rows, cols, s)["pad"] and nkb == expected_nkb(p)


def test_plan_groups_and_slots():
    import blur_algorithms_amd as B
    from blur_algorithms_amd.api import gaussian_frame_sigmas_plan
    rows, cols = 2160, 3840
    pad = lambda s: B.pffft_sizing(rows, cols, s)["pad"]
    cls = lambda s: expected_nkb(pad(s))
    a, a2, b, wide = 5.0, 5.2, 11.0, 80.0
    assert cls(a) == cls(a2) != cls(b) and pad(a) != pad(a2) and cls(wide) == 0
    plan = gaussian_frame_sigmas_plan(rows, cols, (b, a, 0.0, a2, b, a, wide, 0.0, b))
    assert [g for g, _, _, _ in plan] == [0, 1, -1, 1, 0, 1, 2, -1, 0]          # by window class, numbered by first frame
    assert [s for _, _, _, s in plan] == [0, 1, -1, 2, 0, 1, 3, -1, 0]          # equal sigmas share a slot
    assert plan[2] == (-1, 0, 0, -1) and plan[7] == (-1, 0, 0, -1)
    assert plan[6][1] == pad(wide) > 168 and plan[6][2] == 0
    assert plan[1][1:3] == (pad(a), cls(a)) and plan[3][1:3] == (pad(a2), cls(a))
    assert gaussian_frame_sigmas_plan(rows, cols, ()) == []
    assert gaussian_frame_sigmas_plan(rows, cols, (0.0, 0.0)) == [(-1, 0, 0, -1)] * 2
    # the order of the frames, not of the sigmas, numbers the groups
    assert [g for g, _, _, _ in gaussian_frame_sigmas_plan(rows, cols, (a, b))] == [0, 1]
    assert [g for g, _, _, _ in gaussian_frame_sigmas_plan(rows, cols, (b, a))] == [0, 1]


def test_plan_status_codes():
    from blur_algorithms_amd import BlurError
    from blur_algorithms_amd.api import gaussian_frame_sigmas_plan
    L = lib()
    out = (C.c_int * 16)()
    assert L.blur_gaussian_frame_sigmas_plan(100, 100, 3, None, out) == INVALID
    assert L.blur_gaussian_frame_sigmas_plan(100, 100, 3, dbl(1.0, 1.0, 1.0), None) == INVALID
    assert L.blur_gaussian_frame_sigmas_plan(100, 100, -1, dbl(1.0, 1.0), out) == INVALID
    assert L.blur_gaussian_frame_sigmas_plan(100, 100, 3, dbl(1.0, -1.0, 1.0), out) == INVALID
    assert L.blur_gaussian_frame_sigmas_plan(100, 100, 3, dbl(1.0, 1.0, math.nan), out) == INVALID
    assert L.blur_gaussian_frame_sigmas_plan(0, 100, 3, dbl(1.0, 1.0, 1.0), out) == INVALID
    assert L.blur_gaussian_frame_sigmas_plan(40, 90, 3, dbl(1.0, 0.0, 30.0), out) == UNSUPPORTED
    assert L.blur_gaussian_frame_sigmas_plan(100, 100, 0, dbl(1.0), out) == OK
    assert L.blur_gaussian_frame_sigmas_plan(100, 100, 4, dbl(1.0, 1.0, 0.0, 2.0), out) == OK
    with pytest.raises(BlurError):
        gaussian_frame_sigmas_plan(40, 90, (1.0, 30.0, 0.0))


def test_python_wrapper_checks_before_the_library():
    """the sequence must have one sigma per frame; a broadcast source needs `out` (checked on CPU tensors' strides: no device)"""
    import blur_algorithms_amd as B
    from blur_algorithms_amd import api
    ctx = B.BlurContext.__new__(B.BlurContext)          # no device: every case stops in the wrapper
    ctx._lib, ctx._h = lib(), C.c_void_p()
    frames = np.zeros((3, 16, 16, 3), np.uint8)
    for sig in ((1.0, 2.0), (1.0, 2.0, 3.0, 4.0), ()):
        with pytest.raises(ValueError):
            ctx.gaussian_per_frame(frames, sig)
        with pytest.raises(ValueError):
            ctx.gaussian_f32_per_frame(frames.astype(np.float32), sig)
    with pytest.raises(ValueError):
        ctx.gaussian_per_frame(np.zeros((16, 16), np.uint8), (1.0,) * 16)
    import torch
    img = torch.zeros((1, 16, 16, 3), dtype=torch.uint8)
    assert api._broadcast_frames_layout(img.expand(5, -1, -1, -1)) == (48, 0)
    assert api._broadcast_frames_layout(torch.zeros((5, 16, 16, 3), dtype=torch.uint8)) is None
    assert api._broadcast_frames_layout(torch.zeros((1, 32, 32, 3), dtype=torch.uint8)[:, 4:20, 8:24].expand(4, -1, -1, -1)) == (96, 0)
    assert api._broadcast_frames_layout(img.expand(5, -1, -1, -1)[..., :2]) is None      # a channel slice stays refused
