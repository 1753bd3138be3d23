"""Gaussian blur of u16 images of 1, 3 or 4 channels (blur_gaussian_u16_*): every channel blurred on its own as pffft_() blurs one of
its planes, rounded as (uint16_t)((uint32_t)(int32_t)(v + 0.5f) & 0xffff), checked against the float64 oracle per channel under
u16_parity.assert_u16_parity: every window class of the fused kernel's u16 instantiation (ff_kernels.hpp), the plane path, noise
and structured content (wraps past both ends of the range included), ragged shapes, odd-aligned pointers, batches, overlaps,
redzones and the multi-shard entry."""
import ctypes as C

import numpy as np
import pytest

import structured as S
import u16_parity as U
from conftest import assert_u8_parity

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 2          # BLUR_ERR_INVALID, BLUR_ERR_UNSUPPORTED
ROWS, COLS = U.SHAPE
AUTO_MAX_NKB = 15                    # ff_class_in_contract: the library's own choice stops here (pad <= 104)


def sigma_for_pad(rows, cols, lo, hi):
    import blur_algorithms_amd as B
    s = 0.5
    while s < 200:
        pad = B.pffft_sizing(rows, cols, s)["pad"]
        if lo <= pad <= hi:
            return s
        s += 0.05 if pad < lo else -0.01
    raise AssertionError("no sigma with pad in [%d, %d]" % (lo, hi))


def on_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def blur(ctx, img, sigma, **kw):
    import torch
    t = on_dev(img)
    return ctx.gaussian_u16(t, sigma, out=torch.empty_like(t), **kw).cpu().numpy()


def check(got, img, sigma, quirk=True):
    """img [rows, cols, ch] uint16"""
    return U.assert_u16_parity(np.asarray(got).reshape(img.shape), U.oracle_frame(img, sigma, quirk))


def noise_img(seed, rows, cols, ch, top=65535):
    return np.stack([U.noise(seed + 17 * c, rows, cols, top) for c in range(ch)], axis=-1)


def named_frame(names, rows, cols, nkb=None, quirk=True):
    return np.stack([U.plane(n, rows, cols, U.case_levels(n, nkb, quirk)) for n in names], axis=-1)


def named_planes(names, rows, cols, sigma, quirk, nkb=None):
    return np.stack([U.oracle_named(n, rows, cols, sigma, quirk, U.case_levels(n, nkb, quirk)) for n in names])


def fused(ctx, img, sigma, quirk):
    """engine="fused" (family 6): every window class is instantiated for every channel count"""
    got = blur(ctx, img, sigma, nyquist_quirk=quirk, engine="fused")
    assert ctx.last_engine()[0] == 6
    return got


@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("nkb", U.NKB_CLASSES)
@pytest.mark.parametrize("ch", [1, 3, 4])
def test_every_window_class_noise(ctx, ch, nkb, quirk):
    """full-range noise (12-bit noise in the last channel of a multi-channel frame) on a ragged frame, every class on FUSED"""
    sigma = U.class_sigma(nkb)
    img = noise_img(1000 * nkb, ROWS, COLS, ch)
    if ch > 1:
        img[..., ch - 1] = U.noise(7 + nkb, ROWS, COLS, 4095)
    check(fused(ctx, img, sigma, quirk), img, sigma, quirk)


@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("nkb", U.NKB_CLASSES)
@pytest.mark.parametrize("ch", [1, 3, 4])
def test_every_window_class_structured(ctx, ch, nkb, quirk):
    """every structured case at the levels that passed the CPU proof, channel c of frame i taking pattern i + c.  Up to NKB 15 on FUSED (= the
    library's choice).  NKB 17 .. 23: the float kernel is known to exceed 1e-6 of full scale on step content there, so the steps
    run on AUTO (family 0, the same tolerance) and every other pattern on FUSED"""
    sigma = U.class_sigma(nkb)
    names = U.class_patterns(nkb, quirk)
    groups = [(names, "fused")] if nkb <= AUTO_MAX_NKB else [(tuple(n for n in names if n not in U.STEPS), "fused"),
                                                            (tuple(n for n in names if n in U.STEPS), None)]
    for pats, engine in groups:
        assert len(pats) > 0
        for i in range(0, len(pats), 1 if ch == 1 else ch):
            sel = [pats[(i + c) % len(pats)] for c in range(ch)]
            img = named_frame(sel, ROWS, COLS, nkb, quirk)
            if engine == "fused":
                got = fused(ctx, img, sigma, quirk)
            else:
                got = blur(ctx, img, sigma, nyquist_quirk=quirk)
                assert ctx.last_engine()[0] == 0
            try:
                U.assert_u16_parity(got, named_planes(sel, ROWS, COLS, sigma, quirk, nkb))
            except AssertionError as e:
                raise AssertionError("%s (engine %s): %s" % (sel, engine, e))


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_auto_routes(ctx, ch):
    """AUTO: the fused kernel for a pad <= 104, the plane path for one in 105 .. 168"""
    img = noise_img(5, ROWS, COLS, ch)
    for lo, hi, family in ((60, 104, 6), (110, 150, 0)):
        sigma = sigma_for_pad(ROWS, COLS, lo, hi)
        got = blur(ctx, img, sigma)
        assert ctx.last_engine()[0] == family
        check(got, img, sigma)


@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("pads", [(10, 30), (120, 160)])
@pytest.mark.parametrize("ch", [1, 3, 4])
def test_fft_engine_plane_path(ctx, ch, pads, quirk):
    sigma = sigma_for_pad(ROWS, COLS, *pads)
    img = noise_img(9 + pads[0], ROWS, COLS, ch)
    img[..., 0] = U.plane("step_diag", ROWS, COLS)
    got = blur(ctx, img, sigma, nyquist_quirk=quirk, engine="fft")
    assert ctx.last_engine()[0] == 0
    check(got, img, sigma, quirk)


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_zero_frame(ctx, ch):
    z = np.zeros((200, 333, ch), np.uint16)
    assert np.all(blur(ctx, z, 12.0) == 0)
    assert ctx.last_engine()[0] == 6
    assert np.all(blur(ctx, z, 12.0, engine="fft") == 0)
    assert ctx.last_engine()[0] == 0


@pytest.mark.parametrize("engine", ["fused", "fft"])
@pytest.mark.parametrize("ch", [1, 3, 4])
def test_wraps_past_both_ends(ctx, ch, engine):
    """no clamping: with the quirk on a constant 65535 frame leaves the range at the top (v + 0.5 >= 65536 wraps to small values)
    and a 0 / 65533 diagonal step at the bottom (v + 0.5 <= -1 wraps to values near 65535); both cases are checked to contain
    such samples, from the oracle planes"""
    sigma = 9.0
    top = named_planes(["const_top"], ROWS, COLS, sigma, True)[0].astype(np.float64)
    bottom = named_planes(["step_diag"], ROWS, COLS, sigma, True)[0].astype(np.float64)
    assert (top + 0.5 >= 65536).any(), "the constant no longer wraps above 65535.5"
    assert (bottom + 0.5 <= -1).any(), "the step no longer wraps below 0"
    frames = [["const_top"], ["step_diag"]] if ch == 1 else [["const_top", "step_diag", "const_top", "step_diag"][:ch]]
    for names in frames:
        got = blur(ctx, named_frame(names, ROWS, COLS), sigma, engine=engine)
        assert ctx.last_engine()[0] == (6 if engine == "fused" else 0)
        U.assert_u16_parity(got, named_planes(names, ROWS, COLS, sigma, True))
    if ch > 1:
        assert (got[..., 0][top + 0.5 >= 65537] < 1000).all() and (got[..., 1][bottom + 0.5 <= -2] > 64000).all()


@pytest.mark.parametrize("shape", [(130, 3 * 128 + 1, 6.0), (130, 3 * 128 + 2, 6.0), (130, 3 * 128 + 3, 6.0), (150, 261, 7.0), (150, 262, 7.0),
                                   (150, 263, 7.0), (2000, 61, 4.0), (45, 45, 0.0), (33, 90, 0.0)])
@pytest.mark.parametrize("ch", [1, 3, 4])
def test_shapes(ctx, shape, ch):
    """widths 1 .. 3 past a multiple of 128 and of 4, a tall narrow frame, tiny frames at the pad limit (sigma 0: the largest pad
    <= min(rows, cols) - 1 the frame reaches)"""
    import blur_algorithms_amd as B
    rows, cols, sigma = shape
    if sigma == 0.0:
        lim = min(rows, cols) - 1
        sigma = max((0.5 + 0.25 * i for i in range(240)), key=lambda s: (B.pffft_sizing(rows, cols, s)["pad"] <= lim, B.pffft_sizing(rows, cols, s)["pad"], -s))
        assert B.pffft_sizing(rows, cols, sigma)["pad"] <= lim
    img = noise_img(rows * cols + ch, rows, cols, ch)
    got = blur(ctx, img, sigma)
    assert ctx.last_engine()[0] == 6
    check(got, img, sigma)


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_4k_sigma20(ctx, ch):
    rows, cols, sigma = 2160, 3840, 20.0
    img = noise_img(4000 + ch, rows, cols, ch)
    check(blur(ctx, img, sigma), img, sigma)
    assert ctx.last_engine()[0] == 6


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_1080p_sigma20(ctx, ch):
    rows, cols, sigma = 1080, 1920, 20.0
    img = noise_img(1080 + ch, rows, cols, ch, 4095)
    check(blur(ctx, img, sigma), img, sigma)
    assert ctx.last_engine()[0] == 6


GUARD = 32 * 1024                    # 64 KiB of u16 samples


def guarded(n):
    """a host buffer of GUARD + 1 + n + GUARD + 1 samples holding a known pattern"""
    return ((np.arange(2 * GUARD + n + 2, dtype=np.int64) * 40503 + 12345) % 65536).astype(np.uint16)


@pytest.mark.parametrize("engine", [None, "fft"])
@pytest.mark.parametrize("offs", [(1, 0), (0, 1), (1, 1), (0, 0)])
@pytest.mark.parametrize("ch", [1, 3, 4])
def test_odd_pointers_and_redzones(ctx, ch, offs, engine):
    """source and destination at odd element offsets (2-byte but not 4-byte aligned), each alone and both; 64 KiB of a known
    pattern before and after the source and the destination stay as they were"""
    rows, cols, sigma = 150, 261, 7.0
    n = rows * cols * ch
    img = noise_img(offs[0] * 10 + offs[1] * 5 + ch, rows, cols, ch)
    soff, doff = GUARD + offs[0], GUARD + offs[1]
    shost, dhost = guarded(n), guarded(n)
    shost[soff:soff + n] = img.reshape(-1)
    sbuf, dbuf = on_dev(shost), on_dev(dhost)
    assert sbuf.data_ptr() % 4 == 0 and dbuf.data_ptr() % 4 == 0
    src = sbuf[soff:soff + n].view(rows, cols, ch)
    dst = dbuf[doff:doff + n].view(rows, cols, ch)
    assert src.data_ptr() % 4 == 2 * offs[0] and dst.data_ptr() % 4 == 2 * offs[1]
    ctx.gaussian_u16(src, sigma, out=dst, engine=engine)
    assert ctx.last_engine()[0] == (6 if engine is None else 0)
    d = dbuf.cpu().numpy()
    assert np.array_equal(d[:doff], dhost[:doff]) and np.array_equal(d[doff + n:], dhost[doff + n:])
    assert np.array_equal(sbuf.cpu().numpy(), shost)
    check(d[doff:doff + n], img, sigma)


@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("ch", [1, 3, 4])
def test_batch_bitwise_equals_single(ctx, ch, quirk):
    """5 frames of very different content give the same bits as 5 single calls (the scale is a constant of the call)"""
    import torch
    rows, cols, sigma = 260, 301, 11.0
    tops = [65535, 255, 4095, 0, 1023]
    frames = np.stack([noise_img(77 + i, rows, cols, ch, top) for i, top in enumerate(tops)])
    t = on_dev(frames)
    got = ctx.gaussian_u16(t, sigma, out=torch.empty_like(t), nyquist_quirk=quirk).cpu().numpy()
    assert ctx.last_engine()[0] == 6
    for i in range(len(tops)):
        assert np.array_equal(got[i], blur(ctx, frames[i], sigma, nyquist_quirk=quirk))
        if tops[i]:
            check(got[i], frames[i], sigma, quirk)
        else:
            assert np.all(got[i] == 0)
    again = ctx.gaussian_u16(t, sigma, out=torch.empty_like(t), nyquist_quirk=quirk).cpu().numpy()
    assert np.array_equal(got, again)


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_in_place_overlap_and_zero_frames(ctx, ch):
    rows, cols, sigma, n = 120, 201, 6.0, 3
    frames = np.stack([noise_img(i, rows, cols, ch) for i in range(n)])
    fe = rows * cols * ch
    t = on_dev(frames)
    assert ctx.gaussian_u16(t, sigma) is t                                   # in place
    assert ctx.last_engine()[0] == 6
    got = t.cpu().numpy()
    for i in range(n):
        check(got[i], frames[i], sigma)
    # destination one frame past the source
    host = np.zeros(fe * (n + 1), np.uint16)
    host[:fe * n] = frames.reshape(-1)
    buf = on_dev(host)
    src = buf[:fe * n].view(n, rows, cols, ch)
    dst = buf[fe:fe + fe * n].view(n, rows, cols, ch)
    ctx.gaussian_u16(src, sigma, out=dst)
    assert ctx.last_engine()[0] == 6
    assert np.array_equal(dst.cpu().numpy(), got)
    # no frames: nothing happens (the buffer keeps its bits)
    from blur_algorithms_amd._lib import BlurOpts
    o = BlurOpts()
    ctx._lib.blur_opts_default(C.byref(o))
    before = buf.cpu().numpy()
    assert ctx._lib.blur_gaussian_u16_batch_dev(ctx._h, src.data_ptr(), dst.data_ptr(), 0, rows, cols, ch, sigma, C.byref(o)) == 0
    ctx.synchronize()
    assert np.array_equal(buf.cpu().numpy(), before)


@pytest.mark.parametrize("ch", [1, 4])
def test_8bit_frame_in_u16_agrees_with_u8_entry(ctx, ch):
    """an 8-bit frame stored in u16, quirk off, whose oracle output stays inside [0, 255]: the u16 entry and the u8 entry each pass
    their own parity rule on it, from the same oracle planes"""
    import torch
    rows, cols, sigma = 300, 389, 9.0
    img8 = np.stack([np.random.default_rng(3 + c).integers(0, 256, (rows, cols), dtype=np.uint8) for c in range(ch)], axis=-1)
    planes = U.oracle_frame(img8.astype(np.uint16), sigma, False)
    assert planes.min() + 0.5 >= 0 and planes.max() + 0.5 < 256
    got16 = blur(ctx, img8.astype(np.uint16), sigma, nyquist_quirk=False)
    assert ctx.last_engine()[0] == 6
    U.assert_u16_parity(got16, planes)
    t = on_dev(img8)
    got8 = ctx.gaussian(t, sigma, out=torch.empty_like(t), nyquist_quirk=False).cpu().numpy()
    assert ctx.last_engine()[0] == 6
    want8 = np.moveaxis(S.round_u8(planes), 0, -1)
    assert_u8_parity(got8.reshape(rows, cols, ch), want8, planes)


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_host_entry_and_two_shards(ctx, ch):
    import torch
    import blur_algorithms_amd as B
    rows, cols, sigma, n = 270, 481, 20.0, 4
    frames = np.stack([noise_img(40 + i, rows, cols, ch) for i in range(n)])
    t = on_dev(frames)
    want = ctx.gaussian_u16(t, sigma, out=torch.empty_like(t)).cpu().numpy()
    assert ctx.last_engine()[0] == 6
    check(want[0], frames[0], sigma)
    assert np.array_equal(ctx.gaussian_u16(frames, sigma), want)            # numpy: the host entry per frame
    m = B.BlurMulti([0, 0])
    try:
        assert np.array_equal(m.gaussian_u16(frames, sigma), want)
        t = on_dev(frames)
        assert np.array_equal(m.gaussian_u16(t, sigma, out=torch.empty_like(t)).cpu().numpy(), want)
        assert m.gaussian_u16(frames[:0], sigma).shape == frames[:0].shape
    finally:
        m.close()


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_plane_fallback_wide_pad(ctx, ch):
    """pad > 168: no fused kernel; AUTO takes the plane fallback, FUSED refuses"""
    import blur_algorithms_amd as B
    rows, cols = 420, 390
    sigma = sigma_for_pad(rows, cols, 175, 200)
    img = noise_img(7, rows, cols, ch)
    check(blur(ctx, img, sigma), img, sigma)
    assert ctx.last_engine()[0] == 0
    with pytest.raises(B.BlurError) as e:
        blur(ctx, img, sigma, engine="fused")
    assert e.value.code == UNSUPPORTED


def test_zero_frames_and_bad_args_on_device(ctx):
    from blur_algorithms_amd._lib import BlurOpts
    L = ctx._lib
    o = BlurOpts()
    L.blur_opts_default(C.byref(o))
    t = on_dev(np.zeros(64, np.uint16))
    assert L.blur_gaussian_u16_batch_dev(ctx._h, t.data_ptr(), t.data_ptr(), 0, 4, 4, 1, 1.0, C.byref(o)) == 0
    assert L.blur_gaussian_u16_batch_dev(ctx._h, t.data_ptr(), t.data_ptr(), 1, 4, 4, 2, 1.0, C.byref(o)) == INVALID
    o.engine = 3
    assert L.blur_gaussian_u16_batch_dev(ctx._h, t.data_ptr(), t.data_ptr(), 1, 4, 4, 1, 1.0, C.byref(o)) == UNSUPPORTED
