"""Gaussian blur of float32 images of 1, 3 or 4 channels (blur_gaussian_f32_*): every channel blurred on its own as pffft_() blurs
one of its planes, checked against the float64 oracle per channel under the float parity contract |got - oracle| <= 1e-6 max|x|,
across every window class of the fused float kernel (ff_kernels.hpp), value ranges past binary16's, the plane fallback, unaligned
pointers, batches, overlaps and the multi-shard entry."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 2          # BLUR_ERR_INVALID, BLUR_ERR_UNSUPPORTED
NKB_CLASSES = (3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23)
REL_TOL = 1e-6


def sigma_for_pad(rows, cols, lo, hi):
    """a sigma whose pad lies in [lo, hi]"""
    import blur_algorithms_amd as B
    s = 0.5
    while s < 200:
        pad = B.pffft_sizing(rows, cols, s)["pad"]
        if lo <= pad <= hi:
            return s
        s += 0.05 if pad < lo else -0.01
    raise AssertionError("no sigma with pad in [%d, %d]" % (lo, hi))


def sigma_for_class(rows, cols, nkb):
    """a sigma in the upper half of window class nkb (pads 8 (nkb - 4) + 1 .. 8 (nkb - 2))"""
    lo, hi = (1, 8) if nkb == 3 else (8 * (nkb - 4) + 1, 8 * (nkb - 2))
    return sigma_for_pad(rows, cols, (lo + hi) // 2, hi)


def oracle(img, sigma, quirk=True):
    """img [rows, cols, C] float32 -> [rows, cols, C]: ora_pffft_plane_f64 per channel plane"""
    from oracle import oracle as O
    return np.stack([O.pffft_plane_f64(img[..., c], sigma, quirk) for c in range(img.shape[2])], axis=-1)


def check(got, img, sigma, quirk=True):
    want = oracle(img, sigma, quirk)
    got = np.asarray(got, np.float64).reshape(img.shape)
    m = float(np.max(np.abs(img)))
    if m == 0:
        assert np.all(got == 0)
        return 0.0
    err = float(np.max(np.abs(got - want.astype(np.float64))))
    assert err <= REL_TOL * m, "max |error| / max|x| = %.3g" % (err / m)
    return err / m


def rand_img(rng, rows, cols, ch, lo=0.0, hi=1.0):
    return rng.uniform(lo, hi, (rows, cols, ch)).astype(np.float32)


def on_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def blur(ctx, img, sigma, **kw):
    import torch
    t = on_dev(img)
    return ctx.gaussian_f32(t, sigma, out=torch.empty_like(t), **kw).cpu().numpy()


@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("nkb", NKB_CLASSES)
@pytest.mark.parametrize("ch", [1, 3, 4])
def test_every_window_class(ctx, ch, nkb, quirk):
    """the fused kernel of every window class on a ragged width (not a multiple of 4 or 128) and a ragged last row of tiles;
    NKB 23 with 3 or 4 channels has no fused kernel: FUSED refuses, AUTO takes the plane fallback"""
    import blur_algorithms_amd as B
    rows, cols = 397, 517
    sigma = sigma_for_class(rows, cols, nkb)
    img = rand_img(np.random.default_rng(1000 * nkb + ch), rows, cols, ch, -1.0, 1.0)
    if nkb == 23 and ch != 1:
        with pytest.raises(B.BlurError) as e:
            blur(ctx, img, sigma, nyquist_quirk=quirk, engine="fused")
        assert e.value.code == UNSUPPORTED
        got = blur(ctx, img, sigma, nyquist_quirk=quirk)
        assert ctx.last_engine()[0] == 0
    else:
        got = blur(ctx, img, sigma, nyquist_quirk=quirk, engine="fused")
        assert ctx.last_engine()[0] == 6
    check(got, img, sigma, quirk)


RANGES = {
    "u8": (0.0, 255.0),
    "unit": (0.0, 1.0),
    "signed": (-1e3, 1e3),
    "big": (-3e6, 2e6),          # past binary16's range: the scale goes down
    "tiny": (0.0, 1e-6),         # the scale goes up
}


@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("rng_name", sorted(RANGES))
@pytest.mark.parametrize("ch", [1, 3, 4])
def test_value_ranges(ctx, ch, rng_name, quirk):
    rows, cols, sigma = 300, 389, 9.0
    lo, hi = RANGES[rng_name]
    img = rand_img(np.random.default_rng(sorted(RANGES).index(rng_name) + 11), rows, cols, ch, lo, hi)
    check(blur(ctx, img, sigma, nyquist_quirk=quirk), img, sigma, quirk)
    assert ctx.last_engine()[0] == 6


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_constant_and_zero_frames(ctx, ch):
    rows, cols, sigma = 200, 333, 12.0
    img = np.full((rows, cols, ch), 0.7, np.float32)
    check(blur(ctx, img, sigma), img, sigma)
    z = np.zeros((rows, cols, ch), np.float32)
    got = blur(ctx, z, sigma)
    assert np.all(got == 0)


@pytest.mark.parametrize("shape", [(130, 3 * 128 + 5, 6.0), (200, 1027, 20.0), (2000, 61, 4.0), (45, 45, 0.0), (33, 90, 0.0)])
@pytest.mark.parametrize("ch", [1, 3, 4])
def test_shapes(ctx, shape, ch):
    """ragged widths, a tall frame, tiny frames at the pad limit (sigma 0: the largest pad <= min(rows, cols) - 1 the frame reaches)"""
    import blur_algorithms_amd as B
    rows, cols, sigma = shape
    if sigma == 0.0:
        lim = min(rows, cols) - 1                 # (the sizing caps the window on small frames: the largest pad reachable)
        sigma = max((0.5 + 0.25 * i for i in range(240)), key=lambda s: (B.pffft_sizing(rows, cols, s)["pad"] <= lim, B.pffft_sizing(rows, cols, s)["pad"], -s))
        assert B.pffft_sizing(rows, cols, sigma)["pad"] <= lim
    img = rand_img(np.random.default_rng(rows * cols + ch), rows, cols, ch, -5.0, 5.0)
    check(blur(ctx, img, sigma), img, sigma)


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_4k_sigma20(ctx, ch):
    rows, cols, sigma = 2160, 3840, 20.0
    img = rand_img(np.random.default_rng(4000 + ch), rows, cols, ch)
    check(blur(ctx, img, sigma), img, sigma)
    assert ctx.last_engine()[0] == 6


@pytest.mark.parametrize("ch", [1, 3, 4])
@pytest.mark.parametrize("off", [1, 2, 3])
def test_float_offsets_and_guards(ctx, ch, off):
    """source and destination 1 .. 3 floats into their allocations; the floats around the destination stay untouched"""
    import torch
    rows, cols, sigma = 150, 261, 7.0
    n = rows * cols * ch
    img = rand_img(np.random.default_rng(off * 10 + ch), rows, cols, ch, -2.0, 3.0)
    sbuf = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
    sbuf[off:off + n] = on_dev(img).reshape(-1)
    dbuf = torch.full((n + 64,), 1234.5, dtype=torch.float32, device="cuda")
    doff = 32 + off
    src = sbuf[off:off + n].view(rows, cols, ch)
    dst = dbuf[doff:doff + n].view(rows, cols, ch)
    ctx.gaussian_f32(src, sigma, out=dst)
    d = dbuf.cpu().numpy()
    assert np.all(d[:doff] == np.float32(1234.5)) and np.all(d[doff + n:] == np.float32(1234.5))
    check(d[doff:doff + n], img, sigma)


@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("ch", [1, 3, 4])
def test_batch_bitwise_equals_single_no_bleed(ctx, ch, quirk):
    """a batch gives the same bits as one call per frame; frames of very different magnitudes do not bleed into each other"""
    import torch
    rows, cols, sigma = 260, 300, 11.0
    rng = np.random.default_rng(77 + ch)
    scales = [1.0, 1e5, 1e-4, 0.0, 300.0]
    frames = np.stack([rand_img(rng, rows, cols, ch, -1.0, 1.0) * np.float32(s) for s in scales])
    t = on_dev(frames)
    got = ctx.gaussian_f32(t, sigma, out=torch.empty_like(t), nyquist_quirk=quirk).cpu().numpy()
    for i in range(len(scales)):
        one = blur(ctx, frames[i], sigma, nyquist_quirk=quirk)
        assert np.array_equal(got[i].view(np.uint32), one.view(np.uint32))
        check(got[i], frames[i], sigma, quirk)
    again = ctx.gaussian_f32(t, sigma, out=torch.empty_like(t), nyquist_quirk=quirk).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_in_place_and_partial_overlap(ctx, ch):
    import torch
    rows, cols, sigma, n = 120, 200, 6.0, 3
    frames = np.stack([rand_img(np.random.default_rng(i), rows, cols, ch, -1, 1) for i in range(n)])
    want = np.stack([oracle(f, sigma) for f in frames])
    fe = rows * cols * ch
    t = on_dev(frames)
    ctx.gaussian_f32(t, sigma)                                               # in place
    got = t.cpu().numpy()
    for i in range(n):
        assert np.max(np.abs(got[i] - want[i])) <= REL_TOL * np.max(np.abs(frames[i]))
    # destination half a frame past the source
    buf = torch.zeros(fe * (n + 1), dtype=torch.float32, device="cuda")
    buf[:fe * n] = on_dev(frames).reshape(-1)
    src = buf[:fe * n].view(n, rows, cols, ch)
    dst = buf[fe // 2:fe // 2 + fe * n].view(n, rows, cols, ch)
    ctx.gaussian_f32(src, sigma, out=dst)
    got = dst.cpu().numpy()
    for i in range(n):
        assert np.max(np.abs(got[i] - want[i])) <= REL_TOL * np.max(np.abs(frames[i]))


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_host_entry_fft_engine_and_two_shards(ctx, ch):
    import torch
    import blur_algorithms_amd as B
    rows, cols, sigma, n = 270, 480, 20.0, 4
    frames = np.random.default_rng(40 + ch).uniform(-10, 10, (n, rows, cols, ch)).astype(np.float32)
    want = ctx.gaussian_f32(on_dev(frames), sigma, out=torch.empty(frames.shape, dtype=torch.float32, device="cuda")).cpu().numpy()
    assert ctx.last_engine()[0] == 6
    assert np.array_equal(ctx.gaussian_f32(frames, sigma), want)            # numpy: the host entry per frame
    fft = ctx.gaussian_f32(on_dev(frames), sigma, engine="fft").cpu().numpy()
    assert ctx.last_engine()[0] == 0
    for i in range(n):
        m = np.max(np.abs(frames[i]))
        assert np.max(np.abs(fft[i].astype(np.float64) - want[i])) <= 2 * REL_TOL * m
        check(fft[i], frames[i], sigma)
    m = B.BlurMulti([0, 0])
    try:
        assert np.array_equal(m.gaussian_f32(frames, sigma), want)
        t = on_dev(frames)
        assert np.array_equal(m.gaussian_f32(t, sigma, out=torch.empty_like(t)).cpu().numpy(), want)
        assert m.gaussian_f32(frames[:0], sigma).shape == frames[:0].shape
    finally:
        m.close()


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_plane_fallback_wide_pad(ctx, ch):
    """pad > 168: no fused kernel; AUTO takes the plane fallback within the same bound, FUSED refuses"""
    import blur_algorithms_amd as B
    rows, cols = 420, 390
    sigma = sigma_for_pad(rows, cols, 175, 200)
    img = rand_img(np.random.default_rng(7), rows, cols, ch, -1, 4)
    check(blur(ctx, img, sigma), img, sigma)
    assert ctx.last_engine()[0] == 0
    with pytest.raises(B.BlurError) as e:
        blur(ctx, img, sigma, engine="fused")
    assert e.value.code == UNSUPPORTED


def test_zero_frames_and_bad_args_on_device(ctx):
    import torch
    from blur_algorithms_amd._lib import BlurOpts
    L = ctx._lib
    o = BlurOpts()
    L.blur_opts_default(C.byref(o))
    t = torch.zeros(64, dtype=torch.float32, device="cuda")
    assert L.blur_gaussian_f32_batch_dev(ctx._h, t.data_ptr(), t.data_ptr(), 0, 4, 4, 1, 1.0, C.byref(o)) == 0
    assert L.blur_gaussian_f32_batch_dev(ctx._h, t.data_ptr(), t.data_ptr(), 1, 4, 4, 2, 1.0, C.byref(o)) == INVALID
    o.engine = 3
    assert L.blur_gaussian_f32_batch_dev(ctx._h, t.data_ptr(), t.data_ptr(), 1, 4, 4, 1, 1.0, C.byref(o)) == UNSUPPORTED
