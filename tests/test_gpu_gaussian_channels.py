"""Gaussian blur of 1- and 4-channel u8 images (blur_gaussian_u8_*): every channel blurred on its own as pffft_() blurs one of its
three, checked against the float64 oracle per channel plane under the parity contract, across every window class of the fused
kernel (fw_kernels.hpp), the plane fallback, ragged and edge-strip widths, unaligned pointers, batches and the multi-shard entry."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_u8_parity

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 2          # BLUR_ERR_INVALID, BLUR_ERR_UNSUPPORTED
NKB_CLASSES = (3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23)


def sigma_for_pad(rows, cols, lo, hi):
    """a sigma whose pad lies in [lo, hi]"""
    import blur_algorithms_amd as B
    s = 0.5
    while s < 200:
        pad = B.pffft_sizing(rows, cols, s)["pad"]
        if lo <= pad <= hi:
            return s
        s += 0.05 if pad < lo else -0.01
        if pad > hi and s < 0.5:
            break
    raise AssertionError("no sigma with pad in [%d, %d]" % (lo, hi))


def sigma_for_class(rows, cols, nkb):
    """a sigma in the middle of window class nkb (pads 8 (nkb - 4) + 1 .. 8 (nkb - 2))"""
    lo, hi = (1, 8) if nkb == 3 else (8 * (nkb - 4) + 1, 8 * (nkb - 2))
    return sigma_for_pad(rows, cols, (lo + hi) // 2, hi)


def oracle(img, sigma, quirk=True):
    """img [rows, cols, C] uint8 -> (bytes [rows, cols, C], planes [C, rows, cols]): ora_pffft_plane_f64 per channel plane"""
    from oracle import oracle as O
    planes = np.stack([O.pffft_plane_f64(img[..., c].astype(np.float32), sigma, quirk) for c in range(img.shape[2])])
    want = ((planes.astype(np.float32) + np.float32(0.5)).astype(np.int64) & 0xff).astype(np.uint8)
    return np.moveaxis(want, 0, -1), planes


def check(got, img, sigma, quirk=True):
    want, planes = oracle(img, sigma, quirk)
    assert_u8_parity(got.reshape(img.shape), want, planes)


def rand_img(rng, rows, cols, ch):
    return rng.integers(0, 256, (rows, cols, ch), dtype=np.uint8)


def on_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("nkb", NKB_CLASSES)
@pytest.mark.parametrize("ch", [1, 4])
def test_every_window_class(ctx, ch, nkb, quirk):
    """the fused kernel of every window class, a ragged width (not a multiple of 4 or 128) and a ragged last row of tiles"""
    rows, cols = 397, 517
    sigma = sigma_for_class(rows, cols, nkb)
    img = rand_img(np.random.default_rng(1000 * nkb + ch), rows, cols, ch)
    t = on_dev(img)
    got = ctx.gaussian(t, sigma, out=t.clone(), nyquist_quirk=quirk, engine="fused")
    assert ctx.last_engine()[0] == 6
    check(got.cpu().numpy(), img, sigma, quirk)


@pytest.mark.parametrize("ch", [1, 4])
def test_plane_fallback_wide_pad(ctx, ch):
    """pad > 168: no fused kernel; AUTO takes the plane fallback, FUSED refuses"""
    import blur_algorithms_amd as B
    rows, cols = 420, 390
    sigma = sigma_for_pad(rows, cols, 175, 200)
    img = rand_img(np.random.default_rng(7), rows, cols, ch)
    t = on_dev(img)
    got = ctx.gaussian(t, sigma, out=t.clone())
    assert ctx.last_engine()[0] == 0
    check(got.cpu().numpy(), img, sigma)
    with pytest.raises(B.BlurError):
        ctx.gaussian(t, sigma, out=t.clone(), engine="fused")


@pytest.mark.parametrize("ch", [1, 4])
@pytest.mark.parametrize("engine", ["fft", None])
def test_fft_engine_and_auto(ctx, ch, engine):
    rows, cols = 301, 262
    sigma = 6.0
    img = rand_img(np.random.default_rng(11), rows, cols, ch)
    t = on_dev(img)
    got = ctx.gaussian(t, sigma, out=t.clone(), engine=engine)
    assert ctx.last_engine()[0] == (0 if engine == "fft" else 6)
    check(got.cpu().numpy(), img, sigma)


# (rows, cols, sigma): edge-strip boundaries (one and two strips at the left, chunks next to the right edge), widths 1 .. 3 past a
# multiple of 4 and of 128, a tiny frame, a tall one, a frame under 1 MP
SHAPES = [(260, 128 * 3 + 72, 20.0), (260, 128 * 3 + 73, 20.0), (300, 256 + 1, 12.0), (300, 640 + 2, 20.0), (300, 640 + 3, 3.0),
          (333, 1000, 40.0), (40, 33, 3.0), (35, 9, 1.0), (2500, 140, 20.0), (700, 1100, 20.0), (180, 1500, 52.0)]


@pytest.mark.parametrize("ch", [1, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d-s%g" % s for s in SHAPES])
def test_shapes(ctx, ch, shape):
    rows, cols, sigma = shape
    img = rand_img(np.random.default_rng(rows * 7 + cols), rows, cols, ch)
    for quirk in (True, False):
        t = on_dev(img)
        got = ctx.gaussian(t, sigma, out=t.clone(), nyquist_quirk=quirk)
        check(got.cpu().numpy(), img, sigma, quirk)


@pytest.mark.parametrize("ch", [1, 4])
@pytest.mark.parametrize("offset", [1, 2, 3])
def test_unaligned_pointers(ctx, ch, offset):
    import torch
    rows, cols, sigma = 250, 403, 15.0
    img = rand_img(np.random.default_rng(offset), rows, cols, ch)
    fb = img.size
    src = torch.zeros(fb + 8, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(fb + 8, dtype=torch.uint8, device="cuda")
    s = src[offset:offset + fb].view(rows, cols, ch)
    d = dst[3 - offset + 1:3 - offset + 1 + fb].view(rows, cols, ch)
    s.copy_(torch.from_numpy(img))
    ctx.gaussian(s, sigma, out=d)
    assert ctx.last_engine()[0] == 6
    check(d.cpu().numpy(), img, sigma)
    # nothing outside the destination was written
    full = dst.cpu().numpy()
    assert not full[:3 - offset + 1].any() and not full[3 - offset + 1 + fb:].any()


@pytest.mark.parametrize("ch", [1, 4])
@pytest.mark.parametrize("sigma", [20.0, 50.0])
def test_metric_shape(ctx, ch, sigma):
    rows, cols = 2160, 3840
    img = rand_img(np.random.default_rng(int(sigma) + ch), rows, cols, ch)
    t = on_dev(img)
    got = ctx.gaussian(t, sigma, out=torch_empty_like(t))
    check(got.cpu().numpy(), img, sigma)


def torch_empty_like(t):
    import torch
    return torch.empty_like(t)


@pytest.mark.parametrize("ch", [1, 4])
def test_batch_equals_single_calls_no_bleed_in_place(ctx, ch):
    import torch
    rows, cols, sigma, n = 300, 389, 18.0, 5
    rng = np.random.default_rng(5 + ch)
    frames = rng.integers(0, 256, (n, rows, cols, ch), dtype=np.uint8)
    frames[1] = 0                                  # neighbours of constant 0 / 255: any bleed shows
    frames[3] = 255
    t = on_dev(frames)
    batch = ctx.gaussian(t, sigma, out=torch.empty_like(t)).cpu().numpy()
    for f in range(n):
        one = ctx.gaussian(t[f], sigma, out=torch.empty_like(t[f])).cpu().numpy()
        assert np.array_equal(batch[f], one), "frame %d" % f
    check(batch[2], frames[2], sigma)
    c0 = ctx.gaussian(on_dev(np.zeros_like(frames[1])), sigma, out=torch.empty_like(t[1])).cpu().numpy()
    c255 = ctx.gaussian(on_dev(np.full_like(frames[3], 255)), sigma, out=torch.empty_like(t[3])).cpu().numpy()
    assert np.array_equal(batch[1], c0) and np.array_equal(batch[3], c255)
    # in place equals out of place, for the fused kernel and the plane fallback
    for engine in (None, "fft"):
        want = ctx.gaussian(t, sigma, out=torch.empty_like(t), engine=engine).cpu().numpy()
        u = on_dev(frames)
        ctx.gaussian(u, sigma, engine=engine)
        assert np.array_equal(u.cpu().numpy(), want)


@pytest.mark.parametrize("ch", [1, 4])
def test_partial_overlap(ctx, ch):
    """destination = source shifted by one frame and a few bytes: the whole batch range is read from a copy"""
    import torch
    rows, cols, sigma, n = 130, 200, 9.0, 3
    frames = np.random.default_rng(9).integers(0, 256, (n, rows, cols, ch), dtype=np.uint8)
    fb = rows * cols * ch
    for engine in (None, "fft"):
        want = ctx.gaussian(on_dev(frames), sigma, out=torch.empty(frames.shape, dtype=torch.uint8, device="cuda"), engine=engine).cpu().numpy()
        buf = torch.zeros(fb * (n + 2), dtype=torch.uint8, device="cuda")
        src = buf[:fb * n].view(n, rows, cols, ch)
        src.copy_(torch.from_numpy(frames))
        dst = buf[fb + 5:fb + 5 + fb * n].view(n, rows, cols, ch)
        ctx.gaussian(src, sigma, out=dst, engine=engine)
        assert np.array_equal(dst.cpu().numpy(), want)


def test_zero_frames_and_arguments(ctx):
    import torch
    from blur_algorithms_amd._lib import BlurOpts
    L = ctx._lib
    t = torch.full((64,), 7, dtype=torch.uint8, device="cuda")
    o = BlurOpts()
    L.blur_opts_default(C.byref(o))
    assert L.blur_gaussian_u8_batch_dev(ctx._h, t.data_ptr(), t.data_ptr(), 0, 4, 4, 4, 1.0, C.byref(o)) == 0
    torch.cuda.synchronize()
    assert (t.cpu().numpy() == 7).all()
    assert L.blur_gaussian_u8_batch_dev(ctx._h, t.data_ptr(), t.data_ptr(), 1, 4, 4, 2, 1.0, C.byref(o)) == INVALID
    assert L.blur_gaussian_u8_batch_dev(ctx._h, t.data_ptr(), t.data_ptr(), -1, 4, 4, 1, 1.0, C.byref(o)) == INVALID


@pytest.mark.parametrize("ch", [1, 4])
def test_host_entry_and_two_shards(ctx, ch):
    import torch
    import blur_algorithms_amd as B
    rows, cols, sigma, n = 270, 480, 20.0, 4
    frames = np.random.default_rng(40 + ch).integers(0, 256, (n, rows, cols, ch), dtype=np.uint8)
    want = ctx.gaussian(on_dev(frames), sigma, out=torch.empty(frames.shape, dtype=torch.uint8, device="cuda")).cpu().numpy()
    assert np.array_equal(ctx.gaussian(frames, sigma), want)                 # numpy: the host entry per frame
    m = B.BlurMulti([0, 0])
    try:
        assert np.array_equal(m.gaussian(frames, sigma), want)
        t = on_dev(frames)
        assert np.array_equal(m.gaussian(t, sigma, out=torch.empty_like(t)).cpu().numpy(), want)
        assert np.array_equal(m.gaussian(frames[:0], sigma), frames[:0])
    finally:
        m.close()


@pytest.mark.parametrize("shape", [(270, 480, 20.0), (1080, 1920, 30.0), (2160, 3840, 50.0), (301, 517, 3.0)])
def test_three_channels_forward_to_u8c3(ctx, shape):
    """channels = 3 through the new entry is the u8c3 call byte for byte; the 1-channel call takes the fused kernel wherever the
    u8c3 call on the same shape and sigma does (and wherever a fused kernel exists for the pad)"""
    import torch
    rows, cols, sigma = shape
    img = np.random.default_rng(rows).integers(0, 256, (2, rows, cols, 3), dtype=np.uint8)
    t = on_dev(img)
    a = ctx.gaussian(t, sigma, out=torch.empty_like(t)).cpu().numpy()
    fam3 = ctx.last_engine()[0]
    b = ctx.pffft_(t, sigma, out=torch.empty_like(t)).cpu().numpy()
    assert np.array_equal(a, b)
    g = on_dev(img[..., :1])
    ctx.gaussian(g, sigma, out=torch.empty_like(g))
    fam1 = ctx.last_engine()[0]
    assert fam1 == 6 or fam3 != 6
    assert fam1 == 6                                  # every pad of these shapes is <= 168
