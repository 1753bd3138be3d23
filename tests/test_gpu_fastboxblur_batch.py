"""fastboxblur over batches of frames: the batch entries (device, host, several shards) against the CPU oracle frame by
frame and against single calls."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def _frames(rng, n, h, w, ch, kind):
    shape = (n, h, w) if ch == 1 else (n, h, w, ch)
    if kind == "binary":
        return (rng.integers(0, 2, shape) * 255).astype(np.uint8)
    return rng.integers(0, 256, shape, dtype=np.uint8)


def _oracle(frames, ksize, passes):
    from oracle import oracle as O
    return np.stack([O.fastboxblur_u8(f, ksize, passes) for f in frames])


# (w, h, channels, ksize, passes, nframes)
BATCH_SHAPES = [
    (640, 300, 3, 41, 3, 7),      # vertical window of one block (r <= 24), channel-plane horizontal kernel
    (640, 300, 3, 113, 2, 2),     # r = 56: the wider vertical window
    (333, 200, 4, 101, 2, 2),     # r = 50: vertical on the matrix cores, horizontal box wider than its windows (accumulators)
    (512, 200, 1, 121, 3, 2),     # r = 60: wider than every window, accumulators both ways
    (641, 100, 3, 41, 1, 7),      # pitch 1923: no multiple of 4 (vertical accumulator sweeps)
    (300, 40, 3, 41, 3, 7),       # 40 rows: too short for the vertical pipeline (column accumulator kernel)
    (200, 90, 3, 9, 5, 7),        # 90 rows (no multiple of 16), five passes (three + two)
    (256, 130, 1, 9, 2, 1),
    (128, 200, 4, 15, 1, 2),
    (3847, 40, 3, 41, 3, 2),
    (335, 203, 3, 41, 3, 2),
]


@pytest.mark.parametrize("w,h,ch,ksize,passes,n", BATCH_SHAPES)
@pytest.mark.parametrize("kind", ["uniform", "binary"])
def test_batch_equals_the_oracle_per_frame(ctx, w, h, ch, ksize, passes, n, kind):
    torch = _torch()
    frames = _frames(np.random.default_rng(w * 31 + h * 7 + n), n, h, w, ch, kind)
    want = _oracle(frames, ksize, passes)
    got = ctx.fastboxblur_batch(torch.from_numpy(frames.copy()).cuda(), ksize, passes).cpu().numpy()
    for i in range(n):
        assert np.array_equal(got[i], want[i]), "frame %d" % i


@pytest.mark.parametrize("w,h,ksize,passes", [(640, 300, 41, 3), (640, 300, 113, 2), (641, 100, 41, 3), (300, 40, 41, 3)])
def test_no_bleed_between_frames(ctx, w, h, ksize, passes):
    """all-0 and all-255 frames alternate, then frames whose top and bottom rows contrast with each other: a batch blurred as one
    tall image mixes the rows of neighbouring frames"""
    torch = _torch()
    n = 6
    frames = np.zeros((n, h, w, 3), np.uint8)
    frames[1::2] = 255
    extra = np.zeros((4, h, w, 3), np.uint8)
    extra[0, : h // 4] = 255          # white top, black bottom
    extra[1, h - h // 4:] = 255       # black top, white bottom
    extra[2, : h // 4] = 255
    extra[3, h - h // 4:] = 255
    frames = np.concatenate([frames, extra])
    want = _oracle(frames, ksize, passes)
    got = ctx.fastboxblur_batch(torch.from_numpy(frames.copy()).cuda(), ksize, passes).cpu().numpy()
    for i in range(len(frames)):
        assert np.array_equal(got[i], want[i]), "frame %d" % i


def test_batch_equals_single_calls_1080p(ctx):
    """16 1080p frames at BASELINE config 5's box (k = 41, three passes), compared on the GPU"""
    torch = _torch()
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randint(0, 256, (16, 1080, 1920, 3), dtype=torch.uint8, device="cuda", generator=g)
    singles = x.clone()
    for i in range(16):
        ctx.fastboxblur(singles[i], 41, 3)
    got = ctx.fastboxblur_batch(x, 41, 3)
    assert torch.equal(got, singles)


def test_batch_over_2gib_in_chunks_with_guards(ctx):
    """88 4K RGB frames (2.19 GB: more than 2^31 bytes, several chunks) between guard bands: equal to single calls, guards untouched"""
    torch = _torch()
    import blur_algorithms_amd as B
    n, h, w = 88, 2160, 3840
    fpc, chunks, _, _ = B.fastboxblur_batch_plan(n, w, h, 3, 41, 3)
    assert chunks > 1 and fpc * chunks >= n
    fb, guard = h * w * 3, 1 << 16
    buf = torch.empty(n * fb + 2 * guard, dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(88)
    buf.random_(0, 256, generator=g)
    head, tail = buf[:guard].clone(), buf[guard + n * fb:].clone()
    x = buf[guard: guard + n * fb].view(n, h, w, 3)
    singles = x.clone()
    for i in range(n):
        ctx.fastboxblur(singles[i], 41, 3)
    ctx.fastboxblur_batch(x, 41, 3)
    assert torch.equal(x, singles)
    assert torch.equal(buf[:guard], head) and torch.equal(buf[guard + n * fb:], tail)
    del buf, x, singles
    torch.cuda.empty_cache()


def test_host_batch_numpy(ctx):
    frames = _frames(np.random.default_rng(3), 5, 120, 256, 3, "uniform")
    want = _oracle(frames, 41, 3)
    got = ctx.fastboxblur_batch(frames, 41, 3)
    assert np.array_equal(got, want)
    gray = _frames(np.random.default_rng(4), 3, 90, 200, 1, "binary")
    assert np.array_equal(ctx.fastboxblur_batch(gray, 9, 2), _oracle(gray, 9, 2))


@pytest.mark.parametrize("n", [0, 1, 2, 5])
def test_multi_dev_and_host(n):
    """two logical shards on one GPU, device and host memory; fewer frames than shards leaves a shard idle"""
    torch = _torch()
    if not torch.cuda.is_available():
        pytest.skip("no GPU in this process")
    import blur_algorithms_amd as B
    frames = _frames(np.random.default_rng(10 + n), n, 110, 320, 3, "uniform")
    want = _oracle(frames, 41, 3) if n else frames
    m = B.BlurMulti([0, 0])
    try:
        got = m.fastboxblur(torch.from_numpy(frames.copy()).cuda(), 41, 3).cpu().numpy()
        assert np.array_equal(got, want)
        assert np.array_equal(m.fastboxblur(frames, 41, 3), want)
    finally:
        m.close()


def test_zero_frames_and_bad_arguments(ctx):
    torch = _torch()
    x = torch.full((2, 64, 200, 3), 77, dtype=torch.uint8, device="cuda")
    lib, h = ctx._lib, ctx._h
    ctx.use_torch_stream()
    assert lib.blur_fastboxblur_u8_batch_dev(h, x.data_ptr(), 0, 200, 64, 3, 41, 3) == 0     # no-op
    assert lib.blur_fastboxblur_u8_batch_dev(h, None, 0, 200, 64, 3, 41, 3) == 0
    assert lib.blur_fastboxblur_u8_host_batch(h, None, 0, 200, 64, 3, 41, 3) == 0
    torch.cuda.synchronize()
    assert bool((x == 77).all())
    assert lib.blur_fastboxblur_u8_batch_dev(h, None, 2, 200, 64, 3, 41, 3) == 1             # BLUR_ERR_INVALID
    assert lib.blur_fastboxblur_u8_host_batch(h, None, 2, 200, 64, 3, 41, 3) == 1
    assert lib.blur_fastboxblur_u8_batch_dev(h, x.data_ptr(), -1, 200, 64, 3, 41, 3) == 1
    assert lib.blur_fastboxblur_u8_batch_dev(h, x.data_ptr(), 2, 0, 64, 3, 41, 3) == 1
    assert lib.blur_fastboxblur_u8_batch_dev(h, x.data_ptr(), 2**31 - 1, 46341, 46341, 4, 41, 3) == 1
    arr = np.zeros(4, np.uint8)
    assert lib.blur_fastboxblur_u8_host_batch(h, arr.ctypes.data_as(C.c_void_p), -2, 2, 2, 1, 3, 1) == 1
    empty = torch.empty((0, 64, 200, 3), dtype=torch.uint8, device="cuda")
    assert ctx.fastboxblur_batch(empty, 41, 3).shape[0] == 0
