"""fastboxblur batches: the host-only plan (blur_fastboxblur_batch_plan) against the chunking and decline rules that
include/blur_amd.h documents.  No GPU: the plan is host code."""
import itertools

import pytest

from blur_algorithms_amd import BlurError, fastboxblur_batch_plan

CAP = 128 << 20                  # the chunk cap (bytes), blur_amd.h
LIMIT32 = 1 << 31                # the kernels' 32-bit offsets: a chunk's bytes stay below this
MAX_ROWS = 65535 * 8             # rows of a chunk (the margin kernel's grid)


def vert_rule(h, pitch, r, passes):
    """bx_vertical's declines, per frame"""
    if passes <= 0 or r <= 0 or r > 56 or pitch % 4:
        return False
    delta = 24 if r <= 24 else 56
    return h >= min(passes, 3) * delta + 32 and h * pitch < LIMIT32


def horz_rule(rows, w, C, r, passes):
    """bx_horizontal's declines on the rows of a chunk: the channel-plane kernel (three channels) or the interleaved one"""
    pitch = w * C
    if passes <= 0 or r <= 0 or pitch < 128 or pitch * rows >= LIMIT32:
        return False
    if C == 3 and r <= 56:
        return True
    return C in (1, 3, 4) and C * r <= 120 and pitch % 4 == 0


WIDTHS = {1: (20, 130, 131, 640), 3: (40, 640, 641, 1920), 4: (30, 64, 641)}
KSIZES = (1, 3, 41, 49, 51, 113, 115, 121)
HEIGHTS = (20, 90, 300, 1080)


def cases():
    for C, ws in WIDTHS.items():
        for w, k, h, p, n in itertools.product(ws, KSIZES, HEIGHTS, (1, 2, 3, 4, 5), (0, 1, 2, 7, 1000)):
            yield n, w, h, C, k, p
    # frames at and beyond the cap and the 32-bit limit
    for n in (0, 1, 2, 7, 1000):
        yield n, 3840, 2160, 3, 41, 3
        yield n, 7680, 4320, 3, 41, 3
        yield n, 8000, 6000, 3, 41, 3        # one frame above the cap
        yield n, 30000, 30000, 3, 41, 3      # one frame above 2^31 bytes
        yield n, 131, 4, 1, 3, 1             # tiny frames: many per chunk, the row limit


def check(n, w, h, C, k, p):
    fpc, chunks, vmx, hmx = fastboxblur_batch_plan(n, w, h, C, k, p)
    fb = w * h * C
    assert fpc >= 1
    # every frame in exactly one chunk: chunks of fpc frames, the last one possibly shorter, none empty
    assert chunks == -(-n // fpc)
    if n:
        assert (chunks - 1) * fpc < n <= chunks * fpc
        assert fpc <= n
    # limits: a chunk of several frames stays under the cap, 2^31 bytes and the row limit; a larger frame is a chunk of its own
    if fpc > 1:
        assert fpc * fb <= CAP and fpc * fb < LIMIT32 and fpc * h <= MAX_ROWS
    # as large as possible
    best = max(1, min(CAP // fb, (LIMIT32 - 1) // fb, MAX_ROWS // h, max(n, 1)))
    assert fpc == best
    if fb <= CAP and n:
        assert fpc * fb <= CAP
    # matrix-core flags: the documented decline rules
    r = (k - 1) // 2
    assert vmx == int(vert_rule(h, w * C, min(r, h - 1), p))
    assert hmx == int(horz_rule(fpc * h, w, C, min(r, w - 1), min(p, 3)))


def test_plan_grid():
    count = 0
    for case in cases():
        check(*case)
        count += 1
    assert count > 4000


def test_plan_examples():
    # 16 1080p RGB frames: one chunk, both directions on the matrix cores
    assert fastboxblur_batch_plan(16, 1920, 1080, 3, 41, 3) == (16, 1, 1, 1)
    # 88 4K RGB frames (over 2^31 bytes in all): chunks of 5 frames (5 x 24.9 MB <= 128 MiB)
    assert fastboxblur_batch_plan(88, 3840, 2160, 3, 41, 3) == (5, 18, 1, 1)
    # 8K RGB frames are larger than the cap: one per chunk, as a single call
    assert fastboxblur_batch_plan(3, 7680, 4320, 3, 41, 3) == (1, 3, 1, 1)
    # a box wider than the windows and a pitch that is no multiple of 4: the accumulator kernels
    assert fastboxblur_batch_plan(2, 640, 300, 3, 121, 3)[2:] == (0, 0)
    assert fastboxblur_batch_plan(2, 641, 300, 3, 41, 3)[2] == 0
    # no frames: no chunks
    assert fastboxblur_batch_plan(0, 640, 300, 3, 41, 3)[1] == 0


@pytest.mark.parametrize("args", [
    (-1, 64, 64, 3, 3, 1),                       # negative frame count
    (1, 0, 64, 3, 3, 1), (1, 64, 0, 3, 3, 1), (1, 64, 64, 0, 3, 1),   # non-positive sizes
    (1, -64, 64, 3, 3, 1), (1, 64, -64, 3, 3, 1),
    (1, 64, 64, 3, 0, 1), (1, 64, 64, 3, 3, -1),  # ksize, passes
    (1, 1 << 30, 1, 3, 3, 1),                    # w * channels above INT_MAX
    (2**31 - 1, 46341, 46341, 4, 3, 1),          # nframes * w * h * channels overflows
])
def test_plan_refuses_bad_arguments(args):
    with pytest.raises(BlurError) as e:
        fastboxblur_batch_plan(*args)
    assert e.value.code == 1                     # BLUR_ERR_INVALID
