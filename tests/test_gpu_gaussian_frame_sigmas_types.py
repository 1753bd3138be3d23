"""One sigma per frame for uint16, float16 and bfloat16 frames (blur_gaussian_{u16,f16,bf16}_frame_sigmas_*): frame f of the result
is the scalar call of the type on that frame alone with sigmas[f], bit for bit; a half-precision frame's power-of-two scale comes
from its own max|x|; every window class in one call; pitched views, in place, one source frame under several sigmas; and one u16
and one f16 frame of a mixed batch against the float64 oracle under the types' own parity rules, so that the suite does not only
compare the library with itself.

The cases are functions (case_*), as in test_gpu_gaussian_nv12.py, and ONE test runs them in turn, and after them the cases of
test_gpu_gaussian_nv12_frame_sigmas.py (the decoded clips with their own sigmas per frame), printing the case it is at (shown with a
failure): 78 cases that take under three seconds together are one entry in every later run of the suite, not 78."""
import numpy as np
import pytest

import half_parity as H
import structured as S
import u16_parity as U
from test_gpu_gaussian_channels import sigma_for_class, sigma_for_pad
from test_gpu_gaussian_frame_sigmas import CLASSES, mixed_sigmas, view_of
from test_gpu_gaussian_half import on_dev as half_on_dev
from test_gpu_gaussian_nv12 import each
from test_gpu_gaussian_nv12_frame_sigmas import run_clip_cases
from test_gpu_gaussian_sigmas import bits, same

pytestmark = pytest.mark.gpu

ROWS, COLS = S.SHAPE                      # 397 x 517
TYPES = ("u16", "f16", "bf16")
BIG, SMALL = 2.0 ** 6, 2.0 ** -6


def scalar(ctx, t):
    return getattr(ctx, "gaussian_%s" % t)


def per_frame(ctx, t):
    return getattr(ctx, "gaussian_%s_per_frame" % t)


def rotated_sigmas():
    """mixed_sigmas() turned by two frames: classes 13, -, 21, 5, 3, 9, 5, 5 -- the frames of class 5 (pads 17, 17, 18: both pad
    parities and a repeated sigma) are frames 3, 6 and 7 of the batch and positions 0, 1 and 2 of their launch's list"""
    m = mixed_sigmas()
    return m[2:] + m[:2]


def magnitudes(sigmas, rows=ROWS, cols=COLS):
    """2^6 and 2^-6 in turn along every class's frame list (the neighbours of one launch differ by 2^12), the first frame of a class
    large for an even class index and small for an odd one.  A scale taken from the frame's index in the batch instead of its
    position in the list belongs to another frame: 2^12 too large a factor overflows binary16, 2^12 too small loses 12 bits"""
    from blur_algorithms_amd.api import gaussian_frame_sigmas_plan
    seen, mags = {}, []
    for group, _, _, _ in gaussian_frame_sigmas_plan(rows, cols, sigmas):
        k = seen.get(group, 0)
        seen[group] = k + 1
        mags.append(BIG if (k + max(group, 0)) % 2 == 0 else SMALL)
    return mags


def frames_of(t, seed, n, ch, mags=None, rows=ROWS, cols=COLS):
    """n frames [rows, cols, ch] of noise on the device: u16 over the full range; the half types non-negative in [0, mags[f]]"""
    if t == "u16":
        import torch
        return torch.from_numpy(np.random.default_rng(seed).integers(0, 65536, (n, rows, cols, ch), dtype=np.uint16)).cuda()
    mags = mags or [1.0] * n
    a = np.stack([np.stack([H.noise(t, seed + 100 * f + c, rows, cols, mags[f]) for c in range(ch)], axis=-1) for f in range(n)])
    return half_on_dev(t, a)


def scalar_frames(ctx, t, x, sigmas, **kw):
    """what the contract composes: the scalar call on x[f] alone with sigmas[f]; sigma 0: the source frame"""
    import torch
    want = x.clone()
    for f, s in enumerate(sigmas):
        if s != 0:
            scalar(ctx, t)(x[f].contiguous(), s, out=want[f], **kw)
    torch.cuda.synchronize()
    return want


# ---- 1. bit equality with the scalar call, frame by frame ---------------------------------------------------------------------------
def case_bit_equal_to_the_scalar_call(ctx, t, ch, quirk, engine):
    import torch
    from blur_algorithms_amd.api import gaussian_frame_sigmas_plan
    sigmas = rotated_sigmas()
    plan = gaussian_frame_sigmas_plan(ROWS, COLS, sigmas)
    assert [p[2] for p in plan] == [13, 0, 21, 5, 3, 9, 5, 5]
    assert [p[1] for p in plan[6:]] == [17, 18] and plan[3][3] == plan[6][3] != plan[7][3]
    mags = magnitudes(sigmas)
    five = [f for f, p in enumerate(plan) if p[2] == 5]
    assert five == [3, 6, 7] and [mags[f] for f in five] in ([BIG, SMALL, BIG], [SMALL, BIG, SMALL])      # not a prefix; neighbours 2^12 apart
    x = frames_of(t, 1000 * ch + len(t), len(sigmas), ch, mags)
    got = per_frame(ctx, t)(x, sigmas, out=torch.empty_like(x), nyquist_quirk=quirk, engine=engine)
    family = ctx.last_engine()[0]
    want = scalar_frames(ctx, t, x, sigmas, nyquist_quirk=quirk, engine=engine)
    for f in range(len(sigmas)):
        assert same(got[f], want[f]), "frame %d (sigma %g) differs from its scalar call" % (f, sigmas[f])
    assert same(got[1], x[1])                                       # sigma 0: a copy
    if t != "u16":
        assert np.isfinite(got.float().cpu().numpy()).all()
    if engine == "fused":
        assert family == 6
    if engine == "fft":
        assert family == 0


# ---- 2. every window class in one call ----------------------------------------------------------------------------------------------
def case_every_window_class_in_one_call(ctx, t):
    import torch
    sigmas = [sigma_for_class(ROWS, COLS, nkb) for nkb in CLASSES]
    x = frames_of(t, 7 + len(t), len(sigmas), 1, [BIG, SMALL] * 5 + [BIG])
    got = per_frame(ctx, t)(x, sigmas, out=torch.empty_like(x), engine="fused")
    assert ctx.last_engine()[0] == 6
    want = scalar_frames(ctx, t, x, sigmas, engine="fused")
    for f, nkb in enumerate(CLASSES):
        assert same(got[f], want[f]), "class %d differs from its scalar call" % nkb


# ---- 3. views, in place, one source frame under several sigmas (bf16) ------------------------------------------------------------------
def case_bf16_roi_view_in_place_and_scale_space(ctx):
    import torch
    t, ch = "bf16", 3
    rows, cols, n = 203, 261, 4
    sigmas = [sigma_for_class(rows, cols, 5), 0.0, sigma_for_class(rows, cols, 11), sigma_for_pad(rows, cols, 17, 17)]
    sparent = frames_of(t, 61, n, ch, [BIG, SMALL, SMALL, BIG], rows + 9, cols + 21)
    src = view_of(sparent, 3, 5, rows, cols)
    dparent = frames_of(t, 62, n, ch, None, rows + 6, cols + 13)
    dbefore = dparent.clone()
    dst = view_of(dparent, 2, 7, rows, cols)
    per_frame(ctx, t)(src, sigmas, out=dst, engine="fused")
    assert ctx.last_engine()[0] == 6
    want = scalar_frames(ctx, t, src.contiguous(), sigmas, engine="fused")
    assert same(dst, want)
    mask = torch.ones(dparent.shape, dtype=torch.bool, device="cuda")
    view_of(mask, 2, 7, rows, cols)[:] = False
    assert np.array_equal(bits(dparent[mask]), bits(dbefore[mask])), "a byte outside the destination rectangle was written"
    # in place on the view: the same result, the parent's other bytes intact
    sbefore = sparent.clone()
    assert per_frame(ctx, t)(src, sigmas, engine="fused") is src
    assert same(src, want)
    smask = torch.ones(sparent.shape, dtype=torch.bool, device="cuda")
    view_of(smask, 3, 5, rows, cols)[:] = False
    assert np.array_equal(bits(sparent[smask]), bits(sbefore[smask]))
    # one frame, four sigmas, four results (source frame stride 0)
    img = frames_of(t, 63, 1, ch, [BIG], rows, cols)
    out = torch.empty((n, rows, cols, ch), dtype=img.dtype, device="cuda")
    assert per_frame(ctx, t)(img.expand(n, -1, -1, -1), sigmas, out=out) is out
    for k, s in enumerate(sigmas):
        w = img[0] if s == 0 else scalar(ctx, t)(img[0], s, out=torch.empty_like(img[0]))
        assert same(out[k], w), "output %d (sigma %g) differs from the scalar call on the frame" % (k, s)
    with pytest.raises(ValueError):
        per_frame(ctx, t)(img.expand(n, -1, -1, -1), sigmas)            # no in-place result exists


# ---- 4. the float64 oracle ------------------------------------------------------------------------------------------------------------
def case_one_u16_and_one_f16_frame_meet_the_oracle(ctx):
    """the library's own choice (classes up to 15 run fused); the frames checked: class 13 of the u16 batch (frame 0), class 5 at pad
    18 of the f16 batch (frame 7, position 2 of its list, magnitude from magnitudes())"""
    import torch
    sigmas = rotated_sigmas()
    x = frames_of("u16", 41, len(sigmas), 1)
    got = per_frame(ctx, "u16")(x, sigmas, out=torch.empty_like(x))
    f = 0
    plane = x[f, ..., 0].cpu().numpy()
    U.assert_u16_parity(got[f, ..., 0].cpu().numpy(), S.oracle_plane(plane.astype(np.float32), sigmas[f], True))
    mags = magnitudes(sigmas)
    h = frames_of("f16", 42, len(sigmas), 1, mags)
    goth = per_frame(ctx, "f16")(h, sigmas, out=torch.empty_like(h))
    f = 7
    plane = h[f, ..., 0].float().cpu().numpy()
    assert 0.9 * mags[f] < float(np.abs(plane).max()) <= mags[f]
    H.assert_half_parity("f16", goth[f, ..., 0].float().cpu().numpy(), H.oracle_plane(plane, sigmas[f], True), float(np.abs(plane).max()))


# ---- the test: every case in turn ---------------------------------------------------------------------------------------------------------
def test_per_frame_sigmas_of_16_bit_batches_and_decoded_clips(ctx):
    """1. .. 4. above (u16, f16, bf16; 1, 3 and 4 channels; quirk on and off; engine None, fused and fft), then the NV12 / P016 clips"""
    each(case_bit_equal_to_the_scalar_call, ctx, t=TYPES, ch=(1, 3, 4), quirk=(True, False), engine=(None, "fused", "fft"))
    each(case_every_window_class_in_one_call, ctx, t=TYPES)
    each(case_bf16_roi_view_in_place_and_scale_space, ctx)
    each(case_one_u16_and_one_f16_frame_meet_the_oracle, ctx)
    run_clip_cases(ctx)
