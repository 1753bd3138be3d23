"""A decoded clip with its own sigmas per frame (BlurContext.gaussian_nv12_per_frame -> blur_gaussian_nv12_frame_sigmas_batch_dev,
blur_gaussian_p016_frame_sigmas_batch_dev): the planes of frame f are, bit for bit, what gaussian_nv12 returns for that frame alone
with (sigma_y, sigma_c, sigma_c).  The chroma plane runs on the two-channel kernels over a frame list: fw_blur_u8<NKB, Q, 2, true>
behind fc_prepass_frames<2, G>, and ff_blur<uint16_t, NKB, Q, 2> behind ff_prepass_frames<uint16_t, 2, G>.

Surfaces: luma 396 x 516, chroma 198 x 258.  pffft_sizing caps the window at the plane's longer side, so a 258-pixel chroma row
holds pads to 129 only (test_gpu_gaussian_nv12.py); the clips with chroma classes above NKB 17 are 396 x 676 (chroma 198 x 338),
which holds every pad to 168.

The cases are functions (case_*), as in test_gpu_gaussian_nv12.py, and run_clip_cases runs them in turn, printing the case it is at
(shown with a failure).  This module has no entry of its own in the suite: together with the cases of
test_gpu_gaussian_frame_sigmas_types.py they are ONE entry there (test_per_frame_sigmas_of_16_bit_batches_and_decoded_clips), 78
cases that take under three seconds together."""
import numpy as np
import pytest

import structured as S
from conftest import assert_u8_parity
from test_gpu_gaussian_channels import on_dev, sigma_for_class, sigma_for_pad
from test_gpu_gaussian_nv12 import COLS, KINDS, ROWS, WIDE_COLS, assert_surface, each, host, noise, planes_of, surface

CLASSES = S.NKB_CLASSES


def clip(kind, seed, n, rows, cols):
    return noise(kind, seed, (n, rows, cols)), noise(kind, seed + 1, (n, rows // 2, cols // 2, 2))


def scalar_clip(ctx, y, uv, pairs, **kw):
    """what the contract composes: gaussian_nv12 on frame f alone with (sigma_y, sigma_c, sigma_c) -> host arrays (y, uv)"""
    import torch
    ty, tuv = on_dev(y), on_dev(uv)
    oy, ouv = torch.empty_like(ty), torch.empty_like(tuv)
    for f, (sy, sc) in enumerate(pairs):
        ctx.gaussian_nv12(ty[f], tuv[f], (sy, sc, sc), out=(oy[f], ouv[f]), **kw)
    return host(oy), host(ouv)


def per_frame_clip(ctx, y, uv, pairs, **kw):
    """host planes -> contiguous device tensors -> out of place -> host planes, and (family, note)"""
    import torch
    ty, tuv = on_dev(y), on_dev(uv)
    oy, ouv = torch.empty_like(ty), torch.empty_like(tuv)
    ry, ruv = ctx.gaussian_nv12_per_frame(ty, tuv, pairs, out=(oy, ouv), **kw)
    assert ry is oy and ruv is ouv
    last = ctx.last_engine()
    assert np.array_equal(host(ty), y) and np.array_equal(host(tuv), uv), "the source was written"
    return host(oy), host(ouv), last


def assert_frames(gy, guv, wy, wuv, pairs, tag=""):
    for f, (sy, sc) in enumerate(pairs):
        assert np.array_equal(gy[f], wy[f]), "%s frame %d: luma (sigma %g) differs from the scalar surface call" % (tag, f, sy)
        for c, name in enumerate(("Cb", "Cr")):
            assert np.array_equal(guv[f][..., c], wuv[f][..., c]), "%s frame %d: %s (sigma %g) differs from the scalar surface call" % (tag, f, name, sc)


def mixed_pairs(rows=ROWS, cols=WIDE_COLS):
    """8 frames.  Chroma: class 9 at pad 49 and at pad 50 (one launch, both pad parities), 3, a zero, a zero, 21, pad 49 again (one
    table slot for two frames), 13.  Luma, on its own: 7, a zero, 13, 5, a zero, 7 again, 11, 3.  Frame 1: chroma only; frame 3:
    luma only; frame 4: neither"""
    crows, ccols = rows // 2, cols // 2
    a, b = sigma_for_pad(crows, ccols, 49, 49), sigma_for_pad(crows, ccols, 50, 50)
    chroma = (a, b, sigma_for_class(crows, ccols, 3), 0.0, 0.0, sigma_for_class(crows, ccols, 21), a, sigma_for_class(crows, ccols, 13))
    l7 = sigma_for_class(rows, cols, 7)
    luma = (l7, 0.0, sigma_for_class(rows, cols, 13), sigma_for_class(rows, cols, 5), 0.0, l7, sigma_for_class(rows, cols, 11), sigma_for_class(rows, cols, 3))
    return list(zip(luma, chroma))


# ---- 1. equality with the scalar surface call -----------------------------------------------------------------------------------------
def case_every_plane_of_every_frame_equals_the_scalar_call(ctx, kind, quirk, engine):
    from blur_algorithms_amd.api import gaussian_frame_sigmas_plan
    pairs = mixed_pairs()
    cplan = gaussian_frame_sigmas_plan(ROWS // 2, WIDE_COLS // 2, [c for _, c in pairs])
    assert [p[2] for p in cplan] == [9, 9, 3, 0, 0, 21, 9, 13] and [cplan[0][1], cplan[1][1]] == [49, 50] and cplan[0][3] == cplan[6][3]
    assert [p[2] for p in gaussian_frame_sigmas_plan(ROWS, WIDE_COLS, [l for l, _ in pairs])] == [7, 0, 13, 5, 0, 7, 11, 3]
    y, uv = clip(kind, 21, len(pairs), ROWS, WIDE_COLS)
    gy, guv, (family, note) = per_frame_clip(ctx, y, uv, pairs, nyquist_quirk=quirk, engine=engine)
    wy, wuv = scalar_clip(ctx, y, uv, pairs, nyquist_quirk=quirk, engine=engine)
    assert_frames(gy, guv, wy, wuv, pairs, kind)
    assert np.array_equal(guv[3], uv[3]) and np.array_equal(gy[1], y[1]) and np.array_equal(gy[4], y[4]) and np.array_equal(guv[4], uv[4])
    assert not np.array_equal(guv[0][..., 0], guv[0][..., 1])
    if engine == "fused" or kind == "nv12":
        assert family == 6, note
    else:                                       # p016, the library's choice: chroma class 21 is past pad 104
        assert family == 0 and "chroma" in note and "luma" not in note and "frame 5" in note, note


# ---- 2. every window class on the chroma plane in one call ----------------------------------------------------------------------------
def case_every_window_class_on_the_chroma_plane_in_one_call(ctx, kind):
    crows, ccols = ROWS // 2, WIDE_COLS // 2
    pairs = [(0.0 if f % 2 else 2.0, sigma_for_class(crows, ccols, nkb)) for f, nkb in enumerate(CLASSES)]
    y, uv = clip(kind, 31, len(pairs), ROWS, WIDE_COLS)
    gy, guv, (family, note) = per_frame_clip(ctx, y, uv, pairs, engine="fused")
    assert family == 6, note
    assert_frames(gy, guv, *scalar_clip(ctx, y, uv, pairs, engine="fused"), pairs, kind)
    if kind == "p016":                          # the library's choice: the classes above 15 take the plane path, the same bytes as the scalar call's
        gy, guv, (family, note) = per_frame_clip(ctx, y, uv, pairs)
        assert family == 0 and "4 frames on the plane path" in note and "frame 7" in note, note
        assert_frames(gy, guv, *scalar_clip(ctx, y, uv, pairs), pairs, kind)


# ---- 3. a pitched decoder surface with padding rows -------------------------------------------------------------------------------------
def case_a_pitched_clip_in_place_and_out_of_place(ctx, kind, cols):
    """cols = 514: chroma rows of 257 pairs = 514 bytes (NV12), no multiple of 4; odd NV12 pitches; three rows of padding behind
    every surface"""
    n, rows = 4, ROWS
    spitch, dpitch = cols + 13, cols + 31
    crows, ccols = rows // 2, cols // 2
    pairs = [(sigma_for_pad(rows, cols, 37, 37), sigma_for_pad(crows, ccols, 6, 6)), (0.0, sigma_for_pad(crows, ccols, 66, 66)),
             (sigma_for_class(rows, cols, 9), 0.0), (sigma_for_pad(rows, cols, 38, 38), sigma_for_pad(crows, ccols, 7, 7))]
    src = surface(kind, rows, cols, spitch, 41, n=n)
    y, uv = planes_of(src, rows, cols)
    wy, wuv = scalar_clip(ctx, np.ascontiguousarray(y), np.ascontiguousarray(uv), pairs, engine="fused")
    ts = on_dev(src)
    dst = surface(kind, rows, cols, dpitch, 42, n=n)
    td = on_dev(dst)
    ctx.gaussian_nv12_per_frame(*planes_of(ts, rows, cols), pairs, out=planes_of(td, rows, cols), engine="fused")
    assert ctx.last_engine()[0] == 6
    assert np.array_equal(host(ts), src), "the source clip was written"
    assert_surface(host(td), dst, rows, cols, wy, wuv, "out of place")
    ty, tuv = planes_of(ts, rows, cols)
    assert not ty.is_contiguous() and not tuv.is_contiguous()
    ry, ruv = ctx.gaussian_nv12_per_frame(ty, tuv, pairs, engine="fused")
    assert ry is ty and ruv is tuv and ctx.last_engine()[0] == 6
    assert_surface(host(ts), src, rows, cols, wy, wuv, "in place")


# ---- 4. a frame's planes depend on the frame and its sigmas alone ------------------------------------------------------------------------
def case_alone_in_the_batch_and_in_a_permuted_batch(ctx, kind):
    pairs = mixed_pairs()
    y, uv = clip(kind, 21, len(pairs), ROWS, WIDE_COLS)
    gy, guv, _ = per_frame_clip(ctx, y, uv, pairs, engine="fused")
    for f in (0, 5, 6):
        ay, auv, _ = per_frame_clip(ctx, y[f:f + 1], uv[f:f + 1], pairs[f:f + 1], engine="fused")
        assert np.array_equal(ay[0], gy[f]) and np.array_equal(auv[0], guv[f]), "frame %d alone differs from the frame in the batch" % f
    perm = [6, 2, 7, 0, 4, 5, 1, 3]
    py, puv, _ = per_frame_clip(ctx, y[perm], uv[perm], [pairs[i] for i in perm], engine="fused")
    for at, f in enumerate(perm):
        assert np.array_equal(py[at], gy[f]) and np.array_equal(puv[at], guv[f]), "frame %d differs in a permuted batch" % f


# ---- 5. the plane path for one plane among fused ones -----------------------------------------------------------------------------------
def case_plane_path_among_fused_frames(ctx, kind):
    import torch
    import blur_algorithms_amd as B
    crows, ccols = ROWS // 2, WIDE_COLS // 2
    wide = sigma_for_pad(ROWS, WIDE_COLS, 175, 200)
    pairs = [(sigma_for_class(ROWS, WIDE_COLS, 5), sigma_for_class(crows, ccols, 7)), (wide, sigma_for_class(crows, ccols, 3)),
             (sigma_for_class(ROWS, WIDE_COLS, 9), sigma_for_class(crows, ccols, 7))]
    y, uv = clip(kind, 51, len(pairs), ROWS, WIDE_COLS)
    gy, guv, (family, note) = per_frame_clip(ctx, y, uv, pairs)
    assert family == 0 and "luma" in note and "chroma" not in note and "1 frame on the plane path" in note and "frame 1" in note, note
    assert_frames(gy, guv, *scalar_clip(ctx, y, uv, pairs), pairs, kind)
    ty, tuv = on_dev(y), on_dev(uv)
    oy, ouv = on_dev(noise(kind, 52, y.shape)), on_dev(noise(kind, 53, uv.shape))
    by, buv = host(oy).copy(), host(ouv).copy()
    with pytest.raises(B.BlurError) as e:
        ctx.gaussian_nv12_per_frame(ty, tuv, pairs, out=(oy, ouv), engine="fused")
    assert e.value.code == 2
    # a chroma plane without a fused kernel behind fused luma planes: refused before the luma part runs
    cwide = sigma_for_pad(ROWS // 2, 352, 170, 178)
    y2, uv2 = clip(kind, 54, 2, ROWS, 704)
    ty2, tuv2 = on_dev(y2), on_dev(uv2)
    with pytest.raises(B.BlurError) as e:
        ctx.gaussian_nv12_per_frame(ty2, tuv2, [(3.0, 2.0), (3.0, cwide)], engine="fused")
    assert e.value.code == 2
    torch.cuda.synchronize()
    assert np.array_equal(host(oy), by) and np.array_equal(host(ouv), buv), "a refused call wrote to its destination"
    assert np.array_equal(host(ty2), y2) and np.array_equal(host(tuv2), uv2), "a refused in-place call wrote"


# ---- 6. the float64 oracle ------------------------------------------------------------------------------------------------------------------
def case_chroma_of_two_frames_meets_the_oracle(ctx):
    """Cb and Cr of frames 1 (pad 50, chroma only) and 7 (class 13) of the NV12 clip of case 1, under the u8 parity rule"""
    from oracle import oracle as O
    pairs = mixed_pairs()
    y, uv = clip("nv12", 21, len(pairs), ROWS, WIDE_COLS)
    _, guv, (family, _) = per_frame_clip(ctx, y, uv, pairs)
    assert family == 6
    for f in (1, 7):
        planes = np.stack([O.pffft_plane_f64(uv[f][..., c].astype(np.float32), pairs[f][1], True) for c in range(2)])
        assert_u8_parity(guv[f], np.moveaxis(S.round_u8(planes), 0, -1), planes)


# ---- the cases in turn (the one entry is test_gpu_gaussian_frame_sigmas_types.py's) -----------------------------------------------------
def run_clip_cases(ctx):
    """1. .. 6. above: both kinds, quirk on and off, engine None and fused"""
    each(case_every_plane_of_every_frame_equals_the_scalar_call, ctx, kind=KINDS, quirk=(True, False), engine=(None, "fused"))
    each(case_every_window_class_on_the_chroma_plane_in_one_call, ctx, kind=KINDS)
    each(case_a_pitched_clip_in_place_and_out_of_place, ctx, kind=KINDS, cols=(COLS, 514))
    each(case_alone_in_the_batch_and_in_a_permuted_batch, ctx, kind=KINDS)
    each(case_plane_path_among_fused_frames, ctx, kind=KINDS)
    each(case_chroma_of_two_frames_meets_the_oracle, ctx)
