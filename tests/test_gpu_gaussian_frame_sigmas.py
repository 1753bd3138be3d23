"""One sigma per frame (blur_gaussian_*_frame_sigmas_*): frame f of the result is the scalar call on that frame alone with sigmas[f],
bit for bit (u8 with three channels, where the scalar call runs other kernels: the float64 plane oracle under assert_u8_parity, and
the same bytes alone, in a batch and in a permuted batch); sigma = 0 copies the frame; one fused launch per window class; the plane
path for one frame among fused ones; pitched views, in place, one source frame under several sigmas; the numpy route."""
import numpy as np
import pytest

import structured as S
from conftest import assert_u8_parity
from test_gpu_gaussian_channels import on_dev, rand_img, sigma_for_class, sigma_for_pad
from test_gpu_gaussian_sigmas import bits, same

pytestmark = pytest.mark.gpu

ROWS, COLS = S.SHAPE                      # 397 x 517: ragged either way, holds every pad up to 168
CLASSES = (3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23)


def scalar(ctx, t):
    return ctx.gaussian if t == "u8" else ctx.gaussian_f32


def per_frame(ctx, t):
    return ctx.gaussian_per_frame if t == "u8" else ctx.gaussian_f32_per_frame


def host_frames(t, seed, shape):
    rng = np.random.default_rng(seed)
    if t == "u8":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    return (rng.standard_normal(shape) * np.exp2(rng.integers(-3, 4, shape))).astype(np.float32)


def scalar_frames(ctx, t, x, sigmas, **kw):
    """what the contract composes: frame f of the scalar call on x[f] alone with sigmas[f]; sigma 0: the source frame"""
    import torch
    want = x.clone()
    for f, s in enumerate(sigmas):
        if s != 0:
            scalar(ctx, t)(x[f].contiguous(), s, out=want[f], **kw)
    torch.cuda.synchronize()
    return want


def pad_of(sigma, rows=ROWS, cols=COLS):
    import blur_algorithms_amd as B
    return B.pffft_sizing(rows, cols, sigma)["pad"]


def mixed_sigmas():
    """class 5 at pad 17 and at pad 18 (one launch, both pad parities: the quirk's sign), 13, a zero, 21, the first again (one table
    slot for two frames), 3, 9"""
    a, b = sigma_for_pad(ROWS, COLS, 17, 17), sigma_for_pad(ROWS, COLS, 18, 18)
    return (a, b, sigma_for_class(ROWS, COLS, 13), 0.0, sigma_for_class(ROWS, COLS, 21), a, sigma_for_class(ROWS, COLS, 3), sigma_for_class(ROWS, COLS, 9))


# ---- 1. bit equality with the scalar call, frame by frame ---------------------------------------------------------------------
# (u8 with three channels is not here: the scalar call runs other kernels; test_u8c3_* check those frames against the oracle)
@pytest.mark.parametrize("engine", [None, "fused", "fft"])
@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("t,ch", [("u8", 1), ("u8", 4), ("f32", 1), ("f32", 3), ("f32", 4)])
def test_bit_equal_to_the_scalar_call(ctx, t, ch, quirk, engine):
    import torch
    from blur_algorithms_amd.api import gaussian_frame_sigmas_plan
    sigmas = mixed_sigmas()
    plan = gaussian_frame_sigmas_plan(ROWS, COLS, sigmas)
    assert [p[1] for p in plan[:2]] == [17, 18] and plan[0][0] == plan[1][0] and plan[0][3] == plan[5][3] != plan[1][3]
    assert [p[2] for p in plan] == [5, 5, 13, 0, 21, 5, 3, 9]
    x = on_dev(host_frames(t, 100 * ch + len(t), (len(sigmas), ROWS, COLS, ch)))
    got = per_frame(ctx, t)(x, sigmas, out=torch.empty_like(x), nyquist_quirk=quirk, engine=engine)
    family = ctx.last_engine()[0]
    want = scalar_frames(ctx, t, x, sigmas, nyquist_quirk=quirk, engine=engine)
    for f in range(len(sigmas)):
        assert same(got[f], want[f]), "frame %d (sigma %g) differs from its scalar call" % (f, sigmas[f])
    assert same(got[3], x[3])                                       # sigma 0: a copy
    if engine == "fused":
        assert family == 6
    if engine == "fft":
        assert family == 0


# ---- 2. every window class in one call ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", ["u8", "f32"])
def test_every_window_class_in_one_call(ctx, t):
    import torch
    sigmas = [sigma_for_class(ROWS, COLS, nkb) for nkb in CLASSES]
    x = on_dev(host_frames(t, 7 + len(t), (len(sigmas), ROWS, COLS, 1)))
    got = per_frame(ctx, t)(x, sigmas, out=torch.empty_like(x), engine="fused")
    assert ctx.last_engine()[0] == 6
    want = scalar_frames(ctx, t, x, sigmas, engine="fused")
    for f, nkb in enumerate(CLASSES):
        assert same(got[f], want[f]), "class %d differs from its scalar call" % nkb


# ---- 3. u8, three channels: fw_blur_u8<NKB, Q, 3> over a frame list ---------------------------------------------------------------
U8C3_CLASSES = (3, 7, 11, 13, 19)


@pytest.fixture(scope="module")
def u8c3_case():
    """frames, sigmas (one per class and a zero) and, per quirk setting, the oracle of every blurred frame: made once"""
    from oracle import oracle as O
    sigmas = [sigma_for_class(ROWS, COLS, nkb) for nkb in U8C3_CLASSES[:3]] + [0.0] + [sigma_for_class(ROWS, COLS, nkb) for nkb in U8C3_CLASSES[3:]]
    frames = np.stack([rand_img(np.random.default_rng(300 + f), ROWS, COLS, 3) for f in range(len(sigmas))])
    want = {}
    for quirk in (True, False):
        for f, s in enumerate(sigmas):
            if s != 0:
                planes = np.stack([O.pffft_plane_f64(frames[f][..., c].astype(np.float32), s, quirk) for c in range(3)])
                want[quirk, f] = (np.moveaxis(S.round_u8(planes), 0, -1), planes)
    return frames, sigmas, want


@pytest.mark.parametrize("quirk", [True, False])
def test_u8c3_meets_the_oracle_and_depends_on_the_frame_alone(ctx, u8c3_case, quirk):
    import torch
    frames, sigmas, want = u8c3_case
    x = on_dev(frames)
    got = ctx.gaussian_per_frame(x, sigmas, out=torch.empty_like(x), nyquist_quirk=quirk)
    assert ctx.last_engine()[0] == 6
    g = got.cpu().numpy()
    for f, s in enumerate(sigmas):
        if s == 0:
            assert np.array_equal(g[f], frames[f]), "the sigma = 0 frame changed"
        else:
            assert_u8_parity(g[f], *want[quirk, f])
    # alone through the same entry, and in a permuted batch: the same bytes
    for f, s in enumerate(sigmas):
        alone = ctx.gaussian_per_frame(x[f:f + 1].contiguous(), [s], out=torch.empty_like(x[f:f + 1]), nyquist_quirk=quirk)
        assert same(alone[0], got[f]), "frame %d alone differs from the frame in the batch" % f
    perm = [4, 0, 5, 2, 3, 1]
    shuffled = ctx.gaussian_per_frame(x[perm].contiguous(), [sigmas[i] for i in perm], out=torch.empty_like(x), nyquist_quirk=quirk)
    for at, f in enumerate(perm):
        assert same(shuffled[at], got[f]), "frame %d differs in a permuted batch" % f
    # all sigmas equal: still not the u8c3 entry's kernels -- the bytes of the frame as blurred above
    s0 = sigmas[0]
    equal = ctx.gaussian_per_frame(x[:2].contiguous(), [s0, s0], out=torch.empty_like(x[:2]), nyquist_quirk=quirk)
    assert same(equal[0], got[0])


# ---- 4. one launch per window class; no table cache growth -----------------------------------------------------------------------
def test_launch_count_and_no_cache_growth(ctx):
    """48 small BGR frames with seeded continuous sigmas: one fused launch per class present, every frame against the oracle, and the
    device memory of the context does not grow with fresh sigmas.  Stated choice for the last point: device free memory across 20
    repeated calls with fresh sigmas (torch.cuda.mem_get_info).  A table cached per sigma is three allocations of at least one 4 KiB
    page each: 20 calls x 48 sigmas would take 11 MiB or more; the bound is 4 MiB."""
    import torch
    from oracle import oracle as O
    from blur_algorithms_amd.api import gaussian_frame_sigmas_plan
    n, rows, cols = 48, 64, 80
    rng = np.random.default_rng(48)
    sigmas = [float(s) for s in rng.uniform(0.8, 3.0, n)]
    plan = gaussian_frame_sigmas_plan(rows, cols, sigmas)
    assert all(p[1] >= 1 for p in plan)
    classes = {p[2] for p in plan}
    assert classes <= {3, 5}
    frames = rng.integers(0, 256, (n, rows, cols, 3), dtype=np.uint8)
    x = on_dev(frames)
    out = torch.empty_like(x)
    ctx.synchronize()
    ctx.timing()
    ctx.timing_enable(2)
    try:
        ctx.gaussian_per_frame(x, sigmas, out=out)
        t = ctx.timing()
    finally:
        ctx.timing_enable(False)
    assert ctx.last_engine()[0] == 6
    assert t["row_launches"] == len(classes) and t["row_frames"] == n
    g = out.cpu().numpy()
    for f, s in enumerate(sigmas):
        planes = np.stack([O.pffft_plane_f64(frames[f][..., c].astype(np.float32), s, True) for c in range(3)])
        assert_u8_parity(g[f], np.moveaxis(S.round_u8(planes), 0, -1), planes)
    # (the workspaces are as large as they get after the call above: the same shapes and as many distinct sigmas below)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(20):
        ctx.gaussian_per_frame(x, [float(s) for s in rng.uniform(0.8, 3.0, n)], out=out)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    print("device free memory before / after 20 calls with fresh sigmas: %d / %d bytes" % (free0, free1))
    assert free0 - free1 < 4 << 20


# ---- 5. the plane path for one frame among fused ones -------------------------------------------------------------------------------
@pytest.mark.parametrize("t", ["u8", "f32"])
def test_plane_path_among_fused_frames(ctx, t):
    import torch
    import blur_algorithms_amd as B
    wide = sigma_for_pad(ROWS, COLS, 175, 200)
    sigmas = [sigma_for_class(ROWS, COLS, 5), sigma_for_class(ROWS, COLS, 9), wide, sigma_for_class(ROWS, COLS, 5)]
    x = on_dev(host_frames(t, 55, (len(sigmas), ROWS, COLS, 1)))
    got = per_frame(ctx, t)(x, sigmas, out=torch.empty_like(x))
    family, note = ctx.last_engine()
    assert family == 0 and "1 frame on the plane path" in note and "frame 2" in note, note
    want = scalar_frames(ctx, t, x, sigmas)
    for f in range(len(sigmas)):
        assert same(got[f], want[f]), "frame %d differs from its scalar call" % f
    sentinel = torch.full_like(x, 77)
    before = sentinel.clone()
    with pytest.raises(B.BlurError):
        per_frame(ctx, t)(x, sigmas, out=sentinel, engine="fused")
    torch.cuda.synchronize()
    assert same(sentinel, before), "a refused call wrote to its destination"


# ---- 6. pitched views ---------------------------------------------------------------------------------------------------------------
def view_of(parent, y, x, rows, cols):
    return parent[:, y:y + rows, x:x + cols, :]


@pytest.mark.parametrize("t,ch", [("u8", 1), ("u8", 3), ("u8", 4), ("f32", 3)])
def test_roi_source_and_padded_destination(ctx, t, ch):
    import torch
    rows, cols, n = 203, 261, 4
    sigmas = [sigma_for_class(rows, cols, 5), 0.0, sigma_for_class(rows, cols, 11), sigma_for_pad(rows, cols, 17, 17)]
    sparent = on_dev(host_frames(t, 61 + ch, (n, rows + 9, cols + 21, ch)))
    src = view_of(sparent, 3, 5, rows, cols)
    dparent = torch.full((n, rows + 6, cols + 13, ch), 93, dtype=sparent.dtype, device="cuda")
    dbefore = dparent.clone()
    dst = view_of(dparent, 2, 7, rows, cols)
    per_frame(ctx, t)(src, sigmas, out=dst, engine="fused")
    assert ctx.last_engine()[0] == 6
    packed = per_frame(ctx, t)(src.contiguous(), sigmas, out=torch.empty((n, rows, cols, ch), dtype=sparent.dtype, device="cuda"), engine="fused")
    assert same(dst, packed)
    mask = torch.ones(dparent.shape, dtype=torch.bool, device="cuda")
    view_of(mask, 2, 7, rows, cols)[:] = False
    assert np.array_equal(bits(dparent[mask]), bits(dbefore[mask])), "a byte outside the destination rectangle was written"
    # in place on a view: the result of the out-of-place call, the parent's other bytes intact
    sbefore = sparent.clone()
    per_frame(ctx, t)(src, sigmas, engine="fused")
    assert same(src, packed)
    smask = torch.ones(sparent.shape, dtype=torch.bool, device="cuda")
    view_of(smask, 3, 5, rows, cols)[:] = False
    assert np.array_equal(bits(sparent[smask]), bits(sbefore[smask]))


@pytest.mark.parametrize("t,ch", [("u8", 1), ("f32", 3)])
def test_scale_space_one_frame_five_sigmas(ctx, t, ch):
    import torch
    sigmas = [sigma_for_class(ROWS, COLS, nkb) for nkb in (3, 5, 5, 9)] + [sigma_for_pad(ROWS, COLS, 18, 18)]
    img = on_dev(host_frames(t, 71 + ch, (1, ROWS, COLS, ch)))
    out = torch.empty((5, ROWS, COLS, ch), dtype=img.dtype, device="cuda")
    got = per_frame(ctx, t)(img.expand(5, -1, -1, -1), sigmas, out=out)
    assert got is out
    for k, s in enumerate(sigmas):
        want = scalar(ctx, t)(img[0], s, out=torch.empty_like(img[0]))
        assert same(out[k], want), "output %d (sigma %g) differs from the scalar call on the frame" % (k, s)
    with pytest.raises(ValueError):
        per_frame(ctx, t)(img.expand(5, -1, -1, -1), sigmas)            # no in-place result exists


@pytest.mark.parametrize("t", ["u8", "f32"])
def test_in_place_batch_and_all_zero(ctx, t):
    import torch
    sigmas = [sigma_for_class(ROWS, COLS, 7), 0.0, sigma_for_class(ROWS, COLS, 3)]
    x = on_dev(host_frames(t, 81, (3, ROWS, COLS, 4)))
    want = per_frame(ctx, t)(x, sigmas, out=torch.empty_like(x))
    y = x.clone()
    assert per_frame(ctx, t)(y, sigmas) is y
    assert same(y, want)
    z = x.clone()
    per_frame(ctx, t)(z, [0.0, 0.0, 0.0])
    assert same(z, x)
    assert same(per_frame(ctx, t)(x, [0.0, 0.0, 0.0], out=torch.empty_like(x)), x)


# ---- 7. the numpy route ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t,ch", [("u8", 3), ("u8", 1), ("f32", 4)])
def test_numpy_frames_loop_over_the_scalar_host_entry(ctx, t, ch):
    rows, cols = 120, 150
    sigmas = [2.0, 0.0, 5.5]
    a = host_frames(t, 91, (3, rows, cols, ch))
    got = per_frame(ctx, t)(a, sigmas)
    assert got.shape == a.shape and got.dtype == a.dtype
    for f, s in enumerate(sigmas):
        want = a[f] if s == 0 else scalar(ctx, t)(a[f], s)
        assert np.array_equal(got[f].view(np.uint8), np.ascontiguousarray(want).view(np.uint8))
