"""Gaussian blur of pitched frames and regions of interest (blur_gaussian_*_pitched_batch_dev through BlurContext.gaussian*): a view
of a larger tensor as source, another view with another pitch as destination, nothing repacked.  The rectangle must hold, bit for
bit, what the packed call returns for the view's packed copy (same kernels, same arithmetic, same partition of every sum), and no
byte of the destination's parent outside the rectangle may change.  Three-channel u8 with one sigma is the exception: packed it
runs on fx_blur_u8, pitched on fw_blur_u8<NKB, Q, 3>, so it is checked against the float64 oracle under the u8 parity contract."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_gaussian_channels import check as check_u8_oracle, sigma_for_class, sigma_for_pad

pytestmark = pytest.mark.gpu

KINDS = ("u8", "u16", "f32", "f16", "bf16")
ROWS, COLS = 397, 517          # the class sweeps' frame: ragged width, ragged last tile row, left strip, interior chunks, right strips
SENTINEL = 0xA5


def tdtype(kind):
    import torch
    return {"u8": torch.uint8, "u16": torch.uint16, "f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[kind]


def method(ctx, kind):
    return {"u8": ctx.gaussian, "u16": ctx.gaussian_u16, "f32": ctx.gaussian_f32, "f16": ctx.gaussian_f16, "bf16": ctx.gaussian_bf16}[kind]


def rand_parent(kind, shape, seed):
    """a random contiguous CUDA tensor of the kind's dtype (the half types: values a float16 holds without overflow when blurred)"""
    import torch
    rng = np.random.default_rng(seed)
    if kind == "u8":
        return torch.from_numpy(rng.integers(0, 256, shape, dtype=np.uint8)).cuda()
    if kind == "u16":
        return torch.from_numpy(rng.integers(0, 65536, shape, dtype=np.uint16)).cuda()
    a = torch.from_numpy(rng.normal(20.0, 60.0, shape).astype(np.float32)).cuda()
    return a if kind == "f32" else a.to(tdtype(kind))


def sentinel_parent(kind, shape):
    import torch
    t = torch.empty(shape, dtype=tdtype(kind), device="cuda")
    t.view(torch.uint8).fill_(SENTINEL)
    return t


def packed_copy(t):
    """a packed copy of a view (uint16 is copied as int16: the same bits, and a dtype every copy kernel knows)"""
    import torch
    return t.view(torch.int16).contiguous().view(torch.uint16) if t.dtype == torch.uint16 else t.contiguous()


def raw(t):
    """the bytes of a tensor (a view: of its packed copy) as a numpy array [..., bytes of the last dimension]"""
    import torch
    return packed_copy(t).view(torch.uint8).cpu().numpy()


def roi(parent, y, x, rows, cols):
    """rows x cols pixels at (y, x) of [R, W, C], [R, W] or [n, R, W, C]"""
    return parent[..., y:y + rows, x:x + cols, :] if parent.dim() >= 3 else parent[y:y + rows, x:x + cols]


def packed_call(ctx, kind, view, sigma, **kw):
    """today's route: the view's packed copy through the packed entry, into a fresh packed tensor"""
    import torch
    src = packed_copy(view)
    assert src.is_contiguous()
    got = method(ctx, kind)(src, sigma, out=torch.empty_like(src), **kw)
    return got, ctx.last_engine()[0]


def assert_outside_untouched(before, after, y, x, rows, cols):
    """before, after: raw() of the destination's parent [..., R, W, bytes]; everything outside the rectangle is unchanged"""
    b, a = before.copy(), after.copy()
    b[..., y:y + rows, x:x + cols, :] = 0
    a[..., y:y + rows, x:x + cols, :] = 0
    assert np.array_equal(a, b), "bytes outside the destination rectangle were written"


def pitched_case(ctx, kind, ch, rows, cols, sigma, sy=3, sx=5, dy=2, dx=7, spad=16, dpad=29, engine="fused", family=6, quirk=True, seed=1, two_d=False):
    """source: the view at (sy, sx) of a random parent cols + spad wide; destination: the view at (dy, dx) of a sentinel-filled parent
    cols + dpad wide (another pitch).  Checks the family, the rectangle against the packed call and the sentinel around it."""
    tail = () if two_d else (ch,)
    sparent = rand_parent(kind, (rows + sy + 4, cols + spad) + tail, seed)
    dparent = sentinel_parent(kind, (rows + dy + 3, cols + dpad) + tail)
    if two_d:
        sparent3, dparent3 = sparent.unsqueeze(-1), dparent.unsqueeze(-1)
    else:
        sparent3, dparent3 = sparent, dparent
    sv, dv = roi(sparent, sy, sx, rows, cols), roi(dparent, dy, dx, rows, cols)
    assert not sv.is_contiguous() and not dv.is_contiguous() and sv.stride(0) != dv.stride(0)
    src_before, before = raw(sparent3), raw(dparent3)
    kw = dict(nyquist_quirk=quirk, engine=engine)
    got = method(ctx, kind)(sv, sigma, out=dv, **kw)
    fam = ctx.last_engine()[0]
    assert got.data_ptr() == dv.data_ptr()
    if family is not None:
        assert fam == family
    after = raw(dparent3)
    assert np.array_equal(raw(sparent3), src_before), "the source's parent was written"
    assert_outside_untouched(before, after, dy, dx, rows, cols)
    if kind == "u8" and ch == 3:
        check_u8_oracle(raw(dv).reshape(rows, cols, 3), raw(sv).reshape(rows, cols, 3), sigma, quirk)
    else:
        want, wfam = packed_call(ctx, kind, sv, sigma, **kw)
        assert wfam == fam
        assert np.array_equal(raw(dv), raw(want)), "the pitched call's rectangle differs from the packed call's result"
    return sv, dv


# ---- 1. every type x channel count x window class x quirk ----------------------------------------------------------------
@pytest.mark.parametrize("quirk", [True, False], ids=["quirk", "noquirk"])
@pytest.mark.parametrize("nkb", [3, 11, 13, 21])
@pytest.mark.parametrize("ch", [1, 3, 4])
@pytest.mark.parametrize("kind", KINDS)
def test_window_classes(ctx, kind, ch, nkb, quirk):
    pitched_case(ctx, kind, ch, ROWS, COLS, sigma_for_class(ROWS, COLS, nkb), quirk=quirk, seed=100 * nkb + ch)


@pytest.mark.parametrize("quirk", [True, False], ids=["quirk", "noquirk"])
@pytest.mark.parametrize("kind", KINDS)
def test_widest_class_one_channel(ctx, kind, quirk):
    pitched_case(ctx, kind, 1, ROWS, COLS, sigma_for_class(ROWS, COLS, 23), quirk=quirk, seed=23)


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_f32_auto_takes_the_plane_path_pitched(ctx, ch):
    """NKB 17 is outside the library's own choice for float frames: AUTO runs the plane path (family 0), on the views as they are"""
    pitched_case(ctx, "f32", ch, ROWS, COLS, sigma_for_class(ROWS, COLS, 17), engine=None, family=0, seed=17 + ch)


# ---- 2. every byte alignment of a row's start ------------------------------------------------------------------------------
@pytest.mark.parametrize("sx", [1, 2, 3])
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_row_alignments(ctx, kind, sx):
    """one channel; the u8 parents are 523 and 531 bytes wide, so the rows of both views start at every alignment mod 4"""
    pitched_case(ctx, kind, 1, ROWS, COLS, 20.0, sx=sx, dx=sx + 1, spad=523 - COLS, dpad=531 - COLS, seed=sx)
    pitched_case(ctx, kind, 1, ROWS, COLS, 20.0, sx=sx, dx=sx + 2, spad=523 - COLS, dpad=531 - COLS, seed=sx, two_d=True)


# ---- 3. edge geometry ----------------------------------------------------------------------------------------------------------
EDGE_SHAPES = [(260, 128 * 3 + 73, 20.0), (300, 256 + 1, 12.0), (35, 9, 1.0), (2500, 140, 20.0)]        # from test_gpu_gaussian_channels.SHAPES


@pytest.mark.parametrize("ch", [1, 4])
@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=["%dx%d-s%g" % s for s in EDGE_SHAPES])
def test_edge_shapes(ctx, shape, kind, ch):
    rows, cols, sigma = shape
    pitched_case(ctx, kind, ch, rows, cols, sigma, engine=None, family=None, seed=rows + cols)


# ---- 4. a batch of views: the frames lie a whole parent frame apart ----------------------------------------------------------
@pytest.mark.parametrize("kind,ch", [("u8", 4), ("u8", 1), ("u16", 1), ("f32", 3), ("bf16", 4)])
def test_batch_of_views(ctx, kind, ch):
    rows, cols, sigma, n = 150, 261, 6.0, 3
    sparent = rand_parent(kind, (n, rows + 9, cols + 20, ch), 5)
    dparent = sentinel_parent(kind, (n, rows + 6, cols + 33, ch))
    sv, dv = sparent[:, 3:3 + rows, 5:5 + cols], dparent[:, 2:2 + rows, 7:7 + cols]
    assert sv.stride(0) != rows * sv.stride(1)
    before = raw(dparent)
    method(ctx, kind)(sv, sigma, out=dv, engine="fused")
    assert ctx.last_engine()[0] == 6
    assert_outside_untouched(before, raw(dparent), 2, 7, rows, cols)
    for f in range(n):
        want, _ = packed_call(ctx, kind, sv[f], sigma, engine="fused")
        assert np.array_equal(raw(dv[f]), raw(want)), "frame %d of the batch of views" % f


# ---- 5. in place on a view -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [False, True], ids=["frame", "batch"])
@pytest.mark.parametrize("kind,ch", [("u8", 1), ("u8", 3), ("u8", 4), ("u16", 3), ("f32", 3), ("f16", 1)])
def test_in_place_on_a_view(ctx, kind, ch, batch):
    import torch
    rows, cols, sigma = 150, 261, 6.0
    parent = rand_parent(kind, ((2,) if batch else ()) + (rows + 9, cols + 20, ch), 6)
    before = raw(parent)
    view = roi(parent, 3, 5, rows, cols)
    src = packed_copy(view)
    want = method(ctx, kind)(view, sigma, out=torch.empty_like(src), engine="fused")            # out of place, from the view
    got = method(ctx, kind)(view, sigma, engine="fused")                                         # out=None: the view itself
    assert ctx.last_engine()[0] == 6
    assert got.data_ptr() == view.data_ptr() and got.stride() == view.stride()
    assert np.array_equal(raw(view), raw(want))
    assert not np.array_equal(raw(view), raw(src))
    assert_outside_untouched(before, raw(parent), 3, 5, rows, cols)


# ---- 6. two rectangles of one parent -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,ch", [("u8", 4), ("u8", 3), ("u16", 1), ("f32", 3)])
def test_left_half_into_right_half(ctx, kind, ch):
    """the spans of the two halves interleave row by row: the source is read whole (from a gathered copy) before the first write"""
    rows, cols, sigma = 150, 261, 6.0
    parent = rand_parent(kind, (rows, 2 * cols, ch), 8)
    left, right = parent[:, :cols], parent[:, cols:]
    left_before = raw(left)
    want, _ = packed_call(ctx, kind, left, sigma, engine="fused")
    method(ctx, kind)(left, sigma, out=right, engine="fused")
    assert ctx.last_engine()[0] == 6
    assert np.array_equal(raw(left), left_before), "the left half changed"
    if kind == "u8" and ch == 3:
        check_u8_oracle(raw(right), left_before, sigma)
    else:
        assert np.array_equal(raw(right), raw(want))


# ---- 7. the plane fallback, pitched ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 4])
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_plane_fallback_wide_pad(ctx, kind, ch):
    import blur_algorithms_amd as B
    rows, cols = 420, 390
    sigma = sigma_for_pad(rows, cols, 175, 200)
    sv, dv = pitched_case(ctx, kind, ch, rows, cols, sigma, engine=None, family=0, seed=7)
    with pytest.raises(B.BlurError):
        method(ctx, kind)(sv, sigma, out=dv, engine="fused")


def test_plane_fallback_in_place_on_a_view(ctx):
    import torch
    rows, cols, ch = 420, 390, 4
    sigma = sigma_for_pad(rows, cols, 175, 200)
    parent = rand_parent("u8", (2, rows + 5, cols + 11, ch), 9)
    before = raw(parent)
    view = parent[:, 2:2 + rows, 3:3 + cols]
    want = ctx.gaussian(view, sigma, out=torch.empty_like(packed_copy(view)))
    ctx.gaussian(view, sigma)
    assert ctx.last_engine()[0] == 0
    assert np.array_equal(raw(view), raw(want))
    assert_outside_untouched(before, raw(parent), 2, 3, rows, cols)


# ---- 8. one sigma per channel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,ch,sigmas,kept", [("u8", 4, (6.0, 6.0, 6.0, 0.0), 3), ("u16", 3, (0.0, 3.0, 9.0), 0), ("u8", 3, (4.0, 0.0, 11.0), 1),
                                                 ("f32", 4, (0.0, 0.0, 0.0, 0.0), None)])
def test_sigma_per_channel_on_views(ctx, kind, ch, sigmas, kept):
    import torch
    rows, cols = 211, 300
    sparent = rand_parent(kind, (rows + 8, cols + 16, ch), 12)
    dparent = sentinel_parent(kind, (rows + 5, cols + 23, ch))
    sv, dv = roi(sparent, 3, 5, rows, cols), roi(dparent, 2, 7, rows, cols)
    before = raw(dparent)
    method(ctx, kind)(sv, sigmas, out=dv, engine="fused")
    src = packed_copy(sv)
    want = method(ctx, kind)(src, sigmas, out=torch.empty_like(src), engine="fused")
    assert np.array_equal(raw(dv), raw(want))
    assert_outside_untouched(before, raw(dparent), 2, 7, rows, cols)
    es = src.element_size()
    got_px, src_px = raw(dv).reshape(rows, cols, ch, es), raw(src).reshape(rows, cols, ch, es)
    for c in ([kept] if kept is not None else range(ch)):
        assert np.array_equal(got_px[:, :, c], src_px[:, :, c]), "a sigma = 0 channel differs from the source"
    # in place: the sigma = 0 channels are not touched, the others as out of place
    method(ctx, kind)(sv, sigmas, engine="fused")
    assert np.array_equal(raw(sv), raw(want))


# ---- 9. the pitched entry with the packed layout is the packed entry -------------------------------------------------------
@pytest.mark.parametrize("kind,ch", [("u8", 1), ("u8", 4), ("u16", 3), ("f32", 3), ("f16", 4), ("bf16", 1)])
def test_packed_layout_through_the_pitched_entry(ctx, kind, ch):
    import torch
    rows, cols, sigma, n = 150, 261, 6.0, 2
    src = rand_parent(kind, (n, rows, cols, ch), 14)
    want, fam = packed_call(ctx, kind, src, sigma)
    got = torch.empty_like(src)
    o = ctx._opts(True, engine=None)
    ctx.use_torch_stream()
    pitch = cols * ch * src.element_size()
    entry = getattr(ctx._lib, "blur_gaussian_%s_pitched_batch_dev" % kind)
    assert entry(ctx._h, src.data_ptr(), pitch, rows * pitch, got.data_ptr(), pitch, rows * pitch, n, rows, cols, ch, float(sigma), C.byref(o)) == 0
    assert ctx.last_engine()[0] == fam
    assert np.array_equal(raw(got), raw(want))
    # one frame with a frame stride of 0
    one = torch.empty_like(src[0])
    assert entry(ctx._h, src.data_ptr(), pitch, 0, one.data_ptr(), pitch, 0, 1, rows, cols, ch, float(sigma), C.byref(o)) == 0
    assert np.array_equal(raw(one), raw(want[0]))


def test_u8c3_packed_layout_through_the_pitched_entry_meets_the_contract(ctx):
    """three u8 channels: the pitched entry runs fw_blur_u8<NKB, Q, 3> where the packed entry runs fx_blur_u8 -- the oracle decides"""
    import torch
    rows, cols, sigma = 150, 261, 6.0
    src = rand_parent("u8", (rows, cols, 3), 15)
    got = torch.empty_like(src)
    o = ctx._opts(True, engine=None)
    ctx.use_torch_stream()
    assert ctx._lib.blur_gaussian_u8_pitched_batch_dev(ctx._h, src.data_ptr(), cols * 3, 0, got.data_ptr(), cols * 3, 0, 1, rows, cols, 3, sigma, C.byref(o)) == 0
    assert ctx.last_engine()[0] == 6
    check_u8_oracle(raw(got), raw(src), sigma)


def test_refused_views(ctx):
    import torch
    t = torch.zeros(40, 50, 4, dtype=torch.uint8, device="cuda")
    for bad in (t[..., :3], t[:, ::2], t.permute(1, 0, 2)):
        with pytest.raises(ValueError):
            ctx.gaussian(bad, 2.0)
    with pytest.raises(ValueError):
        ctx.gaussian(t, 2.0, out=torch.zeros(40, 50, 8, dtype=torch.uint8, device="cuda")[..., ::2])
