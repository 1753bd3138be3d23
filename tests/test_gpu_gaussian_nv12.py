"""Gaussian blur of NV12 and P016 video surfaces where they lie (BlurContext.gaussian_nv12 -> blur_gaussian_nv12_batch_dev,
blur_gaussian_p016_batch_dev): the luma plane is, bit for bit, what the one-channel entry of the type returns for it, and Cb / Cr
are, bit for bit, what that entry returns for the de-interleaved half-resolution planes -- the chroma plane runs on the two-channel
instantiations fw_blur_u8<NKB, Q, 2> and ff_blur<uint16_t, NKB, Q, 2>.  A difference is a bug in the two-channel staging or
pre-pass, never a tie: no tolerance anywhere but in the one comparison against the float64 oracle.

Frames: luma 396 x 516, chroma 198 x 258 (more than one chunk of 128 columns, ragged last tile and chunk).  pffft_sizing caps the
window at the frame's longer side, so a 258-pixel chroma row holds pads to 129 only: the window classes above NKB 17 run on luma
396 x 676, chroma 198 x 338, which holds every pad to 168 (WIDE_COLS), and the thin planes keep their long side at 2 pad + 3 as
pad_cases.thin_shapes has it.

The cases are functions (case_*) and four tests run them in loops, printing each case before it runs (shown with a failure): 95
cases that take three seconds together are four entries in every later run of the suite, not 95."""
import itertools
import zlib

import numpy as np
import pytest

import structured as S
import u16_parity as U
from conftest import assert_u8_parity
from test_gpu_gaussian_channels import on_dev, sigma_for_class, sigma_for_pad
from test_gpu_gaussian_sigmas import same

pytestmark = pytest.mark.gpu

KINDS = ("nv12", "p016")
DTYPE = {"nv12": np.uint8, "p016": np.uint16}
TOP = {"nv12": 255, "p016": 65535}
ROWS, COLS = 396, 516
CROWS, CCOLS = ROWS // 2, COLS // 2
WIDE_COLS = 676                          # chroma 198 x 338: max(rows, cols) >= 2 * 168 + 1, the sizing does not cap the window


def noise(kind, seed, shape):
    return np.random.default_rng(seed).integers(0, TOP[kind] + 1, shape, dtype=DTYPE[kind])


def host(t):
    """a CONTIGUOUS device tensor as a numpy array"""
    assert t.is_contiguous()
    return t.cpu().numpy()


# ---- the reference: the one-channel entry of the type on a packed plane, computed once per (plane, sigma, options) ------------------
_REF = {}


def plane_ref(ctx, kind, plane, sigma, quirk=True, engine="fused"):
    """what ctx.gaussian / ctx.gaussian_u16 returns for the [rows, cols] plane (sigma 0: the plane itself) -> (array, family)"""
    import torch
    plane = np.ascontiguousarray(plane)
    if sigma == 0:
        return plane, None
    key = (kind, plane.shape, zlib.crc32(plane.tobytes()), float(sigma), bool(quirk), engine)
    if key not in _REF:
        t = on_dev(plane)
        fn = ctx.gaussian if kind == "nv12" else ctx.gaussian_u16
        got = fn(t, sigma, out=torch.empty_like(t), nyquist_quirk=quirk, engine=engine)
        _REF[key] = (host(got), ctx.last_engine()[0])
        _REF[key][0].setflags(write=False)
    return _REF[key]


def want_planes(ctx, kind, y, uv, sigmas, quirk=True, engine="fused"):
    """(luma, chroma) as the contract composes them from three one-channel calls"""
    wy = plane_ref(ctx, kind, y, sigmas[0], quirk, engine)[0]
    wuv = np.stack([plane_ref(ctx, kind, uv[..., c], sigmas[1 + c], quirk, engine)[0] for c in range(2)], axis=-1)
    return wy, wuv


def packed_call(ctx, kind, y, uv, sigmas, quirk=True, engine="fused"):
    """host planes -> contiguous device tensors -> out of place -> host planes, and the family"""
    import torch
    ty, tuv = on_dev(y), on_dev(uv)
    oy, ouv = torch.empty_like(ty), torch.empty_like(tuv)
    ry, ruv = ctx.gaussian_nv12(ty, tuv, sigmas, out=(oy, ouv), nyquist_quirk=quirk, engine=engine)
    assert ry is oy and ruv is ouv
    fam = ctx.last_engine()[0]
    assert np.array_equal(host(ty), y) and np.array_equal(host(tuv), uv), "the source was written"
    return host(oy), host(ouv), fam


def assert_planes(got_y, got_uv, want_y, want_uv, tag=""):
    assert np.array_equal(got_y, want_y), "%s: the luma plane differs from the one-channel entry's result" % tag
    for c, name in enumerate(("Cb", "Cr")):
        assert np.array_equal(got_uv[..., c], want_uv[..., c]), "%s: %s differs from the one-channel entry's result" % (tag, name)


def three_sigmas():
    """three window classes, both pad parities: luma pad 37 (NKB 7), Cb pad 6 (NKB 3), Cr pad 66 (NKB 11)"""
    return (sigma_for_pad(ROWS, COLS, 37, 37), sigma_for_pad(CROWS, CCOLS, 6, 6), sigma_for_pad(CROWS, CCOLS, 66, 66))


# ---- 1. bit equality with the one-channel entries ---------------------------------------------------------------------------------
def case_planes_equal_the_one_channel_entries(ctx, kind, quirk, engine):
    sigmas = three_sigmas()
    y, uv = noise(kind, 1, (ROWS, COLS)), noise(kind, 2, (CROWS, CCOLS, 2))
    gy, guv, fam = packed_call(ctx, kind, y, uv, sigmas, quirk, engine)
    assert fam == (0 if engine == "fft" else 6)
    assert_planes(gy, guv, *want_planes(ctx, kind, y, uv, sigmas, quirk, engine))
    assert not np.array_equal(guv[..., 0], guv[..., 1]) and not np.array_equal(guv, uv)


def case_chroma_meets_the_float64_oracle(ctx, kind, quirk):
    """the contract of the type itself, on the chroma plane: the u8 parity rule (conftest) and the u16 one (u16_parity)"""
    sigmas = three_sigmas()
    y, uv = noise(kind, 1, (ROWS, COLS)), noise(kind, 2, (CROWS, CCOLS, 2))
    _, guv, _ = packed_call(ctx, kind, y, uv, sigmas, quirk, "fused")
    planes = np.stack([S.oracle_plane(uv[..., c].astype(np.float32), sigmas[1 + c], quirk) for c in range(2)])
    if kind == "nv12":
        assert_u8_parity(guv, np.moveaxis(S.round_u8(planes), 0, -1), planes)
    else:
        U.assert_u16_parity(guv, planes)


# ---- 2. every window class on the chroma plane ---------------------------------------------------------------------------------------
def case_every_window_class_on_the_chroma_plane(ctx, kind, nkb, quirk):
    """both channels with one sigma of the class: one launch over the two channel tasks of every strip; the luma plane is left alone"""
    cols = COLS if nkb <= 17 else WIDE_COLS
    s = sigma_for_class(CROWS, cols // 2, nkb)
    sigmas = (0.0, s, s)
    y, uv = noise(kind, 3, (ROWS, cols)), noise(kind, 100 + nkb, (CROWS, cols // 2, 2))
    gy, guv, fam = packed_call(ctx, kind, y, uv, sigmas, quirk, "fused")
    assert fam == 6
    assert_planes(gy, guv, *want_planes(ctx, kind, y, uv, sigmas, quirk, "fused"), tag="NKB %d" % nkb)


# ---- 3. cross-talk between Cb and Cr -----------------------------------------------------------------------------------------------------
def stripes(kind, rows, cols):
    """period-2 stripes along x at full swing: the quirk's terms at their maximum, their sign alternating with x"""
    return (S.pattern("cols2", rows, cols) * TOP[kind]).astype(DTYPE[kind])


def case_a_structured_channel_beside_a_constant_one(ctx, kind, structured_channel, pad):
    s = sigma_for_pad(CROWS, CCOLS, pad, pad)
    uv = np.empty((CROWS, CCOLS, 2), DTYPE[kind])
    uv[..., structured_channel] = stripes(kind, CROWS, CCOLS)
    uv[..., 1 - structured_channel] = TOP[kind] // 3
    y = noise(kind, 4, (ROWS, COLS))
    sigmas = (0.0, s, s)
    gy, guv, _ = packed_call(ctx, kind, y, uv, sigmas, True, "fused")
    wy, wuv = want_planes(ctx, kind, y, uv, sigmas, True, "fused")
    assert_planes(gy, guv, wy, wuv)
    # the constant channel's result does not depend on its neighbour: the same constant beside another constant
    flat = np.full((CROWS, CCOLS, 2), TOP[kind] // 3, DTYPE[kind])
    _, gflat, _ = packed_call(ctx, kind, y, flat, sigmas, True, "fused")
    assert np.array_equal(gflat[..., 1 - structured_channel], guv[..., 1 - structured_channel])


def case_one_hot_channel(ctx, kind, c):
    uv = (S.one_hot_u8(c, 2, CROWS, CCOLS).astype(np.uint32) * (TOP[kind] // 255)).astype(DTYPE[kind])
    y = noise(kind, 5, (ROWS, COLS))
    sigmas = (0.0,) + three_sigmas()[1:]
    gy, guv, _ = packed_call(ctx, kind, y, uv, sigmas, True, "fused")
    assert_planes(gy, guv, *want_planes(ctx, kind, y, uv, sigmas, True, "fused"))
    assert np.array_equal(guv[..., 1 - c], want_planes(ctx, kind, y, np.zeros_like(uv), sigmas, True, "fused")[1][..., 1 - c]), "the empty channel saw its neighbour"


# ---- 4. unequal and zero sigmas ---------------------------------------------------------------------------------------------------------
def case_one_chroma_sigma_zero(ctx, kind, zero):
    """the kept channel is copied out of place and not touched in place (the launch covers the other channel's tasks only)"""
    sigmas = list(three_sigmas())
    sigmas[zero] = 0.0
    y, uv = noise(kind, 6, (ROWS, COLS)), noise(kind, 7, (CROWS, CCOLS, 2))
    wy, wuv = want_planes(ctx, kind, y, uv, sigmas)
    assert np.array_equal(wuv[..., zero - 1], uv[..., zero - 1])
    gy, guv, fam = packed_call(ctx, kind, y, uv, sigmas)
    assert fam == 6
    assert_planes(gy, guv, wy, wuv, "out of place")
    ty, tuv = on_dev(y), on_dev(uv)
    ry, ruv = ctx.gaussian_nv12(ty, tuv, sigmas, engine="fused")
    assert ry is ty and ruv is tuv
    assert_planes(host(ty), host(tuv), wy, wuv, "in place")


def case_luma_only_and_all_zero(ctx, kind):
    import torch
    y, uv = noise(kind, 8, (ROWS, COLS)), noise(kind, 9, (CROWS, CCOLS, 2))
    s0 = three_sigmas()[0]
    gy, guv, fam = packed_call(ctx, kind, y, uv, (s0, 0.0, 0.0))
    assert fam == 6 and np.array_equal(guv, uv)
    assert np.array_equal(gy, plane_ref(ctx, kind, y, s0)[0])
    # all three zero: a copy out of place, nothing at all in place
    gy, guv, _ = packed_call(ctx, kind, y, uv, (0.0, 0.0, 0.0))
    assert np.array_equal(gy, y) and np.array_equal(guv, uv)
    ty, tuv = on_dev(y), on_dev(uv)
    ctx.gaussian_nv12(ty, tuv, (0, 0, 0))
    torch.cuda.synchronize()
    assert np.array_equal(host(ty), y) and np.array_equal(host(tuv), uv)


# ---- 5. a real surface: one allocation, pitch > cols, UV directly behind Y -----------------------------------------------------------
def surface(kind, rows, cols, pitch, seed, n=None, tail_rows=3):
    """host array [n,] rows + rows / 2 + tail_rows, pitch: noise everywhere, the padding included"""
    shape = (rows + rows // 2 + tail_rows, pitch)
    return noise(kind, seed, shape if n is None else (n,) + shape)


def planes_of(surf, rows, cols):
    """the (y, uv) views of a surface (a numpy array or a device tensor): uv [.., rows / 2, cols / 2, 2]"""
    y = surf[..., :rows, :cols]
    c = surf[..., rows:rows + rows // 2, :cols]
    return y, (c.reshape(c.shape[:-1] + (cols // 2, 2)) if isinstance(c, np.ndarray) else c.unflatten(-1, (cols // 2, 2)))


def assert_surface(after, before, rows, cols, wy, wuv, tag):
    """the two rectangles hold the results and every other byte of the surface is what it was"""
    gy, guv = planes_of(after, rows, cols)
    assert_planes(gy, guv, wy, wuv, tag)
    a, b = after.copy(), before.copy()
    for s in (a, b):
        s[..., :rows + rows // 2, :cols] = 0
    assert np.array_equal(a, b), "%s: bytes outside the two rectangles were written" % tag


def case_a_decoder_surface_in_place_and_out_of_place(ctx, kind, cols):
    """cols = 514: chroma rows of 257 pairs = 514 bytes (NV12), no multiple of 4 -- the pre-pass's last dword of a row; the NV12
    pitches are odd, so the rows start at every alignment"""
    rows, spitch, dpitch = ROWS, cols + 13, cols + 31
    sigmas = three_sigmas()
    src = surface(kind, rows, cols, spitch, 10 + cols)
    y, uv = planes_of(src, rows, cols)
    wy, wuv = want_planes(ctx, kind, y, uv, sigmas)
    # out of place, into a surface of another pitch
    ts = on_dev(src)
    dst = surface(kind, rows, cols, dpitch, 11)
    td = on_dev(dst)
    ctx.gaussian_nv12(*planes_of(ts, rows, cols), sigmas, out=planes_of(td, rows, cols), engine="fused")
    assert ctx.last_engine()[0] == 6
    assert np.array_equal(host(ts), src), "the source surface was written"
    assert_surface(host(td), dst, rows, cols, wy, wuv, "out of place")
    # in place
    ty, tuv = planes_of(ts, rows, cols)
    assert not ty.is_contiguous() and not tuv.is_contiguous() and tuv.data_ptr() == ty.data_ptr() + rows * spitch * ts.element_size()
    ctx.gaussian_nv12(ty, tuv, sigmas, engine="fused")
    assert ctx.last_engine()[0] == 6
    assert_surface(host(ts), src, rows, cols, wy, wuv, "in place")


def case_a_surface_on_the_plane_path(ctx, kind):
    """engine = fft: the plane path writes the rectangles only, too"""
    rows, cols, pitch = 120, 164, 200
    sigmas = (4.0, 2.0, 3.0)
    src = surface(kind, rows, cols, pitch, 12)
    y, uv = planes_of(src, rows, cols)
    ts = on_dev(src)
    ctx.gaussian_nv12(*planes_of(ts, rows, cols), sigmas, engine="fft")
    fam, note = ctx.last_engine()
    assert fam == 0 and "luma" in note and "chroma" in note
    assert_surface(host(ts), src, rows, cols, *want_planes(ctx, kind, y, uv, sigmas, True, "fft"), tag="plane path")


# ---- 6. the thinnest legal chroma plane ---------------------------------------------------------------------------------------------------
def case_thinnest_chroma_plane(ctx, kind, nkb, thin):
    """a chroma plane whose short side is pad + 1 (the long side 2 pad + 3 keeps the window uncapped: pad_cases.thin_shapes): across
    the short side every window position but one is a mirrored pixel"""
    import blur_algorithms_amd as B
    pad = 8 * (nkb - 2)
    crows, ccols = (pad + 1, 2 * pad + 3) if thin == "rows" else (2 * pad + 3, pad + 1)
    s = sigma_for_pad(crows, ccols, pad, pad)
    y, uv = noise(kind, 13, (2 * crows, 2 * ccols)), noise(kind, 14, (crows, ccols, 2))
    sigmas = (2.0, s, s)
    gy, guv, fam = packed_call(ctx, kind, y, uv, sigmas)
    assert fam == 6
    assert_planes(gy, guv, *want_planes(ctx, kind, y, uv, sigmas))
    thinner = (y[:2 * pad], uv[:pad]) if thin == "rows" else (y[:, :2 * pad], uv[:, :pad])
    with pytest.raises(B.BlurError) as e:                     # one chroma pixel thinner: refused before anything runs
        packed_call(ctx, kind, thinner[0], thinner[1], sigmas)
    assert e.value.code == 2


# ---- 7. batches, and the host entry -----------------------------------------------------------------------------------------------------
def case_batch_of_three_equals_three_calls_and_the_host_entry(ctx, kind):
    """Y and UV in two allocations with their own frame strides and a common pitch"""
    import torch
    n, rows, cols, pitch = 3, 150, 260, 288
    sigmas = (6.0, 2.5, 4.0)
    ya, uva = noise(kind, 15, (n, rows + 7, pitch)), noise(kind, 16, (n, rows // 2 + 2, pitch))
    ty, tuv = on_dev(ya), on_dev(uva)
    y, uv = ty[:, :rows, :cols], tuv[:, :rows // 2, :cols].unflatten(-1, (cols // 2, 2))
    assert y.stride(0) != 2 * uv.stride(0) and y.stride(1) == uv.stride(1) == pitch
    oy, ouv = torch.empty((n, rows, cols), dtype=ty.dtype, device="cuda"), torch.empty((n, rows // 2, cols // 2, 2), dtype=ty.dtype, device="cuda")
    ctx.gaussian_nv12(y, uv, sigmas, out=(oy, ouv), engine="fused")
    assert ctx.last_engine()[0] == 6
    assert np.array_equal(host(ty), ya) and np.array_equal(host(tuv), uva)
    hy, huv = ya[:, :rows, :cols], uva[:, :rows // 2, :cols].reshape(n, rows // 2, cols // 2, 2)
    for f in range(n):
        sy, suv = torch.empty_like(oy[f]), torch.empty_like(ouv[f])
        ctx.gaussian_nv12(y[f], uv[f], sigmas, out=(sy, suv), engine="fused")
        assert same(sy, oy[f]) and same(suv, ouv[f]), "frame %d of the batch differs from the single call" % f
        assert_planes(host(oy[f]), host(ouv[f]), *want_planes(ctx, kind, hy[f], huv[f], sigmas), tag="frame %d" % f)
    # the host entry (numpy arrays): the same bytes
    gy, guv = ctx.gaussian_nv12(np.ascontiguousarray(hy), np.ascontiguousarray(huv), sigmas, engine="fused")
    assert np.array_equal(gy, host(oy)) and np.array_equal(guv, host(ouv))
    # the batch in place, on the views
    ctx.gaussian_nv12(y, uv, sigmas, engine="fused")
    assert same(y.contiguous() if kind == "nv12" else y.view(torch.int16).contiguous(), oy)
    assert same(uv.contiguous() if kind == "nv12" else uv.view(torch.int16).contiguous(), ouv)


# ---- the tests: each runs its cases in turn and prints the case it is at (shown with a failure) ---------------------------------
def each(case, ctx, **axes):
    for values in itertools.product(*axes.values()):
        kw = dict(zip(axes, values))
        print(case.__name__, kw, flush=True)
        case(ctx, **kw)


def test_planes_equal_the_one_channel_entries(ctx):
    """1. bit equality of all three planes, NV12 and P016, quirk on and off, engine None / fused / fft; the chroma plane against the
    float64 oracle under the type's own parity rule; 8. the engine per plane (defined at the end of the file)"""
    each(case_planes_equal_the_one_channel_entries, ctx, kind=KINDS, quirk=(True, False), engine=(None, "fused", "fft"))
    each(case_chroma_meets_the_float64_oracle, ctx, kind=KINDS, quirk=(True, False))
    each(case_engine_rules_are_the_one_channel_entries, ctx)


def test_every_window_class_on_the_chroma_plane(ctx):
    """2. every window class, engine fused, family 6"""
    each(case_every_window_class_on_the_chroma_plane, ctx, kind=KINDS, nkb=S.NKB_CLASSES, quirk=(True, False))


def test_cross_talk_and_zero_sigmas(ctx):
    """3. and 4. a structured channel beside a constant one and the reverse, a one-hot channel; one chroma sigma 0, luma only, all 0"""
    each(case_a_structured_channel_beside_a_constant_one, ctx, kind=KINDS, structured_channel=(0, 1), pad=(21, 40))
    each(case_one_hot_channel, ctx, kind=KINDS, c=(0, 1))
    each(case_one_chroma_sigma_zero, ctx, kind=KINDS, zero=(1, 2))
    each(case_luma_only_and_all_zero, ctx, kind=KINDS)


def test_surfaces_thin_planes_and_batches(ctx):
    """5., 6. and 7. a decoder surface in place and out of place (cols 516 and 514), on the plane path too; the thinnest legal chroma
    planes of a narrow and a wide class; a batch of three against three calls and the host entry"""
    each(case_a_decoder_surface_in_place_and_out_of_place, ctx, kind=KINDS, cols=(COLS, 514))
    each(case_a_surface_on_the_plane_path, ctx, kind=KINDS)
    each(case_thinnest_chroma_plane, ctx, kind=KINDS, nkb=(5, 21), thin=("rows", "cols"))
    each(case_batch_of_three_equals_three_calls_and_the_host_entry, ctx, kind=KINDS)


# ---- 8. the engine per plane ---------------------------------------------------------------------------------------------------------------
def case_engine_rules_are_the_one_channel_entries(ctx):
    """chroma pad 175 has no fused kernel: AUTO blurs it on the plane path and says so, FUSED refuses before anything is written;
    P016 under AUTO takes the fused kernel to pad 104 only"""
    import torch
    import blur_algorithms_amd as B
    rows, cols = 360, 704                                     # chroma 180 x 352: holds pad 175 uncapped
    y, uv = noise("nv12", 17, (rows, cols)), noise("nv12", 18, (rows // 2, cols // 2, 2))
    s = sigma_for_pad(rows // 2, cols // 2, 170, 178)
    sigmas = (3.0, s, 2.0)
    gy, guv, fam = packed_call(ctx, "nv12", y, uv, sigmas, True, None)
    note = ctx.last_engine()[1]
    assert fam == 0 and "chroma" in note and "luma" not in note
    wy = plane_ref(ctx, "nv12", y, 3.0, True, None)[0]
    wuv = np.stack([plane_ref(ctx, "nv12", uv[..., 0], s, True, None)[0], plane_ref(ctx, "nv12", uv[..., 1], 2.0, True, None)[0]], axis=-1)
    assert_planes(gy, guv, wy, wuv)
    ty, tuv = on_dev(y), on_dev(uv)
    with pytest.raises(B.BlurError) as e:
        ctx.gaussian_nv12(ty, tuv, sigmas, engine="fused")
    assert e.value.code == 2
    torch.cuda.synchronize()
    assert np.array_equal(host(ty), y) and np.array_equal(host(tuv), uv), "a refused call wrote"
    # P016, AUTO: pad 120 on the luma plane is the plane path (as gaussian_u16 has it), fused on request
    y16, uv16 = noise("p016", 19, (rows, cols)), noise("p016", 20, (rows // 2, cols // 2, 2))
    s120 = sigma_for_pad(rows, cols, 120, 120)
    for engine, family in ((None, 0), ("fused", 6)):
        gy, guv, fam = packed_call(ctx, "p016", y16, uv16, (s120, 2.0, 2.0), True, engine)
        assert fam == family
        assert plane_ref(ctx, "p016", y16, s120, True, engine)[1] == family
        assert_planes(gy, guv, *want_planes(ctx, "p016", y16, uv16, (s120, 2.0, 2.0), True, engine))
