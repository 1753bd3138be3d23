"""The texts, codes and order of refusal of the per-channel Gaussian drivers (blur_ch_batch_impl, blur_ch_sigmas_batch_impl,
blur_ch_frame_sigmas_batch_impl, blur_nv_batch_impl, blur_nv_frame_sigmas_batch_impl in csrc/engine.hip), written out as the
library returns them: the five drivers share their engine check, their fused-kernel rules and their plane-path notes, and a caller
that shows blur_last_error or parses blur_last_engine's note sees these bytes.

1. An engine other than AUTO, FUSED and FFT: BLUR_ERR_UNSUPPORTED with the driver's own text, for every pixel type and entry, and
   nothing written.
2. The fused-kernel rules by type, on 176 x 340 frames (the short side just holds a pad of 168, the long side keeps pffft_sizing from
   capping the window: 2 pad + 1 <= 340): float32 with 3 channels has no kernel for pad 153 .. 168 and FUSED is refused; u16 and
   bfloat16 have one for every channel count (ff_class_ok_t) and FUSED runs it.  Under AUTO a pad in 105 .. 152 takes the plane
   path, family 0, the note says why in the driver's words, and the result is the engine = FFT call's bit for bit.
3. Precedence: a layout error comes before an argument error, a size error before a sigma error.

The cases are functions (case_*) behind two tests, as in test_gpu_gaussian_nv12.py."""
import ctypes as C
import itertools

import numpy as np
import pytest

from test_gpu_gaussian_channels import sigma_for_pad

pytestmark = pytest.mark.gpu

KINDS = ("u8", "f32", "u16", "f16", "bf16")
NAME = {"u8": "u8", "f32": "float32", "u16": "u16", "f16": "float16", "bf16": "bfloat16"}
SCALAR = {"u8": "gaussian", "f32": "gaussian_f32", "u16": "gaussian_u16", "f16": "gaussian_f16", "bf16": "gaussian_bf16"}
PER_FRAME = {"u8": "gaussian_per_frame", "f32": "gaussian_f32_per_frame", "u16": "gaussian_u16_per_frame", "f16": "gaussian_f16_per_frame",
             "bf16": "gaussian_bf16_per_frame"}
MUST = ": engine must be AUTO, FUSED or FFT"
ROWS, COLS = 176, 340


def frames(kind, shape, seed):
    """a CUDA tensor of the kind: integers 0 .. 255 (every type holds them exactly)"""
    import torch
    v = np.random.default_rng(seed).integers(0, 256, shape)
    if kind in ("u8", "u16"):
        return torch.from_numpy(v.astype(np.uint8 if kind == "u8" else np.uint16)).cuda()
    return torch.from_numpy(v.astype(np.float32)).to({"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[kind]).cuda()


def raw(t):
    """the bytes of a tensor"""
    import torch
    return t.contiguous().cpu().view(torch.uint8).numpy()


def refused(call, src, outs, text):
    """call(out=...) raises BLUR_ERR_UNSUPPORTED with exactly `text`; the sources and the prefilled results keep their bytes"""
    import torch
    import blur_algorithms_amd as B
    before = [raw(t).copy() for t in tuple(src) + tuple(outs)]
    with pytest.raises(B.BlurError) as e:
        call()
    assert e.value.code == 2 and str(e.value) == "BLUR_ERR_UNSUPPORTED (2): " + text, str(e.value)
    torch.cuda.synchronize()
    for t, b in zip(tuple(src) + tuple(outs), before):
        assert np.array_equal(raw(t), b), "a refused call wrote"


# ---- 1. an engine that the per-channel entries do not have ---------------------------------------------------------------------
def case_unsupported_engine(ctx, kind, engine):
    """32 x 32, 2 frames, sigma 1.  u8 takes 4 channels (3 packed u8 channels are the u8c3 entry, which has these engines); equal
    sigmas per channel are the scalar call, text included"""
    x = frames(kind, (2, 32, 32, 4), 1)
    out = frames(kind, x.shape, 2)
    scalar = ("1- and 4-channel" if kind == "u8" else NAME[kind]) + " images" + MUST
    refused(lambda: getattr(ctx, SCALAR[kind])(x, 1.0, out=out, engine=engine), (x,), (out,), scalar)
    refused(lambda: getattr(ctx, SCALAR[kind])(x, (1.0, 1.0, 1.0, 1.0), out=out, engine=engine), (x,), (out,), scalar)
    refused(lambda: getattr(ctx, SCALAR[kind])(x, (1.0, 1.0, 1.0, 0.0), out=out, engine=engine), (x,), (out,),
            NAME[kind] + " images, one sigma per channel" + MUST)
    refused(lambda: getattr(ctx, PER_FRAME[kind])(x, (1.0, 1.0), out=out, engine=engine), (x,), (out,), NAME[kind] + " images, one sigma per frame" + MUST)
    pitched = frames(kind, (2, 32, 40, 4), 3)                 # the pitched entries: a view with padded rows, in place
    refused(lambda: getattr(ctx, SCALAR[kind])(pitched[:, :, :32], 1.0, engine=engine), (), (pitched,), scalar)


def case_unsupported_engine_nv(ctx, kind, engine):
    y, uv = frames(kind, (2, 32, 32), 4), frames(kind, (2, 16, 16, 2), 5)
    oy, ouv = frames(kind, y.shape, 6), frames(kind, uv.shape, 7)
    text = "NV12 / P016 surfaces" + MUST
    refused(lambda: ctx.gaussian_nv12(y, uv, 1.0, out=(oy, ouv), engine=engine), (y, uv), (oy, ouv), text)
    refused(lambda: ctx.gaussian_nv12_per_frame(y, uv, (1.0, 1.0), out=(oy, ouv), engine=engine), (y, uv), (oy, ouv), text)


# ---- 2. the fused kernel's rules by type ---------------------------------------------------------------------------------------------
NO_CLASS = "fused kernel for float32 images: pad 153 .. 168 has a kernel for 1 channel only"
NO_CONTRACT = {
    "f32": "pad 105 .. 168 exceeds 1e-6 max|x| on full-scale content (1.2e-6); ask for it with engine = FUSED",
    "u16": "pad 105 .. 168 exceeds 1e-6 of full scale on full-scale content (1.2e-6); ask for it with engine = FUSED",
    "bf16": "pad 105 .. 168 is outside the library's own choice, as for float32; ask for it with engine = FUSED",
}
# the scalar driver names both half types; the one-sigma-per-frame driver names the call's
SCALAR_KIND = {"f32": "float32", "u16": "u16", "bf16": "float16 / bfloat16"}


def sigma_with_pad(lo, hi):
    import blur_algorithms_amd as B
    s = sigma_for_pad(ROWS, COLS, lo, hi)
    pad = B.pffft_sizing(ROWS, COLS, s)["pad"]
    assert lo <= pad <= hi and pad <= min(ROWS, COLS) - 1
    return s


def case_widest_class_under_fused(ctx, kind, ch):
    """pad 153 .. 168: float32 has the kernel for 1 channel only, and both drivers say so; u16 and bfloat16 have it for 3 and 4"""
    import torch
    s = sigma_with_pad(153, 168)
    x = frames(kind, (2, ROWS, COLS, ch), 10)
    out = frames(kind, x.shape, 11)
    if kind == "f32":
        refused(lambda: getattr(ctx, SCALAR[kind])(x, s, out=out, engine="fused"), (x,), (out,), NO_CLASS)
        refused(lambda: getattr(ctx, PER_FRAME[kind])(x, (s, s), out=out, engine="fused"), (x,), (out,), NO_CLASS)
        return
    getattr(ctx, SCALAR[kind])(x, s, out=out, engine="fused")
    assert ctx.last_engine() == (6, "fused matrix-core kernel")
    per_frame = getattr(ctx, PER_FRAME[kind])(x, (s, s), out=torch.empty_like(x), engine="fused")
    assert ctx.last_engine() == (6, "fused matrix-core kernel")
    assert np.array_equal(raw(per_frame), raw(out)), "the one-sigma-per-frame entry differs from the scalar entry"


def case_own_choice_stops_at_pad_104(ctx, kind, ch):
    """pad 105 .. 152 under AUTO: the plane path, family 0, each driver's note, and the engine = FFT call's bits"""
    import torch
    s = sigma_with_pad(105, 152)
    x = frames(kind, (2, ROWS, COLS, ch), 12)
    for method, sigma, head, named in ((SCALAR, s, "", SCALAR_KIND[kind]), (PER_FRAME, (s, s), "2 frames on the plane path, the first frame 0 (sigma %g): " % s, NAME[kind])):
        got = getattr(ctx, method[kind])(x, sigma, out=torch.empty_like(x))
        assert ctx.last_engine() == (0, "run-time-planned FFT kernels (not taken: " + head + "fused kernel for " + named + " images: " + NO_CONTRACT[kind] + ")")
        want = getattr(ctx, method[kind])(x, sigma, out=torch.empty_like(x), engine="fft")
        assert ctx.last_engine()[0] == 0
        assert np.array_equal(raw(got), raw(want)), "AUTO on the plane path differs from engine = FFT"
        assert not np.array_equal(raw(got), raw(x))


# ---- 3. precedence ------------------------------------------------------------------------------------------------------------------
def case_layout_error_before_argument_error(ctx):
    """a row pitch below a row's bytes and a negative sigma: the pitch is reported"""
    x = frames("u8", (2, 32, 32, 4), 20)
    before = raw(x).copy()
    o = ctx._opts()
    rc = ctx._lib.blur_gaussian_u8_pitched_batch_dev(ctx._h, x.data_ptr(), 32 * 4 - 1, 32 * 32 * 4, x.data_ptr(), 32 * 4, 32 * 32 * 4, 2, 32, 32, 4, -1.0, C.byref(o))
    assert rc == 1 and ctx._lib.blur_last_error(ctx._h).decode() == "row pitch below cols * channels * sizeof(element)"
    rc = ctx._lib.blur_gaussian_u8_pitched_batch_dev(ctx._h, x.data_ptr(), 32 * 4, 32 * 32 * 4, x.data_ptr(), 32 * 4, 32 * 32 * 4, 2, 32, 32, 4, -1.0, C.byref(o))
    assert rc == 1 and ctx._lib.blur_last_error(ctx._h).decode() == "rows, cols and sigma must be positive"
    assert np.array_equal(raw(x), before)


def case_size_error_before_sigma_error(ctx):
    """an NV12 surface with odd cols and a negative sigma: the size is reported"""
    y, uv = frames("u8", (2, 32, 32), 21), frames("u8", (2, 16, 16, 2), 22)
    before = raw(y).copy(), raw(uv).copy()
    o = ctx._opts()
    sg = (C.c_double * 3)(-1.0, 1.0, 1.0)

    def call(cols):
        return ctx._lib.blur_gaussian_nv12_batch_dev(ctx._h, y.data_ptr(), uv.data_ptr(), 32, 32 * 32, 16 * 32, y.data_ptr(), uv.data_ptr(), 32, 32 * 32, 16 * 32, 2, 32, cols,
                                                     sg, C.byref(o))
    assert call(31) == 1 and ctx._lib.blur_last_error(ctx._h).decode() == "rows and cols must be positive and even (4:2:0 chroma)"
    assert call(32) == 1 and ctx._lib.blur_last_error(ctx._h).decode() == "every sigma must be finite and positive, or 0 for a plane that is left as it is"
    assert np.array_equal(raw(y), before[0]) and np.array_equal(raw(uv), before[1])


# ---- the tests: each runs its cases in turn and prints the case it is at (shown with a failure) -----------------------------------
def each(case, ctx, **axes):
    for values in itertools.product(*axes.values()):
        kw = dict(zip(axes, values))
        print(case.__name__, kw, flush=True)
        case(ctx, **kw)


def test_refusals_and_their_order(ctx):
    """1. and 3.: an engine outside AUTO, FUSED and FFT, for the five pixel types, NV12 and P016, through every entry; layout before
    arguments, size before sigmas"""
    each(case_unsupported_engine, ctx, kind=KINDS, engine=("matrix", "wave-resident"))
    each(case_unsupported_engine_nv, ctx, kind=("u8", "u16"), engine=("matrix", "wave-resident"))
    each(case_layout_error_before_argument_error, ctx)
    each(case_size_error_before_sigma_error, ctx)


def test_fused_kernel_rules_by_type(ctx):
    """2.: pad 153 .. 168 under FUSED and pad 105 .. 152 under AUTO, float32 and u16 with 3 channels, bfloat16 with 4, through the
    scalar and the one-sigma-per-frame entries"""
    for kind, ch in (("f32", 3), ("u16", 3), ("bf16", 4)):
        each(case_widest_class_under_fused, ctx, kind=(kind,), ch=(ch,))
        each(case_own_choice_stops_at_pad_104, ctx, kind=(kind,), ch=(ch,))
