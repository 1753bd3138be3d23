"""Every pad 1 .. 168 through every fused kernel family (fx_blur_u8, fw_blur_u8 of 1, 3 and 4 channels, ff_blur of float32, u16,
float16 and bfloat16), the frames whose side is pad + 1, and the non-finite contract of the float entries.  The cases are
tests/pad_cases.py's; tests/test_pad_cases.py proves them on the CPU.  Every result is compared with the float64 oracle under the
contracts the other GPU tests use, unchanged: assert_u8_parity, u16_parity.assert_u16_parity, half_parity.assert_half_parity and
|got - oracle| <= 1e-6 max|x| for float32.

The other sweeps run one pad per window class.  Inside a class the pad still decides the sign of the quirk terms (its parity), where
the 2 pad + 1 taps sit in the staged window of 16 NKB positions, the transform sizes and the float kernels' frame scale: here every
class runs all of its pads, the period-2 patterns (the quirk terms at their maximum) at both ends and at one pad of each parity,
and the quirk's sign is checked on its own."""
import numpy as np
import pytest

import half_parity as H
import pad_cases as P
import structured as S
import u16_parity as U
from conftest import assert_u8_parity

pytestmark = pytest.mark.gpu

UNSUPPORTED = 2                      # BLUR_ERR_UNSUPPORTED
REL_TOL = 1e-6                       # the float32 contract of include/blur_amd.h (test_gpu_gaussian_f32.REL_TOL)
GUARD = 64 * 1024                    # bytes of a known pattern either side of a guarded destination
NARROW = (3, 5, 7, 9, 11)            # the classes fx_blur_u8 serves: fw_blur_u8<., ., 3> runs there under per-channel sigmas only


def tdtype(kind):
    import torch
    return {"u8": torch.uint8, "u16": torch.uint16, "f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[kind]


def to_dev(kind, img):
    """a frame (or frames) of pad_cases.frame on the device in the sample type (the half types: the narrowing is exact)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(img))
    if kind in H.TYPES:
        t = t.to(tdtype(kind))
    return t.cuda()


def raw(t):
    """the tensor's samples as a numpy array: uint8, uint16 (u16 and the bit patterns of the half types) or float32"""
    import torch
    if t.dtype in (torch.float16, torch.bfloat16):
        t = t.view(torch.uint16)
    return t.cpu().numpy()


def values(kind, bits):
    return H.from_bits(kind, bits) if kind in H.TYPES else bits


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def guard_bytes(n):
    return ((np.arange(n, dtype=np.int64) * 40503 + 12345) % 251).astype(np.uint8)


_device_error = []


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """after a HIP error nothing more of this file is started on the GPU"""
    if _device_error:
        pytest.exit("a device error in an earlier test: %s" % _device_error[0], returncode=3)
    yield


def blur(ctx, kind, img, sigma, quirk, engine, guard=False):
    """blur_() below; any error that is not one of the API's own statuses (INVALID, UNSUPPORTED) ends the file's run"""
    import blur_algorithms_amd as B
    try:
        return blur_(ctx, kind, img, sigma, quirk, engine, guard)
    except B.BlurError as e:
        if e.code not in (1, UNSUPPORTED):
            _device_error.append(str(e))
        raise
    except RuntimeError as e:
        _device_error.append(str(e))
        raise


def blur_(ctx, kind, img, sigma, quirk, engine, guard=False):
    """out of place; 3-channel u8 through pffft_ (fx_blur_u8 / fw_blur_u8 CH 3), everything else through gaussian*; sigma may be a
    sequence (one per channel, gaussian* only).  guard: the destination sits between two bands of GUARD bytes, which must come back
    as they were.  -> raw() of the result"""
    import torch
    t = to_dev(kind, img)
    if kind == "u8":
        fn = ctx.pffft_ if img.shape[-1] == 3 and not isinstance(sigma, tuple) else ctx.gaussian
    else:
        fn = getattr(ctx, "gaussian_" + kind)
    if not guard:
        return raw(fn(t, sigma, out=torch.empty_like(t), nyquist_quirk=quirk, engine=engine))
    n = t.numel() * t.element_size()
    host = guard_bytes(2 * GUARD + n)
    dbuf = torch.from_numpy(host.copy()).cuda()
    dst = dbuf[GUARD:GUARD + n].view(t.dtype).view(t.shape)
    fn(t, sigma, out=dst, nyquist_quirk=quirk, engine=engine)
    back = dbuf.cpu().numpy()
    assert np.array_equal(back[:GUARD], host[:GUARD]), "bytes before the destination changed"
    assert np.array_equal(back[GUARD + n:], host[GUARD + n:]), "bytes after the destination changed"
    return raw(dst)


def refused(ctx, kind, img, sigma, quirk):
    """engine = "fused" fails with BLUR_ERR_UNSUPPORTED"""
    import blur_algorithms_amd as B
    with pytest.raises(B.BlurError) as e:
        blur(ctx, kind, img, sigma, quirk, "fused")
    assert e.value.code == UNSUPPORTED


def check(kind, got, img, planes):
    """got: raw() of one frame [rows, cols, ch]; planes [ch, rows, cols]: the contract of the type"""
    if kind == "u8":
        assert_u8_parity(got, np.moveaxis(S.round_u8(planes), 0, -1), planes)
    elif kind == "u16":
        U.assert_u16_parity(got, planes)
    elif kind in H.TYPES:
        H.assert_half_parity(kind, values(kind, got), planes, float(np.abs(img).max()))
    else:
        m = float(np.max(np.abs(img.astype(np.float64))))
        assert np.all(np.isfinite(got)), "non-finite output"
        err = float(np.max(np.abs(got.astype(np.float64) - np.moveaxis(planes, 0, -1).astype(np.float64)))) / m
        print("max|err| / max|x| = %.3g" % err)
        assert err <= REL_TOL, "max |error| / max|x| = %.3g" % err


def no_float_kernel(kind, nkb, ch):
    """ff_blur_f32 of NKB 23 exists for one channel only (ff_class_ok_t)"""
    return kind == "f32" and nkb == 23 and ch != 1


def run_frame(ctx, kind, nkb, p, specs, rows, cols, quirk, guard=False):
    """one frame on the route its case takes, against the oracle; the family the call reports is asserted"""
    ch = len(specs)
    sigma = P.sigma_for_pad(p)
    img = P.frame(kind, specs, rows, cols)
    planes = P.oracle_planes(kind, specs, rows, cols, sigma, quirk)
    no_prepass = quirk and cols < 4                        # prepare refuses FUSED: the quirk's pre-pass reads groups of 4 pixels
    on_auto = specs[0][0] == "noise" and (kind, p) in P.NOISE_ON_AUTO
    if no_prepass or no_float_kernel(kind, nkb, ch) or on_auto:
        if not on_auto:
            refused(ctx, kind, img, sigma, quirk)
        got = blur(ctx, kind, img, sigma, quirk, None, guard)
        if not no_prepass:
            assert ctx.last_engine()[0] == 0
    else:
        got = blur(ctx, kind, img, sigma, quirk, "fused", guard)
        assert ctx.last_engine()[0] == 6
    check(kind, got, img, planes)
    if kind == "u8" and ch == 3 and nkb in NARROW and not no_prepass:
        # fw_blur_u8<NKB, Q, 3>: sigmas (s, 0, s); the middle channel is left as it is
        got = blur(ctx, kind, img, (sigma, 0.0, sigma), quirk, "fused", guard)
        assert ctx.last_engine()[0] == 6
        assert np.array_equal(got[..., 1], img[..., 1]), "the channel of sigma 0 changed"
        for c in (0, 2):
            check(kind, got[..., c:c + 1], img[..., c:c + 1], planes[c:c + 1])


def collect(fails, what, fn, *args, **kw):
    """run one case; an assertion that fails is kept, with the case's name, so that one run names every failing pad"""
    try:
        fn(*args, **kw)
    except AssertionError as e:
        fails.append("%s: %s" % (what, str(e).splitlines()[0] if str(e) else "assertion failed"))


def names(specs):
    return "+".join(s[1] if s[0] == "pat" else "noise" for s in specs)


# ---- A. every pad of every class -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("nkb", P.NKB_CLASSES)
@pytest.mark.parametrize("kind", P.KINDS)
def test_every_pad_of_the_class(ctx, kind, nkb, quirk):
    """noise with a seed of its own at every pad, frames of 1, 3 and 4 channels; at both ends of the class and at one pad of each
    parity also cols2, rows2 and checker at the levels the class's structured cases use.  u8 with 3 channels: pffft_ (fx_blur_u8 up to
    NKB 11, fw_blur_u8 above) and, up to NKB 11, sigmas (s, 0, s) (fw_blur_u8 with CH 3).  float32 at NKB 23 has a kernel for one
    channel only: FUSED refuses 3 and 4, and the library's own choice is checked instead"""
    rows, cols = P.sweep_shape(nkb)
    fails = []
    for p in P.CLASS_PADS[nkb]:
        for ch, specs in P.sweep_frames(kind, nkb, p, quirk):
            collect(fails, "pad %d, %d ch, %s" % (p, ch, names(specs)), run_frame, ctx, kind, nkb, p, specs, rows, cols, quirk)
    assert not fails, "%d cases fail:\n%s" % (len(fails), "\n".join(fails))


def sign_bound(kind, ref, m):
    """the bound of one call on |got - ref|, for the difference of two calls: 1e-6 max|x| for float32; for the half types that plus
    the oracle's return rounding (half_parity.tolerance) plus half a spacing of the type at the far end of the interval"""
    if kind == "f32":
        return np.full(ref.shape, REL_TOL * m)
    tol = H.tolerance(ref, m)
    return tol + 0.5 * H.ulp(kind, np.abs(ref) + tol)


@pytest.mark.parametrize("nkb", P.NKB_CLASSES)
@pytest.mark.parametrize("kind", P.KINDS)
def test_the_sign_of_the_quirk_terms(ctx, kind, nkb):
    """blur(x, quirk on) - blur(x, quirk off) on cols2 against the same difference of the two oracles, under twice the bound of one
    call, at one even and one odd pad: the quirk's sign is (pad & 1) ? -1 : 1 in every kernel, and a slip doubles the difference
    (tests/test_pad_cases.py: it is of the order of the amplitude)"""
    rows, cols = P.sweep_shape(nkb)
    fails = []

    def one(p, ch):
        sigma = P.sigma_for_pad(p)
        specs = P.sign_specs(kind, ch)
        img = P.frame(kind, specs, rows, cols)
        got, ref = [], []
        for quirk in (True, False):
            got.append(values(kind, blur(ctx, kind, img, sigma, quirk, "fused")).astype(np.float64))
            assert ctx.last_engine()[0] == 6
            ref.append(np.moveaxis(P.oracle_planes(kind, specs, rows, cols, sigma, quirk), 0, -1).astype(np.float64))
        if kind in ("u8", "u16"):                           # one call: the oracle's rounding, or one level off at a tie
            want = [S.round_u8(r) if kind == "u8" else U.round_u16(r) for r in ref]
            d = (got[0] - got[1]) - (want[0].astype(np.float64) - want[1].astype(np.float64))
            assert np.abs(d).max() <= 2, "the difference of the two calls is off by %g levels" % np.abs(d).max()
        else:
            m = float(np.abs(img).max())
            d = np.abs((got[0] - got[1]) - (ref[0] - ref[1]))
            over = d - (sign_bound(kind, ref[0], m) + sign_bound(kind, ref[1], m))
            assert over.max() <= 0, "the difference of the two calls passes its bound by %.3g (max|x| = %g)" % (over.max(), m)

    for p in P.sign_pads(nkb):
        for ch in (1, 3, 4):
            if not no_float_kernel(kind, nkb, ch):
                collect(fails, "pad %d, %d ch" % (p, ch), one, p, ch)
    assert not fails, "%d cases fail:\n%s" % (len(fails), "\n".join(fails))


@pytest.mark.parametrize("kind", [k for k in P.KINDS if k != "u8"])
def test_auto_is_continuous_at_pad_104_105(ctx, kind):
    """the library's own choice on one frame either side of the boundary of ff_class_in_contract: the fused kernel at pad 104, the
    plane path at pad 105, both within the contract"""
    rows, cols = P.AUTO_BOUNDARY_SHAPE
    for p, family in P.AUTO_BOUNDARY:
        sigma = P.sigma_for_pad(p)
        for ch, specs in P.auto_boundary_frames(kind, p):
            img = P.frame(kind, specs, rows, cols)
            got = blur(ctx, kind, img, sigma, True, None)
            assert ctx.last_engine()[0] == family, (p, ch)
            check(kind, got, img, P.oracle_planes(kind, specs, rows, cols, sigma, True))


# ---- B. frames whose side is pad + 1 ---------------------------------------------------------------------------------------------------
THIN = [pytest.param(kind, nkb, end, d, quirk, id="%s-nkb%d-%s-%s-q%d" % (kind, nkb, end, ("rows", "cols")[d], quirk))
        for kind in P.KINDS for nkb in P.NKB_CLASSES for end in P.thin_ends(nkb) for d in (0, 1) for quirk in (True, False)]


@pytest.mark.parametrize("kind,nkb,end,d,quirk", THIN)
def test_thin_frames(ctx, kind, nkb, end, d, quirk):
    """(pad + 1) x (2 pad + 3) and (2 pad + 3) x (pad + 1) at both ends of the class.  The kernels stage PADA = 8 (NKB - 2) halo
    pixels: at the low end that is 7 more than the pad on either side of a frame with room for ONE reflection of pad pixels, and
    what lies beyond may only meet zero taps.  Noise and a one-pixel rim, alone and together in frames of 3 and 4 channels; the
    destination sits between guard bands.  With the quirk on and fewer than 4 columns (pads 1 and 2) FUSED refuses and the
    library's own choice is checked"""
    p = P.thin_ends(nkb)[end]
    rows, cols = P.thin_shapes(p)[d]
    fails = []
    for ch, specs in P.thin_frames(kind, nkb, p, d, quirk):
        collect(fails, "%d x %d, %d ch, %s" % (rows, cols, ch, names(specs)), run_frame, ctx, kind, nkb, p, specs, rows, cols, quirk, guard=True)
    assert not fails, "%d cases fail:\n%s" % (len(fails), "\n".join(fails))


@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("kind", P.KINDS)
def test_thin_batches_equal_single_calls(ctx, kind, quirk):
    """three thin frames as one batch: the bits of three single calls, each within the contract, guard bands intact"""
    for nkb in P.THIN_BATCH_CLASSES:
        p = P.thin_ends(nkb)["low"]
        sigma = P.sigma_for_pad(p)
        for d in (0, 1):
            rows, cols = P.thin_shapes(p)[d]
            engine, family = (None, None) if quirk and cols < 4 else ("fused", 6)
            for ch in (1, 3, 4):
                frames = P.thin_batch(kind, nkb, p, d, quirk, ch)
                imgs = np.stack([P.frame(kind, specs, rows, cols) for specs in frames])
                got = blur(ctx, kind, imgs, sigma, quirk, engine, guard=True)
                assert family is None or ctx.last_engine()[0] == family
                for i, specs in enumerate(frames):
                    single = blur(ctx, kind, imgs[i], sigma, quirk, engine, guard=True)
                    assert same_bits(got[i], single), "frame %d of the batch differs from its single call (%d x %d, %d ch)" % (i, rows, cols, ch)
                    check(kind, got[i], imgs[i], P.oracle_planes(kind, specs, rows, cols, sigma, quirk))


# ---- C. NaN and +-Inf in one frame of a batch ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("engine,family", [("fused", 6), ("fft", 0)])
@pytest.mark.parametrize("kind", P.NONFINITE_KINDS)
def test_non_finite_values_stay_in_their_frame(ctx, kind, engine, family, ch):
    """include/blur_amd.h: NaN or +-Inf in a frame gives unspecified values in that frame and no fault.  The middle frame of three
    holds one of each; the call succeeds, the frames either side are the bits of their single calls and within the contract, the
    guard bands are intact.  The middle frame is not looked at"""
    rows, cols, sigma = P.NONFINITE_SHAPE_SIGMA
    frames = P.nonfinite_frames(kind, ch)
    imgs = np.stack([P.frame(kind, specs, rows, cols) for specs in frames])
    imgs[1, 10, 20, 0] = np.nan
    imgs[1, 75, 130, ch - 1] = np.inf
    imgs[1, 140, 250, 0] = -np.inf
    got = blur(ctx, kind, imgs, sigma, True, engine, guard=True)          # (raises unless the call returns BLUR_OK)
    assert ctx.last_engine()[0] == family
    for i in (0, 2):
        single = blur(ctx, kind, imgs[i], sigma, True, engine, guard=True)
        assert same_bits(got[i], single), "frame %d differs from its single call" % i
        check(kind, got[i], imgs[i], P.oracle_planes(kind, frames[i], rows, cols, sigma, True))
