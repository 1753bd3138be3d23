"""Structured content (tests/structured.py) through every fused kernel class: fx_blur_u8 and fw_blur_u8 (1, 3 and 4 channels),
ff_blur_f32 (1, 3 and 4 channels), the plane fallback and the FFT engine, each compared with the float64 oracle under the project's
own tolerances (assert_u8_parity for bytes, |got - oracle| <= 1e-6 max|x| for float) and each asserting the engine family it ran on.

The other GPU tests are thorough about shapes and feed noise.  These feed frames on which a wrong byte wrap, a wrong float scale,
a wrong mirror or a leak between channels is a first-order error: period-2 stripes and checkers (the quirk terms at their maximum,
bytes past 255.5, the float headroom bound attained), constants at the range ends, steps and blocks (hand-off values spanning the
whole range, an edge at every phase of the tiles and strips), ramps, a bright outermost line, single pixels, one white channel.
tests/test_structured_cases.py checks on the CPU that the tie cap of assert_u8_parity cannot decide any u8 case."""
import functools

import numpy as np
import pytest

import structured as S
from conftest import assert_u8_parity
from test_gpu_gaussian_f32 import REL_TOL, sigma_for_class, sigma_for_pad

pytestmark = pytest.mark.gpu

ROWS, COLS = S.SHAPE
U8C3_FAMILY = {"fallback": 2, "fft": 0}          # the u8c3 entry at (420 x 390, pad 175 .. 200, AUTO) and at (301 x 262, sigma 6, "fft")


@functools.lru_cache(maxsize=None)
def class_sigma(nkb):
    return sigma_for_class(ROWS, COLS, nkb)


def on_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def blur_u8(ctx, img, sigma, quirk, engine):
    """[.., rows, cols, ch] uint8, out of place; 3 channels through pffft_ (fx_blur_u8 / fw_blur_u8 CH = 3), 1 and 4 through gaussian"""
    import torch
    t = on_dev(img)
    fn = ctx.pffft_ if img.shape[-1] == 3 else ctx.gaussian
    return fn(t, sigma, out=torch.empty_like(t), nyquist_quirk=quirk, engine=engine).cpu().numpy()


def blur_f32(ctx, img, sigma, quirk, engine):
    import torch
    t = on_dev(img)
    return ctx.gaussian_f32(t, sigma, out=torch.empty_like(t), nyquist_quirk=quirk, engine=engine).cpu().numpy()


def check_f32(got, want, img, what="", show=False):
    """the contract of include/blur_amd.h: |got - oracle| <= 1e-6 max|x| per pixel and channel, max|x| over the frame"""
    m = float(np.max(np.abs(img.astype(np.float64))))
    assert np.all(np.isfinite(got)), "%s: non-finite output" % what
    err = float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64)))) / m
    if show:                                                                   # the figures of DESIGN.md 2.2 (pytest -s)
        print("%s max|err| / max|x| = %.3g" % (what, err))
    assert err <= REL_TOL, "%s: max |error| / max|x| = %.3g" % (what, err)
    return err


def f32_engine(nkb):
    """(engine, family) of a float case on the library's own route: ff_blur_f32 up to NKB 15 (pad <= 104), the plane path above.
    The fused kernel reaches 1.02e-6 .. 1.11e-6 of max|x| on step frames at NKB 19, 21 and 23 and 1.19e-6 at NKB 17 with max|x| = 0.7e30
    (DESIGN.md 2.2)."""
    return ("fused", 6) if nkb <= S.FF_AUTO_MAX_NKB else (None, 0)


def ident(ch, nkb, quirk, name):
    return "c%d-nkb%d-q%d-%s" % (ch, nkb, quirk, name)


U8_SWEEP = [pytest.param(ch, nkb, quirk, i, id=ident(ch, nkb, quirk, n)) for nkb, quirk, i, n in S.class_cases("u8") for ch in (3, 1, 4)]
F32_SWEEP = [pytest.param(ch, nkb, quirk, i, id=ident(ch, nkb, quirk, n)) for nkb, quirk, i, n in S.class_cases("f32") for ch in (1, 3, 4)]


@pytest.mark.parametrize("ch,nkb,quirk,i", U8_SWEEP)
def test_u8_every_class_every_pattern(ctx, ch, nkb, quirk, i):
    """fx_blur_u8 (3 channels, NKB 3 .. 11) and fw_blur_u8 (3 channels NKB 13 .. 23; 1 and 4 channels every class)"""
    sigma = class_sigma(nkb)
    img, spec = S.u8_frame(S.patterns_for("u8", nkb), i, ch, ROWS, COLS, quirk, nkb)
    got = blur_u8(ctx, img, sigma, quirk, "fused")
    assert ctx.last_engine()[0] == 6
    want, planes = S.oracle_u8_frame(spec, ROWS, COLS, sigma, quirk)
    assert_u8_parity(got, want, planes)
    if not quirk and spec[0][0] in ("ramp_h", "ramp_v"):                       # monotone in, monotone out, exactly
        assert np.all(np.diff(got[..., 0].astype(int), axis=1 if spec[0][0] == "ramp_h" else 0) >= 0)


@pytest.mark.parametrize("ch,nkb,quirk,i", F32_SWEEP)
def test_f32_every_class_every_pattern(ctx, ch, nkb, quirk, i):
    """ff_blur_f32 of NKB 3 .. 15 and the plane fallback the library takes above; the period-2 patterns at +-0.7 attain the bound
    the frame scale is chosen by"""
    sigma = class_sigma(nkb)
    img, spec = S.f32_frame(S.patterns_for("f32", nkb), i, ch, ROWS, COLS)
    engine, family = f32_engine(nkb)
    got = blur_f32(ctx, img, sigma, quirk, engine)
    assert ctx.last_engine()[0] == family
    check_f32(got, S.oracle_f32_frame(spec, ROWS, COLS, sigma, quirk), img, ident(ch, nkb, quirk, spec[0][0]))
    if not quirk and spec[0][0] in ("ramp_h", "ramp_v"):                       # each value within the bound of a monotone plane
        d = np.diff(got[..., 0].astype(np.float64), axis=1 if spec[0][0] == "ramp_h" else 0)
        assert d.min() >= -2 * REL_TOL * float(np.max(np.abs(img)))


# ---- channel identity: one channel white, the others black ----------------------------------------------------------------------
@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("nkb", S.NKB_CLASSES)
@pytest.mark.parametrize("ch", [3, 4])
def test_u8_one_hot(ctx, ch, nkb, quirk):
    """a task that reads a neighbouring channel's quirk sums (Srow, Z, column parts) or bytes errs grossly here; with the quirk off
    the black channels are exactly 0 and the white one exactly 255"""
    sigma = class_sigma(nkb)
    for c in range(ch):
        img = S.one_hot_u8(c, ch, ROWS, COLS)
        spec = [("white" if k == c else "black", (0, 255)) for k in range(ch)]
        got = blur_u8(ctx, img, sigma, quirk, "fused")
        assert ctx.last_engine()[0] == 6
        want, planes = S.oracle_u8_frame(spec, ROWS, COLS, sigma, quirk)
        assert_u8_parity(got, want, planes)
        if not quirk:
            assert np.array_equal(got, img), "white channel %d" % c


@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("nkb", S.NKB_CLASSES)
@pytest.mark.parametrize("ch", [3, 4])
def test_f32_one_hot(ctx, ch, nkb, quirk):
    sigma = class_sigma(nkb)
    engine, family = f32_engine(nkb)
    for c in range(ch):
        img = S.one_hot_f32(c, ch, ROWS, COLS)
        spec = [("white" if k == c else "black", (np.float32(0), S.F32_HI)) for k in range(ch)]
        got = blur_f32(ctx, img, sigma, quirk, engine)
        assert ctx.last_engine()[0] == family
        check_f32(got, S.oracle_f32_frame(spec, ROWS, COLS, sigma, quirk), img, "white channel %d" % c)
        if not quirk:
            black = np.delete(got, c, axis=-1)
            assert np.all(black == 0), "white channel %d leaks into a black one" % c


# ---- the wide float kernels on request ---------------------------------------------------------------------------------------------
# ff_blur_f32 at NKB 17, 19, 21 and 23 is not the library's choice any more, but engine = "fused" still runs it.  Every pattern it holds
# the contract on stays on it; left out, by name: step_v, step_h and step_diag (measured 1.02e-6 at NKB 19, 1.11e-6 at NKB 21 and 23; NKB 17: 9.4e-7 at max|x| = 0.7, 1.19e-6 at 0.7e30).
WIDE_FUSED = [pytest.param(ch, nkb, quirk, i, id=ident(ch, nkb, quirk, n))
              for nkb in S.FF_WIDE_CLASSES for quirk in (True, False) for i, n in enumerate(S.FF_WIDE_PATTERNS) for ch in (1, 3, 4) if nkb < 23 or ch == 1]


@pytest.mark.parametrize("ch,nkb,quirk,i", WIDE_FUSED)
def test_f32_wide_fused_kernels_on_request(ctx, ch, nkb, quirk, i):
    sigma = class_sigma(nkb)
    img, spec = S.f32_frame(S.FF_WIDE_PATTERNS, i, ch, ROWS, COLS)
    got = blur_f32(ctx, img, sigma, quirk, "fused")
    assert ctx.last_engine()[0] == 6
    check_f32(got, S.oracle_f32_frame(spec, ROWS, COLS, sigma, quirk), img, ident(ch, nkb, quirk, spec[0][0]))


@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("nkb", [17, 19, 21])
@pytest.mark.parametrize("ch", [3, 4])
def test_f32_one_hot_wide_fused_kernels(ctx, ch, nkb, quirk):
    sigma = class_sigma(nkb)
    for c in range(ch):
        img = S.one_hot_f32(c, ch, ROWS, COLS)
        spec = [("white" if k == c else "black", (np.float32(0), S.F32_HI)) for k in range(ch)]
        got = blur_f32(ctx, img, sigma, quirk, "fused")
        assert ctx.last_engine()[0] == 6
        check_f32(got, S.oracle_f32_frame(spec, ROWS, COLS, sigma, quirk), img, "white channel %d" % c)
        if not quirk:
            assert np.all(np.delete(got, c, axis=-1) == 0), "white channel %d leaks into a black one" % c


# ---- both sides of every policy switch see the same content ---------------------------------------------------------------------
@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("route", ["fallback", "fft"])
@pytest.mark.parametrize("ch", [1, 3, 4])
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_plane_fallback_and_fft_engine(ctx, kind, ch, route, quirk):
    """pad > 168 under the library's choice (no fused kernel) and engine = "fft" at a pad the fused kernels take"""
    if route == "fallback":
        rows, cols = S.FALLBACK_SHAPE
        sigma, engine = sigma_for_pad(rows, cols, *S.FALLBACK_PAD), None
    else:
        rows, cols, sigma = S.FFT_SHAPE_SIGMA
        engine = "fft"
    # u8 with 3 channels is the u8c3 entry, whose other engines have families of their own; everything else reports 0
    family = U8C3_FAMILY[route] if kind == "u8" and ch == 3 else 0
    names = S.SWITCH_PATTERNS
    for i in range(len(names)):
        if kind == "u8":
            img, spec = S.u8_frame(names, i, ch, rows, cols, quirk, (rows, cols))
            got = blur_u8(ctx, img, sigma, quirk, engine)
            assert ctx.last_engine()[0] == family
            want, planes = S.oracle_u8_frame(spec, rows, cols, sigma, quirk)
            assert_u8_parity(got, want, planes)
        else:
            img, spec = S.f32_frame(names, i, ch, rows, cols)
            got = blur_f32(ctx, img, sigma, quirk, engine)
            assert ctx.last_engine()[0] == family
            check_f32(got, S.oracle_f32_frame(spec, rows, cols, sigma, quirk), img, names[i])


# ---- segments and strips ----------------------------------------------------------------------------------------------------------
SEGMENT_CASES = [("u8",) + s for s in S.SEGMENT_SHAPES] + [("f32",) + s for s in S.SEGMENT_SHAPES_F32]


@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("ch", [1, 3, 4])
@pytest.mark.parametrize("kind,rows,cols,sigma", SEGMENT_CASES, ids=["%s-%dx%d-s%g" % c for c in SEGMENT_CASES])
def test_segments_strips_and_batch(ctx, kind, rows, cols, sigma, ch, quirk):
    """a tall narrow frame (cut into segments of tiles when it is blurred alone) and a wide short one (many strips), alone and as
    frames of a batch of 3 (whole strips): each against the oracle, not only against the single call.  The float wide frame runs
    at sigma 30 on ff_blur_f32 and at sigma 40 (pad > 104) on the plane path the library takes there."""
    import blur_algorithms_amd as B
    names = S.SEGMENT_PATTERNS
    frames, wants = [], []
    for i in range(len(names)):
        if kind == "u8":
            img, spec = S.u8_frame(names, i, ch, rows, cols, quirk, (rows, cols))
            wants.append(S.oracle_u8_frame(spec, rows, cols, sigma, quirk))
        else:
            img, spec = S.f32_frame(names, i, ch, rows, cols)
            wants.append(S.oracle_f32_frame(spec, rows, cols, sigma, quirk))
        frames.append(img)
    blur = blur_u8 if kind == "u8" else blur_f32
    fused = kind == "u8" or B.pffft_sizing(rows, cols, sigma)["pad"] <= 8 * (S.FF_AUTO_MAX_NKB - 2)
    engine, family = ("fused", 6) if fused else (None, 0)
    singles = []
    for img in frames:
        singles.append(blur(ctx, img, sigma, quirk, engine))
        assert ctx.last_engine()[0] == family
    batch = blur(ctx, np.stack(frames), sigma, quirk, engine)
    assert ctx.last_engine()[0] == family
    for i, img in enumerate(frames):
        for how, got in (("alone", singles[i]), ("in the batch", batch[i])):
            if kind == "u8":
                assert_u8_parity(got, wants[i][0], wants[i][1])
            else:
                check_f32(got, wants[i], img, "%s %s" % (names[i], how))


# ---- float magnitude ends ---------------------------------------------------------------------------------------------------------
MAG_NAMES = S.MAGNITUDE_PATTERNS + ("checker",)             # the channels of the 3-channel frames rotate through these
# one narrow and one wide class of ff_blur_f32, and the plane path the library takes at NKB 19
MAG_ROUTES = [(nkb,) + f32_engine(nkb) for nkb in S.MAGNITUDE_CLASSES + (19,)]


@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("nkb,engine,family", MAG_ROUTES, ids=["nkb%d-family%d" % (r[0], r[2]) for r in MAG_ROUTES])
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("name", S.MAGNITUDE_PATTERNS)
@pytest.mark.parametrize("mag", S.MAGNITUDES, ids=["m%g" % m for m in S.MAGNITUDES])
def test_f32_magnitude_ends(ctx, mag, name, ch, nkb, engine, family, quirk):
    """cols2 at +-0.7 m and step_diag at -m / 3 .. 0.7 m, m from 1e-37 (the clamp e = 125 of the fused kernel's scale exponent is
    active: 0.7e-37 2^125 is about 3, far under the 2^13 the scale aims at) to 1e37, on both routes.  Observed figures (pytest -s):
    DESIGN.md section 2.2."""
    sigma = class_sigma(nkb)
    img, spec = S.f32_frame(MAG_NAMES, MAG_NAMES.index(name), ch, ROWS, COLS, mag)
    got = blur_f32(ctx, img, sigma, quirk, engine)
    assert ctx.last_engine()[0] == family
    check_f32(got, S.oracle_f32_frame(spec, ROWS, COLS, sigma, quirk, mag), img, "m=%g %s c%d nkb%d q%d" % (mag, name, ch, nkb, quirk), show=True)


TOP_NAMES = S.HEADROOM + ("step_diag",)
# (nkb, engine, family, the patterns the channels rotate through, channel 0's pattern): the classes of the magnitude test on their
# route, and the wide kernels on request (without the step frame, as above)
TOP_CASES = [(nkb,) + f32_engine(nkb) + (TOP_NAMES, n) for nkb in S.MAGNITUDE_CLASSES + (19,) for n in TOP_NAMES]
TOP_CASES += [(nkb, "fused", 6, S.HEADROOM, n) for nkb in (17, 19, 21) for n in S.HEADROOM]


@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("nkb,engine,family,names,name", TOP_CASES, ids=["nkb%d-family%d-%s" % (c[0], c[2], c[4]) for c in TOP_CASES])
def test_f32_top_of_the_scale_interval(ctx, nkb, engine, family, names, name, ch, quirk):
    """max|x| = 0.9999: x s sits at the top of the binade the frame scale aims at, where the headroom to binary16's range is
    smallest.  With the quirk off B = 1 and the staged values themselves reach 0.9999 2^14."""
    sigma = class_sigma(nkb)
    spec = [(n, S.f32_top_levels(n)) for n in S.channel_patterns(names, names.index(name), ch)]
    img = np.stack([S.f32_plane(n, ROWS, COLS, lv) for n, lv in spec], axis=-1)
    got = blur_f32(ctx, img, sigma, quirk, engine)
    assert ctx.last_engine()[0] == family
    check_f32(got, S.oracle_f32_frame(spec, ROWS, COLS, sigma, quirk), img, "top %s c%d nkb%d q%d" % (name, ch, nkb, quirk))
