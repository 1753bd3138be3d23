"""The parity rule of blur_gaussian_f16_* / blur_gaussian_bf16_* and the test content that goes with it.  Plain module: helpers, no
tests, no GPU.

The rule (assert_half_parity): ref = the float64 oracle plane (oracle.pffft_plane_f64 of the channel widened to float32, exact for
both types), m = max|x| of the frame, tol = 1e-6 m + 1/2 ulp_f32(ref): the float entry's contract (include/blur_amd.h) plus the
oracle's own return rounding (pffft_plane_f64 returns its float64 result rounded to float32).  Rounding is monotone, so a correct
output lies in an interval of the sample type:

    RN_T(ref - tol) <= got <= RN_T(ref + tol)         RN_T: float64 -> T, to nearest even, overflow to +-Inf

A sample is ambiguous where the two ends differ; everywhere else the output must be the correctly rounded reference, bit for bit
(-0 and +0 compare equal).  The rule is only as strong as its unambiguous samples, hence the condition on every case: the ambiguous
share is at most AMBIGUOUS_CAP, asserted in assert_half_parity and proven for the oracle alone, per case, by
tests/test_half_cases.py.  Neither the tolerance nor the cap comes from the code under test."""
import numpy as np

import structured as S

F16, BF16 = "f16", "bf16"
TYPES = (F16, BF16)
AMBIGUOUS_CAP = 0.05
REL_TOL = 1e-6
SHAPE = S.SHAPE
NKB_CLASSES = S.NKB_CLASSES
F16_MAX = 65504.0
BF16_MAX = float(np.float32(3.3895313892515355e38))           # 0x7f7f


# ---- RN_T ------------------------------------------------------------------------------------------------------------------------
def rn_f16(x):
    """float64 -> the nearest binary16 value (ties to even, subnormals, overflow to +-Inf), as float64.  numpy converts double to
    half in one rounding"""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def rn_bf16(x):
    """float64 -> the nearest bfloat16 value in ONE rounding (not through float32), as float64.  Normal range: the 52-bit fraction
    rounded to 7 bits on the bit pattern (a carry moves into the exponent, as it must); below 2^-126: multiples of 2^-133"""
    x = np.asarray(x, np.float64)
    shape = x.shape
    x = np.ascontiguousarray(x).reshape(-1)
    bits = x.view(np.uint64)
    r = bits + np.uint64((1 << 44) - 1) + ((bits >> np.uint64(45)) & np.uint64(1))
    r = (r >> np.uint64(45)) << np.uint64(45)
    with np.errstate(invalid="ignore", over="ignore"):
        normal = r.view(np.float64)
        sub = np.rint(x * 2.0 ** 133) * 2.0 ** -133
        out = np.where(np.abs(x) < 2.0 ** -126, sub, normal)
        out = np.where(np.abs(out) >= 2.0 ** 128, np.copysign(np.inf, x), out)
    return np.where(np.isfinite(x), out, x).reshape(shape)


def rn(kind, x):
    return rn_f16(x) if kind == F16 else rn_bf16(x)


def to_bits(kind, x):
    """values that ARE representable in the type (float64 / float32) -> their uint16 bit patterns"""
    x = np.asarray(x)
    if kind == F16:
        return x.astype(np.float16).view(np.uint16)
    return (np.ascontiguousarray(x.astype(np.float32)).view(np.uint32) >> 16).astype(np.uint16)


def from_bits(kind, bits):
    """uint16 bit patterns -> float32 values (exact)"""
    bits = np.ascontiguousarray(bits, np.uint16)
    if kind == F16:
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << 16).view(np.float32)


def quantise(kind, x):
    """any array -> float32 values representable in the type (the inputs are quantised first: the oracle sees what the kernel sees)"""
    return rn(kind, np.asarray(x, np.float64)).astype(np.float32)


def ulp(kind, x):
    """the spacing of the type at |x| (subnormal spacing below the normal range)"""
    e = np.floor(np.log2(np.maximum(np.abs(np.asarray(x, np.float64)), 1e-300)))
    if kind == F16:
        return 2.0 ** (np.maximum(e, -14) - 10)
    return 2.0 ** (np.maximum(e, -126) - 7)


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def tolerance(ref, maxabs):
    ref32 = np.asarray(ref, np.float32)
    return REL_TOL * float(maxabs) + 0.5 * np.spacing(np.abs(ref32)).astype(np.float64)


def interval(kind, ref, maxabs):
    ref = np.asarray(ref, np.float64)
    tol = tolerance(ref, maxabs)
    return rn(kind, ref - tol), rn(kind, ref + tol)


def ambiguous_share(kind, ref, maxabs):
    lo, hi = interval(kind, ref, maxabs)
    return float((lo != hi).mean())


def assert_half_parity(kind, got, want_planes, maxabs, verbose=False):
    """got: [rows, cols, ch] (or [rows, cols]) values of the type (float16 array, or float32 / float64 holding the widened samples);
    want_planes: [ch, rows, cols] (or [rows, cols]) oracle planes; maxabs: max|x| of the input frame.  Returns the number of
    ambiguous samples."""
    got = np.asarray(got).astype(np.float64)
    planes = np.asarray(want_planes, np.float64)
    if planes.ndim == 2:
        planes = planes[None]
    if got.ndim == 2:
        got = got[..., None]
    planes = np.moveaxis(planes, 0, -1)
    assert got.shape == planes.shape, (got.shape, planes.shape)
    lo, hi = interval(kind, planes, maxabs)
    amb = lo != hi
    share = float(amb.mean())
    if verbose:
        with np.errstate(invalid="ignore"):
            err = np.where(np.isfinite(got), np.abs(got - planes), 0.0)
        print("half parity %s: ambiguous share %.4f, worst |got - ref| / m %.3g" % (kind, share, float(err.max()) / max(float(maxabs), 1e-300)))
    assert share <= AMBIGUOUS_CAP, "the case has %.3f ambiguous samples (cap %.2f): replace the case" % (share, AMBIGUOUS_CAP)
    with np.errstate(invalid="ignore"):
        bad = ~((lo <= got) & (got <= hi))
    if bad.any():
        with np.errstate(invalid="ignore"):
            d = np.where(bad, np.maximum(lo - got, got - hi), 0.0)
        d = np.where(np.isnan(d), np.inf, d)
        i = np.unravel_index(np.argmax(d), d.shape)
        raise AssertionError("%d %s samples outside [RN(ref - tol), RN(ref + tol)]: worst at %s got %r, interval [%r, %r], oracle %r (m = %g)"
                             % (int(bad.sum()), kind, i, got[i], lo[i], hi[i], planes[i], maxabs))
    return int(amb.sum())


def assert_float_side(kind, got, want_planes, maxabs):
    """the optional float-side check for small-output content: |float(got) - ref| <= tol + ulp_T(ref)"""
    got = np.asarray(got).astype(np.float64)
    planes = np.asarray(want_planes, np.float64)
    if planes.ndim == 2:
        planes = planes[None]
    if got.ndim == 2:
        got = got[..., None]
    planes = np.moveaxis(planes, 0, -1)
    bound = tolerance(planes, maxabs) + ulp(kind, planes)
    assert np.all(np.abs(got - planes) <= bound)


# ---- content (all of it quantised to the type) -------------------------------------------------------------------------------------
def noise(kind, seed, rows, cols, top=1.0):
    """uniform noise in [0, top]: non-negative (zero-mean noise blurs to values far below max|x|, where every sample is ambiguous)"""
    return quantise(kind, np.random.default_rng(seed).random((rows, cols)) * top)


# the structured table: structured.PATTERNS + impulses at -1/3 .. 0.7; the period-2 patterns at +-0.7 (the headroom bound of the
# scale) with the quirk on only: with the quirk off they blur to about 0, far below max|x|, and every sample is ambiguous
CANDIDATES = S.PATTERNS + ("impulses",)


def default_levels(name, quirk):
    if name in S.HEADROOM and quirk:
        return (float(-S.F32_HI), float(S.F32_HI))
    return (float(S.F32_LO), float(S.F32_HI))


# (case, window class, quirk, type) whose oracle plane at the default levels has more than AMBIGUOUS_CAP ambiguous samples on the
# SHAPE frame at the class's sigma, and the levels that replace them there (tests/test_half_cases.py measures every case at its
# default levels, holds this table to exactly the ones over the cap, and proves the replacements).  Share at the default levels:
LEVEL_OVERRIDES = {
}


def case_levels(name, nkb, quirk, kind):
    return LEVEL_OVERRIDES.get((name, nkb, bool(quirk), kind), default_levels(name, quirk))


def plane(kind, name, rows, cols, levels):
    return quantise(kind, S.f32_plane(name, rows, cols, (np.float64(levels[0]), np.float64(levels[1]))))


def class_sigma(nkb):
    import u16_parity as U
    return U.class_sigma(nkb)


def oracle_plane(p, sigma, quirk, key=None):
    return S.oracle_plane(np.asarray(p, np.float32), sigma, quirk, None if key is None else ("half",) + tuple(key))


def oracle_named(kind, name, rows, cols, sigma, quirk, levels):
    return oracle_plane(plane(kind, name, rows, cols, levels), sigma, quirk, (kind, name, tuple(levels), rows, cols))


def oracle_frame(img, sigma, quirk):
    """img [rows, cols, ch] float32 (values of the type) -> planes [ch, rows, cols]"""
    return np.stack([oracle_plane(img[..., c], sigma, quirk) for c in range(img.shape[2])])


def scale_exp(maxabs, bscale):
    """ff_kernels.hpp: ff_scale_exp"""
    import math
    maxabs = float(np.float32(maxabs))
    if not maxabs > 0:
        return 0
    _, k = math.frexp(maxabs * bscale)
    return min(max(14 - k, -125), 125)
