"""The parity rule of blur_gaussian_u16_* and the test content that goes with it.  Plain module: helpers, no tests, no GPU.

The rule (assert_u16_parity): with w the float64 oracle plane (oracle.pffft_plane_f64 of the channel widened to float32, which is
exact for u16) the expected sample is int(trunc(w + 0.5)) mod 65536: add 0.5, truncate towards zero, keep the low 16 bits, no
clamping.  A sample must equal it, except where w + 0.5 lies within TIE_TOL_U16 of an integer; there it may be off by exactly one
level, compared modulo 65536 (65535 and 0 are one level apart, as 255 and 0 are for u8).

TIE_TOL_U16 = 1e-6 * 65535 + 2^-9 = 0.0675 grey levels.  1e-6 of full scale is the float entry's contract (include/blur_amd.h), met
by both routes the library's own choice can take; 2^-9 is half a float32 ulp at 65535, because pffft_plane_f64 returns its float64
result rounded to float32.  Neither comes from the code under test.

That tolerance is wide (a noise frame has 2 x 0.0675 = 13.5 % of its samples inside it), so the rule's power comes from the samples
outside it, which must match exactly.  Hence the condition on every case: the share of samples the rule excuses is at most
EXCUSED_CAP, asserted in assert_u16_parity and proven for the oracle alone, per case, by tests/test_u16_cases.py."""
import numpy as np

import structured as S

TIE_TOL_U16 = 1e-6 * 65535 + 2.0 ** -9
EXCUSED_CAP = 0.40
SHAPE = S.SHAPE
NKB_CLASSES = S.NKB_CLASSES


def round_u16(planes):
    """int(trunc(w + 0.5)) mod 65536 of float planes, any shape -> uint16"""
    w = np.asarray(planes, np.float64) + 0.5
    return (np.trunc(w).astype(np.int64) % 65536).astype(np.uint16)


def excused(planes):
    """where the rule lets a sample be one level off: w + 0.5 within TIE_TOL_U16 of an integer"""
    w = np.asarray(planes, np.float64) + 0.5
    return np.abs(w - np.round(w)) <= TIE_TOL_U16


def excused_share(planes):
    return float(excused(planes).mean())


def assert_u16_parity(got, want_planes):
    """got: [rows, cols, ch] (or [rows, cols]) uint16; want_planes: [ch, rows, cols] (or [rows, cols]) oracle planes before rounding.
    Returns the number of samples that used the tie rule."""
    got = np.asarray(got)
    assert got.dtype == np.uint16
    planes = np.asarray(want_planes, np.float64)
    if planes.ndim == 2:
        planes = planes[None]
    if got.ndim == 2:
        got = got[..., None]
    planes = np.moveaxis(planes, 0, -1)
    assert got.shape == planes.shape, (got.shape, planes.shape)
    exc = excused(planes)
    share = float(exc.mean())
    assert share <= EXCUSED_CAP, "the case excuses %.3f of its samples (cap %.2f): replace the case" % (share, EXCUSED_CAP)
    diff = (got.astype(np.int64) - round_u16(planes).astype(np.int64) + 32768) % 65536 - 32768      # 65535 <-> 0: one level
    mism = diff != 0
    if not mism.any():
        return 0
    bad = mism & ~exc
    if bad.any():
        w = planes + 0.5
        dist = np.abs(w - np.round(w))
        i = np.unravel_index(np.argmax(np.where(bad, np.abs(diff), 0)), bad.shape)
        raise AssertionError("%d u16 samples differ from the oracle away from a rounding tie: worst at %s got %d, oracle plane %.4f "
                             "(distance %.4f from a tie, tolerance %.4f)" % (int(bad.sum()), i, int(got[i]), planes[i], dist[i], TIE_TOL_U16))
    assert np.abs(diff[mism]).max() <= 1, "u16 output differs from the oracle by more than one level at a tie"
    return int(mism.sum())


# ---- content ---------------------------------------------------------------------------------------------------------------------
def noise(seed, rows, cols, top=65535):
    """uniform noise 0 .. top (65535: the full range; 4095: a 12-bit sensor in a u16)"""
    return np.random.default_rng(seed).integers(0, top + 1, (rows, cols), dtype=np.uint16)


def ramp(rows, cols):
    y = np.arange(rows, dtype=np.int64)[:, None]
    x = np.arange(cols, dtype=np.int64)[None, :]
    return ((126 * x + y) % 65536).astype(np.uint16)


def two_level(name, rows, cols, lo, hi):
    return (lo + S.pattern(name, rows, cols) * (hi - lo)).astype(np.uint16)


def impulse(rows, cols, level=65535):
    p = np.zeros((rows, cols), np.uint16)
    p[rows // 2, cols // 2] = level
    return p


# name -> (pattern of structured.py, default (lo, hi)); the levels follow the measurements that chose them: period-2 patterns need
# an even sum of their two levels (a 0 / 65535 checker blurs to k + 0.5 with the quirk off: every sample a true tie)
CASES = {
    "blocks": ("blocks", (0, 60001)),
    "step_v": ("step_v", (0, 65533)),
    "step_h": ("step_h", (0, 45874)),
    "step_diag": ("step_diag", (0, 65533)),
    "rim": ("rim", (0, 65535)),
    "const_top": ("white", (0, 65535)),
    "const_65533": ("white", (0, 65533)),
    "const_45874": ("white", (0, 45874)),
    "cols2": ("cols2", (0, 65534)),
    "rows2": ("rows2", (0, 65534)),
    "checker": ("checker", (0, 65534)),
}
GENERATORS = {"ramp": ramp, "impulse": impulse}
STEPS = ("step_v", "step_h", "step_diag")
CANDIDATES = ("ramp", "blocks", "step_v", "step_h", "step_diag", "impulse", "rim", "const_top", "const_65533", "const_45874", "cols2", "rows2",
              "checker")

# (case, window class, quirk) whose oracle plane at the default levels excuses more than EXCUSED_CAP of its samples on the SHAPE frame
# at the class's sigma, and the levels that replace them there (tests/test_u16_cases.py measures every case at its default levels,
# holds this table to exactly the ones over the cap, and proves the replacements).  Excused share at the default levels:
LEVEL_OVERRIDES = {
    ("rim", 3, True): (0, 65000),                          # 0.49
    ("rim", 5, True): (0, 65000),                          # 0.87
    ("step_v", 5, True): (0, 65000),                       # 0.48
    ("const_top", 5, True): (0, 65000),                    # 0.50
    ("const_65533", 5, True): (0, 60001),                  # 0.50
    ("cols2", 17, False): (0, 50000),                      # 1.00 (also at 64000 .. 65534)
    ("rows2", 17, False): (0, 50000),                      # 1.00
    ("blocks", 19, False): (0, 65534),                     # 0.47
}


def case_levels(name, nkb=None, quirk=True):
    """the (lo, hi) of a two-level case in window class nkb (None: the default levels); None for ramp and impulse"""
    if name not in CASES:
        return None
    return LEVEL_OVERRIDES.get((name, nkb, bool(quirk)), CASES[name][1])


def plane(name, rows, cols, levels=None):
    if name in GENERATORS:
        return np.ascontiguousarray(GENERATORS[name](rows, cols))
    lo, hi = CASES[name][1] if levels is None else levels
    return np.ascontiguousarray(two_level(CASES[name][0], rows, cols, lo, hi))


def class_patterns(nkb, quirk):
    """every case runs in every class (LEVEL_OVERRIDES changes levels, it drops nothing)"""
    return CANDIDATES


def class_sigma(nkb):
    """a sigma in the upper half of window class nkb on the SHAPE frame (pads 8 (nkb - 4) + 1 .. 8 (nkb - 2)); host code only"""
    import blur_algorithms_amd as B
    lo, hi = (1, 8) if nkb == 3 else (8 * (nkb - 4) + 1, 8 * (nkb - 2))
    lo = (lo + hi) // 2
    s = 0.5
    while s < 200:
        pad = B.pffft_sizing(SHAPE[0], SHAPE[1], s)["pad"]
        if lo <= pad <= hi:
            return s
        s += 0.05 if pad < lo else -0.01
    raise AssertionError("no sigma for class %d" % nkb)


def oracle_plane(p, sigma, quirk, key=None):
    """float32 oracle plane of a u16 plane (widened to float32: exact)"""
    return S.oracle_plane(np.asarray(p, np.float32), sigma, quirk, None if key is None else ("u16",) + tuple(key))


def oracle_named(name, rows, cols, sigma, quirk, levels=None):
    return oracle_plane(plane(name, rows, cols, levels), sigma, quirk, (name, levels, rows, cols))


def oracle_frame(img, sigma, quirk):
    """img [rows, cols, ch] uint16 -> planes [ch, rows, cols]"""
    return np.stack([oracle_plane(img[..., c], sigma, quirk) for c in range(img.shape[2])])
