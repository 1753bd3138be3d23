"""Structured test content for the fused kernels: deterministic pattern generators, the levels they are mapped to, the table of
cases the CPU and GPU tests share, and a cache of float64 oracle planes.

Uniform noise under a Gaussian collapses to a near-constant, so a whole class of errors cannot show on it: values at and past
the ends of the byte range (the Nyquist quirk takes the oracle outside [0, 255]), the float kernel's headroom bound (only a frame
whose columns alternate +max, -max attains |Srow| = (cols + 2 pad) max|x|), hand-off values spanning the whole range, a wrong
mirror at a border, a channel reading its neighbour's sums.  The patterns below make each of those a first-order error.

Plain module: no fixtures, no GPU.  tests/test_structured_cases.py checks the table itself (generators, tie share of every u8
case, finiteness of every float case); tests/test_gpu_structured.py runs it on the kernels."""
import collections

import numpy as np

SHAPE = (397, 517)                   # the ragged frame of the window-class sweeps: not a multiple of 4, 32 or 128 either way
NKB_CLASSES = (3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23)
TIE_CAP = 2e-3                       # assert_u8_parity's cap on the share of mismatching bytes


def impulse_points(rows, cols):
    """the four corners, either side of the first tile / strip boundary, mid-frame, and the first and last row / column of the
    ragged last tile and strip"""
    pts = [(0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1), (rows // 2, cols // 2)]
    pts += [p for p in ((31, 127), (32, 128)) if p[0] < rows and p[1] < cols]
    ty, tx = 32 * ((rows - 1) // 32), 128 * ((cols - 1) // 128)
    pts += [(ty, tx), (rows - 1, (tx + cols) // 2), ((ty + rows) // 2, cols - 1)]
    return sorted(set(pts))


def _ring(rows, cols, d):
    p = np.zeros((rows, cols))
    p[d, d:cols - d] = p[rows - 1 - d, d:cols - d] = 1
    p[d:rows - d, d] = p[d:rows - d, cols - 1 - d] = 1
    return p


def _gen(name, rows, cols):
    y = np.arange(rows)[:, None]
    x = np.arange(cols)[None, :]
    if name == "cols2":
        return np.broadcast_to(x & 1, (rows, cols))
    if name == "rows2":
        return np.broadcast_to(y & 1, (rows, cols))
    if name == "checker":
        return (x + y) & 1
    if name == "white":
        return np.ones((rows, cols))
    if name == "black":
        return np.zeros((rows, cols))
    if name == "step_v":                                   # a vertical edge
        return np.broadcast_to(x >= cols // 2, (rows, cols))
    if name == "step_h":
        return np.broadcast_to(y >= rows // 2, (rows, cols))
    if name == "step_diag":                                # corner to corner: the edge crosses every tile row and strip
        return x * rows >= y * cols
    if name == "blocks":                                   # squares of side 32, origin shifted by (5, 7)
        return (((y + 5) // 32) + ((x + 7) // 32)) & 1
    if name == "ramp_h":
        return np.broadcast_to(x / (cols - 1), (rows, cols))
    if name == "ramp_v":
        return np.broadcast_to(y / (rows - 1), (rows, cols))
    if name == "rim":
        return _ring(rows, cols, 0)
    if name == "rim2":
        return _ring(rows, cols, 1)
    if name == "impulses":
        p = np.zeros((rows, cols))
        for r, c in impulse_points(rows, cols):
            p[r, c] = 1
        return p
    raise KeyError(name)


def pattern(name, rows, cols):
    """[rows, cols] float64 in 0 .. 1"""
    return np.ascontiguousarray(_gen(name, rows, cols), dtype=np.float64)


TWO_LEVEL = ("cols2", "rows2", "checker", "step_v", "step_h", "step_diag", "blocks", "rim", "rim2", "impulses")
HEADROOM = ("cols2", "rows2", "checker")                   # period 2: the quirk terms at their maximum
PATTERNS = ("cols2", "rows2", "checker", "white", "black", "step_v", "step_h", "step_diag", "blocks", "ramp_h", "ramp_v", "rim",
            "rim2")
# what every class keeps if the product is ever trimmed (the sweeps below are complete)
CORE = ("cols2", "rows2", "checker", "white", "step_diag", "rim")


def patterns_for(kind, nkb):
    """the patterns of one window class.  `impulses` tests the tap table itself: float always; u8 only at NKB 3 and 5 (at
    sigma 20 a 255 impulse peaks at 0.34 grey levels)"""
    return PATTERNS + (("impulses",) if kind == "f32" or nkb <= 5 else ())


# ---- levels ------------------------------------------------------------------------------------------------------------------
# Cases whose oracle plane at the default levels has more rounding ties than assert_u8_parity's cap lets through (they blur to
# 127.5 over an area: tests/test_structured_cases.py measures every case).  They keep their place in the table at other levels.
# (pattern, where, quirk) with `where` the window class of the sweep or the (rows, cols) of another frame; tie share at 0 / 255:
U8_LEVEL_OVERRIDES = {
    ("checker", 23, True): (1, 255),                       # 0.25
    ("blocks", (180, 1500), True): (1, 255),               # over the cap at sigma 40 (9.3e-3 at sigma 52)
    ("blocks", (420, 390), True): (1, 255),                # 1.5e-2 (pad 175 .. 200)
}


def u8_levels(name, quirk, where=None):
    """0 / 255 with the quirk on (the oracle leaves [0, 255]: 256.04 wraps to 0).  With the quirk off a 0 / 255 checker blurs to
    exactly 127.5, every pixel a rounding tie, so two-level and ramp frames take 0 / 254 there; constants keep 255."""
    if (name, where, bool(quirk)) in U8_LEVEL_OVERRIDES:
        return U8_LEVEL_OVERRIDES[(name, where, bool(quirk))]
    return (0, 255) if quirk or name in ("white", "black") else (0, 254)


F32_LO, F32_HI = np.float32(-1.0 / 3.0), np.float32(0.7)   # not dyadic: x s keeps a non-zero `lo` half after the 2^e scale


def f32_levels(name):
    """+-0.7 for the period-2 patterns (the headroom bound is attained only by +max, -max), -1/3 .. 0.7 for the rest"""
    return (-F32_HI, F32_HI) if name in HEADROOM else (F32_LO, F32_HI)


def u8_plane(name, rows, cols, levels):
    lo, hi = levels
    return np.rint(lo + pattern(name, rows, cols) * (hi - lo)).astype(np.uint8)


# the top of the scale interval: max|x| s lies in [2^13, 2^14), and 0.9999 puts it at 0.9999 2^14.  A scale aiming two binades too
# high then takes x s past binary16's largest finite value (65504) in the staging itself; +-0.7 (1.4 2^13) would still fit.
F32_TOP = np.float32(0.9999)


def f32_top_levels(name):
    return (-F32_TOP, F32_TOP) if name in HEADROOM else (F32_LO, F32_TOP)


def f32_plane(name, rows, cols, levels, mag=1.0):
    """levels are float32 values; the magnitude multiplies in float64 and rounds once"""
    lo, hi = np.float64(levels[0]), np.float64(levels[1])
    return ((lo + pattern(name, rows, cols) * (hi - lo)) * np.float64(mag)).astype(np.float32)


# ---- frames: channel c of case i takes pattern (i + c) mod P, so no two channels of a frame agree ------------------------------
def channel_patterns(names, i, ch):
    return [names[(i + c) % len(names)] for c in range(ch)]


def u8_frame(names, i, ch, rows, cols, quirk, where=None):
    """-> (frame [rows, cols, ch] uint8, [(pattern, levels)] per channel)"""
    spec = [(n, u8_levels(n, quirk, where)) for n in channel_patterns(names, i, ch)]
    return np.stack([u8_plane(n, rows, cols, lv) for n, lv in spec], axis=-1), spec


def f32_frame(names, i, ch, rows, cols, mag=1.0):
    spec = [(n, f32_levels(n)) for n in channel_patterns(names, i, ch)]
    return np.stack([f32_plane(n, rows, cols, lv, mag) for n, lv in spec], axis=-1), spec


def one_hot_u8(c, ch, rows, cols):
    f = np.zeros((rows, cols, ch), np.uint8)
    f[..., c] = 255
    return f


def one_hot_f32(c, ch, rows, cols, mag=1.0):
    f = np.zeros((rows, cols, ch), np.float32)
    f[..., c] = np.float32(np.float64(F32_HI) * mag)
    return f


# ---- the oracle, one plane at a time, cached so that channel counts and kernel families share planes ----------------------------
_planes = collections.OrderedDict()
_PLANES_KEPT = 96                    # about 80 MB; the sweeps order their cases so that the frames sharing a plane follow each other


def oracle_plane(plane, sigma, quirk, key=None):
    """float32 plane (the oracle's value before any rounding to bytes) of a float32 / uint8 input plane.  `key` names the input
    ((pattern, levels, shape, magnitude)); without one the plane is computed and not kept."""
    from oracle import oracle as O
    k = None if key is None else (key, float(sigma), bool(quirk))
    if k is not None and k in _planes:
        _planes.move_to_end(k)
        return _planes[k]
    out = O.pffft_plane_f64(np.asarray(plane, np.float32), sigma, quirk)
    if k is not None:
        _planes[k] = out
        while len(_planes) > _PLANES_KEPT:
            _planes.popitem(last=False)
    return out


def oracle_u8(name, levels, rows, cols, sigma, quirk):
    return oracle_plane(u8_plane(name, rows, cols, levels), sigma, quirk, ("u8", name, tuple(levels), rows, cols))


def oracle_f32(name, levels, rows, cols, sigma, quirk, mag=1.0):
    """computed directly at every magnitude (not scaled from the magnitude-1 plane)"""
    key = ("f32", name, (float(levels[0]), float(levels[1])), rows, cols, float(mag))
    return oracle_plane(f32_plane(name, rows, cols, levels, mag), sigma, quirk, key)


def oracle_u8_frame(spec, rows, cols, sigma, quirk):
    """-> (bytes [rows, cols, ch], planes [ch, rows, cols]) as assert_u8_parity takes them"""
    planes = np.stack([oracle_u8(n, lv, rows, cols, sigma, quirk) for n, lv in spec])
    return np.moveaxis(round_u8(planes), 0, -1), planes


def oracle_f32_frame(spec, rows, cols, sigma, quirk, mag=1.0):
    return np.stack([oracle_f32(n, lv, rows, cols, sigma, quirk, mag) for n, lv in spec], axis=-1)


def round_u8(planes):
    """(uint8_t)(v + 0.5f) as the reference, the oracle and the kernels do it: out-of-range values wrap"""
    return ((np.asarray(planes, np.float32) + np.float32(0.5)).astype(np.int64) & 0xff).astype(np.uint8)


def tie_share(plane, tol):
    """share of pixels whose oracle value lies within tol of a rounding boundary k + 0.5"""
    v = np.asarray(plane, np.float64) + 0.5
    return float((np.abs(v - np.round(v)) <= tol).mean())


# ---- the case table ------------------------------------------------------------------------------------------------------------
# beyond the class sweep: (rows, cols, sigma) of the frames cut into segments (tall and narrow), of many strips (wide and short)
SEGMENT_SHAPES = ((2500, 140, 20.0), (180, 1500, 40.0))
# float: the wide frame at sigma 30 as well (pad <= 104: ff_blur_f32 under the library's choice; sigma 40 is the plane path)
SEGMENT_SHAPES_F32 = SEGMENT_SHAPES + ((180, 1500, 30.0),)
# ff_blur_f32 is the library's choice up to this class; the classes above run on request only, on every pattern but the steps
FF_AUTO_MAX_NKB = 15
FF_WIDE_CLASSES = (17, 19, 21, 23)
FF_WIDE_PATTERNS = tuple(n for n in PATTERNS + ("impulses",) if n not in ("step_v", "step_h", "step_diag"))
SEGMENT_PATTERNS = ("blocks", "step_diag", "rim")
# the policy switches: the plane fallback (pad > 168) and engine = "fft"
FALLBACK_SHAPE = (420, 390)
FALLBACK_PAD = (175, 200)
FFT_SHAPE_SIGMA = (301, 262, 6.0)
SWITCH_PATTERNS = ("cols2", "checker", "white", "step_diag", "rim", "blocks")
# float magnitude ends: at 1e-37 the scale exponent's clamp e = 125 is active; 0.7e37 * 1.0003 stays inside float32
MAGNITUDES = (1e-37, 1e-30, 1.0, 1e30, 1e37)
MAGNITUDE_PATTERNS = ("cols2", "step_diag")
MAGNITUDE_CLASSES = (5, 15)          # one narrow and one wide window class of ff_blur_f32 (the test adds the plane path at NKB 19)


def class_cases(kind):
    """[(nkb, quirk, i, pattern)] of the class sweep: every pattern of every window class, quirk on and off"""
    return [(nkb, quirk, i, n) for nkb in NKB_CLASSES for quirk in (True, False) for i, n in enumerate(patterns_for(kind, nkb))]
