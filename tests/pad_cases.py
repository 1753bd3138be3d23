"""Every pad of every window class, and the smallest frames a pad accepts: the cases tests/test_gpu_pad_sweep.py runs on the fused
kernels and tests/test_pad_cases.py proves on the CPU.  Plain module: no fixtures, no GPU.

A fused kernel is instantiated per window class NKB, which serves the pads 8 (NKB - 4) + 1 .. 8 (NKB - 2) (NKB 3: 1 .. 8), but inside
a class the pad still decides the sign of the quirk terms (its parity), where the 2 pad + 1 taps sit in the 16 NKB window (the
kernels stage PADA = 8 (NKB - 2) halo pixels, 0 .. 7 more than the pad), the transform sizes and the float kernels' frame scale.
The other sweeps run one pad per class; this table runs all 168, and the frames whose side is pad + 1, where the staged halo passes
the single reflection the image allows.

A plane is named by a spec, a tuple: ("noise", seed, top) or ("pat", pattern of structured.py, (lo, hi)).  plane() draws it in the
sample type, oracle() gives its float64 oracle plane through structured.py's cache, keyed by the spec, so the frames of 1, 3 and 4
channels share planes.  No two channels of a frame hold the same plane."""
import math

import numpy as np

import half_parity as H
import structured as S
import u16_parity as U

NKB_CLASSES = S.NKB_CLASSES
KINDS = ("u8", "f32", "u16", "f16", "bf16")
MAX_PAD = 168
PERIOD2 = S.HEADROOM                 # cols2, rows2, checker: the quirk terms at their maximum


def sigma_for_pad(p):
    """the centre of the sigma interval whose uncapped window is 2 p + 1: gaussian_window truncates 2 (sigma sqrt(2 ln 255) - 1)
    + 0.5, which is 2 p + 1 here and has a quarter of a pad to either side"""
    return (p + 1.25) / math.sqrt(2.0 * math.log(255.0))


def pada(nkb):
    """the halo the kernels of class nkb stage: the class's largest pad"""
    return 8 * (nkb - 2)


def class_pads(nkb):
    return tuple(range(1 if nkb == 3 else 8 * (nkb - 4) + 1, pada(nkb) + 1))


CLASS_PADS = {nkb: class_pads(nkb) for nkb in NKB_CLASSES}


def class_of(p):
    return next(nkb for nkb in NKB_CLASSES if p in CLASS_PADS[nkb])


def sweep_shape(nkb):
    """(rows, cols) = (PADA + 38, 2 PADA + 135): 46 x 151 .. 206 x 471.  rows % 32 is 6, 14, 22 or 30 (a ragged last tile),
    cols % 4 = 3 and 2 to 4 chunks of 128 with a ragged last one, and max(rows, cols) >= 2 PADA + 1, so the sizing does not cap
    the window"""
    return pada(nkb) + 38, 2 * pada(nkb) + 135


def thin_shapes(p):
    """the smallest frames the API accepts for pad p, thin in rows and thin in columns (pad <= min(rows, cols) - 1, and the long
    side keeps the window uncapped)"""
    return (p + 1, 2 * p + 3), (2 * p + 3, p + 1)


def pattern_pads(nkb):
    """the pads that also run the period-2 patterns: both ends of the class and the two pads at its middle, one of each parity"""
    lo, hi = CLASS_PADS[nkb][0], CLASS_PADS[nkb][-1]
    mid = (lo + hi) // 2
    return lo, mid, mid + 1, hi


def sign_pads(nkb):
    """one even and one odd pad for the direct check of the quirk's sign"""
    return pattern_pads(nkb)[1:3]


def thin_ends(nkb):
    """{name: pad} of the thin-frame cases: the class's ends (NKB 3 also pad 2: with pad 1 the pads whose pad + 1 columns are fewer
    than the 4 the quirk's pre-pass needs)"""
    ends = {"low": CLASS_PADS[nkb][0], "high": CLASS_PADS[nkb][-1]}
    if nkb == 3:
        ends["low2"] = 2
    return ends


# ---- planes ------------------------------------------------------------------------------------------------------------------------
def half_top(p):
    """the range of the half types' noise at pad p: 0 .. 255 on every fourth pad, 0 .. 1 elsewhere (one range per frame: a channel
    far below the frame's max|x| would be ambiguous throughout)"""
    return 255.0 if p % 4 == 1 else 1.0


# Noise planes of the smallest thin frames whose default seed breaks a cap on the oracle alone: on 10 samples one u8 value within
# TIE_TOL of a rounding tie (one mismatching byte is more than assert_u8_parity's 2e-3 of any frame below 500 samples) or one
# ambiguous binary16 sample (0.10 against AMBIGUOUS_CAP = 0.05).  (kind, pad, where, slot) -> what is added to the seed; proven, with the
# quirk on and off, by tests/test_pad_cases.py
SEED_BUMPS = {
    ("u8", 1, 1, 2): 1,
    ("f16", 1, 2, 0): 1,
}
# Levels that replace a case's default ones where the oracle alone breaks a cap (same proof): (kind, pattern, pad, where, quirk) ->
# (lo, hi), where as in noise_spec.  A period-2 pattern blurs to a near-constant (and with the quirk on to a near-constant amplitude),
# so its samples sit at one distance from a rounding tie: a u16 case is excused nowhere or nearly everywhere, pad by pad.  The rim at
# -1/3 .. 0.7 blurs through 0 on the thin frames of pad 8 and 9, where binary16 samples are ambiguous (0.057 .. 0.082 of the frame)
LEVEL_OVERRIDES = {
    ("f16", "rim", 8, 1, True): (0.35, 0.7),
    ("f16", "rim", 8, 2, True): (0.35, 0.7),
    ("f16", "rim", 9, 1, True): (0.35 * 255, 0.7 * 255),
    ("f16", "rim", 9, 2, True): (0.35 * 255, 0.7 * 255),
    # the period-2 patterns of the sweep, found by trying (0, 50000), (0, 60000), .. in turn (u16) and -1/3 .. 0.7 (binary16)
    ("f16", "cols2", 8, 0, True): (-0.3333333333333333, 0.7),
    ("u16", "cols2", 9, 0, False): (0, 50000),
    ("u16", "rows2", 9, 0, False): (0, 50000),
    ("u16", "cols2", 16, 0, True): (0, 60000),
    ("u16", "checker", 16, 0, True): (0, 50000),
    ("u16", "rows2", 24, 0, True): (0, 50000),
    ("u16", "cols2", 32, 0, True): (0, 50000),
    ("u16", "cols2", 32, 0, False): (0, 50000),
    ("u16", "rows2", 32, 0, False): (0, 50000),
    ("u16", "checker", 40, 0, True): (0, 50000),
    ("u16", "cols2", 41, 0, True): (0, 50000),
    ("u16", "cols2", 48, 0, True): (0, 50000),
    ("u16", "cols2", 56, 0, False): (0, 50000),
    ("u16", "rows2", 56, 0, False): (0, 50000),
    ("u16", "rows2", 64, 0, True): (0, 50000),
    ("u16", "checker", 64, 0, True): (0, 50000),
    ("u16", "cols2", 65, 0, True): (0, 50000),
    ("u16", "cols2", 72, 0, True): (0, 60000),
    ("u16", "rows2", 72, 0, True): (0, 50000),
    ("u16", "cols2", 73, 0, True): (0, 50000),
    ("u16", "cols2", 73, 0, False): (0, 50000),
    ("u16", "rows2", 73, 0, False): (0, 50000),
    ("u16", "rows2", 81, 0, True): (0, 50000),
    ("u16", "checker", 112, 0, True): (0, 50000),
    ("u16", "checker", 120, 0, True): (0, 50000),
    ("u16", "rows2", 121, 0, True): (0, 50000),
    ("u16", "cols2", 121, 0, False): (0, 50000),
    ("u16", "rows2", 121, 0, False): (0, 50000),
    ("u16", "checker", 128, 0, True): (0, 50000),
    ("u16", "cols2", 144, 0, True): (0, 50000),
    ("u16", "checker", 161, 0, True): (0, 50000),
    ("u16", "cols2", 168, 0, True): (0, 50000),
}


def noise_spec(kind, p, slot, where=0):
    """noise plane `slot` (0 .. 3) of pad p; where: 0 the sweep frame, 1 / 2 the thin frames.  u16: the last slot is 12-bit noise"""
    seed = 1000003 * KINDS.index(kind) + 1009 * p + 101 * where + 7 * slot + SEED_BUMPS.get((kind, p, where, slot), 0)
    if kind == "u8":
        return ("noise", seed, 255)
    if kind == "u16":
        return ("noise", seed, 4095 if slot == 3 else 65535)
    return ("noise", seed, 1.0 if kind == "f32" else half_top(p))


def default_levels(kind, name, nkb, quirk, top=1.0):
    """the levels the other sweeps use for the pattern in this class: structured.u8_levels / f32_levels, u16_parity.case_levels,
    half_parity.case_levels (times the range of the frame's noise)"""
    if kind == "u8":
        return S.u8_levels(name, quirk, nkb)
    if kind == "u16":
        return U.case_levels(name, nkb, quirk)
    if kind == "f32":
        lo, hi = S.f32_levels(name)
        return float(lo), float(hi)
    lo, hi = H.case_levels(name, nkb, quirk, kind)
    return lo * top, hi * top


def pat_spec(kind, name, p, where, quirk, nkb, top=1.0, swap=False):
    lv = LEVEL_OVERRIDES.get((kind, name, p, where, bool(quirk)), default_levels(kind, name, nkb, quirk, top))
    return ("pat", name, (lv[1], lv[0]) if swap else tuple(lv))


def plane(kind, spec, rows, cols):
    """the plane in the sample type: uint8, uint16, or float32 values (f16 / bf16: values of the type)"""
    if spec[0] == "noise":
        _, seed, top = spec
        if kind == "u8":
            return np.random.default_rng(seed).integers(0, 256, (rows, cols), dtype=np.uint8)
        if kind == "u16":
            return U.noise(seed, rows, cols, top)
        if kind == "f32":
            return np.random.default_rng(seed).uniform(-top, top, (rows, cols)).astype(np.float32)
        return H.noise(kind, seed, rows, cols, top)
    _, name, (lo, hi) = spec
    if kind == "u8":
        return S.u8_plane(name, rows, cols, (lo, hi))
    if kind == "u16":
        return np.ascontiguousarray(U.two_level(name, rows, cols, lo, hi))
    if kind == "f32":
        return S.f32_plane(name, rows, cols, (np.float32(lo), np.float32(hi)))
    return H.plane(kind, name, rows, cols, (lo, hi))


def frame(kind, specs, rows, cols):
    return np.stack([plane(kind, s, rows, cols) for s in specs], axis=-1)


def oracle(kind, spec, rows, cols, sigma, quirk):
    """the float64 oracle of the plane (returned as float32, as every oracle plane of the suite), kept in structured.py's cache"""
    return S.oracle_plane(np.asarray(plane(kind, spec, rows, cols), np.float32), sigma, quirk, ("pad", kind, spec, rows, cols))


def oracle_planes(kind, specs, rows, cols, sigma, quirk):
    """-> [ch, rows, cols]"""
    return np.stack([oracle(kind, s, rows, cols, sigma, quirk) for s in specs])


def maxabs(kind, specs, rows, cols):
    return float(max(np.abs(plane(kind, s, rows, cols).astype(np.float64)).max() for s in specs))


# ---- the frames of the sweep -------------------------------------------------------------------------------------------------------
def channel_slots(ch):
    """which of a case's four planes the channels of a ch-channel frame hold: rotated by the channel count, so that a plane sits
    in a different channel of each"""
    return tuple((ch + c) % 4 for c in range(ch))


def sweep_planes(kind, nkb, p, quirk, patterns):
    """the four planes of a sweep case: noise, or the three period-2 patterns and cols2 again with its levels swapped"""
    if not patterns:
        return [noise_spec(kind, p, slot) for slot in range(4)]
    top = half_top(p) if kind in H.TYPES else 1.0
    names = PERIOD2[p % 3:] + PERIOD2[:p % 3]
    return [pat_spec(kind, n, p, 0, quirk, nkb, top) for n in names] + [pat_spec(kind, names[0], p, 0, quirk, nkb, top, swap=True)]


def sweep_frames(kind, nkb, p, quirk):
    """[(ch, [spec per channel])] of pad p: noise frames of 1, 3 and 4 channels, and on pattern_pads the pattern frames"""
    out = []
    for patterns in (False, True) if p in pattern_pads(nkb) else (False,):
        four = sweep_planes(kind, nkb, p, quirk, patterns)
        out += [(ch, [four[s] for s in channel_slots(ch)]) for ch in (1, 3, 4)]
        if patterns:                     # one channel: every pattern on its own (the frame above holds four[1])
            out += [(1, [four[0]]), (1, [four[2]])]
    return out


def thin_planes(kind, nkb, p, direction, quirk):
    """the four planes of a thin case: three of noise and the rim (a one-pixel border: every reflected halo pixel of a frame this
    small weighs on the result)"""
    top = half_top(p) if kind in H.TYPES else 1.0
    return [noise_spec(kind, p, slot, 1 + direction) for slot in range(3)] + [pat_spec(kind, "rim", p, 1 + direction, quirk, nkb, top)]


def thin_frames(kind, nkb, p, direction, quirk):
    """[(ch, [spec per channel])]: noise and the rim alone, and frames of 3 and 4 channels holding both"""
    four = thin_planes(kind, nkb, p, direction, quirk)
    return [(1, [four[0]]), (1, [four[3]])] + [(ch, [four[s] for s in channel_slots(ch)]) for ch in (3, 4)]


def thin_batch(kind, nkb, p, direction, quirk, ch):
    """three different ch-channel frames of the same four planes"""
    four = thin_planes(kind, nkb, p, direction, quirk)
    return [[four[(i + c) % 4] for c in range(ch)] for i in (1, 2, 3)]


THIN_BATCH_CLASSES = (3, 7, 13, 19)   # the batches of thin frames: the low end of a narrow, two middle and a wide class


def sign_levels(kind):
    """cols2 at levels whose blur stays inside the type's range with the quirk on (1.0003 of the amplitude): no wrap in the
    difference of the two calls"""
    return {"u8": (0, 254), "u16": (0, 50000), "f32": (-0.7, 0.7), "f16": (-0.7, 0.7), "bf16": (-0.7, 0.7)}[kind]


def sign_specs(kind, ch):
    """a ch-channel frame of cols2: the levels, the levels swapped, and both halved"""
    lo, hi = sign_levels(kind)
    half = (lo // 2, hi // 2) if kind in ("u8", "u16") else (lo / 2, hi / 2)
    four = [("pat", "cols2", (lo, hi)), ("pat", "cols2", (hi, lo)), ("pat", "cols2", half), ("pat", "cols2", half[::-1])]
    return [four[s] for s in channel_slots(ch)]


# the library's own choice for float32, u16 and the half types stops at pad 104 (NKB 15): both sides of that boundary on one frame
AUTO_BOUNDARY = ((104, 6), (105, 0))                     # (pad, engine family)
AUTO_BOUNDARY_SHAPE = sweep_shape(17)


def auto_boundary_frames(kind, p):
    return [(ch, [noise_spec(kind, p, s) for s in channel_slots(ch)]) for ch in (1, 3, 4)]


# the non-finite contract (include/blur_amd.h): a batch of three frames whose middle one holds a NaN, a +Inf and a -Inf
NONFINITE_SHAPE_SIGMA = (150, 261, 7.0)
NONFINITE_KINDS = ("f32", "f16", "bf16")


def nonfinite_frames(kind, ch):
    """the specs of the three frames (noise in 0 .. 1 for the half types, -1 .. 1 for float32); the middle one is then poisoned"""
    return [[("noise", 7000 + 1000 * KINDS.index(kind) + 10 * f + c, 1.0) for c in range(ch)] for f in range(3)]


# the float kernels above the library's own choice (NKB 17 .. 23, on request only: DESIGN.md 2.2) whose accumulation passes
# 1e-6 max|x| on noise at some pad: (kind, pad) that run on the library's own choice (family 0, the same bound) instead
NOISE_ON_AUTO = frozenset()
