"""The structured-content case table (tests/structured.py) checked on the CPU: what every generator draws, and the two conditions
the GPU tests rest on.

* u8: assert_u8_parity lets at most 2e-3 of the bytes differ, and only where the oracle sits within TIE_TOL of a rounding boundary.
  Mismatches are a subset of the oracle's ties, so every u8 case must have an oracle tie share below that same 2e-3: then the cap
  cannot be what makes a case pass or fail.  A case that breaks the condition gets other levels (structured.u8_levels), never a
  wider cap.
* f32: every oracle plane is finite and representable in float32 (max|out| / max|x| reaches 1.0003 with the quirk on, so the
  magnitudes stop at 1e37)."""
import numpy as np
import pytest

import structured as S
from conftest import TIE_TOL
from test_gpu_gaussian_f32 import sigma_for_class, sigma_for_pad

ROWS, COLS = S.SHAPE
ALL = S.PATTERNS + ("impulses",)


@pytest.mark.parametrize("shape", [S.SHAPE, (33, 40), (180, 1500)])
@pytest.mark.parametrize("name", ALL)
def test_generators(name, shape):
    rows, cols = shape
    p = S.pattern(name, rows, cols)
    assert p.shape == (rows, cols) and p.dtype == np.float64 and p.flags["C_CONTIGUOUS"]
    assert p.min() >= 0 and p.max() <= 1
    assert np.array_equal(p, S.pattern(name, rows, cols))                      # deterministic
    if name in S.TWO_LEVEL:
        assert set(np.unique(p)) == {0.0, 1.0}
    y, x = np.mgrid[:rows, :cols]
    if name == "cols2":
        assert np.array_equal(p, x % 2)
    if name == "rows2":
        assert np.array_equal(p, y % 2)
    if name == "checker":
        assert np.array_equal(p, (x + y) % 2)
    if name in ("white", "black"):
        assert np.all(p == (name == "white"))
    if name == "step_v":
        assert np.all(p[:, :cols // 2] == 0) and np.all(p[:, cols // 2:] == 1)
    if name == "step_h":
        assert np.all(p[:rows // 2] == 0) and np.all(p[rows // 2:] == 1)
    if name == "step_diag":
        assert p[0, 0] == 1 and p[rows - 1, 0] == 0 and p[0, cols - 1] == 1
        assert np.all(np.diff(p, axis=1) >= 0) and np.all(np.diff(p, axis=0) <= 0)
        assert all(0 < p[r].sum() < cols for r in range(1, rows))              # the edge crosses every row below the first
    if name == "blocks":
        assert np.array_equal(p, ((y + 5) // 32 + (x + 7) // 32) % 2)
        assert p[0, 0] == 0 and p[26, 24] != p[27, 24] and p[26, 24] != p[26, 25]               # edges at row 27 = 32 - 5 and column 25 = 32 - 7
    if name == "ramp_h":
        assert p[0, 0] == 0 and p[0, -1] == 1 and np.all(np.diff(p, axis=1) > 0) and np.all(p == p[:1])
    if name == "ramp_v":
        assert p[0, 0] == 0 and p[-1, 0] == 1 and np.all(np.diff(p, axis=0) > 0) and np.all(p == p[:, :1])
    if name == "rim":
        assert np.all(p[1:-1, 1:-1] == 0)
        assert np.all(p[0] == 1) and np.all(p[-1] == 1) and np.all(p[:, 0] == 1) and np.all(p[:, -1] == 1)
    if name == "rim2":
        assert np.all(p[0] == 0) and np.all(p[-1] == 0) and np.all(p[:, 0] == 0) and np.all(p[:, -1] == 0)
        assert np.all(p[2:-2, 2:-2] == 0)
        assert np.all(p[1, 1:-1] == 1) and np.all(p[-2, 1:-1] == 1) and np.all(p[1:-1, 1] == 1) and np.all(p[1:-1, -2] == 1)
    if name == "impulses":
        pts = S.impulse_points(rows, cols)
        assert p.sum() == len(pts) and all(p[r, c] == 1 for r, c in pts)
        assert {(0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1), (rows // 2, cols // 2)} <= set(pts)


def test_impulse_points_of_the_sweep_frame():
    pts = set(S.impulse_points(ROWS, COLS))
    assert {(31, 127), (32, 128)} <= pts
    assert (384, 512) in pts                                                   # first pixel of the ragged last tile and strip
    assert any(r == ROWS - 1 and c > 512 for r, c in pts) and any(c == COLS - 1 and r > 384 for r, c in pts)


def test_levels_and_frames():
    for name in ALL:
        for quirk in (True, False):
            lo, hi = S.u8_levels(name, quirk)
            b = S.u8_plane(name, ROWS, COLS, (lo, hi))
            assert b.dtype == np.uint8 and b.min() >= lo and b.max() <= hi
            if name in S.TWO_LEVEL:
                assert set(np.unique(b)) == {lo, hi}
        assert S.u8_levels(name, True) == (0, 255)
        lo, hi = S.f32_levels(name)
        f = S.f32_plane(name, ROWS, COLS, (lo, hi))
        assert f.dtype == np.float32
        if name in S.TWO_LEVEL:
            assert set(np.unique(f)) == {lo, hi}
        # not dyadic: after any power-of-two scale the binary16 `hi` half leaves a non-zero `lo` half
        for v in (lo, hi):
            assert float(np.float16(v)) != float(v)
    assert S.u8_levels("checker", False) == (0, 254) and S.u8_levels("white", False) == (0, 255)
    assert len(np.unique(S.u8_plane("ramp_h", ROWS, COLS, (0, 255)))) == 256   # every byte value
    assert len(np.unique(S.u8_plane("ramp_v", ROWS, COLS, (0, 255)))) == 256
    for name in S.HEADROOM:
        lo, hi = S.f32_levels(name)
        assert lo == -hi                                                       # +max, -max: the headroom bound is attained
    # no two channels of a frame agree, and every pattern is channel 0 of some case
    for kind, nkb in (("u8", 3), ("u8", 7), ("f32", 7)):
        names = S.patterns_for(kind, nkb)
        assert ("impulses" in names) == (kind == "f32" or nkb <= 5)
        assert set(S.CORE) <= set(names)
        for i in range(len(names)):
            assert len(set(S.channel_patterns(names, i, 4))) == 4
    f, spec = S.u8_frame(S.PATTERNS, 2, 4, ROWS, COLS, True)
    assert f.shape == (ROWS, COLS, 4) and [n for n, _ in spec] == ["checker", "white", "black", "step_v"]
    for c in range(4):
        h = S.one_hot_u8(c, 4, 8, 9)
        assert np.all(h[..., c] == 255) and h.sum() == 255 * 72
        g = S.one_hot_f32(c, 4, 8, 9, 1e30)
        assert np.all(g[..., c] == np.float32(float(S.F32_HI) * 1e30)) and np.count_nonzero(g) == 72


def test_round_u8_wraps():
    assert list(S.round_u8(np.array([-0.67, -0.4, 0.49, 254.6, 255.49, 255.5, 256.04], np.float32))) == [0, 0, 0, 255, 255, 0, 0]


def _sigmas():
    return {nkb: sigma_for_class(ROWS, COLS, nkb) for nkb in S.NKB_CLASSES}


def test_tie_share_of_every_u8_class_case():
    """the sweep: every pattern x window class x quirk, one plane each (the GPU frames are made of these planes)"""
    sig = _sigmas()
    worst = (0.0, ())
    for nkb, quirk, _, name in S.class_cases("u8"):
        share = S.tie_share(S.oracle_u8(name, S.u8_levels(name, quirk, nkb), ROWS, COLS, sig[nkb], quirk), TIE_TOL)
        worst = max(worst, (share, (name, nkb, quirk)))
        assert share < S.TIE_CAP, "%s NKB %d quirk %d: tie share %.3g" % (name, nkb, quirk, share)
    print("worst tie share %.3g at %s" % worst)


def test_tie_share_of_the_other_u8_cases():
    """segments and strips, the policy switches, one_hot"""
    cases = [(r, c, s, n) for r, c, s in S.SEGMENT_SHAPES for n in S.SEGMENT_PATTERNS]
    r, c = S.FALLBACK_SHAPE
    cases += [(r, c, sigma_for_pad(r, c, *S.FALLBACK_PAD), n) for n in S.SWITCH_PATTERNS]
    r, c, s = S.FFT_SHAPE_SIGMA
    cases += [(r, c, s, n) for n in S.SWITCH_PATTERNS]
    cases += [(ROWS, COLS, s, n) for s in _sigmas().values() for n in ("white", "black")]      # the planes of one_hot
    for rows, cols, sigma, name in cases:
        for quirk in (True, False):
            share = S.tie_share(S.oracle_u8(name, S.u8_levels(name, quirk, (rows, cols)), rows, cols, sigma, quirk), TIE_TOL)
            assert share < S.TIE_CAP, "%s %dx%d sigma %g quirk %d: tie share %.3g" % (name, rows, cols, sigma, quirk, share)


def test_level_overrides_are_needed():
    """every override replaces levels that do break the condition (none is a leftover), and keeps the 255 end"""
    sig = _sigmas()
    for (name, where, quirk), lv in S.U8_LEVEL_OVERRIDES.items():
        assert lv[1] == 255 and quirk
        if isinstance(where, int):
            rows, cols, sigma = ROWS, COLS, sig[where]
        else:
            rows, cols = where
            sigma = dict((s[:2], s[2]) for s in S.SEGMENT_SHAPES).get(where) or sigma_for_pad(rows, cols, *S.FALLBACK_PAD)
        assert S.tie_share(S.oracle_u8(name, (0, 255), rows, cols, sigma, quirk), TIE_TOL) >= S.TIE_CAP


def test_checker_0_255_without_the_quirk_is_all_ties():
    """why the quirk-off cases take 0 / 254: the 0 / 255 checker blurs to 127.5 everywhere"""
    assert S.tie_share(S.oracle_u8("checker", (0, 255), ROWS, COLS, 3.0, False), TIE_TOL) > 0.99


def _finite_f32(plane, limit):
    p = np.asarray(plane)
    assert p.dtype == np.float32 and np.all(np.isfinite(p))
    assert float(np.max(np.abs(p.astype(np.float64)))) <= limit


def test_every_float_class_case_is_finite():
    sig = _sigmas()
    top = 0.0
    for nkb, quirk, _, name in S.class_cases("f32"):
        lv = S.f32_levels(name)
        out = S.oracle_f32(name, lv, ROWS, COLS, sig[nkb], quirk)
        m = float(max(abs(lv[0]), abs(lv[1])))
        _finite_f32(out, 1.01 * m)
        top = max(top, float(np.max(np.abs(out))) / m)
    print("max|out| / max|x| over the sweep: %.5f" % top)
    assert top > 0.99                        # the period-2 frames keep their amplitude under the quirk: the headroom case is real


def test_the_other_float_cases_are_finite():
    """segments and strips, the policy switches (one_hot: a constant plane)"""
    cases = [(r, c, s, n) for r, c, s in S.SEGMENT_SHAPES for n in S.SEGMENT_PATTERNS]
    r, c = S.FALLBACK_SHAPE
    cases += [(r, c, sigma_for_pad(r, c, *S.FALLBACK_PAD), n) for n in S.SWITCH_PATTERNS]
    r, c, s = S.FFT_SHAPE_SIGMA
    cases += [(r, c, s, n) for n in S.SWITCH_PATTERNS]
    for rows, cols, sigma, name in cases:
        for quirk in (True, False):
            _finite_f32(S.oracle_f32(name, S.f32_levels(name), rows, cols, sigma, quirk), 0.71)
    for sigma in _sigmas().values():
        for quirk in (True, False):
            _finite_f32(S.oracle_f32("white", (np.float32(0), S.F32_HI), ROWS, COLS, sigma, quirk), 0.71)


def test_float_magnitude_ends_are_finite():
    sig = _sigmas()
    fmax = float(np.finfo(np.float32).max)
    for mag in S.MAGNITUDES:
        for name in S.MAGNITUDE_PATTERNS:
            lv = S.f32_levels(name)
            x = S.f32_plane(name, ROWS, COLS, lv, mag)
            m = float(np.max(np.abs(x)))
            assert np.all(np.isfinite(x)) and m >= float(np.finfo(np.float32).tiny)       # normal numbers, both ends
            assert abs(m / (0.7 * mag) - 1) < 1e-6
            for nkb in S.MAGNITUDE_CLASSES:
                for quirk in (True, False):
                    _finite_f32(S.oracle_f32(name, lv, ROWS, COLS, sig[nkb], quirk, mag), min(1.01 * m, fmax))


def test_ramps_blur_monotone_without_the_quirk():
    """what the GPU test's extra assertion rests on: the oracle's own rows (ramp_h) and columns (ramp_v) never decrease"""
    for sigma in (1.0, 9.0, 40.0):
        for name, axis in (("ramp_h", 1), ("ramp_v", 0)):
            out = S.oracle_f32(name, S.f32_levels(name), ROWS, COLS, sigma, False)
            assert np.all(np.diff(out.astype(np.float64), axis=axis) >= 0)
            assert np.all(np.diff(S.round_u8(S.oracle_u8(name, (0, 254), ROWS, COLS, sigma, False)).astype(int), axis=axis) >= 0)


def test_top_of_the_scale_interval_cases_are_finite():
    sig = _sigmas()
    assert 0.9999 * 2.0 ** 16 > 65520 > 0.7 * 2.0 ** 16          # past binary16's rounding limit to infinity; 0.7 is not
    for name in S.HEADROOM + ("step_diag",):
        lv = S.f32_top_levels(name)
        assert float(lv[1]) == float(S.F32_TOP) and float(np.float16(lv[1])) != float(lv[1])
        for nkb in S.MAGNITUDE_CLASSES:
            for quirk in (True, False):
                _finite_f32(S.oracle_f32(name, lv, ROWS, COLS, sig[nkb], quirk), 1.01)
