"""The pad sweep's case table (tests/pad_cases.py) proven on the CPU: the sigma helper against the built library for all 168 pads on
every shape the sweep uses, the sweep's completeness (every pad, both parities and both ends of every class), and for every frame
tests/test_gpu_pad_sweep.py feeds to a parity helper, that the float64 oracle ALONE stays inside the share of samples the helper
excuses (assert_u8_parity: ties below 2e-3; u16_parity.EXCUSED_CAP; half_parity.AMBIGUOUS_CAP), so that no cap can decide a case.
A case that breaks a cap gets another seed or other levels in pad_cases.py, never a wider cap."""
import numpy as np
import pytest

import half_parity as H
import pad_cases as P
import structured as S
import u16_parity as U
from conftest import TIE_TOL

SMALL = 500                          # samples: below this one excused u8 byte is more than 2e-3 of the frame


def _sizing_pad(rows, cols, sigma):
    import blur_algorithms_amd as B
    return B.pffft_sizing(rows, cols, sigma)["pad"]


def test_sigma_for_pad_against_the_library():
    """every pad 1 .. 168 on its class's sweep frame and on both thin frames: the sizing gives that pad, the plan that class"""
    import blur_algorithms_amd as B
    for p in range(1, P.MAX_PAD + 1):
        nkb = P.class_of(p)
        sigma = P.sigma_for_pad(p)
        assert B.gaussian_window(sigma) == 2 * p + 1
        for rows, cols in (P.sweep_shape(nkb),) + P.thin_shapes(p):
            assert _sizing_pad(rows, cols, sigma) == p, (p, rows, cols)
            assert B.gaussian_sigmas_plan(rows, cols, [sigma, 0.0, sigma]) == [(0, p, nkb), (-1, 0, 0), (0, p, nkb)]
        for rows, cols in P.thin_shapes(p):           # the smallest: one row or column fewer and the API refuses the pad
            assert min(rows, cols) == p + 1 and max(rows, cols) >= 2 * p + 1
    assert B.gaussian_sigmas_plan(400, 400, [P.sigma_for_pad(P.MAX_PAD + 1)])[0][2] == 0


def test_the_sweep_is_complete():
    """every pad once, 16 per class (8 for NKB 3); the pattern and sign pads hold both parities and both ends of every class; the
    sweep frames are ragged in tiles and chunks and do not cap the window"""
    assert sorted(p for nkb in P.NKB_CLASSES for p in P.CLASS_PADS[nkb]) == list(range(1, P.MAX_PAD + 1))
    for nkb in P.NKB_CLASSES:
        pads = P.CLASS_PADS[nkb]
        assert len(pads) == (8 if nkb == 3 else 16) and pads[-1] == P.pada(nkb) and all(P.class_of(p) == nkb for p in pads)
        assert pads[0] == (1 if nkb == 3 else 8 * (nkb - 4) + 1)
        pp = P.pattern_pads(nkb)
        assert pp[0] == pads[0] and pp[-1] == pads[-1] and set(pp) <= set(pads) and len(set(pp)) == 4
        assert {p & 1 for p in pp[1:3]} == {0, 1} and {p & 1 for p in (pp[0], pp[-1])} == {0, 1}
        assert {p & 1 for p in P.sign_pads(nkb)} == {0, 1} and set(P.sign_pads(nkb)) <= set(pads)
        assert {P.pada(nkb) - p for p in pads} == set(range(8 if nkb == 3 else 16))      # every offset of the taps in the window
        ends = P.thin_ends(nkb)
        assert ends["low"] == pads[0] and ends["high"] == pads[-1]
        rows, cols = P.sweep_shape(nkb)
        assert rows % 32 in (6, 14, 22, 30) and cols % 4 == 3 and cols % 128 != 0 and 2 <= (cols + 127) // 128 <= 4
        assert max(rows, cols) >= 2 * P.pada(nkb) + 1 and min(rows, cols) > P.pada(nkb)
    assert P.sweep_shape(3) == (46, 151) and P.sweep_shape(23) == (206, 471)
    assert P.thin_ends(3)["low2"] == 2
    for ch in (1, 3, 4):
        assert len(set(P.channel_slots(ch))) == ch
    assert len({P.channel_slots(ch)[0] for ch in (1, 3, 4)}) == 3                     # a plane changes its channel with the count


def test_no_two_channels_of_a_frame_agree():
    for kind in P.KINDS:
        for nkb in (3, 13, 23):
            for quirk in (True, False):
                for p in P.pattern_pads(nkb):
                    rows, cols = P.sweep_shape(nkb)
                    for ch, specs in P.sweep_frames(kind, nkb, p, quirk):
                        f = P.frame(kind, specs, rows, cols)
                        assert f.shape == (rows, cols, ch)
                        assert all(not np.array_equal(f[..., a], f[..., b]) for a in range(ch) for b in range(a))
                for d in (0, 1):
                    p = P.thin_ends(nkb)["low"]
                    rows, cols = P.thin_shapes(p)[d]
                    frames = P.thin_frames(kind, nkb, p, d, quirk) + [(4, s) for s in P.thin_batch(kind, nkb, p, d, quirk, 4)]
                    for ch, specs in frames:
                        f = P.frame(kind, specs, rows, cols)
                        assert all(not np.array_equal(f[..., a], f[..., b]) for a in range(ch) for b in range(a))


def _prove(kind, frames, rows, cols, sigma, quirk, what):
    """the oracle of every frame inside the cap of the helper the GPU test checks it with"""
    for ch, specs in frames:
        planes = P.oracle_planes(kind, specs, rows, cols, sigma, quirk)
        assert planes.dtype == np.float32 and np.all(np.isfinite(planes)), (what, specs)
        if kind == "u8":
            for s, pl in zip(specs, planes):
                share = S.tie_share(pl, TIE_TOL)
                if rows * cols < SMALL:
                    assert share == 0, "%s %s: an oracle value within TIE_TOL of a tie on a frame of %d samples" % (what, s, rows * cols)
                assert share < S.TIE_CAP, "%s %s: tie share %.3g" % (what, s, share)
        elif kind == "u16":
            for s, pl in zip(specs, planes):
                share = U.excused_share(pl)
                assert share <= U.EXCUSED_CAP, "%s %s: excused share %.3f" % (what, s, share)
        elif kind in H.TYPES:
            share = H.ambiguous_share(kind, np.moveaxis(planes.astype(np.float64), 0, -1), P.maxabs(kind, specs, rows, cols))
            assert share <= H.AMBIGUOUS_CAP, "%s %s: ambiguous share %.3f" % (what, specs, share)


@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("nkb", P.NKB_CLASSES)
def test_every_sweep_case_keeps_the_rules_sharp(nkb, quirk):
    rows, cols = P.sweep_shape(nkb)
    for p in P.CLASS_PADS[nkb]:
        for kind in P.KINDS:
            _prove(kind, P.sweep_frames(kind, nkb, p, quirk), rows, cols, P.sigma_for_pad(p), quirk, "%s pad %d quirk %d" % (kind, p, quirk))


@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("nkb", P.NKB_CLASSES)
def test_every_thin_case_keeps_the_rules_sharp(nkb, quirk):
    """the frames whose side is pad + 1, the batches among them; u8 frames below 500 samples: no oracle value at a tie at all"""
    for end, p in P.thin_ends(nkb).items():
        for d in (0, 1):
            rows, cols = P.thin_shapes(p)[d]
            for kind in P.KINDS:
                frames = P.thin_frames(kind, nkb, p, d, quirk)
                if nkb in P.THIN_BATCH_CLASSES and end == "low":
                    frames = frames + [(ch, s) for ch in (1, 3, 4) for s in P.thin_batch(kind, nkb, p, d, quirk, ch)]
                _prove(kind, frames, rows, cols, P.sigma_for_pad(p), quirk, "%s thin %dx%d pad %d quirk %d" % (kind, rows, cols, p, quirk))


def test_the_other_frames_keep_the_rules_sharp():
    """both sides of the library's own choice at pad 104 / 105, and the clean frames of the non-finite test"""
    rows, cols = P.AUTO_BOUNDARY_SHAPE
    for kind in P.KINDS[1:]:
        for p, _ in P.AUTO_BOUNDARY:
            assert rows > p and cols >= 2 * p + 1
            _prove(kind, P.auto_boundary_frames(kind, p), rows, cols, P.sigma_for_pad(p), True, "%s boundary pad %d" % (kind, p))
    rows, cols, sigma = P.NONFINITE_SHAPE_SIGMA
    for kind in P.NONFINITE_KINDS:
        for ch in (1, 3):
            frames = P.nonfinite_frames(kind, ch)
            assert len({s for f in frames for s in f}) == 3 * ch
            _prove(kind, [(ch, frames[0]), (ch, frames[2])], rows, cols, sigma, True, "%s non-finite" % kind)


def test_the_sign_frames_have_power():
    """cols2 at sign_levels: the difference of the quirk-on and quirk-off oracles is of the order of the amplitude (a flipped sign
    doubles it), and the quirk-on plane stays inside the type's range (no wrap enters the difference)"""
    for kind in P.KINDS:
        lo, hi = P.sign_levels(kind)
        for nkb in P.NKB_CLASSES:
            rows, cols = P.sweep_shape(nkb)
            for p in P.sign_pads(nkb):
                spec = P.sign_specs(kind, 4)[0]
                on = P.oracle(kind, spec, rows, cols, P.sigma_for_pad(p), True).astype(np.float64)
                off = P.oracle(kind, spec, rows, cols, P.sigma_for_pad(p), False).astype(np.float64)
                assert np.abs(on - off).max() >= 0.4 * (hi - lo), (kind, p)
                if kind == "u8":
                    assert on.min() > -0.5 and on.max() < 255.5
                if kind == "u16":
                    assert on.min() > -0.5 and on.max() < 65535.5
