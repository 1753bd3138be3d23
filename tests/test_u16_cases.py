"""The u16 case table proven for the oracle alone (no GPU): every case the GPU tests feed to assert_u16_parity excuses at most
EXCUSED_CAP of its samples, so the rule keeps its power (the samples outside the tie tolerance must match exactly).  Candidates over
the cap at their default levels take replacement levels in that window class (u16_parity.LEVEL_OVERRIDES); this test measures every
case at both and holds the table to exactly those."""
import numpy as np
import pytest

import u16_parity as U

ROWS, COLS = U.SHAPE


@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("nkb", U.NKB_CLASSES)
def test_structured_cases_keep_the_rule_sharp(nkb, quirk):
    """every case of the class at the levels the GPU sweep uses stays under the cap; the cases whose default levels do not are
    exactly the ones LEVEL_OVERRIDES replaces (nothing is left out of the sweep)"""
    sigma = U.class_sigma(nkb)
    over = set()
    for name in U.CANDIDATES:
        if U.excused_share(U.oracle_named(name, ROWS, COLS, sigma, quirk)) > U.EXCUSED_CAP:
            over.add((name, nkb, quirk))
        levels = U.case_levels(name, nkb, quirk)
        share = U.excused_share(U.oracle_named(name, ROWS, COLS, sigma, quirk, levels))
        assert share <= U.EXCUSED_CAP, (name, levels, share)
    assert over == {k for k in U.LEVEL_OVERRIDES if k[1] == nkb and k[2] == quirk}
    assert U.class_patterns(nkb, quirk) == U.CANDIDATES


@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("nkb", (3, 11, 17, 23))
@pytest.mark.parametrize("top", [65535, 4095, 255])
def test_noise_cases(top, nkb, quirk):
    """noise sits at 2 x TIE_TOL_U16 = 13.5 % whatever its range"""
    share = U.excused_share(U.oracle_plane(U.noise(nkb + top, ROWS, COLS, top), U.class_sigma(nkb), quirk))
    assert 0.10 <= share <= 0.17


def test_wrap_cases_wrap_and_stay_sharp():
    """sigma 9, quirk on: the constant 65535 leaves the range at the top, the 0 / 65533 diagonal step at the bottom"""
    top = U.oracle_named("const_top", ROWS, COLS, 9.0, True).astype(np.float64)
    bottom = U.oracle_named("step_diag", ROWS, COLS, 9.0, True).astype(np.float64)
    assert (top + 0.5 >= 65536).any() and U.round_u16(top).min() < 1000
    assert (bottom + 0.5 <= -1).any() and U.round_u16(bottom).max() > 64000
    assert U.excused_share(top) <= U.EXCUSED_CAP and U.excused_share(bottom) <= U.EXCUSED_CAP


def test_generators():
    for name in U.CANDIDATES:
        p = U.plane(name, 40, 50)
        assert p.dtype == np.uint16 and p.shape == (40, 50)
    assert np.array_equal(U.plane("rim", 9, 9, (0, 65000)), (U.plane("rim", 9, 9) > 0) * np.uint16(65000))
    for name in ("cols2", "rows2", "checker"):                       # period 2: an even sum of the two levels
        p = U.plane(name, 8, 8)
        assert sorted(np.unique(p).tolist()) == [0, 65534]
    assert U.ramp(3, 4)[2, 3] == 126 * 3 + 2 and U.impulse(9, 9).sum() == 65535
