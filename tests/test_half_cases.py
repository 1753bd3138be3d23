"""The half-precision parity helper and its case table proven without a GPU: hand values of RN_T for both types (ties to even,
subnormals, overflow to Inf, -0), the rule rejecting a sample one ulp outside its interval and a case over the cap, and every
(case, window class, quirk, type) of the GPU sweep under AMBIGUOUS_CAP on the oracle alone, so that the rule keeps its power (the
unambiguous samples must be the correctly rounded reference)."""
import numpy as np
import pytest

import half_parity as H

ROWS, COLS = H.SHAPE


def test_rn_f16_hand_values():
    rn = H.rn_f16
    assert rn(1.0 + 2.0 ** -11) == 1.0 and rn(1.0 + 3 * 2.0 ** -11) == 1.0 + 2.0 ** -9        # ties to even, both ways
    assert rn(1.0 + 2.0 ** -11 + 2.0 ** -40) == 1.0 + 2.0 ** -10                              # just past a tie (lost through float32? no: one rounding)
    assert rn(65519.999) == 65504.0 and np.isposinf(rn(65520.0)) and np.isneginf(rn(-65520.0))
    assert rn(2.0 ** -24) == 2.0 ** -24 and rn(2.0 ** -25) == 0.0 and rn(3 * 2.0 ** -25) == 2.0 ** -23     # subnormals, ties to even
    assert rn(2.0 ** -25 * 1.0001) == 2.0 ** -24
    z = rn(np.array([-0.0, -1e-9]))
    assert np.all(z == 0) and np.all(np.signbit(z))


def test_rn_bf16_hand_values():
    rn = H.rn_bf16
    assert rn(1.0 + 2.0 ** -8) == 1.0 and rn(1.0 + 3 * 2.0 ** -8) == 1.0 + 2.0 ** -6         # ties to even
    # one rounding from float64: 1 + 2^-8 + 2^-30 rounds up; through float32 it would first become the tie 1 + 2^-8 and round down
    assert rn(1.0 + 2.0 ** -8 + 2.0 ** -30) == 1.0 + 2.0 ** -7
    assert float(np.float32(1.0 + 2.0 ** -8 + 2.0 ** -30)) == 1.0 + 2.0 ** -8
    assert rn(H.BF16_MAX) == H.BF16_MAX and rn(H.BF16_MAX + 2.0 ** 119 * 0.999) == H.BF16_MAX
    assert np.isposinf(rn(H.BF16_MAX + 2.0 ** 119)) and np.isneginf(rn(-3.4e38))              # the tie goes to the even neighbour: Inf
    assert rn(1.9999) == 2.0                                                                  # the carry moves into the exponent
    assert rn(2.0 ** -133) == 2.0 ** -133 and rn(2.0 ** -134) == 0.0 and rn(3 * 2.0 ** -134) == 2.0 ** -132
    assert rn(2.0 ** -126) == 2.0 ** -126 and rn(2.0 ** -126 * (1 - 2.0 ** -9)) == 2.0 ** -126
    z = rn(np.array([-0.0, -1e-45]))
    assert np.all(z == 0) and np.all(np.signbit(z))
    # every bfloat16 bit pattern is a fixed point, and bits <-> values round-trip
    b = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    with np.errstate(invalid="ignore"):
        v = H.from_bits("bf16", b).astype(np.float64)
    fin = np.isfinite(v)
    assert np.array_equal(rn(v[fin]), v[fin]) and np.array_equal(H.to_bits("bf16", v[fin]), b[fin])
    with np.errstate(invalid="ignore"):
        v = H.from_bits("f16", b).astype(np.float64)
    fin = np.isfinite(v)
    assert np.array_equal(H.rn_f16(v[fin]), v[fin]) and np.array_equal(H.to_bits("f16", v[fin]), b[fin])


@pytest.mark.parametrize("kind", H.TYPES)
def test_rule_rejects_one_ulp_outside_and_a_case_over_the_cap(kind):
    u = H.ulp(kind, 0.4)
    assert u == (2.0 ** -12 if kind == "f16" else 2.0 ** -9)
    ref = np.full((1, 8, 8), float(H.rn(kind, 0.4)) + 0.25 * u)        # a quarter ulp above a representable value: unambiguous
    good = H.rn(kind, ref[0])
    assert H.assert_half_parity(kind, good, ref, 1.0) == 0
    for delta in (u, -u):
        bad = good.copy()
        bad[3, 4] += delta
        with pytest.raises(AssertionError):
            H.assert_half_parity(kind, bad, ref, 1.0)
    nan = good.copy()
    nan[0, 0] = np.nan
    with pytest.raises(AssertionError):
        H.assert_half_parity(kind, nan, ref, 1.0)
    # on a rounding boundary both neighbours pass, but a frame of such samples is over the cap
    tie = np.full((1, 8, 8), float(H.rn(kind, 0.4)) + 0.5 * u)
    lo, hi = H.interval(kind, tie, 1.0)
    assert np.all(hi - lo == u)
    with pytest.raises(AssertionError, match="ambiguous"):
        H.assert_half_parity(kind, lo[0], tie, 1.0)
    mixed = ref.copy()
    mixed[0, 0, :3] = tie[0, 0, :3]                                    # 3 of 64 ambiguous: under the cap, either neighbour passes there
    out = H.rn(kind, mixed[0])
    out[0, :3] = [lo[0, 0, 0], hi[0, 0, 0], lo[0, 0, 0]]
    assert H.assert_half_parity(kind, out, mixed, 1.0) == 3
    # overflow: past the type's largest value the interval's ends are Inf and only Inf passes
    if kind == "f16":
        big = np.full((1, 4, 4), 65600.0)
        assert H.assert_half_parity(kind, np.full((4, 4), np.inf), big, 65504.0) == 0
        with pytest.raises(AssertionError):
            H.assert_half_parity(kind, np.full((4, 4), 65504.0), big, 65504.0)
    H.assert_float_side(kind, good, ref, 1.0)


def case_maxabs(kind):
    """the largest sample of any frame of the structured table: the rule's tolerance grows with max|x|, so a share proven at this
    value bounds the share of every frame the GPU sweep builds from these planes"""
    return float(H.quantise(kind, np.float64(0.7)))


@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("nkb", H.NKB_CLASSES)
@pytest.mark.parametrize("kind", H.TYPES)
def test_structured_cases_keep_the_rule_sharp(kind, nkb, quirk):
    """every case of the class at the levels the GPU sweep uses stays under the cap; the cases whose default levels do not are
    exactly the ones LEVEL_OVERRIDES replaces (nothing is left out of the sweep)"""
    sigma = H.class_sigma(nkb)
    m = case_maxabs(kind)
    over = set()
    for name in H.CANDIDATES:
        d = H.default_levels(name, quirk)
        assert max(abs(d[0]), abs(d[1])) <= m + 1e-3
        if H.ambiguous_share(kind, H.oracle_named(kind, name, ROWS, COLS, sigma, quirk, d), m) > H.AMBIGUOUS_CAP:
            over.add((name, nkb, quirk, kind))
        levels = H.case_levels(name, nkb, quirk, kind)
        assert max(abs(levels[0]), abs(levels[1])) <= max(abs(d[0]), abs(d[1]))
        share = H.ambiguous_share(kind, H.oracle_named(kind, name, ROWS, COLS, sigma, quirk, levels), m)
        assert share <= H.AMBIGUOUS_CAP, (name, levels, share)
    assert over == {k for k in H.LEVEL_OVERRIDES if k[1] == nkb and k[2] == quirk and k[3] == kind}


@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("nkb", (3, 9, 17, 23))
@pytest.mark.parametrize("top", [1.0, 255.0])
@pytest.mark.parametrize("kind", H.TYPES)
def test_noise_cases(kind, top, nkb, quirk):
    p = H.noise(kind, nkb, ROWS, COLS, top)
    assert p.min() >= 0
    share = H.ambiguous_share(kind, H.oracle_plane(p, H.class_sigma(nkb), quirk), float(p.max()))
    assert share <= 0.02


def test_overflow_case():
    """the constant 65504 frame at sigma 9 with the quirk on passes 65520 over part of the frame and stays below it elsewhere"""
    p = H.oracle_plane(np.full((ROWS, COLS), H.F16_MAX, np.float32), 9.0, True).astype(np.float64)
    assert (p >= 65521.0).any() and (p < 65519.0).any()
    assert H.ambiguous_share("f16", p, H.F16_MAX) <= H.AMBIGUOUS_CAP


def test_generators_are_quantised():
    for kind in H.TYPES:
        for name in H.CANDIDATES:
            p = H.plane(kind, name, 40, 50, H.default_levels(name, True))
            assert p.dtype == np.float32 and p.shape == (40, 50)
            assert np.array_equal(H.from_bits(kind, H.to_bits(kind, p)), p)
        p = H.plane(kind, "cols2", 8, 8, H.default_levels("cols2", True))
        assert p.min() == -p.max() and abs(p.max() - 0.7) < 4e-3
        q = H.plane(kind, "cols2", 8, 8, H.default_levels("cols2", False))
        assert q.min() < 0 and abs(q.min() + 1.0 / 3.0) < 2e-3
