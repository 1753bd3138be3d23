"""One sigma per channel (blur_gaussian_*_sigmas_*): channel c of the result is channel c of the scalar call with sigmas[c], bit for
bit (u8 with three channels, where the scalar call runs other kernels: the float64 plane oracle under assert_u8_parity, through
every narrow window class of fw_blur_u8<NKB, Q, 3>); sigma = 0 leaves a channel as it is; batches, the host and multi-shard
entries, overlaps, a refused call, the plane path for one group among fused ones, and one 4K case per type family."""
import ctypes as C

import numpy as np
import pytest

import structured as S
from conftest import assert_u8_parity
from test_gpu_gaussian_channels import SHAPES, on_dev, rand_img, sigma_for_class, sigma_for_pad

pytestmark = pytest.mark.gpu

ROWS, COLS = S.SHAPE                      # 397 x 517: ragged either way
TYPES = ("u8", "u16", "f32", "f16", "bf16")
NARROW = (3, 5, 7, 9, 11)


def method(ctx, t):
    return getattr(ctx, "gaussian" if t == "u8" else "gaussian_" + t)


def host_frames(t, seed, shape):
    """random frames for type t as a numpy array: uint8, uint16, or float32 values over a few binades, both signs"""
    rng = np.random.default_rng(seed)
    if t == "u8":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if t == "u16":
        return rng.integers(0, 65536, shape, dtype=np.uint16)
    return (rng.standard_normal(shape) * np.exp2(rng.integers(-3, 4, shape))).astype(np.float32)


def to_dev(t, a):
    """host_frames' array on the device in type t (the half types: rounded there)"""
    import torch
    d = on_dev(a)
    return d if t in ("u8", "u16", "f32") else d.to(torch.float16 if t == "f16" else torch.bfloat16)


def frames_of(t, seed, shape):
    return to_dev(t, host_frames(t, seed, shape))


def raw(x):
    """the tensor's samples as integers of the same width (a view: channel slices copy bit patterns, NaNs included, and stay clear of
    the operators torch lacks for uint16)"""
    import torch
    return x.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[x.element_size()])


def bits(x):
    """the tensor's bytes as a numpy array (NaN-safe, bfloat16 included)"""
    import torch
    return x.contiguous().view(torch.uint8).cpu().numpy()


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def scalar_channels(ctx, t, x, sigmas, **kw):
    """what the contract composes: channel c of the scalar call with sigmas[c]; sigma 0: the source's channel"""
    import torch
    want = x.clone()
    done = {}
    for c, s in enumerate(sigmas):
        if s == 0:
            continue
        if s not in done:
            done[s] = method(ctx, t)(x, s, out=torch.empty_like(x), **kw)
        raw(want)[..., c] = raw(done[s])[..., c]
    return want


def oracle_channel(img, c, sigma, quirk):
    """-> (bytes [rows, cols, 1], plane [1, rows, cols]) of channel c"""
    from oracle import oracle as O
    plane = O.pffft_plane_f64(img[..., c].astype(np.float32), sigma, quirk)[None]
    return np.moveaxis(S.round_u8(plane), 0, -1), plane


def check_u8_channels(got, img, sigmas, quirk):
    """every channel of a u8 frame against its own sigma's oracle plane; sigma 0: the source's bytes"""
    for c, s in enumerate(sigmas):
        if s == 0:
            assert np.array_equal(got[..., c], img[..., c]), "channel %d (sigma 0) changed" % c
        else:
            want, plane = oracle_channel(img, c, s, quirk)
            assert_u8_parity(got[..., c:c + 1], want, plane)


def mixed_sigmas(ch):
    """one narrow class, one of NKB 13 .. 15, one repeated (and for four channels a third class)"""
    a, b, c = sigma_for_class(ROWS, COLS, 5), sigma_for_class(ROWS, COLS, 13), sigma_for_class(ROWS, COLS, 9)
    return (a, b, a) if ch == 3 else (a, b, a, c)


# ---- 1. bit equality with the scalar call -------------------------------------------------------------------------------------
# (u8 with three channels is not here: the scalar call runs other kernels; test_u8c3_* check those channels against the oracle)
TYPE_CH = [(t, ch) for t in TYPES for ch in (3, 4) if (t, ch) != ("u8", 3)]


@pytest.mark.parametrize("engine", [None, "fused", "fft"])
@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("t,ch", TYPE_CH)
def test_bit_equal_to_the_scalar_call(ctx, t, ch, quirk, engine):
    import torch
    sigmas = mixed_sigmas(ch)
    x = frames_of(t, 100 * ch + len(t), (ROWS, COLS, ch))
    got = method(ctx, t)(x, sigmas, out=torch.empty_like(x), nyquist_quirk=quirk, engine=engine)
    family = ctx.last_engine()[0]
    want = scalar_channels(ctx, t, x, sigmas, nyquist_quirk=quirk, engine=engine)
    assert same(got, want)
    assert family == (0 if engine == "fft" else 6)


# ---- 2. u8, three channels: the narrow instantiations of the one-channel-per-workgroup kernel ----------------------------------
@pytest.mark.parametrize("quirk", [True, False])
@pytest.mark.parametrize("at", [0, 1, 2])
@pytest.mark.parametrize("nkb", NARROW)
def test_u8c3_narrow_classes_random(ctx, nkb, at, quirk):
    """class nkb as the sigma of channel `at`, a wide class and a 0 on the other two"""
    import torch
    sig = [0.0, 0.0, 0.0]
    sig[at] = sigma_for_class(ROWS, COLS, nkb)
    sig[(at + 1) % 3] = sigma_for_class(ROWS, COLS, 15)
    img = rand_img(np.random.default_rng(31 * nkb + at), ROWS, COLS, 3)
    t = on_dev(img)
    got = ctx.gaussian(t, sig, out=torch.empty_like(t), nyquist_quirk=quirk, engine="fused")
    assert ctx.last_engine()[0] == 6
    check_u8_channels(got.cpu().numpy(), img, sig, quirk)


U8C3_STRUCTURED = [pytest.param(nkb, quirk, i, id="nkb%d-q%d-%s" % (nkb, quirk, n)) for nkb, quirk, i, n in S.class_cases("u8") if nkb in NARROW]


@pytest.mark.parametrize("nkb,quirk,i", U8C3_STRUCTURED)
def test_u8c3_narrow_classes_structured(ctx, nkb, quirk, i):
    """the patterns of tests/structured.py: channels 0 and 2 through class nkb, channel 1 through its neighbour class"""
    import torch
    other = 5 if nkb == 3 else nkb - 2
    s_own, s_other = sigma_for_class(ROWS, COLS, nkb), sigma_for_class(ROWS, COLS, other)
    sig = (s_own, s_other, s_own)
    where = (nkb, other, nkb)
    names = S.channel_patterns(S.patterns_for("u8", nkb), i, 3)
    spec = [(n, S.u8_levels(n, quirk, where[c])) for c, n in enumerate(names)]
    img = np.stack([S.u8_plane(n, ROWS, COLS, lv) for n, lv in spec], axis=-1)
    t = on_dev(img)
    got = ctx.gaussian(t, sig, out=torch.empty_like(t), nyquist_quirk=quirk, engine="fused").cpu().numpy()
    assert ctx.last_engine()[0] == 6
    for c, (n, lv) in enumerate(spec):
        plane = S.oracle_u8(n, lv, ROWS, COLS, sig[c], quirk)[None]
        assert_u8_parity(got[..., c:c + 1], np.moveaxis(S.round_u8(plane), 0, -1), plane)


WIDTHS = [(300, 128 * 2 + 1), (300, 128 * 2 + 2), (300, 128 * 2 + 3), (300, 4 * 41 + 1), (300, 4 * 41 + 2), (300, 4 * 41 + 3)]


@pytest.mark.parametrize("shape", WIDTHS + [s[:2] for s in SHAPES], ids=lambda s: "%dx%d" % s)
def test_u8c3_staging_shapes(ctx, shape):
    """widths 1 .. 3 past a multiple of 4 and of 128 and the edge-strip boundaries of the 1- and 4-channel tests, three different
    narrow sigmas (as many as the frame's shorter side allows)"""
    import blur_algorithms_amd as B
    import torch
    rows, cols = shape
    room = min(rows, cols) - 1
    sig = [s for s in (1.0, 3.0, 6.0, 11.0) if B.pffft_sizing(rows, cols, s)["pad"] <= room][-3:]
    sig = (sig + [0.0, 0.0])[:3]
    img = rand_img(np.random.default_rng(rows * 7 + cols), rows, cols, 3)
    for quirk in (True, False):
        t = on_dev(img)
        got = ctx.gaussian(t, sig, out=torch.empty_like(t), nyquist_quirk=quirk)
        assert ctx.last_engine()[0] == 6
        check_u8_channels(got.cpu().numpy(), img, sig, quirk)


@pytest.mark.parametrize("ch", [3, 4])
@pytest.mark.parametrize("off", [1, 2, 3])
def test_u8_pointer_offsets_and_guard_bytes(ctx, ch, off):
    import torch
    rows, cols = 150, 259
    sig = (2.0, 0.0, 5.0) if ch == 3 else (2.0, 0.0, 5.0, 2.0)
    img = rand_img(np.random.default_rng(off + ch), rows, cols, ch)
    n = img.size
    src = torch.full((n + 64,), 7, dtype=torch.uint8, device="cuda")
    dst = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    src[off:off + n] = on_dev(img).reshape(-1)
    ctx.gaussian(src[off:off + n].view(rows, cols, ch), sig, out=dst[16 + off:16 + off + n].view(rows, cols, ch))
    assert ctx.last_engine()[0] == 6
    d = dst.cpu().numpy()
    assert np.all(d[:16 + off] == 0xA5) and np.all(d[16 + off + n:] == 0xA5), "guard bytes around the destination changed"
    check_u8_channels(d[16 + off:16 + off + n].reshape(rows, cols, ch), img, sig, True)


# ---- 3. sigma = 0 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES)
def test_bgra_alpha_untouched(ctx, t):
    """(s, s, s, 0): the alpha is the source's, BGR are channels 0 .. 2 of the scalar 4-channel call; out of place and in place, the
    frame between a constant-low and a constant-high frame of a batch"""
    import torch
    s = 4.0
    a = host_frames(t, 5, (ROWS, COLS, 4))
    x = to_dev(t, np.stack([np.zeros_like(a), a, np.full_like(a, 255 if t in ("u8", "u16") else 1.0)]))
    mid = x[1].clone()
    full = method(ctx, t)(x, s, out=torch.empty_like(x))
    want = full.clone()
    raw(want)[..., 3] = raw(x)[..., 3]
    got = method(ctx, t)(x, (s, s, s, 0), out=torch.empty_like(x))
    assert ctx.last_engine()[0] == 6
    assert same(got, want)
    inplace = x.clone()
    assert method(ctx, t)(inplace, (s, s, s, 0)) is inplace
    assert same(inplace, want)
    alone = method(ctx, t)(mid, (s, s, s, 0), out=torch.empty_like(mid))
    assert same(alone, want[1])


@pytest.mark.parametrize("ch", [1, 3, 4])
@pytest.mark.parametrize("t", TYPES)
def test_all_zeros_is_a_copy(ctx, t, ch):
    import torch
    x = frames_of(t, 9, (2, 61, 75, ch))
    out = torch.empty_like(x)
    out.view(torch.uint8).fill_(0x5A)
    got = method(ctx, t)(x, [0] * ch, out=out)
    assert same(got, x)
    keep = x.clone()
    method(ctx, t)(x, [0] * ch)
    assert same(x, keep)


@pytest.mark.parametrize("t", TYPES)
def test_zero_channel_copy_unaligned(ctx, t):
    """the strided channel copy: three channels, a destination that is not 16-byte aligned, a frame that is no multiple of 16 bytes"""
    import torch
    x = frames_of(t, 11, (3, 45, 67, 3))
    flat = torch.empty(x.numel() + 8, dtype=x.dtype, device="cuda")
    out = flat[1:1 + x.numel()].view(x.shape)
    sig = (0, 2.0, 0)
    got = method(ctx, t)(x, sig, out=out)
    if t == "u8":
        for f in range(3):
            check_u8_channels(got[f].cpu().numpy(), x[f].cpu().numpy(), sig, True)
    else:
        assert same(got, scalar_channels(ctx, t, x, sig))


# ---- 4. equal sigmas ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 3, 4])
@pytest.mark.parametrize("t", TYPES)
def test_equal_sigmas_are_the_scalar_call(ctx, t, ch):
    import torch
    x = frames_of(t, 13, (2, 200, 300, ch))
    want = method(ctx, t)(x, 6.0, out=torch.empty_like(x))
    fam = ctx.last_engine()[0]
    got = method(ctx, t)(x, [6.0] * ch, out=torch.empty_like(x))
    assert ctx.last_engine()[0] == fam
    assert same(got, want)
    if t == "u8" and ch == 3:
        for f in range(2):
            assert same(got[f], ctx.pffft_(x[f].clone(), 6.0))


# ---- 5. batch, host, multi, overlap --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES)
def test_batch_host_and_multi_agree(ctx, t):
    import blur_algorithms_amd as B
    import torch
    sig = (3.0, 0.0, 9.0)
    x = frames_of(t, 17, (3, 180, 260, 3))
    batch = method(ctx, t)(x, sig, out=torch.empty_like(x))
    for f in range(3):
        assert same(method(ctx, t)(x[f], sig, out=torch.empty_like(x[f])), batch[f])
    host_in = x.cpu() if t == "bf16" else x.cpu().numpy()
    host = method(ctx, t)(host_in, sig)
    host = host if t == "bf16" else torch.from_numpy(host)
    assert same(host, batch.cpu())
    m = B.BlurMulti([0, 0])
    try:
        assert same(method(m, t)(x, sig, out=torch.empty_like(x)), batch)
        mh = method(m, t)(host_in, sig)
        assert same(mh if t == "bf16" else torch.from_numpy(mh), batch.cpu())
        # zero frames: a no-op (valid pointers, nothing written)
        out = torch.empty_like(x)
        out.view(torch.uint8).fill_(0x77)
        sg = (C.c_double * 3)(*sig)
        assert getattr(m._lib, "blur_gaussian_%s_sigmas_batch_multi_dev" % t)(m._h, x.data_ptr(), out.data_ptr(), 0, 180, 260, 3, sg, None) == 0
        assert getattr(ctx._lib, "blur_gaussian_%s_sigmas_batch_dev" % t)(ctx._h, x.data_ptr(), out.data_ptr(), 0, 180, 260, 3, sg, None) == 0
        torch.cuda.synchronize()
        assert np.all(bits(out) == 0x77)
    finally:
        m.close()


@pytest.mark.parametrize("t", ["u8", "f32"])
def test_partial_overlap_equals_the_disjoint_call(ctx, t):
    """destination = source + one frame + 5 bytes"""
    import torch
    sig = (3.0, 0.0, 9.0, 3.0)
    x = frames_of(t, 19, (3, 90, 130, 4))
    want = method(ctx, t)(x, sig, out=torch.empty_like(x))
    nb = x.numel() * x.element_size()
    fbytes = nb // 3
    buf = torch.zeros(2 * nb + 64, dtype=torch.uint8, device="cuda")
    base = 16 if t == "u8" else 0
    shift = fbytes + (5 if t == "u8" else 8)              # float32 frames stay 4-byte aligned: one frame + 8 bytes
    buf[base:base + nb] = x.view(torch.uint8).reshape(-1)
    src = buf[base:base + nb].view(x.dtype).view(x.shape)
    dst = buf[base + shift:base + shift + nb].view(x.dtype).view(x.shape)
    got = method(ctx, t)(src, sig, out=dst)
    assert same(got, want)


# ---- 6. a refused call wrote nothing ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES)
def test_refused_call_writes_nothing(ctx, t):
    import blur_algorithms_amd as B
    import torch
    rows, cols = 40, 90
    assert B.pffft_sizing(rows, cols, 30.0)["pad"] > rows - 1
    x = frames_of(t, 23, (2, rows, cols, 3))
    out = torch.empty_like(x)
    out.view(torch.uint8).fill_(0x3C)
    with pytest.raises(B.BlurError) as e:
        method(ctx, t)(x, (2.0, 0.0, 30.0), out=out)
    assert e.value.code == 2
    torch.cuda.synchronize()
    assert np.all(bits(out) == 0x3C)
    keep = x.clone()
    with pytest.raises(B.BlurError):
        method(ctx, t)(x, (2.0, 0.0, 30.0))
    torch.cuda.synchronize()
    assert same(x, keep)


# ---- 7. one group past the fused kernel's pads -----------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES)
def test_wide_pad_group_takes_the_plane_path(ctx, t):
    import blur_algorithms_amd as B
    import torch
    rows, cols = S.FALLBACK_SHAPE
    wide = sigma_for_pad(rows, cols, *S.FALLBACK_PAD)
    sig = (3.0, wide, 3.0, 0.0)
    x = frames_of(t, 29, (rows, cols, 4))
    got = method(ctx, t)(x, sig, out=torch.empty_like(x))
    family, note = ctx.last_engine()
    assert family == 0
    assert ("sigma %g " % wide) in note and "0x2" in note and "sigma 3 " not in note
    assert same(got, scalar_channels(ctx, t, x, sig))
    with pytest.raises(B.BlurError):
        method(ctx, t)(x, sig, out=torch.empty_like(x), engine="fused")


@pytest.mark.parametrize("quirk", [True, False])
def test_u8c3_plane_path(ctx, quirk):
    """u8 with three channels on the plane path (reached from this driver only): every group with engine = "fft", and under the
    library's own choice one group past the fused kernel's pads beside a fused one and a 0"""
    import torch
    img = rand_img(np.random.default_rng(53), ROWS, COLS, 3)
    t = on_dev(img)
    sig = (sigma_for_class(ROWS, COLS, 5), 0.0, sigma_for_class(ROWS, COLS, 13))
    got = ctx.gaussian(t, sig, out=torch.empty_like(t), nyquist_quirk=quirk, engine="fft")
    family, note = ctx.last_engine()
    assert family == 0 and "0x1" in note and "0x4" in note
    check_u8_channels(got.cpu().numpy(), img, sig, quirk)
    rows, cols = S.FALLBACK_SHAPE
    wide = sigma_for_pad(rows, cols, *S.FALLBACK_PAD)
    img = rand_img(np.random.default_rng(59), rows, cols, 3)
    t = on_dev(img)
    sig = (wide, 3.0, 0.0)
    got = ctx.gaussian(t, sig, out=torch.empty_like(t), nyquist_quirk=quirk)
    family, note = ctx.last_engine()
    assert family == 0 and ("sigma %g " % wide) in note and "0x1" in note and "sigma 3 " not in note
    check_u8_channels(got.cpu().numpy(), img, sig, quirk)


# ---- 8. 4K ----------------------------------------------------------------------------------------------------------------------
def test_4k_u8c3_luminance_kept(ctx):
    import torch
    rows, cols = 2160, 3840
    sig = (0.0, 11.0, 11.0)
    img = rand_img(np.random.default_rng(41), rows, cols, 3)
    t = on_dev(img)
    got = ctx.gaussian(t, sig, out=torch.empty_like(t))
    assert ctx.last_engine()[0] == 6
    check_u8_channels(got.cpu().numpy(), img, sig, True)


def test_4k_f32_three_sigmas(ctx):
    import torch
    sig = (3.0, 7.0, 11.0)
    x = frames_of("f32", 43, (2160, 3840, 3))
    got = ctx.gaussian_f32(x, sig, out=torch.empty_like(x))
    assert ctx.last_engine()[0] == 6
    assert same(got, scalar_channels(ctx, "f32", x, sig))
