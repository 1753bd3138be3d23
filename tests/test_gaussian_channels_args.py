"""blur_gaussian_u8_*: argument validation that needs no device (the checks run before the context is touched, so ctx may be
NULL), the bindings of the new entry points, and the host-side geometry of the one-channel-per-workgroup fused kernel's staging and
stores (fw_kernels.hpp: fw_blur_u8 for 1, 3 and 4 channels) mirrored in Python."""
import ctypes as C

import pytest

INVALID, UNSUPPORTED = 1, 2


def lib():
    from blur_algorithms_amd import _lib
    return _lib.load()


def opts():
    from blur_algorithms_amd._lib import BlurOpts
    o = BlurOpts()
    lib().blur_opts_default(C.byref(o))
    return o


BUF = (C.c_uint8 * 64)()
P = C.addressof(BUF)


@pytest.mark.parametrize("channels", [0, 2, 5, -1, 3 * 256])
def test_bad_channel_count(channels):
    o = opts()
    L = lib()
    assert L.blur_gaussian_u8_batch_dev(None, P, P, 1, 4, 4, channels, 1.0, C.byref(o)) == INVALID
    assert L.blur_gaussian_u8_dev(None, P, P, 4, 4, channels, 1.0, C.byref(o)) == INVALID
    assert L.blur_gaussian_u8_host(None, P, P, 4, 4, channels, 1.0, C.byref(o)) == INVALID
    assert L.blur_gaussian_u8_batch_multi_dev(None, P, P, 1, 4, 4, channels, 1.0, C.byref(o)) == INVALID
    assert L.blur_gaussian_u8_batch_multi_host(None, P, P, 1, 4, 4, channels, 1.0, C.byref(o)) == INVALID


@pytest.mark.parametrize("channels", [1, 3, 4])
def test_null_pointers_and_counts(channels):
    o = opts()
    L = lib()
    for src, dst in ((None, P), (P, None), (None, None)):
        assert L.blur_gaussian_u8_batch_dev(None, src, dst, 1, 4, 4, channels, 1.0, C.byref(o)) == INVALID
        assert L.blur_gaussian_u8_dev(None, src, dst, 4, 4, channels, 1.0, C.byref(o)) == INVALID
        assert L.blur_gaussian_u8_host(None, src, dst, 4, 4, channels, 1.0, C.byref(o)) == INVALID
    assert L.blur_gaussian_u8_batch_dev(None, P, P, -1, 4, 4, channels, 1.0, C.byref(o)) == INVALID
    for rows, cols, sigma in ((0, 4, 1.0), (4, -1, 1.0), (4, 4, 0.0), (4, 4, -2.0)):
        assert L.blur_gaussian_u8_batch_dev(None, P, P, 1, rows, cols, channels, sigma, C.byref(o)) == INVALID


@pytest.mark.parametrize("channels", [1, 3, 4])
def test_sigma_too_large_for_the_shape(channels):
    """pad > min(rows, cols) - 1 -> BLUR_ERR_UNSUPPORTED (the reference's reflect-101 would read outside the image), before the
    device; a valid call without a context is BLUR_ERR_INVALID"""
    import blur_algorithms_amd as B
    o = opts()
    L = lib()
    rows, cols = 40, 90
    big = 30.0
    assert B.pffft_sizing(rows, cols, big)["pad"] > rows - 1
    assert L.blur_gaussian_u8_batch_dev(None, P, P, 1, rows, cols, channels, big, C.byref(o)) == UNSUPPORTED
    assert L.blur_gaussian_u8_dev(None, P, P, rows, cols, channels, big, C.byref(o)) == UNSUPPORTED
    assert L.blur_gaussian_u8_host(None, P, P, rows, cols, channels, big, C.byref(o)) == UNSUPPORTED
    small = 2.0
    assert B.pffft_sizing(rows, cols, small)["pad"] <= rows - 1
    assert L.blur_gaussian_u8_batch_dev(None, P, P, 1, rows, cols, channels, small, C.byref(o)) == INVALID


def test_python_shapes():
    from blur_algorithms_amd.api import _gauss_frames_shape
    assert _gauss_frames_shape((5, 7)) == (1, 5, 7, 1)
    assert _gauss_frames_shape((5, 7, 4)) == (1, 5, 7, 4)
    assert _gauss_frames_shape((3, 5, 7, 1)) == (3, 5, 7, 1)
    for bad in ((5, 7, 2), (5,), (2, 5, 7, 5), (1, 2, 3, 4, 5), (0, 5), (4, 0, 1), (2, 4, 0, 3)):
        with pytest.raises(ValueError):
            _gauss_frames_shape(bad)


def test_multi_refuses_a_mismatched_out_before_the_library():
    """BlurMulti.gaussian on the numpy path: an `out` of another shape, dtype or layout is refused before the library is called (it
    would be written past its end)"""
    import numpy as np
    from blur_algorithms_amd import api

    class NoLib:
        def blur_opts_default(self, o):
            pass

        def __getattr__(self, name):
            def called(*args):
                raise AssertionError("the library was called: %s" % name)
            return called

    m = object.__new__(api.BlurMulti)
    m._lib = NoLib()
    m._h = None
    m.devices = [0]
    frames = np.zeros((2, 8, 8, 4), np.uint8)
    for bad in (np.zeros((1, 8, 8, 4), np.uint8), np.zeros((2, 8, 8, 4), np.float32), np.zeros((2, 8, 8, 4), np.uint8)[:, ::-1], [0] * 512):
        with pytest.raises(ValueError):
            api.BlurMulti.gaussian(m, frames, 2.0, out=bad)
    with pytest.raises(ValueError):
        api.BlurMulti.gaussian_f32(m, frames.astype(np.float32), 2.0, out=np.zeros((2, 8, 8, 4), np.uint8))


# ---- host mirror of the staging and store geometry of fw_blur_u8 --------------------------------------------------------
def fw_cfg(nkb):
    pada = 8 * (nkb - 2)
    win = 128 + 2 * pada
    gpr = win // 4
    per = (gpr + 7) // 8
    cs = max(nkb, 9)
    ips = (per + cs - 6) // (cs - 5)
    return pada, win, gpr, per, cs, ips


# the kernel's instantiations (fw_conv.hip, one object per window class): 1 and 4 channels for every window class, 3 for the wide ones (NKB >= 13)
FW_KERNELS = [(ch, nkb) for ch in (1, 3, 4) for nkb in (3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23) if ch != 3 or nkb >= 13]


@pytest.mark.parametrize("ch, nkb", FW_KERNELS)
def test_staging_covers_the_window_once(ch, nkb):
    """thread (row, g0) loads the groups g0 + 8 k (4 pixels = 4 ch bytes each; ch = 3: twelve-byte groups at 12 g0 + 96 k) at byte
    4 ch g0 + 32 ch k of a window row; the groups past the window's last one reload group g0 (their halfs land in the row's
    padding); the column-pass slots 5 .. cs - 1 commit ips items each, which must cover all per of them"""
    pada, win, gpr, per, cs, ips = fw_cfg(nkb)
    assert ips * (cs - 5) >= per
    seen = {}
    for g0 in range(8):
        for k in range(per):
            inside = gpr % 8 == 0 or k < per - 1 or g0 < gpr % 8
            off = 4 * ch * g0 + (32 * ch * k if inside else 0)
            assert off + 4 * ch <= ch * win, "a load past the window row"
            if inside:
                grp = g0 + 8 * k
                assert off == 4 * ch * grp
                seen[grp] = seen.get(grp, 0) + 1
    assert sorted(seen) == list(range(gpr)) and set(seen.values()) == {1}
    # the LDS row (32 per halfs) holds every committed group: 4 g0 + 32 k + 4 <= 32 per <= pitch
    assert 4 * 7 + 32 * (per - 1) + 4 <= 32 * per


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_output_stores_stay_in_the_frame(ch):
    """CH = 1: lane q of quad Q stores pixels 4 Q .. 4 Q + 3 of row 8 gq + 4 h + q as one dword when all four lie in the image,
    else (ragged widths) bytes for the ones that do; CH = 3, 4: byte c of the lane's pixel.  Every pixel of a tile is stored once."""
    for cols in (1, 2, 3, 4, 5, 127, 128, 129, 130, 131, 517):
        for x0 in range(0, cols, 128):
            written = {}
            for wave in range(4):
                for m in range(32):
                    if ch == 1:
                        xq = x0 + 32 * wave + 4 * (m >> 2)
                        qn = 0 if xq >= cols else min(4, cols - xq)
                        px = list(range(xq, xq + 4)) if qn == 4 else list(range(xq, xq + qn))
                    else:
                        xcol = x0 + 32 * wave + m
                        px = [xcol] if xcol < cols else []
                    for x in px:
                        assert x < cols
                        written[x] = written.get(x, 0) + 1
            want = set(range(x0, min(x0 + 128, cols)))
            assert set(written) == want
            # CH = 1: the four lanes of a quad store the same pixels, each in its own row; CH = 3, 4: one lane per pixel
            assert set(written.values()) == {4 if ch == 1 else 1}


@pytest.mark.parametrize("ch", [3, 4])
def test_byte_store_offsets(ch):
    """CH = 3, 4: the byte of (row 32 tile + 8 gq + 4 h + k, pixel xcol, channel c) goes to (row cols + xcol) ch + c, whether the
    kernel adds the row group's offset to the lane's offset in row 4 h (CH = 3) or computes it whole (CH = 4); in-frame bytes lie
    inside the output resource (rows cols ch bytes)"""
    rows, cols = 70, 131
    size = rows * cols * ch
    rowstep = cols * ch
    for c in range(ch):
        for xcol in (0, 1, 127, 128, 130):
            for h in (0, 1):
                lane_out = (4 * h * cols + xcol) * ch + c
                for tile in (0, 1, 2):
                    for gq in range(4):
                        row0 = 32 * tile + 8 * gq + 4 * h
                        split = lane_out + (32 * tile + 8 * gq) * rowstep
                        whole = (row0 * cols + xcol) * ch + c
                        assert split == whole
                        for k in range(4):
                            if row0 + k < rows:
                                o = whole + k * rowstep
                                assert o == ((row0 + k) * cols + xcol) * ch + c and o < size
